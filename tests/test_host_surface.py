"""CPU-side tests of the boundary metrics: the references of tests/surface_ref.py against scipy, and the public
surface of the feature (entry points, names, argument checks) as far as it exists without a GPU."""
import inspect

import numpy as np
import pytest
import torch

import surface_ref as R

SHAPES = [(17, 23, 12), (24, 20)]


def label_pair(shape, C=5, seed=1):
    a = R.voronoi_labels(shape, C, seed)
    return a, R.rolled(a)


# ================================================================================================ the references against scipy
@pytest.mark.parametrize("shape", SHAPES)
def test_surface_is_mask_minus_its_erosion(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    nd = len(shape)
    for lab in label_pair(shape):
        for c in range(5):
            m = (lab[0, 0] == c)
            assert bool(m.any()), c
            want = m.numpy() & ~ndi.binary_erosion(m.numpy())
            got = R.surface(m, nd).numpy()
            assert np.array_equal(got, want)
            assert 0 < got.sum() <= m.sum()


@pytest.mark.parametrize("shape", SHAPES)
def test_edt_sq_is_scipys_transform_squared(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    nd = len(shape)
    for lab in label_pair(shape):
        for c in range(5):
            f = R.surface(lab == c, nd)
            want = np.rint(ndi.distance_transform_edt(~f[0, 0].numpy()) ** 2).astype(np.int64)
            got = R.edt_sq(f)[0, 0].numpy().astype(np.int64)
            assert np.array_equal(got, want)


def test_reference_conventions():
    """an empty set gives EDT_INF; a 2-D surface ignores the missing depth; the distances of a hand-made pair"""
    assert bool((R.edt_sq(torch.zeros(1, 1, 3, 4, 5, dtype=torch.bool)) == R.EDT_INF).all())
    full = torch.ones(1, 1, 5, 6, dtype=torch.bool)
    s = R.surface(full, 2)[0, 0]
    assert int(s.sum()) == 5 * 6 - 3 * 4 and not bool(s[1:-1, 1:-1].any())
    assert bool(R.surface(full.unsqueeze(2), 3).all())                     # the depth-1 volume under the 6-neighbour rule: all surface
    a = torch.zeros(1, 1, 16, 16, 16, dtype=torch.int64)
    b = a.clone()
    a[..., 4:10, 4:10, 4:10] = 1
    b[..., 4:10, 4:10, 6:12] = 1
    r = R.surface_distances(a, b, 3)
    assert r["hd"][0, 1] == 2.0 and r["n_a"][0, 1] == r["n_b"][0, 1] == 6 ** 3 - 4 ** 3
    assert np.isnan(r["hd"][0, 2]) and r["n_a"][0, 2] == 0
    assert r["hist"][0, 1, 0].sum() == r["n_a"][0, 1] and r["hist"].shape[-1] == 3 * 15 ** 2 + 1


# ================================================================================================ the public surface
def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    for n in ("pulpo_edt_sq", "pulpo_surface_distances", "pulpo_surface_distances_ws_bytes", "pulpo_surface_distances_bins"):
        assert n in protos, n
    assert len(protos["pulpo_surface_distances"][1]) == 15 and len(protos["pulpo_edt_sq"][1]) == 7
    assert header_abi_version() == 8


def test_library_exports_and_checks_arguments():
    import ctypes
    from pulpo_amd._lib import lib
    assert lib.query("pulpo_abi_version") == 8
    edt, sd = lib.raw("pulpo_edt_sq"), lib.raw("pulpo_surface_distances")
    assert lib.query("pulpo_surface_distances_bins", 160, 160, 160) == 3 * 159 ** 2 + 1
    assert lib.query("pulpo_surface_distances_bins", 1, 24, 20) == 23 ** 2 + 19 ** 2 + 1
    # 160^3, C = 36: the counts, four classes of int32 distance planes, the histograms
    assert lib.query("pulpo_surface_distances_ws_bytes", 1, 36, 160, 160, 160) == 4 * (4 * 160 ** 3 + 2 * 36 + 2 * 36 * (3 * 159 ** 2 + 1))
    # the distance planes do not grow with C
    assert (lib.query("pulpo_surface_distances_ws_bytes", 1, 72, 160, 160, 160) - lib.query("pulpo_surface_distances_ws_bytes", 1, 36, 160, 160, 160)
            == 4 * 36 * (2 + 2 * (3 * 159 ** 2 + 1)))
    assert lib.query("pulpo_surface_distances_ws_bytes", 1, 4, 1025, 8, 8) == 0
    buf = (ctypes.c_int * 4096)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.POINTER(ctypes.c_int))
    for shape in ((1, 1025, 4, 4), (1, 4, 1025, 4), (1, 4, 4, 1025), (0, 4, 4, 4), (1, 0, 4, 4)):          # refused before any launch
        assert edt(p, ip, *shape, None) != 0, shape
        assert sd(p, p, 0, 3, 95.0, p, None, p, ip, *shape, 3, None) != 0, shape
    assert edt(None, ip, 1, 4, 4, 4, None) != 0 and edt(p, None, 1, 4, 4, 4, None) != 0
    good = (1, 4, 4, 4, 3, None)
    assert sd(None, p, 0, 3, 95.0, p, None, p, ip, *good) != 0 and sd(p, p, 0, 3, 95.0, p, None, None, ip, *good) != 0
    assert sd(p, p, 2, 3, 95.0, p, None, p, ip, *good) != 0 and sd(p, p, 0, 0, 95.0, p, None, p, ip, *good) != 0
    assert sd(p, p, 0, 3, 101.0, p, None, p, ip, *good) != 0 and sd(p, p, 0, 257, 95.0, p, None, p, ip, *good) != 0
    assert sd(p, p, 0, 3, 95.0, p, None, p, ip, 1, 4, 4, 4, 2, None) != 0                                  # nd = 2 needs depth 1


def test_cpu_tensors_are_refused():
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    assert ops.EDT_INF == 1 << 29 == R.EDT_INF
    m = torch.zeros(1, 1, 4, 5, 6, dtype=torch.bool)
    lab = torch.zeros(1, 1, 4, 5, 6, dtype=torch.uint8)
    for call in (lambda: ops.edt_sq(m), lambda: ops.edt_sq(m[:, :, 0]), lambda: ops.surface_distances(lab, lab, 3),
                 lambda: ops.surface_distances(lab[:, :, 0], lab[:, :, 0], 3, return_hist=True)):
        with pytest.raises(PulpoHipError):
            call()
    with pytest.raises(ValueError):
        ops.surface_distances(lab, lab, 3, percentile=101.0)


def test_evaluation_names_and_arguments():
    from pulpo_amd import evaluation
    assert evaluation.SURFACE_METRICS == ("HD95", "ASSD")
    for fn in (evaluation.level_scores, evaluation.performance):
        params = inspect.signature(fn).parameters
        assert params["surface"].default is False and params["include_background"].default is False
    z = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="surface"):
        evaluation.level_scores({0: z}, {0: torch.zeros(1, 3, 4, 4, 4)}, z, surface=True)
    with pytest.raises(ValueError, match="surface"):
        evaluation.performance(None, z, z, surface=True)
