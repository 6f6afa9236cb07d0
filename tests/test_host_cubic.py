"""Cubic B-spline interpolation without a GPU: the float64 definition of tests/cubic_ref.py against scipy.ndimage
(spline_filter and map_coordinates, order 3, mode "mirror") and against itself (integer coordinates, the tridiagonal identity, autograd
against the definition's gradient expression, the half-voxel round trip), and the public surface - header, library argument checks, the
refusals of pulpo_amd.ops / models / refine / evaluation.  tests/test_gpu_cubic.py holds the kernels to this definition."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import affine_ref as AR
import cubic_ref as CR
from oracle import pulpo_oracle as O

FB = list(O.FEEDBACK_DEFAULT)
# (field grid, image size) of the scipy comparisons; every field pushes a share of its samples outside the volume
SCIPY_CASES = [((5, 6, 7), (5, 6, 7)), ((9, 11, 14), (7, 12, 10)), ((2, 3, 4), (2, 3, 4))]
SCIPY_TOL = 1e-12                       # max abs, images in [0, 1]
ROUND_TRIP_SIZE = (24, 20, 28)


def unit_image(B, C, size, seed):
    return torch.rand(B, C, *size, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def round_trip_image(dtype=torch.float64):
    """smoothed noise at ROUND_TRIP_SIZE: uniform noise under two passes of a separable [1 2 1] / 4 filter, replicate-padded"""
    img = unit_image(1, 1, ROUND_TRIP_SIZE, 11)
    k = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
    for _ in range(2):
        for dim in (2, 3, 4):
            shape = [1, 1, 1, 1, 1]
            shape[dim] = 3
            pad = [0] * 6
            pad[2 * (4 - dim)] = pad[2 * (4 - dim) + 1] = 1
            img = torch.nn.functional.conv3d(torch.nn.functional.pad(img, pad, mode="replicate"), k.view(shape))
    return img.to(dtype)


# ================================================================================================ the definition against scipy
@pytest.mark.parametrize("grid,isize", SCIPY_CASES)
def test_prefilter_is_scipys_spline_filter(grid, isize):
    import scipy.ndimage as ndi
    img = unit_image(2, 2, isize, 1)
    got = CR.prefilter(img)
    for b in range(2):
        for c in range(2):
            want = ndi.spline_filter(img[b, c].numpy(), order=3, mode="mirror", output=np.float64)
            assert float((got[b, c] - torch.from_numpy(want)).abs().max()) <= SCIPY_TOL


@pytest.mark.parametrize("grid,isize", SCIPY_CASES)
def test_value_is_scipys_map_coordinates_at_the_clamped_coordinate(grid, isize):
    import scipy.ndimage as ndi
    B, C = 2, 2
    img = unit_image(B, C, isize, 2)
    df = CR.smooth_field(B, grid, 3, 2.0) if min(grid) >= 4 else 2.0 * torch.randn(B, 3, *grid, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    assert CR.outside_fraction(df, isize) > 0.02, "no sample outside the volume"
    got = CR.warp(df, img)
    c, _, _ = CR.coords(df, isize)
    for b in range(B):
        for ch in range(C):
            want = ndi.map_coordinates(img[b, ch].numpy(), c[b].reshape(3, -1).numpy(), order=3, mode="mirror", output=np.float64)
            assert float((got[b, ch].reshape(-1) - torch.from_numpy(want)).abs().max()) <= SCIPY_TOL


# ================================================================================================ the definition against itself
def test_integer_coordinates_return_the_image():
    from test_host_affine import integer_landing_field
    Sg, Si = (6, 5, 7), (12, 10, 14)
    img = unit_image(1, 2, Si, 4)
    df = integer_landing_field(Sg, Si, (1, -1, 2))
    c, _, _ = CR.coords(df, Si)
    assert float((c - c.round()).abs().max()) < 1e-12
    idx = c.round().long()
    want = AR._gather(img, idx[:, 0], idx[:, 1], idx[:, 2])
    assert float((CR.warp(df, img) - want).abs().max()) < 1e-12


@pytest.mark.parametrize("size", [(5, 6, 7), (2, 3, 4), (1, 9, 70)])
def test_tridiagonal_identity(size):
    """(c[m(k-1)] + 4 c[k] + c[m(k+1)]) / 6 = s[k] along every axis of at least two samples, applied in turn, gives the image back"""
    img = unit_image(1, 2, size, 5)
    back = CR.prefilter(img)
    for dim in (2, 3, 4):
        N = back.shape[dim]
        if N == 1:
            continue
        k = torch.arange(N)
        back = (back.index_select(dim, CR.mirror(k - 1, N)) + 4 * back + back.index_select(dim, CR.mirror(k + 1, N))) / 6
    assert float((back - img).abs().max()) < 1e-13


def test_mirror_index():
    assert CR.mirror(torch.arange(-1, 7), 5).tolist() == [1, 0, 1, 2, 3, 4, 3, 2]
    assert CR.mirror(torch.arange(-1, 4), 2).tolist() == [1, 0, 1, 0, 1]
    assert CR.mirror(torch.arange(-1, 3), 1).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("grid,isize", [((5, 6, 7), (5, 6, 7)), ((9, 11, 14), (7, 12, 10)), ((1, 8, 9), (1, 8, 9))])
def test_gradient_expression_is_autograd_of_the_value(grid, isize):
    """the definition's gdf (B' along the axis, dscale) = torch autograd through the 64-tap sum, float64; clamped samples included"""
    B, C = 2, 2
    coef = CR.prefilter(unit_image(B, C, isize, 6))
    df = CR.smooth_field(B, grid, 7, 1.5)
    g = torch.randn(B, C, *grid, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    auto, expr = CR.gdf(df, coef, g), CR.gdf_analytic(df, coef, g)
    assert float((auto - expr).abs().max()) <= 1e-12 * float(expr.abs().max())
    if grid[0] == 1:
        assert bool((expr[:, 0] == 0).all())
    _, _, dscale = CR.coords(df, isize)
    assert float((dscale[:, 1:] == 0).double().mean()) > 0.01, "nothing clamped"


def test_half_voxel_round_trip_is_sharper_than_linear():
    """the image warped by a half-voxel shift and then by that shift's exact inverse, both in the sampler's own coordinates: the interior
    RMSE against the original is lower with the cubic interpolant than with the trilinear one (a condition; the figures are printed)"""
    img = round_trip_image()
    there, back = CR.shift_pair(ROUND_TRIP_SIZE)
    c, _, _ = CR.coords(there, ROUND_TRIP_SIZE)
    assert float((c[:, :, 4:-4, 4:-4, 4:-4] - c[:, :, 4:-4, 4:-4, 4:-4].floor() - 0.5).abs().max()) < 1e-9, "not a half-voxel shift"
    lin = AR.warp_field(back, AR.warp_field(there, img))
    cub = CR.warp(back, CR.warp(there, img))
    e_lin, e_cub = CR.interior_rmse(lin, img), CR.interior_rmse(cub, img)
    print(f"FIGURE half-voxel round trip, interior RMSE: linear {e_lin:.4f}, cubic {e_cub:.4f}")
    assert e_cub < e_lin


# ================================================================================================ the public surface
def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert protos["pulpo_bspline_prefilter"] == (I, [P, P, I, I, I, I, P])
    assert protos["pulpo_warp3d_cubic_fwd"] == (I, [P, P, P] + [I] * 8 + [P])
    assert protos["pulpo_warp3d_cubic_bwd"] == (I, [P, P, P, P] + [I] * 8 + [P])
    assert header_abi_version() == 8


def test_library_refuses_bad_arguments():
    """null pointers, zero extents, an in-place prefilter, a depth-1 grid on a 3-D image: the library's error code before any launch"""
    from pulpo_amd._lib import lib
    buf, buf2 = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    p, q = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(ctypes.addressof(buf2))
    f = lib.raw("pulpo_bspline_prefilter")
    assert f(None, q, 1, 2, 2, 2, None) != 0 and f(p, None, 1, 2, 2, 2, None) != 0 and f(p, p, 1, 2, 2, 2, None) != 0
    for bad in range(4):
        dims = [1, 2, 2, 2]
        dims[bad] = 0
        assert f(p, q, *dims, None) != 0, bad
    ok = (1, 1, 2, 2, 2, 2, 2, 2)
    for name, nptr in (("pulpo_warp3d_cubic_fwd", 3), ("pulpo_warp3d_cubic_bwd", 4)):
        f = lib.raw(name)
        for bad in range(nptr):
            args = [p] * nptr
            args[bad] = None
            assert f(*args, *ok, None) != 0, (name, bad)
        for bad in range(8):
            dims = list(ok)
            dims[bad] = 0
            assert f(*[p] * nptr, *dims, None) != 0, (name, bad)
        assert f(*[p] * nptr, 1, 1, 1, 2, 2, 2, 2, 2, None) != 0 and b"2-D" in lib.raw("pulpo_last_error")()


def test_cpu_tensors_and_wrong_arguments_are_refused():
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    img, df = torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)
    with pytest.raises(PulpoHipError):
        ops.bspline_prefilter(img)
    with pytest.raises(PulpoHipError):
        ops.warp3d_cubic(df, img)
    with pytest.raises(PulpoHipError):
        ops.warp3d_cubic(df, coef=img)
    with pytest.raises(PulpoHipError):
        ops.warp3d_cubic(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match="exactly one"):
        ops.warp3d_cubic(df)
    with pytest.raises(ValueError, match="exactly one"):
        ops.warp3d_cubic(df, img, coef=img)
    with pytest.raises(ValueError, match="data"):
        ops.warp3d_cubic(df, img.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="data"):
        ops.bspline_prefilter(img.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ops.warp3d_cubic(torch.zeros(1, 2, 4, 4, 4), img)                   # two components on a volume
    with pytest.raises(ValueError):
        ops.warp3d_cubic(torch.zeros(2, 3, 4, 4, 4), img)                   # another batch
    with pytest.raises(ValueError):
        ops.warp3d_cubic(df, torch.zeros(1, 1, 4, 4))                       # a volume field on a slice
    with pytest.raises(ValueError):
        ops.warp3d_cubic(torch.zeros(1, 3, 4, 1, 4), img)                   # a grid extent of 1 along H
    with pytest.raises(ValueError):
        ops.warp3d_cubic(torch.zeros(1, 3, 1, 4, 4), img)                   # a depth-1 grid on a 3-D image
    with pytest.raises(ValueError):
        ops.bspline_prefilter(torch.zeros(4, 4, 4))
    for bad in ("nearest", None, "Cubic"):
        with pytest.raises(ValueError, match="interpolation"):
            ops.check_interpolation(bad, "test")
    assert ops.check_interpolation("linear", "test") == "linear" and ops.check_interpolation("cubic", "test") == "cubic"


def test_surface_takes_interpolation_and_refuses_unknown_values():
    """a CPU model and CPU tensors: every entry has interpolation="linear" as its default; an unknown value raises ValueError before anything
    else; "cubic" reaches the operators, which refuse the CPU tensors"""
    import src.models as models
    from pulpo_amd import evaluation, refine
    from pulpo_amd._lib import PulpoHipError
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2).eval()
    for fn in (m.predict, m.predict_deterministic, m.predict_bidirectional, m.refine, refine.refine_interpolated, refine.Objective.__init__,
               evaluation.performance):
        assert inspect.signature(fn).parameters["interpolation"].default == "linear", fn
    assert "interpolation" not in inspect.signature(refine.refine).parameters          # (its argument list is pinned by tests/test_host_refine.py)
    with pytest.raises(TypeError):
        refine.refine_interpolated(m, torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 16), "cubic", no_such_argument=1)
    x = torch.zeros(1, 1, 16, 16, 16)
    for call in (lambda **kw: m.predict(x, x, **kw), lambda **kw: m.predict_deterministic(x, x, **kw),
                 lambda **kw: m.predict_bidirectional(x, x, **kw), lambda **kw: m.refine(x, x, **kw),
                 lambda **kw: evaluation.performance(m, x, x, **kw)):
        with pytest.raises(ValueError, match="interpolation"):
            call(interpolation="nearest")
        with pytest.raises(PulpoHipError):
            call(interpolation="cubic")
