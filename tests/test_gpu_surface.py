"""GPU tests of the boundary metrics: ops.edt_sq and ops.surface_distances against the definitions of
tests/surface_ref.py - integer results for equality, the metrics (evaluated in double on both sides, stored as fp32) to rtol 1e-6 - and the
HD95 / ASSD rows of evaluation.performance."""
import numpy as np
import pytest
import torch

import surface_ref as R
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FB = list(O.FEEDBACK_DEFAULT)
KEYS = ("hd", "hd_pct", "assd")


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    return ops


# ------------------------------------------------------------------------------------------------ 1. edt_sq
# The 70-long shapes put a line longer than one wave, and an x extent beyond one 64-wide tile, on each axis in turn; (5, 4, 65) crosses the
# x tile and the 64-voxel ballot word by one, (2, 3, 129) two words by one; 241 / 481 / 961 cross, by one, the line lengths at which the
# LDS tile narrows to 32, 16 and 8 voxels in x - along H and along D; their W = 33 / 17 / 9 twins cross the narrowed x tile by one (several x
# tiles and a partial last one at each tile width); 1024 is the longest line; (24, 20) and (3, 130) are 2-D.
EDT_SHAPES = [(16, 16, 16), (17, 23, 12), (9, 3, 70), (3, 70, 9), (70, 3, 9), (5, 4, 65), (2, 3, 129), (2, 241, 9), (241, 2, 9), (2, 481, 5),
              (481, 2, 5), (961, 1, 3), (1, 961, 3), (2, 241, 33), (241, 2, 33), (2, 481, 17), (481, 2, 17), (1, 961, 9), (961, 1, 9),
              (1024, 2), (2, 1024), (24, 20), (3, 130)]


def check_edt(ops, mask):
    got = ops.edt_sq(mask.cuda())
    want = R.edt_sq(mask.cuda())
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(mask.shape)
    assert torch.equal(got, want)
    return got


@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_random_masks(api, shape):
    gen = torch.Generator().manual_seed(sum(shape))
    for density in (0.5, 0.01):
        mask = torch.rand((2, 1) + shape, generator=gen) < density
        if not bool(mask[1].any()):
            mask[1].view(-1)[int(torch.randint(0, mask[1].numel(), (1,), generator=gen))] = True
        got = check_edt(api, mask)
        assert torch.equal(api.edt_sq(mask.to(torch.uint8).cuda()), got)                 # bool and uint8 inputs
        assert torch.equal(api.edt_sq((mask.to(torch.uint8) * 7).cuda()), got)           # non-zero = set


@pytest.mark.parametrize("shape", [(16, 16, 16), (17, 23, 12), (9, 3, 70), (70, 3, 9), (24, 20), (3, 130)], ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_special_masks(api, shape):
    nd = len(shape)
    corner = torch.zeros((2, 1) + shape, dtype=torch.bool)
    corner[(0, 0) + (0,) * nd] = True                                # item 0: the first corner; item 1: the last
    corner[(1, 0) + tuple(s - 1 for s in shape)] = True
    got = check_edt(api, corner)
    assert int(got[0].max()) == sum((s - 1) ** 2 for s in shape) and int(got[1].reshape(-1)[0]) == sum((s - 1) ** 2 for s in shape)
    full = torch.ones((1, 1) + shape, dtype=torch.bool)
    assert not bool(api.edt_sq(full.cuda()).any())
    empty = torch.zeros((1, 1) + shape, dtype=torch.uint8)
    assert bool((api.edt_sq(empty.cuda()) == api.EDT_INF).all())
    mixed = torch.zeros((2, 1) + shape, dtype=torch.bool)            # an empty item next to a non-empty one
    mixed[(1, 0) + tuple(s // 2 for s in shape)] = True
    got = check_edt(api, mixed)
    assert bool((got[0] == api.EDT_INF).all()) and int(got[1].max()) < api.EDT_INF


def test_edt_sq_refuses_bad_inputs(api):
    from pulpo_amd._lib import PulpoHipError
    for bad in (torch.zeros(1, 1, 4, 4, 4).cuda(), torch.zeros(1, 2, 4, 4, 4, dtype=torch.bool).cuda(), torch.zeros(1, 1, 2, 1025, dtype=torch.bool).cuda(),
                torch.zeros(1, 1, 4, 4, 4, dtype=torch.bool)):
        with pytest.raises(PulpoHipError):
            api.edt_sq(bad)


# ------------------------------------------------------------------------------------------------ 2. surface_distances against the reference
_PAIRS = {}


def label_pair(shape, C):
    """Voronoi label maps (B = 2: the map and its rolled copy swapped in the second item, so that the two directions differ per item) and the
    reference's results at q = 95, 50, 100, computed once per (shape, C) on the device"""
    key = (shape, C)
    if key not in _PAIRS:
        a1 = R.voronoi_labels(shape, C, 1)
        b1 = R.rolled(a1)
        a2 = R.voronoi_labels(shape, C, 2)
        a, b = torch.cat([a1, R.rolled(a2)]), torch.cat([b1, a2])
        ref = {q: R.surface_distances(a.cuda(), b.cuda(), C, q) for q in (95.0, 50.0, 100.0)}
        _PAIRS[key] = (a, b, ref)
    return _PAIRS[key]


def check_against(res, ref, with_hist=True):
    assert res["n_a"].dtype == torch.int32 and res["n_b"].dtype == torch.int32
    assert np.array_equal(res["n_a"].cpu().numpy(), ref["n_a"]) and np.array_equal(res["n_b"].cpu().numpy(), ref["n_b"])
    if with_hist:
        assert res["hist"].dtype == torch.int32 and np.array_equal(res["hist"].cpu().numpy().astype(np.int64), ref["hist"])
    for k in KEYS:
        got = res[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref[k].shape and res[k].dtype == torch.float32
        assert np.array_equal(np.isnan(got), np.isnan(ref[k])), k
        ok = ~np.isnan(got)
        np.testing.assert_allclose(got[ok], ref[k][ok], rtol=1e-6, atol=0.0, err_msg=k)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("C", [2, 5, 36])
@pytest.mark.parametrize("shape", [(17, 23, 12), (24, 20)], ids=["3d", "2d"])
def test_surface_distances_against_reference(api, shape, C, dtype):
    run_against_reference(api, shape, C, dtype)


# W = 70: two ballot words in the row pass on labels and two x tiles in the histogram pass; (241, 2, 33): the histogram pass (lines along D)
# on 32-wide tiles, two of them, the last partial; (3, 241, 33): the same for the pass along H in front of it; (3, 130): two words in 2-D
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("shape", [(9, 3, 70), (241, 2, 33), (3, 241, 33), (3, 130)], ids=lambda s: "x".join(map(str, s)))
def test_surface_distances_across_tile_edges(api, shape, dtype):
    run_against_reference(api, shape, 5, dtype)


def test_surface_distances_mixed_dtypes(api):
    """a uint8 map against an int32 one: the same results, and an int32 label above 255 is not wrapped into range"""
    a, b, ref = label_pair((17, 23, 12), 5)
    check_against(api.surface_distances(a.to(torch.uint8).cuda(), b.to(torch.int32).cuda(), 5, return_hist=True), ref[95.0])
    bad = b.to(torch.int32).cuda()
    bad[0, 0, 3, 4, 5] = 256 + int(bad[0, 0, 3, 4, 5])
    with pytest.raises(IndexError):
        api.surface_distances(a.to(torch.uint8).cuda(), bad, 5)
    with pytest.raises(IndexError):
        api.surface_distances(bad, a.to(torch.uint8).cuda(), 5)


def run_against_reference(api, shape, C, dtype):
    a, b, ref = label_pair(shape, C)
    assert int((ref[95.0]["n_a"] > 0).sum()) == 2 * C and int((ref[95.0]["n_b"] > 0).sum()) == 2 * C    # every class in both maps
    la, lb = a.to(dtype).cuda(), b.to(dtype).cuda()
    for q in (95.0, 50.0, 100.0):
        res = api.surface_distances(la, lb, C, percentile=q, return_hist=True)
        assert set(res) == {"hd", "hd_pct", "assd", "n_a", "n_b", "hist"}
        check_against(res, ref[q])
    plain = api.surface_distances(la, lb, C)
    assert set(plain) == {"hd", "hd_pct", "assd", "n_a", "n_b"}
    check_against(plain, ref[95.0], with_hist=False)
    # percentile = 100 is the Hausdorff distance
    r100 = api.surface_distances(la, lb, C, percentile=100.0)
    assert torch.equal(r100["hd_pct"].nan_to_num(-1.0), r100["hd"].nan_to_num(-1.0))


def test_surface_distances_absent_classes_and_chunks(api):
    """C = 11 at 17 x 23 x 12 with classes 3 and 7 removed from one map each and class 10 from both: NaN exactly there, the counts exact;
    eleven classes also end on a short last chunk of classes"""
    C = 11
    a = R.voronoi_labels((17, 23, 12), C, 4)
    b = R.rolled(a)
    a[a == 3] = 0
    b[b == 7] = 1
    a[a == 10] = 2
    b[b == 10] = 2
    ref = R.surface_distances(a.cuda(), b.cuda(), C)
    for c, (na, nb) in ((3, (False, True)), (7, (True, False)), (10, (False, False))):
        assert (ref["n_a"][0, c] > 0, ref["n_b"][0, c] > 0) == (na, nb) and np.isnan(ref["hd"][0, c])
    res = api.surface_distances(a.to(torch.uint8).cuda(), b.to(torch.uint8).cuda(), C, return_hist=True)
    check_against(res, ref)
    assert bool(torch.isnan(res["hd"][0, [3, 7, 10]]).all()) and int(torch.isnan(res["hd"]).sum()) == 3


def test_surface_distances_analytic(api):
    a = torch.zeros(1, 1, 16, 16, 16, dtype=torch.uint8)
    b = a.clone()
    a[..., 4:10, 4:10, 4:10] = 1
    b[..., 4:10, 4:10, 6:12] = 1
    same = api.surface_distances(a.cuda(), a.cuda(), 2, return_hist=True)
    for k in KEYS:
        assert bool((same[k] == 0).all()), k
    assert torch.equal(same["n_a"], same["n_b"]) and int(same["n_a"][0, 1]) == 6 ** 3 - 4 ** 3
    assert int(same["hist"][0, 1, 0, 0]) == 6 ** 3 - 4 ** 3 and int(same["hist"][0, 1].sum()) == 2 * (6 ** 3 - 4 ** 3)
    res = api.surface_distances(a.cuda(), b.cuda(), 3)
    assert float(res["hd"][0, 1]) == 2.0 and float(res["hd_pct"][0, 1]) <= 2.0 and 0.0 < float(res["assd"][0, 1]) < 2.0
    assert bool(torch.isnan(res["hd"][0, 2])) and int(res["n_a"][0, 2]) == 0 and int(res["n_b"][0, 2]) == 0
    only_a = a.clone()
    only_a[0, 0, 0, 0, 0] = 2                                               # class 2 in one map only
    res = api.surface_distances(only_a.cuda(), b.cuda(), 3)
    assert all(bool(torch.isnan(res[k][0, 2])) for k in KEYS) and (int(res["n_a"][0, 2]), int(res["n_b"][0, 2])) == (1, 0)
    assert float(res["hd"][0, 1]) == 2.0


def test_surface_distances_bitwise_repeatable_and_checked(api):
    from pulpo_amd._lib import PulpoHipError
    a, b, _ = label_pair((17, 23, 12), 5)
    la, lb = a.to(torch.uint8).cuda(), b.to(torch.uint8).cuda()
    r1 = api.surface_distances(la, lb, 5, return_hist=True)
    r2 = api.surface_distances(la, lb, 5, return_hist=True)
    for k in r1:
        assert torch.equal(r1[k].view(torch.int32) if r1[k].is_floating_point() else r1[k], r2[k].view(torch.int32) if r2[k].is_floating_point() else r2[k]), k
    for dtype in (torch.uint8, torch.int32):
        bad = la.to(dtype).clone()
        bad[1, 0, 16, 22, 11] = 5
        with pytest.raises(IndexError):
            api.surface_distances(bad, lb.to(dtype), 5)
        with pytest.raises(IndexError):
            api.surface_distances(lb.to(dtype), bad, 5)
    with pytest.raises(PulpoHipError):
        api.surface_distances(la, lb[:, :, :16], 5)                        # shape mismatch
    with pytest.raises(PulpoHipError):
        api.surface_distances(la.cpu(), lb, 5)
    with pytest.raises(PulpoHipError):
        api.surface_distances(la.long(), lb.long(), 5)


# ------------------------------------------------------------------------------------------------ 3. the HD95 / ASSD rows of performance
def small_model(golden, res="level_res"):
    import src.models as models
    import src.network_blocks as nb
    g = golden("step_T3L2_n4_16")
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    torch.manual_seed(0)                                                    # for parameters the fixture does not carry in this shape
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0, df_resolution=res)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("sd0.") and k[4:] in sd and tuple(sd[k[4:]].shape) == tuple(v.shape):
            sd[k[4:]] = T(v.copy())
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(T(g[f"eps.{l}"])[:1].cuda())          # the latents keep their level sizes
    return model, g, L, size


def row_mean(ref, key, first):
    v = ref[key][:, first:]
    return float(np.nanmean(v)) if np.isfinite(v).any() else 0.0


def test_performance_surface_rows(api, golden):
    from pulpo_amd.evaluation import SURFACE_METRICS, PerformanceTable, performance
    model, g, L, size = small_model(golden)
    C = 5
    x, y = T(g["x"])[:1].cuda(), T(g["y"])[:1].cuda()
    seg_x = R.voronoi_labels(size, C, 1).to(torch.uint8).cuda()
    seg_y = R.rolled(R.voronoi_labels(size, C, 1)).to(torch.uint8).cuda()
    base = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C)
    res = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C, surface=True)
    assert set(res) == set(base) | set(SURFACE_METRICS)
    for m in base:                                                          # every earlier row: the same bits
        for l in range(L):
            assert torch.equal(base[m][l], res[m][l]), (m, l)
    with torch.no_grad():
        outputs, ind = model.predict_deterministic(x, y)
        _, final = model.combine_dfs(ind)
    warped = api.warp_labels(final[0], seg_x, C, argmax=True)
    ref = R.surface_distances(warped, seg_y, C)
    assert np.isfinite(ref["hd_pct"][:, 1:]).all() and row_mean(ref, "hd_pct", 1) > 0.0
    bg = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C, surface=True, include_background=True)
    for name, key in (("HD95", "hd_pct"), ("ASSD", "assd")):
        assert res[name][0].is_cuda and res[name][0].dim() == 0
        np.testing.assert_allclose(float(res[name][0]), row_mean(ref, key, 1), rtol=1e-6)
        np.testing.assert_allclose(float(bg[name][0]), row_mean(ref, key, 0), rtol=1e-6)
        assert row_mean(ref, key, 0) != row_mean(ref, key, 1)
        assert all(float(res[name][l]) == 0.0 for l in range(1, L))         # level_res: the coarser fields are not on seg_y's grid
    table = PerformanceTable(list(base) + list(SURFACE_METRICS), L, ["val"], 1)
    table.add(0, 0, res)
    data, (sets, mets) = table.mean()
    col = list(mets).index("HD95")
    np.testing.assert_allclose(data[0, col], float(res["HD95"][0]), rtol=1e-7)
    assert np.isnan(data[1, col])
    with pytest.raises(ValueError, match="surface"):
        performance(model, x, y, surface=True)


def test_performance_surface_rows_full_res(api, golden):
    from pulpo_amd.evaluation import performance
    model, g, L, size = small_model(golden, "full_res")
    C = 5
    x, y = T(g["x"])[:1].cuda(), T(g["y"])[:1].cuda()
    seg_x = R.voronoi_labels(size, C, 1).to(torch.uint8).cuda()
    seg_y = R.rolled(R.voronoi_labels(size, C, 1)).to(torch.uint8).cuda()
    res = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C, surface=True)
    with torch.no_grad():
        outputs, ind = model.predict_deterministic(x, y)
        _, final = model.combine_dfs(ind)
    for l in range(L):
        assert tuple(final[l].shape[2:]) == tuple(size)
        ref = R.surface_distances(api.warp_labels(final[l], seg_x, C, argmax=True), seg_y, C)
        for name, key in (("HD95", "hd_pct"), ("ASSD", "assd")):
            np.testing.assert_allclose(float(res[name][l]), row_mean(ref, key, 1), rtol=1e-6)
            assert float(res[name][l]) > 0.0


def test_level_scores_moving_segmentation_on_another_grid(api):
    """seg_x at twice the resolution of the field and of seg_y: warp_labels brings it onto the field's grid, and the rows are computed"""
    from pulpo_amd.evaluation import level_scores
    gen = torch.Generator().manual_seed(9)
    C, S = 5, 16
    y = torch.rand(1, 1, S, S, S, generator=gen).cuda()
    outputs = {0: torch.rand(1, 1, S, S, S, generator=gen).cuda()}
    final = {0: (1.5 * torch.randn(1, 3, S, S, S, generator=gen)).cuda()}
    seg_y = R.voronoi_labels((S, S, S), C, 1).to(torch.uint8).cuda()
    seg_x = R.voronoi_labels((2 * S, 2 * S, 2 * S), C, 3).to(torch.uint8).cuda()
    res = level_scores(outputs, final, y, seg_x=seg_x, seg_y=seg_y, num_classes=C, surface=True)
    ref = R.surface_distances(api.warp_labels(final[0], seg_x, C, argmax=True), seg_y, C)
    for name, key in (("HD95", "hd_pct"), ("ASSD", "assd")):
        assert row_mean(ref, key, 1) > 0.0
        np.testing.assert_allclose(float(res[name][0]), row_mean(ref, key, 1), rtol=1e-6)
