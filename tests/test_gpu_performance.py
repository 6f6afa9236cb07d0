"""GPU tests of the deterministic evaluation harness (pulpo_amd.evaluation = Evaluate.performance, evaluate.py:1379-1498) and its two
kernels: pulpo_field_quality (mean / std / % <= 0 of the Jacobian determinant in one pass, no determinant map) and
pulpo_warp_labels_soft_dice (the level Dice without a one-hot tensor), against fp64 on the CPU oracle, against the composed routes they
replace on the device and against the golden made from the reference's own classes (tests/golden/make_golden_performance.py)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from metrics_ref import jacobian_det_2d
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FB = list(O.FEEDBACK_DEFAULT)
METRICS = ["RMSE", "JDetStd", "JDetLeq0", "Dice", "LM_MAE", "LM_Euclid"]


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb


def one_hot(lab, C):
    """(B, 1, ...) labels -> (B, C, ...) fp32 one-hot"""
    oh = F.one_hot(lab[:, 0].long(), C)
    return oh.permute(0, oh.dim() - 1, *range(1, oh.dim() - 1)).float().contiguous()


def build_from_golden(models, nb, g, key="sd0."):
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith(key):
            sd[k[len(key):]] = T(v.copy())
    model.load_state_dict(sd, strict=True)
    return model.cuda(), (Tl, L, n0, B, size)


def pin_noise(model, nb, g, L):
    """predict_deterministic decodes mu, but the feedback to the level above carries `samples` (pulpo.py:202), a draw of the level's
    sampler: pin it to the fixture's noise (first batch row), as the golden generator does"""
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(T(g[f"eps.{l}"])[:1].cuda())


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ------------------------------------------------------------------------------------------------ 1. field_quality
def folded_field(B, grid, amplitude=3.0):
    """a coarse random field interpolated up: smooth, and large enough to fold"""
    nd = len(grid)
    c = (torch.rand(B, nd, *[max(2, s // 3) for s in grid], generator=torch.Generator().manual_seed(5)) * 2 - 1) * amplitude
    return F.interpolate(c, size=grid, mode="trilinear" if nd == 3 else "bilinear", align_corners=False)


# (batch, grid, amplitude of the recipe).  Amplitude 3 meets both guards below in fp64 at every shape, normalised or not (checked on the
# CPU: 3.9 - 9.1 % of the voxels fold when normalised, 33 % at (2, 5, 7), 40 - 52 % unnormalised; no |J| <= 1e-5 anywhere).
# (2, 5, 7): both neighbours clamped along an axis; (40, 36, 44): many blocks, ragged rows; (24, 20): the 2-D form.
FIELD_SHAPES = [(2, (12, 10, 14), 3.0), (2, (9, 11, 13), 3.0), (2, (16, 16, 16), 3.0), (1, (2, 5, 7), 3.0), (1, (40, 36, 44), 3.0),
                (2, (24, 20), 3.0)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,grid,amplitude", FIELD_SHAPES)
def test_field_quality_against_fp64(api, B, grid, amplitude, normalize):
    """mean / std within max(4 x the fp32 CPU oracle's own deviation from fp64, 1e-6) relative; the J <= 0 count equal to the fp64 count up
    to the voxels with |J64| <= 1e-5; the std of the existing jdet_std kernel; bit-identical from call to call.
    Observed on the MI355X, relative deviation from fp64 over the 12 cases: mean 6.6e-9 ... 8.7e-8, and 2.4e-7 at (16, 16, 16) unnormalised,
    where the mean (0.30) is small beside the std (44) and the oracle's own deviation sets the bound at 3.5e-6; std 3.5e-9 ... 8.2e-8; the
    count equal to the fp64 count in every case (the test prints the figures: pytest -s)."""
    from pulpo_amd import eval_metrics, ops
    df = folded_field(B, grid, amplitude)
    jac = O.jacobian_det if len(grid) == 3 else jacobian_det_2d
    j64, j32 = jac(df.double(), normalize), jac(df, normalize)
    n = j64.numel()
    near = int((j64.abs() <= 1e-5).sum())
    count64 = int((j64 <= 0).sum())
    assert count64 > 0.01 * n, "the field does not fold: the count comparison would be vacuous"
    assert near <= 0.001 * n
    mean, std, pct = ops.field_quality(df.cuda(), normalize)
    assert mean.dim() == 0 and std.dim() == 0 and pct.dim() == 0 and mean.dtype == torch.float32
    count = round(float(pct) * n / 100.0)
    assert abs(float(pct) * n / 100.0 - count) < 0.01
    assert abs(count - count64) <= near, (count, count64, near)
    tol_mean = max(4.0 * rel(j32.mean(), j64.mean()), 1e-6)
    tol_std = max(4.0 * rel(j32.std(), j64.std()), 1e-6)
    print(f"field_quality {B} {grid} normalize={normalize}: mean dev {rel(mean, j64.mean()):.2e} (tol {tol_mean:.2e}), "
          f"std dev {rel(std, j64.std()):.2e} (tol {tol_std:.2e}), count {count} / fp64 {count64}")
    assert rel(mean, j64.mean()) <= tol_mean
    assert rel(std, j64.std()) <= tol_std
    # the existing kernels, which do not move: same determinant (so the same count, exactly), same std
    d = df.cuda()
    np.testing.assert_allclose(float(std), float(ops.jdet_std(d, 1.0, normalize)), rtol=1e-5)
    jd = ops.jacobian_det(d, normalize)
    assert count == int((jd <= 0).sum())
    np.testing.assert_allclose(float(pct), float(ops.percent_leq0(jd)), rtol=1e-6)
    again = ops.field_quality(d, normalize)
    assert all(torch.equal(a, b) for a, b in zip((mean, std, pct), again))
    if normalize:
        assert all(torch.equal(a, b) for a, b in zip((mean, std, pct), eval_metrics.field_quality(d)))


# ------------------------------------------------------------------------------------------------ 2. soft Dice across grids
def warp_cpu(df, img):
    """SpatialTransformer.forward (network_blocks.py:101-121) on the CPU in the dtype of df; 3-D: the oracle's, 2-D: the same recipe"""
    if df.dim() == 5:
        return O.warp(df, img)
    size = df.shape[2:]
    axes = [torch.arange(s, dtype=df.dtype) for s in size]
    loc = torch.stack(torch.meshgrid(*axes, indexing="ij")).unsqueeze(0) + df
    comps = [2 * (loc[:, i] / (size[i] - 1) - 0.5) for i in range(2)]
    return F.grid_sample(img, torch.stack(comps[::-1], dim=-1), mode="bilinear", padding_mode="border", align_corners=False)


def soft_dice_cpu(df, lab_x, lab_y, C, dtype):
    """the level Dice of evaluate.py:1427, 1454-1455 per (b, c), sum form (src/losses.py:137-145), in `dtype` on the CPU"""
    grid = tuple(df.shape[2:])
    p = warp_cpu(df.to(dtype), one_hot(lab_x, C).to(dtype))
    t = one_hot(lab_y, C).to(dtype)
    t = F.interpolate(t, size=grid, mode="trilinear" if len(grid) == 3 else "bilinear", align_corners=False)     # the identity at equal size
    dims = list(range(2, p.dim()))
    return ((2.0 * t * p).sum(dim=dims) + 1e-6) / ((t ** 2).sum(dim=dims) + (p ** 2).sum(dim=dims) + 1e-6)


# (batch, field grid, label-map size): identity resize; ragged; 2x2x2 centre taps; 4x; batch; non-integer ratio (general taps); 2-D
DICE_SHAPES = [(1, (16, 16, 16), (16, 16, 16)), (1, (17, 23, 12), (17, 23, 12)), (1, (8, 8, 8), (16, 16, 16)), (1, (4, 4, 4), (16, 16, 16)),
               (2, (8, 8, 8), (16, 16, 16)), (1, (6, 10, 7), (16, 16, 16)), (1, (12, 10), (24, 20))]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("C", [2, 5, 36])
def test_soft_dice_across_grids(api, C, dtype):
    """Per class and in the mean within tol = max(4 x the fp32 CPU oracle's deviation from fp64, 1e-6) relative.  The oracle's deviation is
    taken in the maximum norm over (b, c): a class met by a handful of voxels has a deviation of its own that is small or large by chance
    in either implementation, and the mean's error is bounded by the largest per-class error.  Classes absent from both maps give exactly
    1e-6 / 1e-6 = 1.  Equal to the composed route on the device (warp3d on the one-hot map, resized one-hot target, Soft_dice_loss) to
    rtol 1e-5; bit-identical from call to call.  Observed on the MI355X: at C = 2 and 5 per class 1.7e-8 ... 1.5e-7 and in the mean
    1.4e-9 ... 8.6e-8 (bound 1e-6); at C = 36, where a class has a handful of voxels, per class 4.5e-7 ... 2.6e-5 against bounds of
    1.9e-6 ... 1.0e-4 (a quarter of the bound: the same near-empty class carries the fp32 oracle's deviation and the kernel's) and in the
    mean 7.4e-9 ... 4.8e-8 (the test prints the figures: pytest -s)."""
    from pulpo_amd import losses, ops
    gen = torch.Generator().manual_seed(40 + C)
    hi = C if C == 2 else C - 2                              # the two highest classes are absent from both maps
    for B, grid, img in DICE_SHAPES:
        nd = len(grid)
        lab_x = torch.randint(0, hi, (B, 1) + img, generator=gen).to(dtype)
        lab_y = torch.randint(0, hi, (B, 1) + img, generator=gen).to(dtype)
        df = 1.5 * torch.randn(B, nd, *grid, generator=gen)             # leaves the volume in places (border clamp)
        d64, d32 = soft_dice_cpu(df, lab_x, lab_y, C, torch.float64), soft_dice_cpu(df, lab_x, lab_y, C, torch.float32)
        tol = max(4.0 * float(((d32.double() - d64).abs() / d64).max()), 1e-6)
        dice, mean = ops.warp_labels_soft_dice(df.cuda(), lab_x.cuda(), C, lab_y.cuda())
        assert tuple(dice.shape) == (B, C) and mean.dim() == 0 and dice.dtype == torch.float32
        dev = float(((dice.cpu().double() - d64).abs() / d64).max())
        dev_mean = rel(mean, d64.mean())
        print(f"soft dice C={C} {dtype} {grid} on {img}: per-class dev {dev:.2e}, mean dev {dev_mean:.2e} (tol {tol:.2e})")
        assert dev <= tol, (grid, img, dev, tol)
        assert dev_mean <= tol, (grid, img, dev_mean, tol)
        if C > 2:
            assert bool((dice[:, hi:] == 1.0).all())
        # the composed route this replaces
        ohx, ohy = one_hot(lab_x, C).cuda(), one_hot(lab_y, C).cuda()
        hier = losses.HierarchicalReconstructionLoss(["dice"], {0: 1.0}, False, nd, {0: 1.0})
        img_y = torch.zeros((B, 1) + img, device="cuda")
        _, level = hier({0: torch.zeros((B, 1) + grid, device="cuda")}, img_y, y_hat_seg={0: ops.warp3d(df.cuda(), ohx)}, seg_y=ohy, gamma=1, dice_factor=1)
        composed = 1.0 - float(level[0]) / float(np.prod(grid))
        np.testing.assert_allclose(float(mean), composed, rtol=1e-5)
        d2, m2 = ops.warp_labels_soft_dice(df.cuda(), lab_x.cuda(), C, lab_y.cuda())
        assert torch.equal(dice, d2) and torch.equal(mean, m2)


def test_soft_dice_label_out_of_range(api):
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    gen = torch.Generator().manual_seed(1)
    C = 5
    df = torch.randn(1, 3, 8, 8, 8, generator=gen).cuda()
    for dtype in (torch.uint8, torch.int32):
        lab = torch.randint(0, C, (1, 1, 16, 16, 16), generator=gen).to(dtype).cuda()
        bad = lab.clone()
        bad[0, 0, 15, 15, 15] = C
        with pytest.raises(IndexError):
            ops.warp_labels_soft_dice(df, bad, C, lab)
        with pytest.raises(IndexError):
            ops.warp_labels_soft_dice(df, lab, C, bad)
        with pytest.raises(PulpoHipError):
            ops.warp_labels_soft_dice(df, lab.cpu(), C, lab)


# ------------------------------------------------------------------------------------------------ 3. no one-hot memory
def test_level_scores_allocate_no_one_hot_map(api):
    from pulpo_amd.evaluation import level_scores
    S, C = 48, 36
    gen = torch.Generator().manual_seed(3)
    y = torch.rand(1, 1, S, S, S, generator=gen).cuda()
    outputs = {0: torch.rand(1, 1, S, S, S, generator=gen).cuda()}
    final = {0: (1.5 * torch.randn(1, 3, S, S, S, generator=gen)).cuda()}
    seg_x = torch.randint(0, C, (1, 1, S, S, S), generator=gen).to(torch.uint8).cuda()
    seg_y = torch.randint(0, C, (1, 1, S, S, S), generator=gen).to(torch.uint8).cuda()
    level_scores(outputs, final, y, seg_x=seg_x, seg_y=seg_y, num_classes=C)          # first-call workspaces
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = level_scores(outputs, final, y, seg_x=seg_x, seg_y=seg_y, num_classes=C)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert 0.0 < float(res["Dice"][0]) < 1.0
    assert grown < C * S ** 3 * 4, grown                     # one fp32 one-hot map; the composed route holds three


# ------------------------------------------------------------------------------------------------ 4. against the reference golden
def check_scores(res, g, case, L):
    assert set(res) == set(METRICS)
    for l in range(L):
        for m in ("RMSE", "JDetStd", "Dice"):
            np.testing.assert_allclose(float(res[m][l]), g[f"{case}.{m}"][l], rtol=1e-4, err_msg=f"{m} level {l}")
        jd = g[f"{case}.jdet.{l}"]
        near = float((np.abs(jd) <= 1e-5).sum()) * 100.0 / jd.size          # a determinant within rounding of 0 may fall on either side
        assert abs(float(res["JDetLeq0"][l]) - g[f"{case}.JDetLeq0"][l]) <= near + 1e-4, l
        for m in ("LM_MAE", "LM_Euclid"):
            if g[f"{case}.{m}"][l] == 0:
                assert float(res[m][l]) == 0.0
            else:
                np.testing.assert_allclose(float(res[m][l]), g[f"{case}.{m}"][l], rtol=1e-5, err_msg=f"{m} level {l}")
    for d in res.values():
        assert all(v.is_cuda and v.dim() == 0 for v in d.values())


def test_level_scores_match_reference_on_folded_fields(api, golden):
    from pulpo_amd.evaluation import level_scores
    g = golden("performance_T3L2_n4_16")
    C = int(g["cfg"][3])
    outputs = {l: T(g[f"b.outputs.{l}"]).cuda() for l in (0, 1)}
    final = {l: T(g[f"b.final_dfs.{l}"]).cuda() for l in (0, 1)}
    y = T(g["b.y"]).cuda()
    seg_x, seg_y, lm_x, lm_y = (T(g[k]).cuda() for k in ("seg_x", "seg_y", "lm_x", "lm_y"))
    assert float(g["b.JDetLeq0"].min()) > 1.0                                # folding occurs at both levels
    res = level_scores(outputs, final, y, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=C)
    check_scores(res, g, "b", 2)
    # the reference's float one-hot maps, int64 label maps: the same bits
    oh = level_scores(outputs, final, y, seg_x=one_hot(seg_x, C), seg_y=one_hot(seg_y, C), lm_x=lm_x, lm_y=lm_y)
    i64 = level_scores(outputs, final, y, seg_x=seg_x.long(), seg_y=seg_y.long(), num_classes=C)
    for l in (0, 1):
        assert torch.equal(oh["Dice"][l], res["Dice"][l]) and torch.equal(i64["Dice"][l], res["Dice"][l])
    plain = level_scores(outputs, final, y)
    assert set(plain) == {"RMSE", "JDetStd", "JDetLeq0"}
    for m in plain:
        for l in (0, 1):
            assert torch.equal(plain[m][l], res[m][l])
    assert set(i64) == {"RMSE", "JDetStd", "JDetLeq0", "Dice"}
    empty = level_scores(outputs, final, y, lm_x=torch.zeros(1, 0, 3), lm_y=torch.zeros(1, 0, 3))
    assert float(empty["LM_MAE"][0]) == 0.0 and float(empty["LM_Euclid"][0]) == 0.0 and float(empty["LM_MAE"][1]) == 0.0


def test_performance_matches_reference_model(api, golden):
    models, nb = api
    from pulpo_amd.evaluation import performance
    g, gs = golden("performance_T3L2_n4_16"), golden("step_T3L2_n4_16")
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, gs)
    model.eval()
    pin_noise(model, nb, gs, L)
    C = int(g["cfg"][3])
    x, y = T(gs["x"])[:1].cuda(), T(gs["y"])[:1].cuda()
    seg_x, seg_y, lm_x, lm_y = (T(g[k]).cuda() for k in ("seg_x", "seg_y", "lm_x", "lm_y"))
    res = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=C)
    check_scores(res, g, "a", L)
    assert set(performance(model, x, y)) == {"RMSE", "JDetStd", "JDetLeq0"}


def test_performance_2d_matches_composed_route(api, golden):
    """a 2-D model (train.py --ndims 2) through performance() with segmentations and landmarks, against the loose parts on the device"""
    models, nb = api
    from pulpo_amd import eval_metrics, losses, ops
    from pulpo_amd.evaluation import performance
    g = golden("step2d_T3L2_n4_32x24")
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, g)
    assert len(size) == 2 and model.ndims == 2
    model.eval()
    pin_noise(model, nb, g, L)
    C = 5
    gen = torch.Generator().manual_seed(8)
    x, y = T(g["x"])[:1].cuda(), T(g["y"])[:1].cuda()
    seg_x = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    seg_y = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    lm_x = torch.stack([torch.randint(0, s, (6,), generator=gen) for s in size], dim=-1)[None].float().cuda()
    lm_y = (lm_x + torch.randn(lm_x.shape, generator=gen).cuda()).clamp(0, min(size) - 1)
    res = performance(model, x, y, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=C)
    assert set(res) == set(METRICS)
    with torch.no_grad():
        outputs, ind = model.predict_deterministic(x, y)
        _, final = model.combine_dfs(ind)
        ones = lambda: {l: 1.0 for l in range(L)}
        ohx, ohy = one_hot(seg_x, C), one_hot(seg_y, C)
        pred = {l: model.autoencoder.decoders[l].spatial_transform(final[l], ohx) for l in range(L)}
        _, mse = losses.HierarchicalReconstructionLoss(["mse"], ones(), False, 2, ones())(outputs, y, pred, ohy, gamma=1, dice_factor=1)
        _, jstd = losses.HierarchicalRegularization(losses.JDetStd, ones(), False)(final, lamb=1)
        _, dice = losses.HierarchicalReconstructionLoss(["dice"], ones(), False, 2, ones())(outputs, y, pred, ohy, gamma=1, dice_factor=1)
        for l in range(L):
            npix = float(np.prod(outputs[l].shape[2:]))
            np.testing.assert_allclose(float(res["RMSE"][l]), float(torch.sqrt(mse[l] / npix)), rtol=1e-5)
            # JDetStd: the composed route is the existing determinant map (the same bits field_quality sees) and its std, taken in double.
            # HierarchicalRegularization(JDetStd), the training loss, is not the yardstick on these near-identity fields (|J - 1| ~ 1e-2):
            # its kernel sums J and J^2 uncentred in fp32 and its std came out 3.6e-4 (level 0) off here, beyond the 1e-5 asked; the
            # fp64 determinant of the same field on the CPU says which of the two is right.
            jd = eval_metrics.jdet(final[l])
            np.testing.assert_allclose(float(res["JDetStd"][l]), float(jd.double().std()), rtol=1e-5)
            std64 = float(jacobian_det_2d(final[l].cpu().double()).std())
            print(f"2-D level {l}: JDetStd {float(res['JDetStd'][l]):.8f}, fp64 {std64:.8f}, jdet_std loss kernel {float(jstd[l]):.8f}")
            assert rel(res["JDetStd"][l], std64) <= 1e-6
            assert rel(jstd[l], std64) <= 1e-2
            np.testing.assert_allclose(float(res["JDetLeq0"][l]), float(eval_metrics.jdet_leq0_percent(final[l])), rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(float(res["Dice"][l]), 1.0 - float(dice[l]) / npix, rtol=1e-5)
        moved = ops.warp_landmarks(lm_x, final[0])
        np.testing.assert_allclose(float(res["LM_MAE"][0]), float(torch.median(torch.abs(moved - lm_y).sum(dim=2))), rtol=1e-5)
        np.testing.assert_allclose(float(res["LM_Euclid"][0]), float(torch.mean(torch.sqrt(((moved - lm_y) ** 2).sum(dim=2)))), rtol=1e-5)
        assert all(float(res[m][l]) == 0.0 for m in ("LM_MAE", "LM_Euclid") for l in range(1, L))


# ------------------------------------------------------------------------------------------------ 5. table and baseline
def test_performance_table_on_device_scalars(api):
    from pulpo_amd.evaluation import PerformanceTable
    names = ["RMSE", "LM_MAE"]
    table = PerformanceTable(names, 2, ["long", "short"], 3)
    vals = np.zeros((2, 2, 2, 3))
    rng = np.random.default_rng(0)
    for k, n_in in enumerate((3, 2)):                           # loaders of unequal length
        for j in range(n_in):
            v = rng.uniform(0.5, 2.0, size=(2, 2)).astype(np.float32)
            v[1, 1] = 0.0                                       # LM metrics carry the reference's 0 above level 0
            vals[:, :, k, j] = v
            table.add(k, j, {m: {l: torch.tensor(v[h, l]).cuda() for l in range(2)} for h, m in enumerate(names)})
    data, (sets, mets) = table.mean()
    ref = vals.copy()
    ref[ref == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # "Mean of empty slice": LM_MAE at level 1
        ref = np.concatenate(np.nanmean(ref, axis=-1).T, axis=1)
    np.testing.assert_array_equal(data, ref)
    assert list(sets) == ["long", "long", "short", "short"] and list(mets) == names * 2


def test_affine_scores_are_the_loose_metrics(api):
    from pulpo_amd import eval_metrics
    from pulpo_amd.evaluation import affine_scores
    gen = torch.Generator().manual_seed(6)
    x, y = torch.rand(1, 1, 9, 10, 11, generator=gen).cuda(), torch.rand(1, 1, 9, 10, 11, generator=gen).cuda()
    sx = torch.softmax(3 * torch.randn(1, 4, 9, 10, 11, generator=gen), dim=1).cuda()
    sy = torch.softmax(3 * torch.randn(1, 4, 9, 10, 11, generator=gen), dim=1).cuda()
    lx, ly = 10 * torch.rand(1, 7, 3, generator=gen).cuda(), 10 * torch.rand(1, 7, 3, generator=gen).cuda()
    res = affine_scores(x, y, sx, sy, lx, ly)
    assert set(res) == {"RMSE", "Dice", "LM_MAE", "LM_Euclid"}
    assert torch.equal(res["RMSE"], eval_metrics.rmse(x, y)) and torch.equal(res["Dice"], eval_metrics.dsc(sx, sy))
    assert torch.equal(res["LM_MAE"], torch.median(torch.abs(lx - ly).sum(dim=2)))
    assert torch.equal(res["LM_Euclid"], torch.mean(torch.sqrt(((lx - ly) ** 2).sum(dim=2))))
    assert torch.equal(res["LM_MAE"], eval_metrics.lm_mae(lx, ly)) and torch.equal(res["LM_Euclid"], eval_metrics.lm_euclid(lx, ly))
    assert set(affine_scores(x, y)) == {"RMSE"}
