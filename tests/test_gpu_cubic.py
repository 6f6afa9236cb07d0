"""Cubic B-spline interpolation on the MI355X against the float64 definition of tests/cubic_ref.py: the prefilter, the
64-tap gather and its field gradient element by element, their determinism, and the interpolation= argument of the public surface.

Shapes (field grid / image size): (5,6,7) one block; (9,11,14) on (7,12,10) with B = 2, C = 2 - odd extents, sizes that differ, a batch and a
channel stride; (40,36,44) many blocks, a voxel count no multiple of the block; (1,20,24) the 2-D form through the 2-D interface; (6,5,200)
one long line: the prefilter's W pass takes four 64-column LDS chunks, the last one partial, and carries the recursion across them.
Fields are smooth noise (a 4^3 randn lattice interpolated up) of 1 to 3 voxels; every case asserts that between 2 % and 90 % of its samples
lie outside the volume, so the clamp and the mirror taps are exercised.
Bounds.  Every comparison is element by element against float64 under max(4 x the error of the same reference run in fp32 on the CPU against
float64, 1e-6 max|ref|) (metrics_ref.bound), and check() shows that the bound rejects a 1e-3 max|ref| error.  The gradient comparison leaves
out voxels where a float64 coordinate lies within 1e-3 of 0 or Si - 1: dscale jumps there by definition, and an fp32 coordinate may fall on
the other side; at most 0.5 % of the voxels may be left out.  Every comparison prints a RATIO line (pytest -s)."""
import functools

import pytest
import torch

import affine_ref as AR
import cubic_ref as CR
import metrics_ref as M
import refine_ref as RR
from oracle import pulpo_oracle as O
from test_gpu_affine import check
from test_host_affine import integer_landing_field
from test_host_cubic import ROUND_TRIP_SIZE, round_trip_image

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
OUTSIDE_MIN, OUTSIDE_MAX = 0.02, 0.90
EDGE_EPS, EDGE_MAX_SHARE = 1e-3, 0.005

# name: (grid, image size, B, C, seed, field amplitude in voxels)
CASES = {
    "one-block": ((5, 6, 7), (5, 6, 7), 1, 1, 1, 1.0),
    "odd-unequal": ((9, 11, 14), (7, 12, 10), 2, 2, 2, 1.5),
    "multi-block": ((40, 36, 44), (40, 36, 44), 1, 1, 3, 3.0),
    "slice": ((1, 20, 24), (1, 20, 24), 1, 2, 4, 2.0),
    "long-line": ((6, 5, 200), (6, 5, 200), 1, 1, 5, 2.0),
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    return ops


@functools.lru_cache(maxsize=None)
def case(name: str):
    """inputs (float64 tensors holding fp32 values) and the float64 / fp32 references of one case, computed once on the CPU"""
    grid, isize, B, C, seed, amp = CASES[name]
    df = CR.smooth_field(B, grid, seed, amp).float().double()
    img = AR.smooth_image(B, C, isize, seed + 10, lattice_div=3).float().double()
    g = torch.randn(B, C, *grid, generator=torch.Generator().manual_seed(seed + 20)).double()
    outside = CR.outside_fraction(df, isize)
    print(f"FIGURE case {name}: {100 * outside:.1f} % of the samples outside the volume")
    assert OUTSIDE_MIN <= outside <= OUTSIDE_MAX, f"case {name}: {outside:.3f} of the samples lie outside the volume"
    coef64, coef32 = CR.prefilter(img), CR.prefilter(img.float())
    # value and gradient references on the fp32-rounded coefficients the device kernels would see from a float64-exact prefilter
    cq = coef64.float().double()
    val64, val32 = CR.warp_coef(df, cq), CR.warp_coef(df.float(), cq.float())
    gdf64, gdf32 = CR.gdf(df, cq, g), CR.gdf(df.float(), cq.float(), g.float())
    _, raw, _ = CR.coords(df, isize)
    near = torch.zeros_like(raw[:, 0], dtype=torch.bool)
    for a in range(3):
        if grid[a] > 1:
            near |= (raw[:, a].abs() < EDGE_EPS) | ((raw[:, a] - (isize[a] - 1)).abs() < EDGE_EPS)
    share = float(near.double().mean())
    print(f"FIGURE case {name}: {share:.2e} of the voxels within {EDGE_EPS} of a clamp bound")
    assert share <= EDGE_MAX_SHARE, f"case {name}: {share:.4f} of the voxels lie within {EDGE_EPS} of a clamp bound"
    keep = (~near).unsqueeze(1).expand_as(gdf64)
    return dict(grid=grid, isize=isize, df=df, img=img, g=g, coef64=coef64, coef32=coef32, cq=cq, val64=val64, val32=val32, gdf64=gdf64,
                gdf32=gdf32, keep=keep)


def dev(t):
    return t.float().to(DEV)


def field_args(name, df):
    """the field as the operator takes it: the slice case goes through the 2-D interface (two components, no depth axis)"""
    return dev(df[:, 1:, 0]).contiguous() if CASES[name][0][0] == 1 else dev(df)


def image_args(name, img):
    return dev(img[:, :, 0]).contiguous() if CASES[name][0][0] == 1 else dev(img)


def lift(name, t):
    return t.unsqueeze(2) if CASES[name][0][0] == 1 else t


def lift_field(name, t):
    return torch.cat([torch.zeros_like(t[:, :1]), t], dim=1).unsqueeze(2) if CASES[name][0][0] == 1 else t


# ================================================================================================ the kernels
@pytest.mark.parametrize("name", list(CASES))
def test_prefilter_vs_float64(ops, name):
    c = case(name)
    got = lift(name, ops.bspline_prefilter(image_args(name, c["img"])))
    check(f"prefilter {name}", got, c["coef64"], M.bound(c["coef32"], c["coef64"], 1e-6))


@pytest.mark.parametrize("name", list(CASES))
def test_value_vs_float64(ops, name):
    c = case(name)
    got = lift(name, ops.warp3d_cubic(field_args(name, c["df"]), coef=image_args(name, c["cq"])))
    check(f"warp3d_cubic {name}", got, c["val64"], M.bound(c["val32"], c["val64"], 1e-6))
    # the whole route, prefilter included, against the float64 route from the image
    whole = lift(name, ops.warp3d_cubic(field_args(name, c["df"]), image_args(name, c["img"])))
    ref64, ref32 = CR.warp_coef(c["df"], c["coef64"]), CR.warp_coef(c["df"].float(), c["coef32"])
    check(f"warp3d_cubic from the image {name}", whole, ref64, M.bound(ref32, ref64, 1e-6))


@pytest.mark.parametrize("name", list(CASES))
def test_field_gradient_vs_float64(ops, name):
    c = case(name)
    df = field_args(name, c["df"]).requires_grad_(True)
    out = ops.warp3d_cubic(df, coef=image_args(name, c["cq"]))
    out.backward(image_args(name, c["g"]))
    got = lift_field(name, df.grad)
    keep = c["keep"]
    ref64, ref32 = c["gdf64"][keep], c["gdf32"][keep]
    check(f"warp3d_cubic gdf {name}", got[keep.to(DEV)], ref64, M.bound(ref32, ref64, 1e-6))
    if CASES[name][0][0] == 1:
        assert bool((got[:, 0] == 0).all()), "a depth-1 grid has no depth gradient"
    _, _, dscale = CR.coords(c["df"], c["isize"])
    clamped = (dscale == 0) & c["keep"]
    assert bool((got[clamped.to(DEV)] == 0).all()), "a clamped coordinate has a gradient"


@pytest.mark.parametrize("name", ["odd-unequal", "slice", "long-line"])
def test_same_bits_every_call_and_in_deterministic_mode(ops, name):
    c = case(name)
    img, g = image_args(name, c["img"]), image_args(name, c["g"])

    def run():
        df = field_args(name, c["df"]).requires_grad_(True)
        coef = ops.bspline_prefilter(img)
        out = ops.warp3d_cubic(df, img)
        out.backward(g)
        return coef, out.detach(), df.grad, ops.warp3d_cubic(df.detach(), coef=coef)

    first, second = run(), run()
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        det = run()
    finally:
        ops.set_deterministic(prev)
    for a, b, d in zip(first, second, det):
        assert torch.equal(a, b), "two calls differ"
        assert torch.equal(a, d), "deterministic mode differs"
    assert torch.equal(first[1], first[3]), "warp3d_cubic(df, coef=prefilter(img)) differs from warp3d_cubic(df, img)"


def test_integer_landing_field_returns_the_image(ops):
    Sg, Si = (6, 5, 7), (12, 10, 14)
    img = AR.smooth_image(1, 2, Si, 31, lattice_div=3).float().double()
    df = integer_landing_field(Sg, Si, (1, -1, 2)).float().double()
    idx = CR.coords(integer_landing_field(Sg, Si, (1, -1, 2)), Si)[0].round().long()
    want = AR._gather(img, idx[:, 0], idx[:, 1], idx[:, 2])
    ref64, ref32 = CR.warp(df, img), CR.warp(df.float(), img.float())
    tol = M.bound(ref32, ref64, 1e-6)
    got = ops.warp3d_cubic(dev(df), dev(img))
    check("integer landing against the reference", got, ref64, tol)
    check("integer landing against the image", got, want, tol + float((ref64 - want).abs().max()))


def test_round_trip_on_the_device_is_sharper_than_linear(ops):
    """tests/test_host_cubic.py's half-voxel round trip through ops.warp3d and ops.warp3d_cubic: the same condition"""
    img = dev(round_trip_image())
    there, back = (dev(t) for t in CR.shift_pair(ROUND_TRIP_SIZE))
    lin = ops.warp3d(back, ops.warp3d(there, img))
    cub = ops.warp3d_cubic(back, ops.warp3d_cubic(there, img))
    e_lin, e_cub = CR.interior_rmse(lin, img), CR.interior_rmse(cub, img)
    print(f"FIGURE half-voxel round trip on the device, interior RMSE: linear {e_lin:.4f}, cubic {e_cub:.4f}")
    assert e_cub < e_lin


# ================================================================================================ the public surface
@pytest.fixture(scope="module")
def setup(ops):
    import src.models as models
    import src.network_blocks as nb
    size = (16, 16, 16)
    torch.manual_seed(4)
    model = models.PULPo(3, 2, 0.1, list(size), feedback=FB, n0=4).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    for l in range(model.latent_levels):                # pinned samplers: two predictions agree bit for bit
        shape = (1, model.ndims) + tuple(model.autoencoder.level_sizes[l + model.lk_offset])
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(shape, generator=g).to(DEV))
    x, y = RR.pair(size, 1, 21, dtype=torch.float32)
    return model, x.to(DEV), y.to(DEV)


def same_levels(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[l], b[l]) for l in a)


def test_linear_is_todays_route_and_cubic_changes_the_outputs_only(ops, setup):
    model, x, y = setup
    with torch.no_grad():
        out0, dfs0 = model.predict_deterministic(x, y)
        out1, dfs1 = model.predict_deterministic(x, y, interpolation="linear")
        outc, dfsc = model.predict_deterministic(x, y, interpolation="cubic")
        assert same_levels(out0, out1) and same_levels(dfs0, dfs1), "interpolation='linear' is not today's route"
        assert same_levels(dfs0, dfsc), "the fields depend on the interpolation"
        final = model.combine_dfs(dfs0)[1]
        level_x = model.autoencoder.level_images(x)
        for l in outc:
            assert torch.equal(outc[l], ops.warp3d_cubic(final[l], level_x[l])), l
            assert not torch.equal(outc[l], out0[l]), l
        p0, p1 = model.predict(x, y), model.predict(x, y, interpolation="linear")
        assert same_levels(p0[0], p1[0]) and same_levels(p0[1], p1[1])
        pc = model.predict(x, y, interpolation="cubic")
        pfinal = model.combine_dfs(pc[1])[1]
        assert same_levels(p0[1], pc[1]) and all(torch.equal(pc[0][l], ops.warp3d_cubic(pfinal[l], x)) for l in pfinal)


def test_bidirectional_outputs(ops, setup):
    """outputs_inv warps the fixed image the way the linear route does - the full-resolution y under final_dfs_inv[l] - through the cubic gather"""
    model, x, y = setup
    b0 = model.predict_bidirectional(x, y, deterministic=True)
    b1 = model.predict_bidirectional(x, y, deterministic=True, interpolation="linear")
    bc = model.predict_bidirectional(x, y, deterministic=True, interpolation="cubic")
    for k in b0:
        assert same_levels(b0[k], b1[k]), k
    for k in ("individual_dfs", "final_dfs", "final_dfs_inv"):
        assert same_levels(b0[k], bc[k]), k
    level_x = model.autoencoder.level_images(x)
    for l in bc["outputs"]:
        assert torch.equal(bc["outputs"][l], ops.warp3d_cubic(bc["final_dfs"][l], level_x[l])), l
        assert torch.equal(bc["outputs_inv"][l], ops.warp3d_cubic(bc["final_dfs_inv"][l], y)), l
    bs = model.predict_bidirectional(x, y, N=1, interpolation="cubic")
    assert all(torch.equal(bs["outputs"][l], ops.warp3d_cubic(bs["final_dfs"][l], x)) for l in bs["outputs"])


def test_refine_with_the_cubic_image_model(ops, setup):
    """iters = 0: the prediction's fields, and outputs = x under them through the cubic gather (refine warps the full-resolution x at every
    level, as its linear route does: level 0 is predict_deterministic's cubic output bit for bit); iters = 10: the objective does not rise"""
    model, x, y = setup
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        r0 = model.refine(x, y, iters=0, interpolation="cubic")
        l0 = model.refine(x, y, iters=0)
        l1 = model.refine(x, y, iters=0, interpolation="linear")
        r10 = model.refine(x, y, iters=10, interpolation="cubic")
        with torch.no_grad():
            outc, dfs = model.predict_deterministic(x, y, interpolation="cubic")
    finally:
        ops.set_deterministic(prev)
    assert all(torch.equal(l0[k][l], l1[k][l]) for k in ("individual_dfs", "final_dfs", "outputs") for l in l0[k]) and torch.equal(l0["history"], l1["history"])
    assert same_levels(r0["individual_dfs"], dfs)
    assert torch.equal(r0["outputs"][0], outc[0])
    for l in r0["outputs"]:
        assert torch.equal(r0["outputs"][l], ops.warp3d_cubic(r0["final_dfs"][l], x)), l
    assert not torch.equal(r0["history"], l0["history"]), "the objective does not see the cubic outputs"
    h = r10["history"]
    print(f"FIGURE refine, cubic image model: total {float(h[0, 0]):.4f} -> {float(h[-1, 0]):.4f}")
    assert bool(torch.isfinite(h).all()) and float(h[-1, 0]) <= float(h[0, 0])
    assert torch.equal(h[0], r0["history"][0])
    for l in r10["outputs"]:
        assert torch.equal(r10["outputs"][l], ops.warp3d_cubic(r10["final_dfs"][l], x)), l


def test_performance_scores_the_cubic_outputs(ops, setup):
    from pulpo_amd import evaluation
    model, x, y = setup
    B = x.shape[0]
    g = torch.Generator().manual_seed(12)
    seg_x = torch.randint(0, 3, (B, 1, 16, 16, 16), generator=g).to(DEV)
    seg_y = torch.randint(0, 3, (B, 1, 16, 16, 16), generator=g).to(DEV)
    mask_x = (torch.rand(B, 1, 16, 16, 16, generator=g) > 0.3).float().to(DEV)
    kw = dict(seg_x=seg_x, seg_y=seg_y, num_classes=3, mask_x=mask_x, mind=True, mi=True)
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        plain = evaluation.performance(model, x, y, **kw)
        lin = evaluation.performance(model, x, y, interpolation="linear", **kw)
        cub = evaluation.performance(model, x, y, interpolation="cubic", **kw)
        outc, dfs = model.predict_deterministic(x, y, interpolation="cubic")
        want = evaluation.level_scores(outc, model.combine_dfs(dfs)[1], y, **kw)
        theta = AR.theta_generic(B, 5, shift=1.0, dtype=torch.float32).to(DEV)
        aff = evaluation.performance(model, x, y, affine=theta, interpolation="cubic")
        xa = ops.affine_warp(theta, x)
        fa = {l: ops.affine_compose(theta, f, x.shape[2:]) for l, f in model.combine_dfs(model.predict_deterministic(xa, y)[1])[1].items()}
    finally:
        ops.set_deterministic(prev)
    image_rows = ("RMSE", "RMSE_masked", "MIND", "MI")
    assert plain.keys() == lin.keys() == cub.keys()
    for k in plain:
        for l in plain[k]:
            assert torch.equal(plain[k][l], lin[k][l]), (k, l)
            assert torch.equal(cub[k][l], want[k][l]), (k, l)
            if k not in image_rows:
                assert torch.equal(cub[k][l], plain[k][l]), (k, l)
    # the RMSE row is sqrt(l2_loss / voxels), ops.rmse sqrt(mean of squares): two fp32 reductions of the same 4096 (or 64) squares, each good
    # to a few 1e-7 relative - 1e-5 relative between them
    at_level = lambda out: y if tuple(out.shape[2:]) == tuple(y.shape[2:]) else ops.resize_trilinear(y, tuple(out.shape[2:]))
    for l in outc:
        want_rmse = float(ops.rmse(outc[l], at_level(outc[l])))
        assert abs(float(cub["RMSE"][l]) - want_rmse) <= 1e-5 * want_rmse, (l, float(cub["RMSE"][l]), want_rmse)
        assert float(cub["RMSE"][l]) != float(plain["RMSE"][l]), l
    for l in fa:                                        # affine=: the ORIGINAL x, once, under the composed field
        one = ops.warp3d_cubic(fa[l], x)
        want_rmse = float(ops.rmse(one, at_level(one)))
        assert abs(float(aff["RMSE"][l]) - want_rmse) <= 1e-5 * want_rmse, (l, float(aff["RMSE"][l]), want_rmse)
