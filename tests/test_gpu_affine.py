"""Affine pre-alignment on the MI355X against the float64 definition of tests/affine_ref.py: the four kernels element by
element, the fitting loop, and performance(affine=).

Shapes: the smallest at which the kernels can go wrong - (5,6,7) one block, odd extents, rows no multiple of 4; a grid (9,10,11) on an image
(12,8,10); (24,20,28) with B = 2 and a transform per element: many blocks, a batch stride, a voxel count no multiple of the block; (1,24,20)
the 2-D form; one case whose translation pushes a third of the samples into the clamp; C in {1, 3}; and the sizes at which a kernel takes
another path - (72,64,60), past the gradient kernel's capped grid, 132^3, where a looped forward kernel lost bit equality with warp3d, and
208 x 204 x 200, past the capped grids of the field and compose kernels (device-side float64 references there).
Bounds.  An operator: max(4 x the error of the same reference run in fp32 on the CPU against float64, 1e-6 max|ref|) (metrics_ref.bound).
The fit: 8 x the distance between the reference's own fp32 and float64 runs (the rule of test_gpu_refine.py), theta per entry in voxels (the
matrix entries scaled by the half extent, so that every entry is a displacement of the volume's edge) and history row by row, relative.
Inputs are smooth and the transforms generic (affine_ref.theta_lattice): each case asserts in float64 that no sample coordinate lies within
1e-4 of an integer or of a clamp bound, where the coordinate gradient is discontinuous and an fp32 coordinate may fall on the other side.
Every comparison prints a RATIO line (pytest -s; profiles/affine_gpu_tests.txt)."""
import functools

import pytest
import torch

import affine_ref as AR
import metrics_ref as M
import pyramid_ref as R
from oracle import pulpo_oracle as O
from test_host_affine import END_MAX, START_MIN, integer_landing_field

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
FIT_FACTOR = 8.0


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import affine, evaluation, ops
    from pulpo_amd._lib import lib
    lib.load()
    return ops, affine, evaluation


def check(name, got, ref, tol, power=-1):
    """max |got - ref| <= tol element by element; and the bound rejects ref with element `power` moved by 1e-3 max|ref|"""
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    ref = ref.to(got.device)
    r = R.ratio(got, ref, tol)
    print(f"RATIO {name} {r:.3g}")
    assert r <= 1.0, f"{name}: max error / tolerance = {r:.3g}"
    if power is not None:
        assert R.ratio(got, R.perturbed(ref, power), tol) > 1.0, f"{name}: the bound does not reject a 1e-3 max|ref| error"


# ================================================================================================ the operators
# name: (grid, image size, B, theta seed, shift in voxels)
CASES = {
    "one-block": ((5, 6, 7), (5, 6, 7), 1, 4, 1.0),
    "unequal": ((9, 10, 11), (12, 8, 10), 1, 5, 1.5),
    "batch": ((24, 20, 28), (24, 20, 28), 2, 6, 2.0),
    "slice": ((1, 24, 20), (1, 24, 20), 2, 7, 1.5),
    "clamp": ((9, 10, 11), (9, 10, 11), 1, 8, 0.5),
    # 276 480 voxels, past the 1024 x 256 of the gradient kernel's capped grid: its stride loop takes a second trip
    "two-trips": ((72, 64, 60), (72, 64, 60), 1, 9, 2.0),
}
# the clamp case: a fixed translation on top of the generic transform, in 64ths of a voxel: 3.4 and -3.7 voxels along y and x
CLAMP_SHIFT = (0, 218, -237)


@functools.lru_cache(maxsize=None)
def case_inputs(name: str, C: int):
    """(theta (B,3,4), img (B,C,*isize), gout (B,C,*grid)) as float64 tensors holding fp32 values, grid, isize; asserts the case is generic"""
    grid, isize, B, seed, shift = CASES[name]
    theta = AR.theta_lattice(B, seed, grid, isize, shift=shift, extra=CLAMP_SHIFT if name == "clamp" else (0, 0, 0))
    if grid[0] == 1:
        theta = AR.lift_theta(theta[:, 1:, 1:].contiguous())
    theta = theta.float().double()
    img = AR.smooth_image(B, C, isize, seed + 10, lattice_div=3).float().double()
    gout = torch.randn(B, C, *grid, generator=torch.Generator().manual_seed(seed + 20)).double()
    _, raw, dscale = AR.sample_coords(AR.grid(grid, torch.float64).unsqueeze(0) + AR.field(theta, grid), grid, isize)
    hi = torch.tensor([s - 1 for s in isize], dtype=torch.float64).view(1, 3, 1, 1, 1)
    near = ((raw - raw.round()).abs() < 1e-4) & (raw > -1e-4) & (raw < hi + 1e-4)
    assert not bool(near.any()), f"case {name}: {int(near.sum())} sample coordinates within 1e-4 of an integer or a clamp bound - pick another seed"
    if name == "clamp":
        clamped = float((dscale[:, 1:] == 0).any(dim=1).double().mean())
        assert clamped >= 1.0 / 3.0, f"the clamp case clamps {clamped:.2f} of the samples"
    return theta, img, gout, grid, isize


def to_dev(t):
    return t.float().to(DEV)


def ops_args(name, theta, img):
    """the operator's arguments on the device: the slice case goes through the 2-D interface"""
    if CASES[name][0][0] == 1:
        return to_dev(theta[:, 1:, 1:]).contiguous(), to_dev(img[:, :, 0])
    return to_dev(theta), to_dev(img)


def lift_out(name, t):
    return t.unsqueeze(2) if CASES[name][0][0] == 1 else t


@pytest.mark.parametrize("name", list(CASES))
def test_affine_field_vs_float64(api, name):
    ops = api[0]
    theta, img, _, grid, _ = case_inputs(name, 1)
    th, _ = ops_args(name, theta, img)
    got = ops.affine_field(th, grid[1:] if grid[0] == 1 else grid)
    if grid[0] == 1:
        assert tuple(got.shape) == (theta.shape[0], 2, *grid[1:])
        got = torch.cat([torch.zeros_like(got[:, :1]), got], dim=1).unsqueeze(2)
    ref = AR.field(theta, grid)
    check(f"affine_field {name}", got, ref, M.bound(AR.field(theta.float(), grid), ref, 1e-6))
    ident = ops.affine_field(to_dev(AR.identity(1)), (5, 6, 7))
    assert bool((ident == 0).all()), "the identity's displacement is not exactly zero"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_affine_warp_forward(api, name, C):
    """C = 1: bit-identical to ops.warp3d on the materialised field.  C = 3: held to the float64 bound instead - bit equality with
    pulpo_warp3d_fwd is out of reach there, because the compiler builds warp_fwd_kernel<3>'s interpolation from packed multiplies and
    separate adds where the same source expression in affine_warp_fwd_kernel<3> becomes fused multiply-adds; the
    differing elements and their distance are printed (measured: about one element in five, by 1 ulp: 1.2e-7 at values of 0.5).
    Both: within the bound of the float64 reference; inputs left alone."""
    ops = api[0]
    theta, img, _, grid, _ = case_inputs(name, C)
    th, im = ops_args(name, theta, img)
    size = grid[1:] if grid[0] == 1 else grid
    keep = (th.clone(), im.clone())
    got = ops.affine_warp(th, im, size)
    via_field = ops.warp3d(ops.affine_field(th, size), im)
    diff = got != via_field
    worst = float((got.double() - via_field.double()).abs().max())
    print(f"FIGURE affine_warp {name} C{C}: {int(diff.sum())} of {diff.numel()} elements differ from warp3d(affine_field), largest {worst:.3g}")
    if C == 1:
        assert torch.equal(got, via_field), "affine_warp differs from warp3d(affine_field(theta), img)"
    ref = AR.warp(theta, img, grid)
    check(f"affine_warp fwd {name} C{C}", lift_out(name, got), ref, M.bound(AR.warp(theta.float(), img.float(), grid), ref, 1e-6))
    assert torch.equal(th, keep[0]) and torch.equal(im, keep[1])
    if name == "one-block":
        assert torch.equal(ops.affine_warp(th, im), got), "size=None is the image's own grid"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_affine_warp_gtheta(api, name, C):
    """the gradient with respect to theta against the float64 analytic reference and against ops.warp3d's displacement gradient reduced in
    float64 on the host; two calls bit-identical with determinism off and on; the depth row and column of the 2-D form exactly 0"""
    ops = api[0]
    theta, img, gout, grid, _ = case_inputs(name, C)
    th3, im5, g = to_dev(theta), to_dev(img), to_dev(gout)
    keep = (th3.clone(), im5.clone())

    def run():
        leaf = th3.clone().requires_grad_(True)
        ops.affine_warp(leaf, im5, grid).backward(g)
        return leaf.grad

    got = run()
    ref = AR.gtheta(theta, img, gout, grid)
    tol = M.bound(AR.gtheta(theta.float(), img.float(), gout.float(), grid), ref, 1e-6)
    check(f"gtheta {name} C{C}", got, ref, tol, power=5)
    # the route through the existing operators: warp3d's gdf, reduced on the host in float64
    df = ops.affine_field(th3, grid).requires_grad_(True)
    ops.warp3d(df, im5).backward(g)
    gdf = df.grad.double().cpu()
    u = AR.grid(grid, torch.float64) - AR.centre(grid, torch.float64).view(3, 1, 1, 1)
    host = torch.cat([torch.einsum("badhw,jdhw->baj", gdf, u), gdf.flatten(2).sum(2, keepdim=True)], dim=2)
    check(f"gtheta {name} C{C} vs warp3d gdf", got, host, tol, power=5)
    prev = ops.DETERMINISTIC
    try:
        for mode in (False, True):
            ops.set_deterministic(mode)
            assert torch.equal(run(), got) and torch.equal(run(), got), f"gtheta differs from call to call (deterministic={mode})"
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(th3, keep[0]) and torch.equal(im5, keep[1])
    if grid[0] == 1:
        assert bool((got[:, 0] == 0).all()) and bool((got[:, :, 0] == 0).all()), "2-D form: depth row / column of the gradient not exactly 0"
        th2, im4 = ops_args(name, theta, img)
        leaf = th2.clone().requires_grad_(True)
        ops.affine_warp(leaf, im4).backward(g[:, :, 0])
        assert torch.equal(leaf.grad, got[:, 1:, 1:])


def test_affine_warp_forward_bit_equal_at_large_sizes(api):
    """C = 1 at 128^3 (the largest grid of 8192 blocks) and 132^3: a forward kernel with a grid-stride loop agreed with pulpo_warp3d_fwd up to
    128^3 and differed in the last bit of a quarter of the voxels from 132^3 on (the compiler packed the coordinate arithmetic of two trips)"""
    ops = api[0]
    from pulpo_amd import synthetic
    g = torch.Generator(device=DEV).manual_seed(0)
    theta = synthetic.default_theta_gen(1, DEV)
    for S in (128, 132):
        img = ops.resize_trilinear(torch.rand((1, 1, S // 8, S // 8, S // 8), device=DEV, generator=g), (S, S, S)).contiguous()
        got, via_field = ops.affine_warp(theta, img), ops.warp3d(ops.affine_field(theta, (S, S, S)), img)
        ndiff = int((got != via_field).sum())
        print(f"FIGURE affine_warp {S}^3 C1: {ndiff} of {got.numel()} elements differ from warp3d(affine_field)")
        assert ndiff == 0


def test_field_and_compose_beyond_one_trip(api):
    """208 x 204 x 200 = 8.5 M voxels, past the 8193 x 256 float4 groups of the capped grids of the field and compose kernels: their stride
    loops take a second trip.  The float64 reference (and its fp32 run, for the bound) is evaluated on the device."""
    ops = api[0]
    size = (208, 204, 200)
    theta = AR.theta_generic(1, 21, shift=2.0).float()
    got = ops.affine_field(theta.to(DEV), size)
    ref = AR.field(theta.double().to(DEV), size)
    check("affine_field 208x204x200", got, ref, M.bound(AR.field(theta.to(DEV), size), ref, 1e-6))
    del got
    g = torch.Generator(device=DEV).manual_seed(2)
    df = ops.resize_trilinear((torch.rand((1, 3, 13, 12, 12), device=DEV, generator=g) * 2 - 1) * 3.0, size).contiguous()
    got = ops.affine_compose(theta.to(DEV), df)
    ref = AR.compose(theta.double().to(DEV), df.double())
    check("affine_compose 208x204x200", got, ref, M.bound(AR.compose(theta.to(DEV), df), ref, 1e-6))


def test_affine_warp_refusals(api):
    ops = api[0]
    theta, img, _, grid, _ = case_inputs("one-block", 1)
    with pytest.raises(ValueError, match="data"):
        ops.affine_warp(to_dev(theta), to_dev(img).requires_grad_(True))
    out = ops.affine_warp(to_dev(theta), to_dev(img))                       # theta without grad: nothing to differentiate, no error
    assert not out.requires_grad


COMPOSE_CASES = {"equal": ((12, 10, 14), (12, 10, 14), 1), "half": ((6, 5, 7), (12, 10, 14), 2), "slice": ((1, 12, 16), (1, 12, 16), 1)}


def _compose_inputs(name):
    Sg, Si, B = COMPOSE_CASES[name]
    theta = AR.theta_generic(B, 12, shift=1.0)
    if Sg[0] == 1:
        theta = AR.lift_theta(theta[:, 1:, 1:].contiguous())
    theta = theta.float().double()
    df = ((AR.smooth_image(B, 3, Sg, 13) * 2 - 1) * 2.5).float().double()          # up to 2.5 voxels: some samples clamp at the border
    if Sg[0] == 1:
        df[:, 0] = 0
    return theta, df, Sg, Si


@pytest.mark.parametrize("name", list(COMPOSE_CASES))
def test_affine_compose_vs_float64(api, name):
    ops = api[0]
    theta, df, Sg, Si = _compose_inputs(name)
    if Sg[0] == 1:
        got = ops.affine_compose(to_dev(theta[:, 1:, 1:]).contiguous(), to_dev(df[:, 1:, 0]), Si[1:])
        got = torch.cat([torch.zeros_like(got[:, :1]), got], dim=1).unsqueeze(2)
    else:
        keep = to_dev(df)
        got = ops.affine_compose(to_dev(theta), keep, Si)
        assert torch.equal(keep, to_dev(df))
    ref = AR.compose(theta, df, Si)
    check(f"affine_compose {name}", got, ref, M.bound(AR.compose(theta.float(), df.float(), Si), ref, 1e-6))


def test_compose_equals_two_steps_without_a_second_interpolation(api):
    """df lands the first sampling on integer indices: warp3d(compose(theta, df), img) and warp3d(df, affine_warp(theta, img)) agree with the
    float64 value of either within the bound (they differ by the second interpolation only, which is absent here)"""
    ops = api[0]
    Sg, Si = (6, 5, 7), (12, 10, 14)
    img = AR.smooth_image(1, 2, Si, 6).float().double()
    theta = AR.theta_generic(1, 7).float().double()
    df = integer_landing_field(Sg, Si, (1, -1, 2))
    ref = AR.warp_field(AR.compose(theta, df, Si), img)
    two32 = AR.warp_field(df.float(), AR.warp(theta.float(), img.float()))
    one32 = AR.warp_field(AR.compose(theta.float(), df.float(), Si), img.float())
    tol = max(M.bound(two32, ref, 1e-6), M.bound(one32, ref, 1e-6))
    th, im, d = to_dev(theta), to_dev(img), to_dev(df)
    one = ops.warp3d(ops.affine_compose(th, d, Si), im)
    two = ops.warp3d(d, ops.affine_warp(th, im))
    check("compose one step", one, ref, tol)
    check("compose two steps", two, ref, tol)


# ================================================================================================ the fit
# (size, loss, dof, masked, recovery asserted)
FIT_CASES = [((32, 32, 32), "ncc", 12, False, True), ((24, 32, 28), "ncc", 12, False, True), ((16, 20, 18), "mse", 12, False, False),
             ((16, 20, 18), "ncc", 12, True, False), ((16, 20, 18), "ncc", 6, False, False)]


def theta_voxels(theta, size):
    """theta with its matrix entries scaled by the half extent of the grid: every entry a displacement of the volume's edge in voxels"""
    return torch.cat([theta[:, :, :3] * ((max(size) - 1) / 2), theta[:, :, 3:]], dim=2)


def hist_rel(h, h64):
    return (h[:, 0].double().cpu() - h64[:, 0]).abs() / h64[:, 0].abs()


@pytest.mark.parametrize("size,loss,dof,masked,recovery", FIT_CASES)
def test_fit_vs_float64(api, size, loss, dof, masked, recovery):
    """affine.fit with its defaults against affine_ref.fit in float64 on the same pair: theta (in voxels of edge displacement) and the
    history (row by row, relative) within 8 x the distance between the reference's own fp32 and float64 runs; the two NCC cases at 32^3
    and 24 x 32 x 28 also meet the recovery condition - corner error at most 1.0 voxel from at least 4.4."""
    ops, affine, _ = api
    th64, h64, want, x, y, mx, my = AR.fit_reference(size, loss, dof, masked)
    th32, h32, *_ = AR.fit_reference(size, loss, dof, masked, torch.float32)
    own_t = M.spread(theta_voxels(th32, size), theta_voxels(th64, size))
    own_h = float(hist_rel(h32, h64).max())
    print(f"FIGURE fit {size} {loss} dof {dof} masked {masked}: reference fp32 against float64 theta {own_t:.3g} voxels, history {own_h:.3g} relative")
    res = affine.fit(to_dev(x), to_dev(y), dof=dof, loss=loss, mask_x=None if mx is None else to_dev(mx), mask_y=None if my is None else to_dev(my))
    got, hist = res["theta"], res["history"]
    assert tuple(hist.shape) == tuple(h64.shape) and torch.equal(hist[:, 1].cpu().double(), h64[:, 1])
    tag = f"fit {size} {loss} dof {dof} masked {masked}"
    rt = R.ratio(theta_voxels(got, size).cpu(), theta_voxels(th64, size), FIT_FACTOR * own_t)
    rh = float(hist_rel(hist, h64).max()) / (FIT_FACTOR * own_h)
    start, end = AR.corner_error(AR.identity(1), want, size), float(affine.corner_error(got.cpu(), want, size))
    print(f"RATIO {tag} theta {rt:.3g}")
    print(f"RATIO {tag} history {rh:.3g}")
    print(f"FIGURE {tag}: corner error {start:.3f} -> {end:.3f}")
    assert rt <= 1.0 and rh <= 1.0, (rt, rh)
    if recovery:
        assert start >= START_MIN and end <= END_MAX
    assert float(hist[-1, 0]) <= float(hist[sum(AR.DEFAULT_ITERS[:2]), 0]), "the finest level's loss rose"


def test_fit_is_deterministic_and_synthetic_pair(api):
    """synthetic.affine_pair's triple; two fits under ops.set_deterministic(True) are bit-identical; theta0 = the result with no iterations
    returns it"""
    ops, affine, _ = api
    from pulpo_amd import synthetic
    size = (16, 20, 18)
    x, y, want = synthetic.affine_pair(size, 1, 3, DEV)
    assert tuple(want.shape) == (1, 3, 4) and x.shape == y.shape == (1, 1, *size)
    gen = synthetic.default_theta_gen(1, DEV)
    assert torch.equal(x, ops.affine_warp(gen, y))
    assert float((want.cpu().double() - AR.expected_fit(gen.cpu().double(), size)).abs().max()) < 1e-5
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        a = affine.fit(x, y, levels=2, iters=(6, 6), win=(7, 5))
        b = affine.fit(x, y, levels=2, iters=(6, 6), win=(7, 5))
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(a["theta"], b["theta"]) and torch.equal(a["history"], b["history"])
    assert not torch.equal(a["theta"], affine.identity(1, DEV))
    c = affine.fit(x, y, levels=1, iters=(0,), win=(5,), theta0=a["theta"])
    assert float((c["theta"] - a["theta"]).abs().max()) < 1e-5 and tuple(c["history"].shape) == (1, 2)
    with pytest.raises(NotImplementedError):
        affine.fit(x[:, :, 0], y[:, :, 0], loss="mind")
    s = affine.fit(x[:, :, 8].contiguous(), y[:, :, 8].contiguous(), levels=2, iters=(4, 4), win=(7, 5))
    assert tuple(s["theta"].shape) == (1, 2, 3) and bool(torch.isfinite(s["history"]).all())


# ================================================================================================ performance(affine=)
def test_performance_with_an_affine(api):
    """performance(model, x, y, seg_x, lm_x, affine=theta) on the small T3/L2 model at 16^3 = level_scores by hand on
    model.predict_deterministic(affine_warp(theta, x), y) with the fields composed by hand; affine=None is the call without the argument"""
    import src.models as models
    import src.network_blocks as nb
    ops, affine, evaluation = api
    size, C = (16, 16, 16), 4
    torch.manual_seed(4)
    model = models.PULPo(3, 2, 0.1, list(size), feedback=FB, n0=4).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    for l in range(model.latent_levels):
        shape = (1, model.ndims) + tuple(model.autoencoder.level_sizes[l + model.lk_offset])
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(shape, generator=g).to(DEV))
    y = to_dev(AR.smooth_image(1, 1, size, 30))
    theta = to_dev(AR.theta_generic(1, 31, shift=1.0))
    x = to_dev(AR.smooth_image(1, 1, size, 32))
    seg_x = torch.randint(0, C, (1, 1, *size), generator=g).to(torch.uint8).to(DEV)
    seg_y = torch.randint(0, C, (1, 1, *size), generator=g).to(torch.uint8).to(DEV)
    lm_x = torch.stack([torch.randint(2, s - 2, (6,), generator=g) for s in size], dim=-1)[None].float().to(DEV)
    lm_y = (lm_x + torch.randn(lm_x.shape, generator=g).to(DEV)).clamp(0, min(size) - 1)
    kw = dict(seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=C, surface=True)
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            got = evaluation.performance(model, x, y, affine=theta, **kw)
            x_aff = ops.affine_warp(theta, x)
            outputs, ind = model.predict_deterministic(x_aff, y)
            final = {l: ops.affine_compose(theta, df, size) for l, df in model.combine_dfs(ind)[1].items()}
            want = evaluation.level_scores(outputs, final, y, **kw)
            none = evaluation.performance(model, x, y, affine=None, **kw)
            plain = evaluation.performance(model, x, y, **kw)
            fitted = evaluation.performance(model, x, y, affine={"levels": 2, "iters": (3, 3), "win": (7, 5)})
    finally:
        ops.set_deterministic(prev)
    for a, b in ((got, want), (none, plain)):
        assert a.keys() == b.keys()
        for k in a:
            for l in a[k]:
                assert torch.equal(a[k][l], b[k][l]), (k, l, float(a[k][l]), float(b[k][l]))
    assert float(got["RMSE"][0]) != float(plain["RMSE"][0]) and float(got["Dice"][0]) != float(plain["Dice"][0])
    assert bool(torch.isfinite(fitted["RMSE"][0]))
    base = evaluation.affine_scores(x, y, lm_x=lm_x, lm_y=lm_y, theta=theta)
    assert torch.equal(base["RMSE"], evaluation.affine_scores(ops.affine_warp(theta, x), y)["RMSE"])
    assert float(base["LM_MAE"]) != float(evaluation.affine_scores(x, y, lm_x=lm_x, lm_y=lm_y)["LM_MAE"])
