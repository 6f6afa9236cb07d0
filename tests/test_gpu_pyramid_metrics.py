"""The optional losses (--recon_loss mse / dice, --regularizer jdet, --nondiagonal), the evaluation scalars, the streaming Monte-Carlo
moments and the fused Adam against float64 references (tests/metrics_ref.py, evaluated with plain torch ops on the GPU), at the smallest
shapes that cross each launch policy's thresholds: the second grid-stride trip of every capped grid (pulpo_metric_blocks: 1024 blocks =
262,144 threads; the element-wise backward grids: 4096 blocks = 1,048,576 threads; pulpo_dice_blocks: 256 blocks per plane = 65,536
threads; the moments: 8192 blocks = 2,097,152 threads; Adam: 4096 blocks x 256 threads x float4 = 4,194,304 elements), more than 64 planes
for the Dice finishers, plane boundaries, tails.

One rule bounds every comparison: max(4 x the reference's own fp32 deviation from float64, a floor of 1e-6 = 8 fp32 roundings, relative
to max|ref|).  The factor 4 allows for a kernel that rounds in another operation order than the fp32 reference; the floor for a reference
that happens to round nothing.  Tensors are compared element by element, and every such comparison is shown to have power: the same bound
must reject the reference with one element - the last, the first of the second grid-stride trip, or the first of the last plane - moved by
1e-3 max|ref|.  Each test prints `RATIO <name> <error / bound>` lines (pytest -s)."""
import pytest
import torch

import metrics_ref as M
import pyramid_ref as R
from oracle import pulpo_oracle as O
from test_gpu_performance import folded_field

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 1e-6                    # 8 roundings of 2^-23: what a handful of fp32 operations per element may differ by
FWD_TRIP = 1024 * 256           # pulpo_metric_blocks
BWD_TRIP = 4096 * 256           # the element-wise backward kernels
DICE_TRIP = 256 * 256           # per plane
MOM_TRIP = 8192 * 256
ADAM_TRIP = 4096 * 256 * 4
UP = 1.7                        # upstream gradient of every loss


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def amax(t) -> float:
    return float(t.detach().abs().max())


def check(name, got, ref, tol, power=-1):
    """max |got - ref| <= tol element by element; and the bound rejects ref with element `power` (flat index) moved by 1e-3 max|ref|"""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    r = R.ratio(got, ref, tol)
    print(f"RATIO {name} {r:.3g}")
    assert r <= 1.0, f"{name}: max error / tolerance = {r:.3g}"
    if power is not None:
        assert R.ratio(got, R.perturbed(ref, power), tol) > 1.0, f"{name}: the bound does not reject a 1e-3 max|ref| error in element {power}"


def check_tensor(name, got, ref64, ref32, power=-1, floor=FLOOR):
    """check() under the rule: tol = max(4 x max|ref32 - ref64|, floor x max|ref64|).  Returns (relative error, relative bound)"""
    tol = M.bound(ref32, ref64, floor)
    scale = max(amax(ref64), 1e-300)
    err, own = R.ratio(got, ref64, 1.0) / scale, M.spread(ref32, ref64) / scale
    print(f"FIGURE {name}: error {err:.3g} of max|ref|, fp32 reference {own:.3g}, bound {tol / scale:.3g}")
    check(name, got, ref64.detach(), tol, power)
    return err, tol / scale


def check_scalar(name, got, ref64, ref32, floor=FLOOR):
    """a 0-d fp32 result: |got - ref64| / |ref64| <= max(4 x the fp32 reference's own relative deviation, floor).  Returns (deviation, bound)"""
    assert got.dim() == 0 and got.dtype == torch.float32, (name, got.shape, got.dtype)
    tol = max(4.0 * M.rel(ref32, ref64), floor)
    dev = M.rel(got, ref64)
    print(f"RATIO {name} {dev / tol:.3g}   (deviation {dev:.3g}, fp32 reference {M.rel(ref32, ref64):.3g}, bound {tol:.3g})")
    assert dev <= tol, f"{name}: relative deviation {dev:.3g} from float64 {float(ref64):.9g}, bound {tol:.3g}"
    return dev, tol


def grads_of(fn, inputs, dtype):
    """(value, gradients with the upstream gradient UP) of fn on detached copies of `inputs` in `dtype`"""
    xs = [t.detach().to(dtype).requires_grad_(True) for t in inputs]
    val = fn(*xs)
    return (val.detach(),) + torch.autograd.grad(val, xs, grad_outputs=torch.tensor(UP, dtype=dtype, device=val.device))


def trip_index(n: int, trip: int) -> int:
    """the first element of the second grid-stride trip where there is one, else the last element"""
    return trip if n > trip else n - 1


# ================================================================================================ L2_loss, rmse
# 420 elements (the golden's shape); one past the forward's first trip at 270,336; past the backward's first trip at 1,088,640; a slice pair
L2_SHAPES = [(2, 1, 5, 6, 7), (1, 1, 64, 66, 64), (2, 3, 56, 60, 54), (2, 1, 40, 36)]


@pytest.mark.parametrize("shape", L2_SHAPES)
def test_l2_loss_and_rmse_vs_float64(ops, shape):
    """ops.l2_loss with its gradient (sqdiff_fwd / sqdiff_bwd) and ops.rmse, also with a target that broadcasts over the batch.
    Observed on the MI355X, relative to float64: loss 9.2e-10 ... 6.3e-9, rmse 1.9e-9 ... 3.3e-8 (bound 1e-6); gradient 8.5e-8 ... 1.4e-7 of
    max|ref| (bound 1e-6, the fp32 reference's own the same)."""
    g = gen(sum(shape))
    a, b = torch.randn(shape, device=DEV, generator=g), torch.randn(shape, device=DEV, generator=g)
    n = a.numel()
    ag = a.clone().requires_grad_(True)
    loss = ops.l2_loss(ag, b)
    ga, = torch.autograd.grad(loss, [ag], grad_outputs=torch.tensor(UP, device=DEV))
    f = lambda x, y: M.l2_loss(x, y)
    l64, g64, _ = grads_of(f, (a, b), torch.float64)
    l32, g32, _ = grads_of(f, (a, b), torch.float32)
    name = f"l2 {shape}"
    check_scalar(name + " loss", loss.detach(), l64, l32)
    check_tensor(name + " grad", ga, g64, g32, power=trip_index(n, BWD_TRIP) if n > BWD_TRIP else trip_index(n, FWD_TRIP))
    check_scalar(name + " rmse", ops.rmse(a, b), M.rmse(a.double(), b.double()), M.rmse(a, b))
    if shape[0] > 1:
        check_scalar(name + " rmse broadcast", ops.rmse(a, b[:1]), M.rmse(a.double(), b[:1].double()), M.rmse(a, b[:1]))


# ================================================================================================ Soft dice, dsc
# 6 planes of 120 voxels (the golden's shape); V = 67,200 (a second trip within the plane); 72 planes (the finishers' second 64-plane trip)
DICE_SHAPES = [(2, 3, 6, 5, 4), (1, 2, 40, 42, 40), (2, 36, 6, 7, 9)]


@pytest.mark.parametrize("dice_factor", [1, 4])
@pytest.mark.parametrize("shape", DICE_SHAPES)
def test_soft_dice_and_dsc_vs_float64(ops, shape, dice_factor):
    """ops.soft_dice_loss with its gradient (dice_sums / dice_finalize / dice_bwd) and ops.dsc (dsc_finalize) on soft maps against binary
    targets; plane 0's target is all zero, and in the last plane input and target are both zero (the 1e-6 epsilons alone: dice 1, loss
    term 0, gradient 0).
    Observed on the MI355X, relative to float64: loss 4.4e-11 ... 2.8e-8, dsc 6.1e-9 ... 5.3e-8 (bound 1e-6); gradient 9.8e-8 ... 1.4e-7 of
    max|ref| (bound 1e-6)."""
    g = gen(sum(shape) + dice_factor)
    inp = torch.rand(shape, device=DEV, generator=g)
    tgt = (torch.rand(shape, device=DEV, generator=g) > 0.5).float()
    tgt[0, 0] = 0.0
    inp[-1, -1] = 0.0
    tgt[-1, -1] = 0.0
    V = inp[0, 0].numel()
    nplanes = shape[0] * shape[1]
    ig = inp.clone().requires_grad_(True)
    loss = ops.soft_dice_loss(ig, tgt, dice_factor)
    gi, = torch.autograd.grad(loss, [ig], grad_outputs=torch.tensor(UP, device=DEV))
    f = lambda x, t: M.soft_dice(x, t, dice_factor)
    l64, g64, _ = grads_of(f, (inp, tgt), torch.float64)
    l32, g32, _ = grads_of(f, (inp, tgt), torch.float32)
    name = f"dice {shape} f{dice_factor}"
    check_scalar(name + " loss", loss.detach(), l64, l32)
    # the last plane's gradient is exactly 0: the element with power is the first of the last plane but one (past its first trip where it has one)
    check_tensor(name + " grad", gi, g64, g32, power=(nplanes - 2) * V + (DICE_TRIP if V > DICE_TRIP else 0))
    assert bool((gi[-1, -1] == 0).all()), "input and target both zero: the gradient of that plane is exactly 0"
    if dice_factor == 1:
        check_scalar(name + " dsc", ops.dsc(inp, tgt), M.dsc(inp.double(), tgt.double()), M.dsc(inp, tgt))


# ================================================================================================ Jacobian determinant, jdet_std
# (2, 5, 7): both neighbours clamped; 274,560 voxels: the forward's second trip; 1,060,800: the backward's; (24, 20): the 2-D form
JAC_SHAPES = [(1, (2, 5, 7)), (2, (9, 11, 13)), (2, (20, 20, 20)), (1, (40, 40, 40)), (1, (66, 64, 65)), (1, (104, 100, 102)), (2, (24, 20))]
AMPLITUDES = [3.0, 3e-2, 3e-3, 3e-4]


def _jdet_refs(df, lamb, normalize):
    f = lambda d: M.jdet_std(d, lamb, normalize)
    return grads_of(f, (df,), torch.float64), grads_of(f, (df,), torch.float32)


def _jdet_std_case(ops, name, df, lamb, normalize):
    """loss and gradient of ops.jdet_std against float64 under the rule; returns the loss's (deviation, bound, fp32 reference's deviation)"""
    from pulpo_amd._lib import PulpoHipError
    (l64, g64), (l32, g32) = _jdet_refs(df, lamb, normalize)
    dg = df.clone().requires_grad_(True)
    loss = ops.jdet_std(dg, lamb, normalize)
    dev, tol = check_scalar(name + " loss", loss.detach(), l64, l32)
    if ops.DETERMINISTIC:              # float atomics: no deterministic form, the backward refuses
        with pytest.raises(PulpoHipError):
            torch.autograd.grad(loss, [dg])
        return dev, tol, M.rel(l32, l64)
    gd, = torch.autograd.grad(loss, [dg], grad_outputs=torch.tensor(UP, device=DEV))
    gtol = M.bound(g32, g64, FLOOR)
    n = df.numel() // df.shape[1]
    # at the smallest amplitudes the fp32 reference's own gradient is 1e-3 max|ref| off: the rule's bound cannot reject that much there
    power = (trip_index(n, BWD_TRIP) if n > BWD_TRIP else df.numel() - 1) if gtol < 4e-4 * amax(g64) else None
    print(f"RATIO {name} grad bound / max|ref| {gtol / amax(g64):.3g} error / max|ref| {R.ratio(gd, g64, 1.0) / amax(g64):.3g}")
    check(name + " grad", gd, g64, gtol, power)
    return dev, tol, M.rel(l32, l64)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,grid", JAC_SHAPES)
def test_jacobian_det_and_std_vs_float64(ops, B, grid, normalize):
    """the determinant map of ops.jacobian_det element by element, and ops.jdet_std with its gradient (jacdet_fwd, jdetstd_finalize,
    jdetstd_bwd: float atomics, so no bits are compared; under PULPO_DETERMINISTIC the backward refuses), on a folding field (amplitude 3).
    Observed on the MI355X over the 14 cases: determinant 1.0e-7 ... 1.8e-7 of max|ref| (bound 1e-6); loss 1.6e-10 ... 9.4e-8 relative
    (bound 1e-6); gradient 1.5e-7 ... 3.1e-7 of max|ref| against bounds of 1e-6 ... 1.7e-6, at most 0.31 of the bound."""
    df = folded_field(B, grid, 3.0).to(DEV)
    name = f"jdet {B}/{grid}/norm={normalize}"
    jd = ops.jacobian_det(df, normalize)
    n = jd.numel()
    check_tensor(name + " map", jd, M.jacobian_det(df.double(), normalize), M.jacobian_det(df, normalize), power=trip_index(n, FWD_TRIP))
    _jdet_std_case(ops, name, df, 0.3, normalize)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("amplitude", AMPLITUDES)
@pytest.mark.parametrize("B,grid", [(2, (20, 20, 20)), (1, (40, 40, 40))])
def test_jdet_std_near_the_identity_vs_float64(ops, B, grid, amplitude, normalize):
    """the `jdet` regulariser on fields from folding (amplitude 3) down to near-identity (3e-4 voxel): |std - std64| / std64 within
    max(4 x the fp32 reference's own deviation, 1e-6), the rule of test_field_quality_against_fp64, and the gradient within the same rule
    relative to max|ref|.
    With uncentred fp32 sums of J and J^2 the kernel lost the std to cancellation (J sits near 1): on the MI355X, normalised, its deviation
    was 1.2e-4 / 9.0e-3 / 1.0 (the variance clamped to 0) at amplitudes 3e-2 / 3e-3 / 3e-4 on 2 x 20^3 and 4.1e-5 / 5.2e-4 / 1.0 on 40^3,
    against bounds of 1e-6 / 3.1e-5 / 4.6e-4 and 1e-6 / 1.6e-5 / 3.6e-4 (10 of the 16 cases failed).  With the sums of J - 1 and (J - 1)^2
    kept in double: 7.8e-8 / 9.0e-8 / 3.3e-6 / 7.6e-5 at amplitudes 3 / 3e-2 / 3e-3 / 3e-4 on 2 x 20^3 and 1.6e-8 / 4.1e-8 / 1.6e-6 / 7.5e-5
    on 40^3 (the fp32 reference's own: 3.6e-9 / 1.5e-7 / 7.8e-6 / 1.1e-4 and 1.6e-8 / 6.8e-8 / 4.0e-6 / 9.0e-5), at most 0.21 of the bound
    in all 16 cases; the gradient 1.5e-7 ... 7.6e-4 of max|ref| against bounds of 1.1e-6 ... 4.9e-3, at most 0.26 of the bound."""
    df = folded_field(B, grid, amplitude).to(DEV)
    _jdet_std_case(ops, f"jdet_std {B}/{grid}/amp{amplitude:g}/norm={normalize}", df, 0.3, normalize)


def test_jdet_std_of_the_zero_field_is_zero_with_a_zero_gradient(ops):
    """J = 1 everywhere: std 0, and the backward's `sd > 0` guard gives exact zeros instead of 0 / 0"""
    dg = torch.zeros(2, 3, 9, 11, 13, device=DEV, requires_grad=True)
    loss = ops.jdet_std(dg, 0.3, True)
    assert float(loss) == 0.0
    if not ops.DETERMINISTIC:
        gd, = torch.autograd.grad(loss, [dg])
        assert bool((gd == 0).all())


@pytest.mark.parametrize("B,grid", [(2, (20, 20, 20)), (1, (40, 40, 40)), (2, (24, 20))])
def test_field_quality_and_jdet_std_agree_near_the_identity(ops, B, grid):
    """ops.field_quality's std and ops.jdet_std(df, 1.0) at amplitude 3e-3 (test_field_quality_against_fp64 compares them at amplitude 3
    only): both within the rule's bound of the float64 std, so within twice that bound of each other.
    Observed on the MI355X: both 1.6e-6 ... 3.3e-6 from float64 (bounds 4.4e-6 ... 3.1e-5, at most 0.74 of the bound, at (24, 20)); with the
    uncentred sums jdet_std was 5.2e-4 ... 1.7e-2 off."""
    df = folded_field(B, grid, 3e-3).to(DEV)
    s64, s32 = M.jdet_std(df.double(), 1.0), M.jdet_std(df, 1.0)
    _, tol = check_scalar(f"field_quality {B}/{grid} std", ops.field_quality(df)[1], s64, s32)
    check_scalar(f"jdet_std {B}/{grid} lamb=1", ops.jdet_std(df, 1.0), s64, s32)
    assert M.rel(ops.field_quality(df)[1], ops.jdet_std(df, 1.0)) <= 2 * tol


# ================================================================================================ KL_nondiagonal
# (shape, planes shifted by 100 p): the golden's shape, the minimum, both kernels' second trips at 1,088,640 elements, the D == 1 form
KLN_CASES = [((2, 3, 5, 6, 7), False), ((2, 3, 5, 6, 7), True), ((1, 3, 2, 2, 2), False), ((2, 3, 56, 60, 54), False), ((2, 3, 56, 60, 54), True),
             ((2, 2, 24, 20), False), ((2, 2, 24, 20), True)]


@pytest.mark.parametrize("shape,shifted", KLN_CASES)
def test_kl_nondiagonal_vs_float64(ops, shape, shifted):
    """ops.kl_nondiagonal with gmu and gsigma (kln_fwd / kln_finalize / kln_bwd), sigma log-uniform on [0.05, 5].  shifted: plane p of mu
    carries the offset 100 p, so a neighbour read across a plane boundary would show in the loss and in gmu.
    Observed on the MI355X, relative to float64: loss 1.5e-9 ... 8.7e-8 (bound 1e-6); gmu 7.2e-8 ... 1.5e-7, gsigma 7.7e-8 ... 1.3e-7 of
    max|ref| (bound 1e-6)."""
    g = gen(sum(shape) + shifted)
    mu = torch.randn(shape, device=DEV, generator=g)
    sg = 0.05 * 100.0 ** torch.rand(shape, device=DEV, generator=g)
    if shifted:
        mu += 100.0 * torch.arange(shape[0] * shape[1], device=DEV, dtype=torch.float32).reshape(shape[0], shape[1], *([1] * (len(shape) - 2)))
    mg, sgg = mu.clone().requires_grad_(True), sg.clone().requires_grad_(True)
    loss = ops.kl_nondiagonal(mg, sgg, 20.0)
    gm, gs = torch.autograd.grad(loss, [mg, sgg], grad_outputs=torch.tensor(UP, device=DEV))
    f = lambda m, s: M.kl_nondiagonal(m, s, 20.0)
    l64, m64, s64 = grads_of(f, (mu, sg), torch.float64)
    l32, m32, s32 = grads_of(f, (mu, sg), torch.float32)
    name = f"kln {shape} shifted={shifted}"
    n = mu.numel()
    V = mu[0, 0].numel()
    check_scalar(name + " loss", loss.detach(), l64, l32)
    # gmu: the first element of the last plane (its lower neighbours belong to the plane before); gsigma: the second trip, or the last element
    check_tensor(name + " gmu", gm, m64, m32, power=n - V)
    check_tensor(name + " gsigma", gs, s64, s32, power=trip_index(n, BWD_TRIP))
    if n > BWD_TRIP:
        assert R.ratio(gm, R.perturbed(m64, BWD_TRIP), M.bound(m32, m64, FLOOR)) > 1.0


# ================================================================================================ percent_leq0, warp_landmarks
def test_percent_leq0_counts_exactly_past_the_first_trip(ops):
    """270,336 elements, one past the first trip: 1000 zeros, 777 negative zeros and 4321 negatives at known places (the first and last
    element and the first of the second trip among them), the rest positive down to the smallest normal number"""
    n = 64 * 66 * 64
    x = torch.rand(n, device=DEV, generator=gen(1)) + 0.5
    x[5::1000] = torch.finfo(torch.float32).tiny
    perm = torch.randperm(n, device=DEV, generator=gen(2))
    head = torch.tensor([0, n - 1, FWD_TRIP], device=DEV)
    perm = torch.cat([head, perm[~torch.isin(perm, head)]])
    x[perm[:1000]] = 0.0
    x[perm[1000:1777]] = -0.0
    x[perm[1777:6098]] = -torch.rand(4321, device=DEV, generator=gen(3)) - 1e-30
    count = 6098
    assert int((x <= 0).sum()) == count and float(x[0]) == 0.0 and float(x[n - 1]) == 0.0 and float(x[FWD_TRIP]) == 0.0
    pct = ops.percent_leq0(x.reshape(1, 64, 66, 64))
    assert pct.dim() == 0 and pct.dtype == torch.float32
    got = float(pct) * n / 100.0
    print(f"RATIO percent_leq0 count {got:.3f} of {count}")
    assert round(got) == count and abs(got - count) < 0.01
    assert abs(float(pct) - M.percent_leq0(x)) <= 2 * 2.0 ** -23 * M.percent_leq0(x)        # (count / n) and * 100 round once each


def _landmarks(g, size, nlm):
    """(1, nlm, ndims) float coordinates: every axis' last valid index, 0, -1 and -S (which wrap), fractions that truncate toward zero
    (3.9 -> 3, -0.5 -> 0, -1.5 -> -1), the rest random on [-S, S)"""
    nd = len(size)
    S = torch.tensor(size, device=DEV, dtype=torch.float32)
    lm = torch.floor((torch.rand(nlm, nd, device=DEV, generator=g) * 2 - 1) * S).clamp(min=-S, max=S - 1)
    lm[0] = S - 1
    lm[1] = -S
    lm[2] = -1.0
    lm[3] = 0.0
    lm[4] = torch.tensor([3.9, -0.5, -1.5], device=DEV)[:nd]
    lm[5] = S - 0.01
    return lm[None]


@pytest.mark.parametrize("size", [(6, 7, 9), (11, 13)])
def test_warp_landmarks_of_many_pairs_vs_float64(ops, size):
    """40 landmarks on 5 samples: 200 (landmark, sample) pairs, two blocks of the kernel.  One fp32 subtraction per element: 2^-23 max|ref|"""
    g = gen(len(size))
    nd = len(size)
    df = torch.randn(5, nd, *size, device=DEV, generator=g) * 3
    lm = _landmarks(g, size, 40)
    out = ops.warp_landmarks(lm, df)
    ref = M.warp_landmarks(lm.double(), df.double())
    assert ref.shape == (5, 40, nd)
    check(f"landmarks {size}", out, ref, 2.0 ** -23 * amax(ref))
    check(f"landmarks {size} host lm", ops.warp_landmarks(lm.cpu(), df), ref, 2.0 ** -23 * amax(ref), power=128 * nd)
    for k, c, v in ((39, nd - 1, float(size[-1])), (17, 0, float(-size[0] - 1)), (0, 1, size[1] + 0.5)):
        bad = lm.clone()
        bad[0, k, c] = v
        with pytest.raises(IndexError):
            ops.warp_landmarks(bad, df)


# ================================================================================================ streaming moments
def _fold(ops, stack):
    sm = ops.StreamingMoments()
    for s in stack:
        sm.update(s)
    return sm


def test_streaming_moments_past_the_first_trip_vs_float64(ops):
    """3 samples of (1, 3, 90, 90, 90) = 2,187,000 elements: mc_update's second trip; mean, M2 and the std map against the float64 stack.
    Observed on the MI355X: mean 7.7e-8, M2 8.5e-8, std map 1.2e-7 of max|ref| (bounds 1e-6; torch's fp32: 1.2e-7, 9.5e-8, 1.4e-7)."""
    g = gen(9)
    stack = torch.randn(3, 1, 3, 90, 90, 90, device=DEV, generator=g) * 3 + 1.5
    sm = _fold(ops, stack)
    s64 = stack.double()
    dev2 = lambda t: ((t - t.mean(dim=0)) ** 2).sum(dim=0)
    check_tensor("moments 90^3 mean", sm.mean(), s64.mean(dim=0), stack.mean(dim=0), power=MOM_TRIP)
    check_tensor("moments 90^3 m2", sm.m2(), dev2(s64), dev2(stack), power=MOM_TRIP)
    check_tensor("moments 90^3 std_map", sm.std_map()[0], M.mc_std_map(s64[:, 0]), M.mc_std_map(stack[:, 0]))


def test_streaming_moments_of_a_large_mean_vs_float64(ops):
    """64 samples whose mean (1e3) is large beside their spread (1e-2), against the float64 std of the stack; the bound comes from torch's
    own fp32 std of the same stack (a fp32 reference is not adequate here).
    Observed on the MI355X: std map 1.7e-3 of max|ref|, twice torch's own fp32 deviation of 8.5e-4 (fp32 Welford steps round the running
    mean to 6e-5, beside a spread of 1e-2), 0.49 of the bound 3.4e-3; mean 2.6e-7 of max|ref| (bound 1e-6)."""
    g = gen(10)
    stack = 1e3 + 1e-2 * torch.randn(64, 1, 3, 6, 7, 9, device=DEV, generator=g)
    sm = _fold(ops, stack)
    s64 = stack.double()
    check_tensor("moments large-mean mean", sm.mean(), s64.mean(dim=0), stack.mean(dim=0))
    # torch's own fp32 std is 8.5e-4 of max|ref| off here, so the rule's bound (3.4e-3) cannot reject a 1e-3 max|ref| error: no power check
    e, b = check_tensor("moments large-mean std_map", sm.std_map()[0], M.mc_std_map(s64[:, 0]), M.mc_std_map(stack[:, 0]), power=None)
    print(f"RATIO moments large-mean: std map error {e:.3g} of max|ref|, bound {b:.3g}")


def test_streaming_moments_masked_std_map_of_a_batch_vs_float64(ops):
    """B = 2 with a per-voxel scale (B, 1, D, H, W), zeros and negative weights among it: std(m x) = |m| std(x) per batch row"""
    g = gen(11)
    stack = torch.randn(5, 2, 3, 6, 7, 9, device=DEV, generator=g) * 2 - 0.5
    scale = (torch.rand(2, 1, 6, 7, 9, device=DEV, generator=g) > 0.3).float() * (torch.rand(2, 1, 6, 7, 9, device=DEV, generator=g) * 2 - 1)
    sm = _fold(ops, stack)
    ref = lambda st, sc: torch.stack([M.mc_std_map(st[:, b], sc[b]) for b in range(2)])
    check_tensor("moments masked std_map", sm.std_map(scale=scale), ref(stack.double(), scale.double()), ref(stack, scale), power=6 * 7 * 9)
    check_tensor("moments B2 std_map", sm.std_map(), ref(stack.double(), torch.ones_like(scale).double()), ref(stack, torch.ones_like(scale)),
                 power=6 * 7 * 9)


# ================================================================================================ Adam
# tails of 1, 2 and 3 elements beside the float4 body, no body at all (n < 4), and a second trip of the body with a tail of 3
ADAM_SIZES = [1, 2, 3, 5, 1003, ADAM_TRIP + 1203]


def _adam_grad(g, n, step):
    gr = torch.randn(n, device=DEV, generator=g)
    gr[step::7] = 0.0                     # exact zeros: with zero moments, 0 / (sqrt(0) + eps) = 0 and p stays
    gr[step + 3::11] = 1e-12              # v = 1e-27 (1 - beta2): sqrt(v) far below eps
    return gr


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_vs_float64(ops, n, gscale):
    """three consecutive ops.adam_step from zero moments, then one at step 1000 from non-zero moments: p, m and v element by element
    against the float64 Adam on the same fp32 gradients, each chain carrying its own state; the bound from the fp32 evaluation of the same
    reference.  At the gradients of 1e-12 m and v are also held to 1e-6 of their own value after the first step.
    The kernel took 1 - beta from the fp32 betas (1 - (float)0.999 is 1.3e-5 off 0.001): on the MI355X v was 1.3e-5 of max|ref| off and m
    2.1e-7 ... 2.8e-7, against the bound 1e-6 (all 12 cases failed).  With 1 - beta formed in double: p 8.3e-10 ... 1.1e-7, m 4.3e-9 ...
    9.0e-8, v 4.1e-10 ... 1.9e-7 of max|ref| (the fp32 reference's own: up to 1.1e-7, 1.1e-7 and 1.9e-7)."""
    g = gen(n % 1000 + int(gscale * 10))
    lr = 1e-3
    p = torch.randn(n, device=DEV, generator=g)
    state = {torch.float32: [p.clone(), torch.zeros_like(p), torch.zeros_like(p)],
             torch.float64: [p.double(), torch.zeros_like(p).double(), torch.zeros_like(p).double()]}
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pw = ADAM_TRIP if n > ADAM_TRIP else n - 1

    def compare(tag):
        for k, (name, got) in enumerate((("p", p), ("m", m), ("v", v))):
            check_tensor(f"adam n={n} gscale={gscale} {tag} {name}", got, state[torch.float64][k], state[torch.float32][k], power=pw if k == 0 else n - 1)

    for step in (1, 2, 3):
        gr = _adam_grad(g, n, step)
        ops.adam_step(p, gr, m, v, lr, step, gscale=gscale)
        for dt in state:
            state[dt] = list(M.adam_ref(*state[dt][:1], gr.to(dt), *state[dt][1:], lr, step, gscale=gscale))
        compare(f"step {step}")
        if step == 1:
            tiny = gr == 1e-12
            for got, ref in ((m, state[torch.float64][1]), (v, state[torch.float64][2])):
                if bool(tiny.any()):
                    assert float(((got[tiny].double() - ref[tiny]).abs() / ref[tiny]).max()) <= FLOOR
            zero = gr == 0
            assert torch.equal(p[zero], state[torch.float64][0][zero].float()) and bool((m[zero] == 0).all()) and bool((v[zero] == 0).all())
    m = torch.randn(n, device=DEV, generator=g) * 0.1
    v = torch.rand(n, device=DEV, generator=g) * 0.01
    state = {dt: [p.to(dt, copy=True), m.to(dt, copy=True), v.to(dt, copy=True)] for dt in state}
    gr = _adam_grad(g, n, 0)
    ops.adam_step(p, gr, m, v, lr, 1000, gscale=gscale)
    for dt in state:
        state[dt] = list(M.adam_ref(*state[dt][:1], gr.to(dt), *state[dt][1:], lr, 1000, gscale=gscale))
    compare("step 1000")


# ================================================================================================ the optional terms of one step
def test_optional_loss_terms_of_the_step_vs_float64():
    """a T3 / L2 model at 16^3 with regularizer="jdet", nondiagonal=True and recon_loss=["mse", "dice"] under fixed noise: the
    regularisation, KL and reconstruction terms of _forward_and_losses are the float64 references evaluated on the model's own outputs
    (final_dfs; mus, sigmas; y_hat and the warped segmentations), rtol 1e-4.
    Observed on the MI355X: regularisation 9.0e-8, KL 2.5e-8, reconstruction 4.0e-9 (with the uncentred jdet sums the regularisation term
    was 1.2e-6 off, inside this test's 1e-4: the near-identity test above is the one that shows that defect)."""
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    torch.manual_seed(0)
    model = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=list(O.FEEDBACK_DEFAULT), n0=2, recon_loss=["mse", "dice"], regularizer="jdet", segs=True,
                         nondiagonal=True, dice_factor=4).cuda().train()
    g = torch.Generator().manual_seed(4)
    for l in range(2):
        s = 16 // 2 ** (l + 1)
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=g).cuda())
    x, y = torch.rand(1, 1, 16, 16, 16, generator=g).cuda(), torch.rand(1, 1, 16, 16, 16, generator=g).cuda()
    seg_x, seg_y = (torch.rand(1, 1, 16, 16, 16, generator=g) > 0.5).float().cuda(), (torch.rand(1, 1, 16, 16, 16, generator=g) > 0.5).float().cuda()
    outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y, seg_x, seg_y)
    mus, sigmas, final_dfs, y_hat = outs[0], outs[1], outs[6], outs[7]
    with torch.no_grad():
        y_hat_seg = model.transform_segmentation(final_dfs, seg_x)
    d = lambda t: t.detach().double()
    ref_reg = sum(w * M.jdet_std(d(final_dfs[l]), model.hparams.lamb, True) for l, w in model.hierarchical_regularization.weight_dict.items())
    ref_kl = model.beta * sum(w * M.kl_nondiagonal(d(mus[l]), d(sigmas[l]), 20.0) for l, w in model.hierarchical_kl_loss.weight_dict.items())
    ref_rec = 0.0
    for l, w in model.hierarchical_recon_loss.weight_dict.items():
        size = tuple(y_hat[l].shape[2:])
        ref_rec = ref_rec + (w * M.l2_loss(d(y_hat[l]), R.resize_ref(d(y), size))
                             + w * M.soft_dice(d(y_hat_seg[l]), R.resize_ref(d(seg_y), tuple(y_hat_seg[l].shape[2:])), 4)) / 2
    for name, got, ref in (("reg", reg, ref_reg), ("kl", kl, ref_kl), ("rec", rec, ref_rec)):
        print(f"RATIO step {name} {M.rel(got, ref) / 1e-4:.3g}   (deviation {M.rel(got, ref):.3g})")
    for name, got, ref in (("reg", reg, ref_reg), ("kl", kl, ref_kl), ("rec", rec, ref_rec)):
        assert M.rel(got, ref) <= 1e-4, (name, float(got), float(ref))
    total.backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
