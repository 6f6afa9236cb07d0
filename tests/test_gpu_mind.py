"""The MIND-SSC similarity term on the GPU: ops.mind_descriptor / mind_loss / mind_loss_masked against the float64
definition of tests/mind_ref.py (evaluated with plain torch ops on the GPU), its way through the loss module, the model's step and the
score table.

Inputs are uniform noise and uniform noise passed twice through the clamped 3^3 box mean: both free of ties in min_j D_j.  (Smooth
synthetic anatomy with a zero background has exact ties, where fp32 and fp64 pick different arg-min channels and the gradient is a
sub-gradient: such data is compared by value only.)

Bounds.  Loss and gradient: those of test_gpu_pyramid_ops.test_ncc_vs_float64 - loss 1e-4 |ref|, gradient 5e-5 max|ref| element by
element with an upstream factor of 1.7, each gradient comparison shown to reject the reference with one element moved by 1e-3 max|ref|.
Descriptor: DESC_TOL = 9.2e-6 absolute, element by element = 8 x 1.15e-6, the largest error of an fp32 CPU evaluation of
mind_ref.descriptor over CASES x both inputs x both seeds (the factor leaves room for the device's exp and another summation order; a
host build of the kernels' own arithmetic reached 1.7e-6 on the same inputs; the MI355X 0.24 of the bound).  Every comparison prints a RATIO line: pytest -s."""
import functools
import os

import pytest
import torch

import masked_ref as K
import mind_ref as M
import pyramid_ref as R
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
SIZE = [16, 16, 16]
DESC_TOL = 9.2e-6

# (B, size, dilation): every voxel on a face; extents at d + 1 and W past one wave; an extent below d, W one past 64, a batch boundary; the
# coarsest pyramid level; several tiles; one past the 8 x 8 x 32 tile (d = 2), the 4 x 8 x 32 tile (d = 3: two staged images with a halo
# of 4 no longer fit 64 KiB at 8 x 8 x 32) and the 8 x 8 x 16 tile of volumes with W <= 16
CASES = [(2, (5, 6, 7), 1), (1, (3, 4, 70), 2), (2, (2, 9, 65), 3), (1, (10, 10, 10), 3), (1, (20, 24, 20), 2), (1, (9, 9, 33), 2), (1, (5, 9, 33), 3),
         (1, (9, 9, 9), 1)]
MASK_CASES = [(2, (5, 6, 7), 1), (1, (20, 24, 20), 2)]
MASKS = ["ones", "ball", "rand", "ball_x_rand"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb


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


@functools.lru_cache(maxsize=None)
def _data(B, size, smooth):
    """(pred, true) in fp32 on the device, made once and left unchanged; the float64 reference sees the same fp32 values"""
    return M.noise(B, size, 1, smooth).float().to(DEV), M.noise(B, size, 2, smooth).float().to(DEV)


@functools.lru_cache(maxsize=None)
def _mask_planes(B, size):
    g = torch.Generator().manual_seed(7 + size[2])
    ball = K.ball(B, size, device=DEV)
    assert 0 < float(ball.sum()) < ball.numel()
    return {"ones": torch.ones(B, 1, *size, device=DEV), "ball": ball, "rand": torch.rand(B, 1, *size, generator=g).to(DEV)}


def _masks(B, size, kind):
    d = _mask_planes(B, size)
    return (d["ball"], d["rand"]) if kind == "ball_x_rand" else (d[kind], None)


def _run(ops, p, t, dil, mask=None, mask2=None, up=1.7):
    pg = p.clone().requires_grad_(True)
    loss = ops.mind_loss(pg, t, dil) if mask is None else ops.mind_loss_masked(pg, t, mask, mask2, dil)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    gp, = torch.autograd.grad(loss, [pg], grad_outputs=torch.tensor(up, device=DEV))
    return loss.detach(), gp


# ================================================================================================ operators against float64
@pytest.mark.parametrize("smooth", [0, 2])
@pytest.mark.parametrize("B,size,dil", CASES)
def test_descriptor_vs_float64(ops, B, size, dil, smooth):
    p, _ = _data(B, size, smooth)
    f = ops.mind_descriptor(p, dil)
    assert f.shape == (B, 12) + tuple(size) and f.dtype == torch.float32
    ref = M.descriptor(p.double(), dil)
    check(f"descriptor {B}/{size}/d{dil}/s{smooth}", f, ref, DESC_TOL, power=None)
    assert R.ratio(f, R.perturbed(ref, -1, 1e-4), DESC_TOL) > 1.0                     # an error of 1e-4 in one element is rejected
    assert float(f.max(dim=1).values.min()) == 1.0 and float(f.min()) > 0.0
    check(f"descriptor of 1 - I {B}/{size}/d{dil}/s{smooth}", ops.mind_descriptor(1.0 - p, dil), ref, DESC_TOL, power=None)


@pytest.mark.parametrize("smooth", [0, 2])
@pytest.mark.parametrize("B,size,dil", CASES)
def test_loss_and_gradient_vs_float64(ops, B, size, dil, smooth):
    p, t = _data(B, size, smooth)
    loss, gp = _run(ops, p, t, dil)
    ref = M.loss(p.double(), t.double(), dil)
    name = f"mind {B}/{size}/d{dil}/s{smooth}"
    check(f"{name} loss", loss, ref, 1e-4 * abs(float(ref)), power=None)
    rg = M.grad(p.double(), t.double(), dil, upstream=1.7)
    check(f"{name} grad", gp, rg, 5e-5 * amax(rg))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,size,dil", MASK_CASES)
def test_masked_loss_and_gradient_vs_float64(ops, B, size, dil, kind):
    p, t = _data(B, size, 0)
    mask, mask2 = _masks(B, size, kind)
    loss, gp = _run(ops, p, t, dil, mask, mask2)
    m64 = [None if m is None else m.double() for m in (mask, mask2)]
    ref = M.loss_masked(p.double(), t.double(), *m64, dilation=dil)
    name = f"mind_masked {B}/{size}/d{dil}/{kind}"
    check(f"{name} loss", loss, ref, 1e-4 * abs(float(ref)), power=None)
    rg = M.grad(p.double(), t.double(), dil, mask=m64[0], mask2=m64[1], upstream=1.7)
    last = int(torch.nonzero(K.product(mask, mask2).reshape(-1) > 0).reshape(-1)[-1])
    check(f"{name} grad", gp, rg, 5e-5 * amax(rg), power=last)
    if kind == "ones":               # ones reproduce the unmasked loss
        loss0, gp0 = _run(ops, p, t, dil)
        assert abs(float(loss) - float(loss0)) <= 1e-6 * abs(float(loss0))
        assert amax(gp - gp0) <= 1e-6 * amax(gp0)
    if mask2 is not None:            # two masks are their product mask
        loss1, gp1 = _run(ops, p, t, dil, mask * mask2, None)
        assert abs(float(loss1) - float(loss)) <= 1e-6 * abs(float(loss))
        assert amax(gp1 - gp) <= 1e-6 * amax(gp)


@pytest.mark.parametrize("B,size,dil", MASK_CASES)
def test_zero_mask_gives_exactly_zero(ops, B, size, dil):
    p, t = _data(B, size, 0)
    zero = torch.zeros_like(p)
    for mask, mask2 in ((zero, None), (torch.ones_like(p), zero)):
        loss, gp = _run(ops, p, t, dil, mask, mask2)
        assert float(loss) == 0.0 and not bool(gp.any()) and bool(torch.isfinite(gp).all())


def test_only_pred_gets_a_gradient(ops):
    p, t = _data(2, (5, 6, 7), 0)
    pg, tg = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    mg = torch.ones_like(p).requires_grad_(True)
    gp, gt, gm = torch.autograd.grad(ops.mind_loss_masked(pg, tg, mg, None, 1), [pg, tg, mg], allow_unused=True)
    assert gp is not None and gt is None and gm is None


def test_backward_is_bit_identical_run_to_run(ops):
    """the default mode: no atomics anywhere, so PULPO_DETERMINISTIC needs no second path"""
    B, size, dil = 1, (20, 24, 20), 2
    p, t = _data(B, size, 0)
    mask, mask2 = _masks(B, size, "ball_x_rand")
    for args in ((), (mask, mask2)):
        l1, g1 = _run(ops, p, t, dil, *args)
        l2, g2 = _run(ops, p, t, dil, *args)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_aligned_beats_shifted_under_inverted_contrast_and_mse_does_not(ops):
    a, inv, sh = (v.float().to(DEV) for v in M.shifted_pair())
    aligned, shifted = float(ops.mind_loss(a, inv, 2)), float(ops.mind_loss(sh, inv, 2))
    print(f"mind aligned {aligned:.3g} shifted {shifted:.3g}")
    assert shifted > 100.0 and shifted > M.SHIFT_FACTOR * aligned
    assert float(ops.l2_loss(sh, inv)) < float(ops.l2_loss(a, inv))


def test_values_on_synthetic_anatomy(ops):
    """multimodal_pair (ties in min_j D_j on its smooth texture and zero background): values only - loss to 1e-4, descriptor within DESC_TOL;
    the gradient is finite and zero on the background beyond the reach of the head"""
    from pulpo_amd import synthetic
    x, y = synthetic.multimodal_pair((20, 24, 20), 1, 3, DEV)
    assert float(y.max()) <= 1.0 and float(y.min()) >= 0.0
    loss, gp = _run(ops, x, y, 2)
    ref = M.loss(x.double(), y.double(), 2)
    check("mind multimodal loss", loss, ref, 1e-4 * abs(float(ref)), power=None)
    check("descriptor multimodal", ops.mind_descriptor(y, 2), M.descriptor(y.double(), 2), DESC_TOL, power=None)
    assert bool(torch.isfinite(gp).all()) and amax(gp) > 0.0
    assert float(ops.mind_loss(torch.zeros_like(x), torch.zeros_like(x))) == 0.0


def test_argument_errors(ops):
    from pulpo_amd._lib import PulpoHipError
    p, t = _data(2, (5, 6, 7), 0)
    with pytest.raises(PulpoHipError):
        ops.mind_loss(p, t, 0)
    with pytest.raises(PulpoHipError):
        ops.mind_loss(p, t, 2, eps=0.0)
    with pytest.raises(PulpoHipError):
        ops.mind_descriptor(p[:, :, :1], 2)                                          # an extent below 2
    with pytest.raises(NotImplementedError, match="3-D"):
        ops.mind_loss(p[:, :, 0], t[:, :, 0])
    with pytest.raises(ValueError):
        ops.mind_loss_masked(p, t, torch.ones(2, 1, 5, 6, 8, device=DEV))
    with pytest.raises(PulpoHipError):
        ops.mind_loss_masked(p, t, torch.ones(2, 1, 5, 6, 7))                        # a CPU mask


# ================================================================================================ loss module, step, score table
def _model(api, recon, mask=False, train=True, **kw):
    """T3 / L2 / n0 = 4 at 16^3, the same weights and noise for every call"""
    models, nb = api
    torch.manual_seed(0)
    m = models.PULPo(3, 2, 0.1, SIZE, feedback=FB, n0=4, recon_loss=list(recon), mask=mask, **kw).cuda()
    m = m.train() if train else m.eval()
    g = torch.Generator().manual_seed(4)
    for l in range(2):
        s = 16 // 2 ** (l + 1)
        m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=g).cuda())
    return m


@functools.lru_cache(maxsize=None)
def _pair():
    from pulpo_amd import synthetic
    x, y = synthetic.uniform_pair(SIZE, 1, 8, DEV)
    return x, y, K.ball(1, SIZE, device=DEV), K.ball(1, SIZE, outer=0.8, inner=0.2, device=DEV)


def _ref_levels(model, outs, y, mask_x=None, mask_y=None, ncc=False):
    """{l: w_l * term_l} in float64 on the step's own y_hat (and final_dfs for the level masks)"""
    final_dfs, y_hat = outs[6], outs[7]
    rl = model.hierarchical_recon_loss
    res = {}
    for l, w in rl.weight_dict.items():
        size = tuple(y_hat[l].shape[2:])
        target = R.resize_ref(y.double(), size)
        pred = y_hat[l].detach().double()
        if mask_x is None and mask_y is None:
            term = M.loss(pred, target, rl.mind_dilation, rl.mind_eps)
        else:
            wx = R.warp_ref(final_dfs[l].detach().double(), mask_x.double()) if mask_x is not None else None
            wy = R.resize_ref(mask_y.double(), size) if mask_y is not None else None
            ma, mb = (wx, wy) if wx is not None else (wy, None)
            term = M.loss_masked(pred, target, ma, mb, rl.mind_dilation, rl.mind_eps)
        if ncc:
            term = (term + R.ncc_ref(pred, target, rl.window_size[l], model.hparams.gamma)) / 2
        res[l] = w * term
    return res


@pytest.mark.parametrize("masked", [False, True])
def test_step_with_the_mind_term(api, masked):
    """every per-level reconstruction term is w_l x mind_ref.loss (the masked form with ball masks) on the step's own y_hat[l] and resized y
    (rtol 1e-4, the step bound of test_gpu_masks); training_step's gradients are finite and reach the velocity-field convolutions"""
    x, y, ball_x, ball_y = _pair()
    mx, my = (ball_x, ball_y) if masked else (None, None)
    model = _model(api, ["mind"], mask=masked)
    assert model.hparams.mind_dilation == 2
    outs, _, (total, kl, rec, reg), (_, rec_levels, _) = model._forward_and_losses(x, y, None, None, mx, my)
    ref = _ref_levels(model, outs, y, mx, my)
    assert rec_levels.keys() == ref.keys() and len(ref) == 2
    for l in ref:
        r = abs(float(rec_levels[l]) - float(ref[l])) / (1e-4 * abs(float(ref[l])))
        print(f"RATIO step mind{' masked' if masked else ''} level {l} {r:.3g}")
        assert r <= 1.0, (l, float(rec_levels[l]), float(ref[l]))
    assert abs(float(rec) - sum(float(v) for v in ref.values())) <= 1e-4 * abs(float(rec))
    model.zero_grad(set_to_none=True)
    model.training_step((x, y, None, None, None, None, mx, my), 0).backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    flow = [k for k in grads if "velocity_field" in k and k.endswith("weight")]
    assert flow and all(amax(grads[k]) > 0.0 for k in flow), flow


def test_step_with_ncc_and_mind(api):
    x, y, _, _ = _pair()
    model = _model(api, ["ncc", "mind"], mind_dilation=1)
    assert model.hierarchical_recon_loss.mind_dilation == 1
    outs, _, (total, kl, rec, reg), (_, rec_levels, _) = model._forward_and_losses(x, y)
    ref = _ref_levels(model, outs, y, ncc=True)
    for l in ref:
        assert abs(float(rec_levels[l]) - float(ref[l])) <= 1e-4 * abs(float(ref[l])), (l, float(rec_levels[l]), float(ref[l]))
    total.backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def test_ncc_step_is_unchanged_by_the_new_keywords(api):
    """recon_loss=["ncc"] keeps its bits whatever the MIND hyper-parameters are"""
    from pulpo_amd import ops
    x, y, _, _ = _pair()
    env_det = os.environ.get("PULPO_DETERMINISTIC", "0") == "1"
    ops.set_deterministic(True)
    try:
        res = []
        for kw in ({}, {"mind_dilation": 3, "mind_eps": 1e-3}):
            model = _model(api, ["ncc"], **kw)
            total = model._forward_and_losses(x, y)[2][0]
            total.backward()
            res.append((total.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    finally:
        ops.set_deterministic(env_det)
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])


def test_performance_mind_row(api):
    from pulpo_amd import evaluation
    x, y, _, _ = _pair()
    model = _model(api, ["mind"], train=False)
    plain = evaluation.performance(model, x, y)
    res = evaluation.performance(model, x, y, mind=True)
    assert set(res) == set(plain) | set(evaluation.MIND_METRICS)
    for k in plain:
        for l in plain[k]:
            assert torch.equal(plain[k][l], res[k][l]), (k, l)
    outputs, _ = model.predict_deterministic(x, y)
    for l, out in outputs.items():
        size = tuple(out.shape[2:])
        vox = size[0] * size[1] * size[2]
        ref = float(M.loss(out.detach().double(), R.resize_ref(y.double(), size), 2)) / vox
        got = res["MIND"][l]
        assert got.is_cuda and got.dim() == 0
        print(f"RATIO performance MIND level {l} {abs(float(got) - ref) / (1e-4 * abs(ref)):.3g}")
        assert abs(float(got) - ref) <= 1e-4 * abs(ref), (l, float(got), ref)
    res3 = evaluation.performance(model, x, y, mind=True, mind_dilation=1)
    assert float(res3["MIND"][0]) != float(res["MIND"][0])
