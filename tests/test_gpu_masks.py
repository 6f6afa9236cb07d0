"""Cost-function masking on the GPU: ops.ncc_loss_masked / l2_loss_masked / rmse_masked against the float64
definitions of tests/masked_ref.py (evaluated with plain torch ops on the GPU), the special masks (ones, zeros, bounded support), the
masks' way through the model's step and through the score table.

Bounds are those of test_gpu_pyramid_ops.test_ncc_vs_float64 on random images: loss 1e-4 |ref|, gradient 5e-5 max|ref| element by
element, each comparison shown to reject the reference with one voxel of the mask's last plane moved by 1e-3 max|ref|.  An fp32
evaluation of the same formula on a CPU stayed below 8e-7 (loss) and 9e-6 max|ref| (gradient) on every case and mask below.  Every
comparison prints a RATIO line (error / bound): pytest -s."""
import functools
import os

import pytest
import torch

import masked_ref as M
import pyramid_ref as R
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
GAMMA = 0.05


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


# (B, size, window): W = 2 (64 - 2 pad) and one past it (wave segments of the W pass); an extent below the pad (D = 3, w = 11); w = 13 (the
# tap-form kernels: box_axis / ncc_final<MASKED> / ncc_bwd_final); H = 1 (no march for the H pass); D = 1 (2-D window count); a voxel count
# that straddles the batch boundary; two pyramid level shapes
CASES = [(2, (4, 5, 112), 9), (2, (4, 5, 113), 9), (1, (3, 12, 70), 11), (1, (10, 12, 40), 13), (2, (6, 1, 70), 5), (2, (1, 20, 130), 7),
         (2, (17, 19, 23), 7), (1, (24, 28, 20), 3), (1, (40, 40, 40), 5)]
MASKS = ["ones", "ball", "rand", "ball_x_rand"]


@functools.lru_cache(maxsize=None)
def _data(B, size, win):
    """uniform random images and the mask planes of one case, made once and left unchanged"""
    g = torch.Generator(device=DEV).manual_seed(win * 1000 + size[2] + B)
    p, t = torch.rand(B, 1, *size, device=DEV, generator=g), torch.rand(B, 1, *size, device=DEV, generator=g)
    ball = M.ball(B, size, device=DEV)
    assert 0 < float(ball.sum()) < ball.numel()
    return p, t, {"ones": torch.ones_like(p), "ball": ball, "rand": torch.rand(B, 1, *size, device=DEV, generator=g)}


def _masks(d, kind):
    return (d["ball"], d["rand"]) if kind == "ball_x_rand" else (d[kind], None)


def _last_counted(mask, mask2) -> int:
    """flat index of the last voxel with m > 0: a voxel of the mask's last plane"""
    return int(torch.nonzero(M.product(mask, mask2).reshape(-1) > 0).reshape(-1)[-1])


def _run(ops, p, t, mask, mask2, win, up=1.7):
    pg = p.clone().requires_grad_(True)
    loss = ops.ncc_loss_masked(pg, t, mask, mask2, win, GAMMA)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    gp, = torch.autograd.grad(loss, [pg], grad_outputs=torch.tensor(up, device=DEV))
    return loss.detach(), gp


# ================================================================================================ operators against float64
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,size,win", CASES)
def test_ncc_masked_vs_float64(ops, B, size, win, kind):
    p, t, d = _data(B, size, win)
    mask, mask2 = _masks(d, kind)
    loss, gp = _run(ops, p, t, mask, mask2, win)
    m64 = [None if m is None else m.double() for m in (mask, mask2)]
    ref = M.ncc_masked_ref(p.double(), t.double(), *m64, win, GAMMA)
    name = f"ncc_masked {B}/{size}/w{win}/{kind}"
    check(f"{name} loss", loss, ref, 1e-4 * abs(float(ref)))
    rg = 1.7 * M.ncc_masked_grad_ref(p.double(), t.double(), *m64, win, GAMMA)
    check(f"{name} grad", gp, rg, 5e-5 * amax(rg), power=_last_counted(mask, mask2))
    if mask2 is not None:           # the same weights as one product mask
        loss1, gp1 = _run(ops, p, t, mask * mask2, None, win)
        assert abs(float(loss1) - float(loss)) <= 1e-6 * abs(float(loss))
        assert amax(gp1 - gp) <= 1e-6 * amax(gp)


SQ_CASES = [(2, (17, 19, 23)), (1, (24, 28, 20)), (2, (6, 1, 70))]


@pytest.mark.parametrize("kind", ["rand", "ball_x_rand"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B,size", SQ_CASES)
def test_l2_and_rmse_masked_vs_float64(ops, B, size, C, kind):
    """values and gradients within 1e-5 max(1, |ref|) (the bound of the head / L2 tests of test_gpu_pyramid_ops); the mask is broadcast
    over the channels and its sum counted once per voxel"""
    g = torch.Generator(device=DEV).manual_seed(C * 100 + size[2] + B)
    a, b = torch.rand(B, C, *size, device=DEV, generator=g), torch.rand(B, C, *size, device=DEV, generator=g)
    d = {"ball": M.ball(B, size, device=DEV), "rand": torch.rand(B, 1, *size, device=DEV, generator=g)}
    mask, mask2 = _masks(d, kind)
    m64 = [None if m is None else m.double() for m in (mask, mask2)]
    name = f"{B}/{size}/C{C}/{kind}"
    # channel 0 of the last batch row, at the last voxel the mask counts
    power = ((B - 1) * C) * (a.numel() // (B * C)) + _last_counted(mask[-1:], None if mask2 is None else mask2[-1:])
    for fn, reffn in ((ops.l2_loss_masked, M.l2_masked_ref), (lambda *x: ops.rmse_masked(*x)[0], lambda *x: M.rmse_masked_ref(*x)[0])):
        ag = a.clone().requires_grad_(True)
        val = fn(ag, b, mask, mask2)
        assert val.dim() == 0 and val.dtype == torch.float32
        ga, = torch.autograd.grad(val, [ag], grad_outputs=torch.tensor(1.7, device=DEV))
        a64 = a.double().requires_grad_(True)
        ref = reffn(a64, b.double(), *m64)
        rga, = torch.autograd.grad(ref, [a64], grad_outputs=torch.tensor(1.7, dtype=torch.float64, device=DEV))
        kindname = "l2_masked" if fn is ops.l2_loss_masked else "rmse_masked"
        check(f"{kindname} {name} value", val.detach(), ref.detach(), 1e-5 * max(1.0, abs(float(ref.detach()))))
        check(f"{kindname} {name} grad", ga, rga, 1e-5 * max(1.0, amax(rga)), power=None)
        # power of the gradient comparison on the gradient's own scale (max(1, .) would hide a 1e-3 max|ref| error of a small gradient)
        check(f"{kindname} {name} grad(own scale)", ga, rga, 1e-5 * amax(rga), power=power)
    frac = ops.rmse_masked(a, b, mask, mask2)[1]
    ref_frac = M.rmse_masked_ref(a.double(), b.double(), *m64)[1]
    check(f"mask_frac {name}", frac, ref_frac, 1e-5 * max(1.0, abs(float(ref_frac))))


# ================================================================================================ special masks
@pytest.mark.parametrize("B,size,win", [(2, (17, 19, 23), 7), (1, (10, 12, 40), 13)])
def test_a_mask_of_ones_is_the_unmasked_operator(ops, B, size, win):
    """loss and gradient of ops.ncc_loss / ops.l2_loss to 1e-6 relative, with one and with two masks of ones"""
    p, t, d = _data(B, size, win)
    ones = d["ones"]
    pg = p.clone().requires_grad_(True)
    l0 = ops.ncc_loss(pg, t, win, GAMMA)
    g0, = torch.autograd.grad(l0, [pg], grad_outputs=torch.tensor(1.7, device=DEV))
    l0 = l0.detach()
    for mask2 in (None, ones):
        l1, g1 = _run(ops, p, t, ones, mask2, win)
        assert abs(float(l1) - float(l0)) <= 1e-6 * abs(float(l0)), (float(l1), float(l0))
        assert bool(((g1 - g0).abs() <= 1e-6 * g0.abs()).all()), amax(g1 - g0) / amax(g0)
    a = torch.cat([p, t, p * t], 1)
    b = torch.cat([t, p, t * t], 1)
    ag = a.clone().requires_grad_(True)
    s0 = ops.l2_loss(ag, b)
    h0, = torch.autograd.grad(s0, [ag])
    ag1 = a.clone().requires_grad_(True)
    s1 = ops.l2_loss_masked(ag1, b, ones)
    h1, = torch.autograd.grad(s1, [ag1])
    s0, s1 = s0.detach(), s1.detach()
    assert abs(float(s1) - float(s0)) <= 1e-6 * abs(float(s0))
    assert bool(((h1 - h0).abs() <= 1e-6 * h0.abs()).all())
    rmse, frac = ops.rmse_masked(a, b, ones)
    assert abs(float(rmse) - float(ops.rmse(a, b))) <= 1e-6 * float(rmse) and float(frac) == 1.0


@pytest.mark.parametrize("B,size,win", [(2, (17, 19, 23), 7), (1, (10, 12, 40), 13)])
def test_an_empty_mask_gives_exact_zeros(ops, B, size, win):
    p, t, d = _data(B, size, win)
    zero = torch.zeros_like(p)
    for mask, mask2 in ((zero, None), (d["rand"], zero)):
        loss, gp = _run(ops, p, t, mask, mask2, win)
        assert float(loss) == 0.0 and bool(torch.isfinite(gp).all()) and not bool(gp.any())
        ag = p.clone().requires_grad_(True)
        for fn in (ops.l2_loss_masked, lambda *x: ops.rmse_masked(*x)[0]):
            val = fn(ag, t, mask, mask2)
            ga, = torch.autograd.grad(val, [ag])
            assert float(val) == 0.0 and bool(torch.isfinite(ga).all()) and not bool(ga.any())
        assert float(ops.rmse_masked(p, t, mask, mask2)[1]) == 0.0


def test_two_runs_give_equal_bits(ops):
    p, t, d = _data(2, (17, 19, 23), 7)
    runs = [_run(ops, p, t, d["ball"], d["rand"], 7) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    a = torch.cat([p, t], 1)
    vals = [ops.l2_loss_masked(a, a.flip(1), d["ball"], d["rand"]) for _ in range(2)]
    assert torch.equal(vals[0], vals[1])


@pytest.mark.parametrize("B,size,win", [(2, (17, 19, 23), 7), (1, (10, 12, 40), 13), (1, (40, 40, 40), 5)])
def test_gradient_is_exactly_zero_out_of_the_masks_reach(ops, B, size, win):
    """farther than win // 2 from the mask's support every window of the backward box sums holds zeros only"""
    p, t, _ = _data(B, size, win)
    mask = torch.zeros_like(p)
    mask[:, :, : max(1, size[0] // 4), 2:5, 3:9] = 0.5
    far = M.outside_reach(mask, None, win)
    assert 0 < int(far.sum()) < far.numel()
    _, gp = _run(ops, p, t, mask, None, win)
    assert not bool(gp[far].any()) and bool(gp[~far].any())


def test_slices_run_as_depth_one_volumes(ops):
    """a 2-D (1,1,24,20) pair with (1,1,24,20) masks: the win x win window count"""
    g = torch.Generator(device=DEV).manual_seed(11)
    p, t, w = (torch.rand(1, 1, 24, 20, device=DEV, generator=g) for _ in range(3))
    ball = M.ball(1, (24, 20), device=DEV)
    pg = p.clone().requires_grad_(True)
    loss = ops.ncc_loss_masked(pg, t, ball, w, 5, GAMMA)
    gp, = torch.autograd.grad(loss, [pg])
    lift = lambda x: x.double().unsqueeze(2)
    ref = M.ncc_masked_ref(lift(p), lift(t), lift(ball), lift(w), 5, GAMMA)
    rg = M.ncc_masked_grad_ref(lift(p), lift(t), lift(ball), lift(w), 5, GAMMA)[:, :, 0]
    assert gp.shape == p.shape
    check("ncc_masked 2-D loss", loss.detach(), ref, 1e-4 * abs(float(ref)))
    check("ncc_masked 2-D grad", gp, rg, 5e-5 * amax(rg), power=_last_counted(ball, w))
    ref2 = M.l2_masked_ref(lift(p), lift(t), lift(ball), lift(w))
    check("l2_masked 2-D", ops.l2_loss_masked(p, t, ball, w), ref2, 1e-5 * max(1.0, float(ref2)))


def test_masks_of_another_dtype_and_of_a_wrong_shape(ops):
    p, t, d = _data(2, (17, 19, 23), 7)
    as_bool = d["ball"] > 0
    assert torch.equal(ops.ncc_loss_masked(p, t, as_bool, None, 7, GAMMA), ops.ncc_loss_masked(p, t, d["ball"], None, 7, GAMMA))
    assert torch.equal(ops.l2_loss_masked(p, t, as_bool.to(torch.uint8)), ops.l2_loss_masked(p, t, d["ball"]))
    for bad in (d["ball"][:1], d["ball"][:, :, :-1], d["ball"].expand(-1, 2, -1, -1, -1), d["ball"][:, 0]):
        with pytest.raises(ValueError):
            ops.ncc_loss_masked(p, t, bad, None, 7, GAMMA)
        with pytest.raises(ValueError):
            ops.ncc_loss_masked(p, t, d["ball"], bad, 7, GAMMA)
        with pytest.raises(ValueError):
            ops.l2_loss_masked(p, t, bad)
        with pytest.raises(ValueError):
            ops.rmse_masked(p, t, d["ball"], bad)


# ================================================================================================ the dispatcher
# (term, B, size, keywords): H = 1 (no march in the H pass) and window 13 (the tap-form kernels) for "ncc" / "mse"; the smallest 3-D case of
# test_gpu_mind for "mind"; the 2-D forms
SIM_CASES = [(kind, B, size, dict(win=win)) for kind in ("ncc", "mse") for B, size, win in ((2, (6, 1, 70), 5), (1, (10, 12, 40), 13), (2, (20, 130), 7))]
SIM_CASES.append(("mind", 2, (5, 6, 7), dict(dilation=1)))


def _named_operator(ops, kind, kw):
    """(unmasked, masked) operators of a term, called the way ops.similarity's caller would have to call them"""
    if kind == "ncc":
        return (lambda p, t: ops.ncc_loss(p, t, kw["win"], GAMMA)), (lambda p, t, m, m2: ops.ncc_loss_masked(p, t, m, m2, kw["win"], GAMMA))
    if kind == "mse":
        return ops.l2_loss, ops.l2_loss_masked
    return (lambda p, t: ops.mind_loss(p, t, kw["dilation"])), (lambda p, t, m, m2: ops.mind_loss_masked(p, t, m, m2, kw["dilation"]))


@pytest.mark.parametrize("kind,B,size,kw", SIM_CASES)
def test_similarity_is_the_named_operator(ops, kind, B, size, kw):
    """ops.similarity against the operator it names, value and gradient bit for bit (the same kernels on the same inputs, no atomics), for
    no mask, one mask in either argument and two; gamma reaches "ncc" only; "mind" on a slice raises NotImplementedError"""
    g = torch.Generator(device=DEV).manual_seed(size[-1] + B)
    p, t, m1, m2 = (torch.rand(B, 1, *size, device=DEV, generator=g) for _ in range(4))
    plain, masked = _named_operator(ops, kind, kw)

    def value_and_grad(fn):
        pg = p.clone().requires_grad_(True)
        val = fn(pg)
        assert val.dim() == 0
        gp, = torch.autograd.grad(val, [pg], grad_outputs=torch.tensor(1.7, device=DEV))
        return val.detach(), gp

    for pair, named in (((None, None), lambda x: plain(x, t)), ((m1, None), lambda x: masked(x, t, m1, None)),
                        ((None, m1), lambda x: masked(x, t, m1, None)), ((m1, m2), lambda x: masked(x, t, m1, m2))):
        got = value_and_grad(lambda x: ops.similarity(kind, x, t, *pair, gamma=GAMMA, **kw))
        want = value_and_grad(named)
        which = tuple(m is not None for m in pair)
        assert torch.equal(got[0], want[0]), (kind, which, float(got[0]), float(want[0]))
        assert torch.equal(got[1], want[1]) and bool(got[1].any()), (kind, which)
    if kind == "mind":                      # 3-D only, through the dispatcher as through ops.mind_loss(_masked)
        for pair in ((None, None), (m1[:, :, 0], None), (None, m1[:, :, 0])):
            with pytest.raises(NotImplementedError):
                ops.similarity("mind", p[:, :, 0], t[:, :, 0], *pair)


# ================================================================================================ the masks' own warp
@pytest.mark.parametrize("B,grid,img", [(2, (9, 10, 11), (9, 10, 11)), (1, (8, 8, 8), (16, 16, 16)), (1, (20, 24, 18), (20, 24, 18))])
def test_warp_mask_is_the_warp_and_keeps_constants(ops, B, grid, img):
    """ops.warp_mask against the float64 SpatialTransformer (pyramid_ref.warp_ref) within 3e-5: the sample coordinate (up to 24 here, one
    ulp 1.9e-6) passes four fp32 roundings, at most 8e-6 per axis, and a volume with values in [0, 1] changes by at most 1 per voxel
    along each of the three axes; equal to ops.warp3d (the same coordinates, some ten roundings of values up to 1) to 1e-6; and exact
    on constant volumes - where ops.warp3d is not"""
    g = torch.Generator(device=DEV).manual_seed(grid[0] * 7 + B)
    df = 3.0 * torch.randn(B, 3, *grid, device=DEV, generator=g)
    mask = torch.rand(B, 1, *img, device=DEV, generator=g)
    got = ops.warp_mask(df, mask)
    assert got.shape == (B, 1, *grid) and got.dtype == torch.float32 and not got.requires_grad
    check(f"warp_mask {B}/{grid}/{img}", got, R.warp_ref(df.double(), mask.double()), 3e-5)
    assert amax(got - ops.warp3d(df, mask)) <= 1e-6
    for c in (1.0, 0.0, 0.3):
        const = torch.full_like(mask, c)
        assert torch.equal(ops.warp_mask(df, const), torch.full_like(got, c)), c
    assert not torch.equal(ops.warp3d(df, torch.ones_like(mask)), torch.ones_like(got)), "warp3d kept ones: warp_mask would not be needed"
    assert torch.equal(ops.warp_mask(df, mask > 0.5), ops.warp_mask(df, (mask > 0.5).float()))
    with pytest.raises(ValueError):
        ops.warp_mask(df, mask.expand(-1, 2, -1, -1, -1))


def test_warp_mask_of_slices(ops):
    g = torch.Generator(device=DEV).manual_seed(3)
    df, mask = 2.0 * torch.randn(1, 2, 24, 20, device=DEV, generator=g), torch.rand(1, 1, 24, 20, device=DEV, generator=g)
    got = ops.warp_mask(df, mask)
    assert got.shape == mask.shape and amax(got - ops.warp3d(df, mask)) <= 1e-6
    assert torch.equal(ops.warp_mask(df, torch.ones_like(mask)), torch.ones_like(mask))


# ================================================================================================ model and step
SIZE = [16, 16, 16]


def _model(api, recon, mask, train=True):
    """T3 / L2 / n0 = 2 at 16^3, the same weights and noise for every call"""
    models, nb = api
    torch.manual_seed(0)
    m = models.PULPo(3, 2, 0.1, SIZE, feedback=FB, n0=2, recon_loss=[recon], mask=mask).cuda()
    m = m.train() if train else m.eval()
    g = torch.Generator().manual_seed(4)
    for l in range(2):
        s = 16 // 2 ** (l + 1)
        m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=g).cuda())
    return m


@functools.lru_cache(maxsize=None)
def _pair():
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(1, 1, *SIZE, generator=g).cuda(), torch.rand(1, 1, *SIZE, generator=g).cuda()
    box = torch.zeros(1, 1, *SIZE, device=DEV)
    box[:, :, 3:13, 2:12, 4:14] = 1.0
    return x, y, box, M.ball(1, SIZE, device=DEV)


def _step(model, x, y, mask_x=None, mask_y=None):
    model.zero_grad(set_to_none=True)
    outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y, None, None, mask_x, mask_y)
    total.backward()
    return outs, total.detach(), rec.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _ref_recon(model, recon, outs, y, mask_x, mask_y):
    """the reconstruction term in float64 on the model's own y_hat and final_dfs, the level masks rebuilt with pyramid_ref"""
    final_dfs, y_hat = outs[6], outs[7]
    total = 0.0
    for l, w in model.hierarchical_recon_loss.weight_dict.items():
        size = tuple(y_hat[l].shape[2:])
        target = R.resize_ref(y.double(), size)
        wx = R.warp_ref(final_dfs[l].detach().double(), mask_x.double()) if mask_x is not None else None
        wy = R.resize_ref(mask_y.double(), size) if mask_y is not None else None
        ma, mb = (wx, wy) if wx is not None else (wy, None)
        if recon == "ncc":
            term = M.ncc_masked_ref(y_hat[l].detach().double(), target, ma, mb, model.hierarchical_recon_loss.window_size[l], model.hparams.gamma)
        else:
            term = M.l2_masked_ref(y_hat[l].detach().double(), target, ma, mb)
        total = total + w * term
    return total


def _deterministic(fn):
    """fn() with the ordered weight-gradient sums (ops.set_deterministic): two evaluations of one step then agree bit for bit, so a
    difference between two steps is a difference of what they compute"""
    from pulpo_amd import ops
    env_det = os.environ.get("PULPO_DETERMINISTIC", "0") == "1"
    try:
        ops.set_deterministic(True)
        return fn()
    finally:
        ops.set_deterministic(env_det)


@pytest.mark.parametrize("recon", ["ncc", "mse"])
def test_masks_of_ones_give_the_unmasked_step(api, recon):
    """mask=True with masks of ones against mask=False: the total loss and every parameter gradient within rtol 1e-5 / atol 1e-7, in the
    deterministic mode (where two unmasked steps agree bit for bit).  It rests on ops.warp_mask returning ones for ones: with the
    moving mask under ops.warp3d (1 - 1.19e-7 at 517 of the 4096 level-0 voxels) 181 (ncc) / 336 (mse) of the 11652 gradient elements
    were outside this bound, worst 9.3e-6 / 3.2e-5 beside max|g| = 31 / 51 - the step amplifies an ulp that far on its own (the unmasked
    ncc step with gamma (1 + 2e-7): 187 elements outside, chiefly biases in front of a BatchNorm, whose true gradient is 0)."""
    x, y, _, _ = _pair()
    ones = torch.ones_like(x)

    def run():
        _, total0, _, grads0 = _step(_model(api, recon, False), x, y)
        _, total1, _, grads1 = _step(_model(api, recon, True), x, y, ones, ones)
        return total0, grads0, total1, grads1
    total0, grads0, total1, grads1 = _deterministic(run)
    torch.testing.assert_close(total1, total0, rtol=1e-5, atol=1e-7)
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    outside = sum(int(((grads1[k] - grads0[k]).abs() > 1e-7 + 1e-5 * grads0[k].abs()).sum()) for k in grads0)
    worst = max(float((grads1[k] - grads0[k]).abs().max()) for k in grads0)
    print(f"step {recon}, masks of ones: {outside} of {sum(g.numel() for g in grads0.values())} gradient elements outside rtol 1e-5 / atol 1e-7, "
          f"worst absolute difference {worst:.3g}")
    for k in grads0:
        torch.testing.assert_close(grads1[k], grads0[k], rtol=1e-5, atol=1e-7, msg=lambda s, k=k: f"{k}: {s}")


@pytest.mark.parametrize("recon", ["ncc", "mse"])
def test_level_masks_of_exact_ones_change_no_bit(api, recon):
    """the masked loss terms fed level masks that are exactly 1 (two per level): the total loss within rtol 1e-6 of the unmasked step's,
    and every parameter gradient bit-equal to it - the masked backward kernels hand on the unmasked kernels' bits (-gamma V / M with
    M = B V is -gamma / B, and m = 1 multiplies exactly)"""
    x, y, _, _ = _pair()
    ones = torch.ones_like(x)

    def run():
        _, total0, _, grads0 = _step(_model(api, recon, False), x, y)
        model = _model(api, recon, True)
        model.level_masks = lambda final_dfs, mask_x=None, mask_y=None: {l: (torch.ones_like(df[:, :1]), torch.ones_like(df[:, :1]))
                                                                         for l, df in final_dfs.items()}
        _, total1, _, grads1 = _step(model, x, y, ones, ones)
        return total0, grads0, total1, grads1
    total0, grads0, total1, grads1 = _deterministic(run)
    torch.testing.assert_close(total1, total0, rtol=1e-6, atol=0.0)
    assert grads1.keys() == grads0.keys() and len(grads0) > 20
    for k in grads0:
        assert torch.equal(grads1[k], grads0[k]), (k, float((grads1[k] - grads0[k]).abs().max()))


@pytest.mark.parametrize("recon", ["ncc", "mse"])
def test_mask_false_and_empty_masks_change_nothing(api, recon):
    """mask=False with masks in the batch, and mask=True with empty masks, reproduce the unmasked loss bit for bit"""
    x, y, box, ball = _pair()
    empty = torch.empty((0,), device=DEV)

    def run():
        _, total0, rec0, grads0 = _step(_model(api, recon, False), x, y)
        _, total0m, rec0m, grads0m = _step(_model(api, recon, False), x, y, box, ball)
        _, total_e, rec_e, _ = _step(_model(api, recon, True), x, y, empty, empty)
        return total0, rec0, grads0, total0m, rec0m, grads0m, total_e, rec_e
    total0, rec0, grads0, total0m, rec0m, grads0m, total_e, rec_e = _deterministic(run)
    assert torch.equal(total0m, total0) and torch.equal(rec0m, rec0)
    assert torch.equal(total_e, total0) and torch.equal(rec_e, rec0)
    for k in grads0:
        assert torch.equal(grads0m[k], grads0[k]), k


@pytest.mark.parametrize("recon", ["ncc", "mse"])
def test_masked_reconstruction_term_of_the_step_vs_float64(api, recon):
    """with a box mask_x and a ball mask_y, and with either alone, the reconstruction term is the float64 reference evaluated on the
    model's own y_hat and final_dfs, the level masks rebuilt with pyramid_ref.warp_ref / resize_ref (rtol 1e-4)"""
    x, y, box, ball = _pair()
    _, _, rec0, _ = _step(_model(api, recon, False), x, y)
    for mx, my in ((box, ball), (box, None), (None, ball)):
        model = _model(api, recon, True)
        outs, total, rec, grads = _step(model, x, y, mx, my)
        ref = _ref_recon(model, recon, outs, y, mx, my)
        print(f"RATIO step {recon} rec {abs(float(rec) - float(ref)) / (1e-4 * abs(float(ref))):.3g}")
        assert abs(float(rec) - float(ref)) <= 1e-4 * abs(float(ref)), (float(rec), float(ref))
        assert abs(float(rec) - float(rec0)) > 1e-3 * abs(float(rec0)), "the masks did not reach the loss"
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())


@pytest.mark.parametrize("recon", ["ncc", "mse"])
def test_one_eager_stepper_step_with_masks(api, recon):
    from pulpo_amd.dp import DataParallelStepper
    x, y, box, ball = _pair()
    e = torch.empty((0,), device=DEV)
    _, want, _, _ = _step(_model(api, recon, True), x, y, box, ball)
    model = _model(api, recon, True)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = DataParallelStepper(model, lr=1e-3).step((x, y, e, e, e, e, box, ball))
    torch.cuda.synchronize()
    torch.testing.assert_close(loss.detach().reshape(()), want, rtol=1e-6, atol=0.0)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert sum(int(not torch.equal(p, before[k])) for k, p in model.named_parameters()) > 20


# ================================================================================================ score table
def test_performance_adds_the_masked_rows(api):
    from pulpo_amd import evaluation
    assert evaluation.MASK_METRICS == ("RMSE_masked", "MaskFrac")
    x, y, box, ball = _pair()
    model = _model(api, "ncc", False, train=False)
    old = evaluation.performance(model, x, y)
    for mx, my in ((box, ball), (box, None), (None, ball)):
        new = evaluation.performance(model, x, y, mask_x=mx, mask_y=my)
        assert set(new) == set(old) | set(evaluation.MASK_METRICS)
        for name in old:
            for l in old[name]:
                assert torch.equal(new[name][l], old[name][l]), (name, l)
        with torch.no_grad():
            outputs, individual = model.predict_deterministic(x, y)
            _, final_dfs = model.combine_dfs(individual)
        for l in outputs:
            size = tuple(outputs[l].shape[2:])
            wx = R.warp_ref(final_dfs[l].double(), mx.double()) if mx is not None else None
            wy = R.resize_ref(my.double(), size) if my is not None else None
            ma, mb = (wx, wy) if wx is not None else (wy, None)
            rmse, frac = M.rmse_masked_ref(outputs[l].double(), R.resize_ref(y.double(), size), ma, mb)
            for name, ref in (("RMSE_masked", rmse), ("MaskFrac", frac)):
                got = new[name][l]
                assert got.dim() == 0 and got.is_cuda
                print(f"RATIO performance {name}[{l}] {abs(float(got) - float(ref)) / (1e-4 * abs(float(ref))):.3g}")
                assert abs(float(got) - float(ref)) <= 1e-4 * abs(float(ref)), (name, l, float(got), float(ref))
            assert 0.0 < float(new["MaskFrac"][l]) < 1.0
            assert abs(float(new["RMSE_masked"][l]) - float(old["RMSE"][l])) > 1e-4 * float(old["RMSE"][l])
