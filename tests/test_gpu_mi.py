"""The mutual-information similarity term on the GPU: ops.joint_histogram / mi_loss / mi_loss_masked against the
float64 definition of tests/mi_ref.py, and the term's way through the loss module, the model's step, refine, the score table and affine.fit.

Bounds: 8 x the distance of mi_ref's own float32 evaluation from float64 (mi_ref.P_OWN / LOSS_OWN / GRAD_OWN, re-measured by
test_host_mi) - the factor of the other kernel tests (FIT_FACTOR), because the kernels sum in another order than torch: the joint histogram
p element by element, the loss relative, the gradient relative in L2.  Every comparison prints a RATIO line: pytest -s."""
import ctypes
import functools

import pytest
import torch

import affine_ref as AR
import mi_ref as M
import pyramid_ref as R
from oracle import pulpo_oracle as O
from test_host_affine import END_MAX, START_MIN

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
SIZE = [16, 16, 16]
FACTOR = 8.0
PLAIN = [c for c in M.CASES if c[4] is None]
MASKED = [c for c in M.CASES if c[4] is not None]


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


def dev(t):
    return None if t is None else t.float().to(DEV)


def cid(c):
    return f"{c[0]}/{'x'.join(map(str, c[1]))}/K{c[2]}/{c[3]}/{c[4]}"


def _run(ops, p, t, bins, mask=None, mask2=None, up=M.UPSTREAM):
    pg = p.clone().requires_grad_(True)
    loss = ops.mi_loss(pg, t, bins) if mask is None else ops.mi_loss_masked(pg, t, mask, mask2, bins)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    gp, = torch.autograd.grad(loss, [pg], grad_outputs=torch.tensor(up, device=DEV))
    assert gp.shape == p.shape
    return loss.detach(), gp


def _compare(ops, c):
    B, size, bins, kind, masks = c
    pred, true, m1, m2, p64, mi64, l64, g64 = M.case(*c)
    p, t, w1, w2 = dev(pred), dev(true), dev(m1), dev(m2)
    hp, hmi = ops.joint_histogram(p, t, bins, w1, w2)
    assert hp.shape == (B, bins, bins) and hp.dtype == torch.float64 and hmi.shape == (B,) and hmi.dtype == torch.float64
    loss, gp = _run(ops, p, t, bins, w1, w2)
    rp = R.ratio(hp.cpu(), p64, FACTOR * M.P_OWN)
    rl = abs(float(loss) - float(l64)) / abs(float(l64)) / (FACTOR * M.LOSS_OWN)
    rg = M.rel_l2(gp.cpu(), g64) / (FACTOR * M.GRAD_OWN)
    rm = float(((hmi.cpu() - mi64).abs() / mi64.abs()).max()) / (FACTOR * M.LOSS_OWN)
    print(f"FIGURE mi {cid(c)}: loss {float(loss):.6g} (float64 {float(l64):.6g}), MI {[round(float(v), 4) for v in hmi]}")
    for name, r in (("p", rp), ("loss", rl), ("MI", rm), ("grad", rg)):
        print(f"RATIO mi {cid(c)} {name} {r:.3g}")
    assert rp <= 1.0 and rl <= 1.0 and rm <= 1.0 and rg <= 1.0, (rp, rl, rm, rg)
    assert abs(float(hp.sum()) - B) <= 1e-5 * B
    return p, t, w1, w2, loss, gp


# ================================================================================================ operators against float64
@pytest.mark.parametrize("c", PLAIN, ids=cid)
def test_histogram_loss_and_gradient_vs_float64(ops, c):
    p, t, _, _, loss, gp = _compare(ops, c)
    out = (p < 0) | (p > 1)
    if c[3] == "edges":
        assert int(out.sum()) > 0 and int(((p == 0) | (p == 1)).sum()) > 0
    assert not bool(gp[out].any()), "a voxel strictly outside [0,1] has a gradient"
    if c[3] == "sparse":
        assert float((p == 0).float().mean()) >= 0.88


@pytest.mark.parametrize("c", MASKED, ids=cid)
def test_masked_vs_float64(ops, c):
    p, t, w1, w2, loss, gp = _compare(ops, c)
    assert not bool(gp[(w1 if w2 is None else w1 * w2) == 0].any())
    if w2 is not None:                                     # both masks multiply
        l1, g1 = _run(ops, p, t, c[2], w1 * w2, None)
        assert torch.equal(l1, loss) and torch.equal(g1, gp)


@pytest.mark.parametrize("c", [(2, (20, 24, 20), 32, "smooth", None), (2, (33, 47), 64, "smooth", None), (1, (5, 6, 7), 33, "smooth", None)], ids=cid)
def test_ones_mask_is_bit_equal_and_zero_mask_gives_zero(ops, c):
    pred, true = M.make_pair(c[0], c[1], c[3])
    p, t = dev(pred), dev(true)
    ones, zeros = torch.ones_like(p), torch.zeros_like(p)
    l0, g0 = _run(ops, p, t, c[2])
    for pair in ((ones, None), (ones, ones)):
        l1, g1 = _run(ops, p, t, c[2], *pair)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
    h0, h1 = ops.joint_histogram(p, t, c[2]), ops.joint_histogram(p, t, c[2], ones)
    assert torch.equal(h0[0], h1[0]) and torch.equal(h0[1], h1[1])
    for pair in ((zeros, None), (ones, zeros)):
        l1, g1 = _run(ops, p, t, c[2], *pair)
        assert float(l1) == 0.0 and not bool(g1.any()) and bool(torch.isfinite(g1).all())
        hp, hmi = ops.joint_histogram(p, t, c[2], *pair)
        assert not bool(hp.any()) and not bool(hmi.any())
    half = torch.cat([ones[:1], zeros[1:]]) if c[0] == 2 else None
    if half is not None:                                   # an empty mask in one batch element leaves the other's term
        l1, g1 = _run(ops, p, t, c[2], half)
        ref = M.loss_masked(pred, true, half.double().cpu(), None, c[2])
        assert abs(float(l1) - float(ref)) <= FACTOR * M.LOSS_OWN * abs(float(ref)) and not bool(g1[1].any()) and bool(torch.isfinite(g1).all())


def test_only_pred_gets_a_gradient(ops):
    pred, true = M.make_pair(2, (5, 6, 7), "smooth")
    pg, tg = dev(pred).requires_grad_(True), dev(true).requires_grad_(True)
    mg = torch.ones_like(pg).requires_grad_(True)
    gp, gt, gm = torch.autograd.grad(ops.mi_loss_masked(pg, tg, mg), [pg, tg, mg], allow_unused=True)
    assert gp is not None and gt is None and gm is None


@pytest.mark.parametrize("det", [False, True])
def test_bit_identical_run_to_run(ops, det):
    """no atomics anywhere: the default mode gives equal bits, the 90 %-zeros image included, and PULPO_DETERMINISTIC needs no second path"""
    prev = ops.DETERMINISTIC
    ops.set_deterministic(det)
    try:
        for c in ((2, (20, 24, 20), 32, "sparse", None), (2, (20, 24, 20), 64, "smooth", "ball_x_rand"), (2, (33, 47), 33, "smooth", None)):
            pred, true = M.make_pair(c[0], c[1], c[3])
            p, t = dev(pred), dev(true)
            w1, w2 = (dev(m) for m in M.make_masks(c[0], c[1], c[4]))
            a, b = _run(ops, p, t, c[2], w1, w2), _run(ops, p, t, c[2], w1, w2)
            ha, hb = ops.joint_histogram(p, t, c[2], w1, w2), ops.joint_histogram(p, t, c[2], w1, w2)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ha[0], hb[0]) and torch.equal(ha[1], hb[1])
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("c", [(2, (20, 24, 20), 32, "smooth", None), (2, (7, 9, 11), 64, "smooth", None), (1, (5, 6, 7), 4, "smooth", None)], ids=cid)
def test_every_slab_row_read_is_written(ops, c):
    """pulpo_mi_fwd on NaN-filled scratch and outputs gives the bits of the ops call"""
    from pulpo_amd._lib import lib
    B, size, bins = c[0], c[1], c[2]
    pred, true = M.make_pair(B, size, c[3])
    p, t = dev(pred), dev(true)
    V = p.numel() // B
    nan = lambda n, dt=torch.float32: torch.full((n,), float("nan"), device=DEV, dtype=dt)
    nfl = lib.query("pulpo_mi_scratch_floats", B, V, bins)
    assert nfl == lib.query("pulpo_mi_blocks", B, V) * (32 if bins <= 32 else 64) ** 2
    slab, hp, hmi, G, loss = nan(nfl), nan(B * bins * bins, torch.float64), nan(B, torch.float64), nan(B * bins * bins), nan(1)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    lib.call("pulpo_mi_fwd", ptr(t), ptr(p), None, None, ptr(slab), ptr(hp), ptr(hmi), ptr(G), ptr(loss), B, V, bins, 0.05,
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want_p, want_mi = ops.joint_histogram(p, t, bins)
    assert bool(torch.isfinite(slab).all()) and bool(torch.isfinite(G).all())
    assert torch.equal(hp.view(B, bins, bins), want_p) and torch.equal(hmi, want_mi) and torch.equal(loss[0], ops.mi_loss(p, t, bins))


def test_memory_stays_below_a_quarter_of_one_weight_matrix(ops):
    """64^3, K = 32: forward and backward allocate less than V K bytes beyond the inputs and the gradient (a dense V x K fp32 weight matrix
    is 4 V K)"""
    B, size, bins = 1, (64, 64, 64), 32
    pred, true = M.make_pair(B, size, "smooth")
    p, t = dev(pred).requires_grad_(True), dev(true)
    V = p.numel()
    float(ops.mi_loss(p.detach(), t, bins))                 # (the library and the allocator are warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = ops.mi_loss(p, t, bins)
    gp, = torch.autograd.grad(loss, [p])
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - 4 * V
    print(f"FIGURE mi memory at 64^3 K 32: {extra} bytes beyond the inputs and the gradient, bound {V * bins}")
    assert extra < V * bins and bool(torch.isfinite(gp).all())


def test_argument_errors(ops):
    from pulpo_amd._lib import PulpoHipError
    pred, true = M.make_pair(2, (5, 6, 7), "smooth")
    p, t = dev(pred), dev(true)
    for bins in (3, 65):
        with pytest.raises(ValueError, match="bins"):
            ops.mi_loss(p, t, bins)
    with pytest.raises(ValueError):
        ops.mi_loss_masked(p, t, torch.ones(2, 1, 5, 6, 8, device=DEV))
    with pytest.raises(PulpoHipError):
        ops.mi_loss_masked(p, t, torch.ones(2, 1, 5, 6, 7))                          # a CPU mask
    with pytest.raises(PulpoHipError):
        ops.mi_loss(torch.cat([p, p], 1), torch.cat([t, t], 1))                      # two channels
    assert torch.equal(ops.similarity("mi", p, t, bins=16, gamma=0.1), ops.mi_loss(p, t, 16, 0.1))
    ones = torch.ones_like(p)
    assert torch.equal(ops.similarity("mi", p, t, None, ones, bins=16), ops.mi_loss_masked(p, t, ones, None, 16))


# ================================================================================================ loss module, step, refine, score table
def _model(api, recon, mask=False, train=True, **kw):
    """T3 / L2 / n0 = 2 at 16^3, the same weights and noise for every call"""
    models, nb = api
    torch.manual_seed(0)
    m = models.PULPo(3, 2, 0.1, SIZE, feedback=FB, n0=2, recon_loss=list(recon), mask=mask, **kw).cuda()
    m = m.train() if train else m.eval()
    g = torch.Generator().manual_seed(4)
    for l in range(2):
        s = 16 // 2 ** (l + 1)
        m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=g).cuda())
    return m


@functools.lru_cache(maxsize=None)
def _pair():
    from pulpo_amd import synthetic
    x, y = synthetic.multimodal_pair(SIZE, 1, 8, DEV)
    return x, y, dev(M.ball(1, SIZE, 0.45)), dev(M.ball(1, SIZE, 0.35))


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
            term = M.loss(pred, target, rl.mi_bins, model.hparams.gamma)
        else:
            wx = R.warp_ref(final_dfs[l].detach().double(), mask_x.double()) if mask_x is not None else None
            wy = R.resize_ref(mask_y.double(), size) if mask_y is not None else None
            ma, mb = (wx, wy) if wx is not None else (wy, None)
            term = M.loss_masked(pred, target, ma, mb, rl.mi_bins, model.hparams.gamma)
        if ncc:
            term = (term + R.ncc_ref(pred, target, rl.window_size[l], model.hparams.gamma)) / 2
        res[l] = w * term
    return res


@pytest.mark.parametrize("recon,masked", [(("mi",), False), (("mi",), True), (("ncc", "mi"), False)])
def test_step_with_the_mi_term(api, recon, masked):
    """every per-level reconstruction term is w_l x mi_ref.loss (the masked form with ball masks; averaged with NCC) on the step's own
    y_hat[l] and resized y within 8 x LOSS_OWN; training_step's loss and gradients are finite; mi_bins = 16 changes the value"""
    x, y, ball_x, ball_y = _pair()
    mx, my = (ball_x, ball_y) if masked else (None, None)
    model = _model(api, recon, mask=masked)
    assert model.hierarchical_recon_loss.mi_bins == 32
    outs, _, (total, kl, rec, reg), (_, rec_levels, _) = model._forward_and_losses(x, y, None, None, mx, my)
    ref = _ref_levels(model, outs, y, mx, my, ncc="ncc" in recon)
    assert rec_levels.keys() == ref.keys() and len(ref) == 2
    tol = FACTOR * M.LOSS_OWN
    for l in ref:
        r = abs(float(rec_levels[l]) - float(ref[l])) / (tol * abs(float(ref[l])))
        print(f"RATIO step {recon}{' masked' if masked else ''} level {l} {r:.3g}  (term {float(rec_levels[l]):.6g})")
        assert r <= 1.0, (l, float(rec_levels[l]), float(ref[l]))
    assert abs(float(rec) - sum(float(v) for v in ref.values())) <= tol * abs(float(rec))
    model.zero_grad(set_to_none=True)
    loss = model.training_step((x, y, None, None, None, None, mx, my), 0)
    loss.backward()
    assert bool(torch.isfinite(loss))
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    flow = [k for k in grads if "velocity_field" in k and k.endswith("weight")]
    assert flow and all(float(grads[k].abs().max()) > 0.0 for k in flow), flow
    model.hierarchical_recon_loss.mi_bins = 16
    outs, _, (_, _, rec16, _), (_, rec_levels16, _) = model._forward_and_losses(x, y, None, None, mx, my)
    ref16 = _ref_levels(model, outs, y, mx, my, ncc="ncc" in recon)
    assert abs(float(rec16) - float(rec)) > 1e-3 * abs(float(rec))
    for l in ref16:
        assert abs(float(rec_levels16[l]) - float(ref16[l])) <= tol * abs(float(ref16[l])), l


def test_refine_with_the_mi_term(api):
    from pulpo_amd import refine
    x, y, _, _ = _pair()
    model = _model(api, ["ncc"], train=False)
    model.hierarchical_recon_loss.mi_bins = 16
    obj = refine.Objective(model, x, y, recon_loss=["mi"])
    assert obj.recon is not model.hierarchical_recon_loss and obj.recon.mi_bins == 16 and obj.recon.recon_loss == ["mi"]
    assert refine.Objective(model, x, y).recon is model.hierarchical_recon_loss
    res = model.refine(x, y, iters=3, recon_loss=["mi"])
    h = res["history"].cpu()
    print(f"FIGURE refine mi history {[round(float(v), 4) for v in h[:, 0]]}")
    assert tuple(h.shape) == (4, 4) and bool(torch.isfinite(h).all()) and float(h[-1, 0]) <= float(h[0, 0])
    with pytest.raises(ValueError, match="recon_loss"):
        model.refine(x, y, iters=1, recon_loss=["nmi"])


def test_performance_mi_row(api, ops):
    from pulpo_amd import evaluation
    x, y, _, _ = _pair()
    model = _model(api, ["mi"], train=False)
    plain = evaluation.performance(model, x, y)
    assert "MI" not in plain
    torch.manual_seed(1)
    res = evaluation.performance(model, x, y, mi=True, mi_bins=16)
    assert sorted(res["MI"].keys()) == [0, 1]
    outputs, dfs = model.predict_deterministic(x, y)
    for l in res["MI"]:
        size = tuple(outputs[l].shape[2:])
        target = y if size == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)
        want = ops.joint_histogram(outputs[l], target, 16)[1].mean()
        ref = M.mi(outputs[l].double().cpu(), target.double().cpu(), 16).mean()
        print(f"FIGURE performance MI level {l}: {float(res['MI'][l]):.5f}")
        assert res["MI"][l].dim() == 0 and abs(float(res["MI"][l]) - float(want)) <= 1e-6 * abs(float(want))
        assert abs(float(res["MI"][l]) - float(ref)) <= FACTOR * M.LOSS_OWN * abs(float(ref))
    table = evaluation.PerformanceTable(list(evaluation.METRICS) + list(evaluation.MI_METRICS), 2, ["val"], 1)
    table.add(0, 0, res)


# ================================================================================================ affine.fit(loss="mi")
FIT_SIZE = (32, 32, 32)


@functools.lru_cache(maxsize=None)
def _fit_reference(dtype):
    """affine_ref.fit with mi_ref.loss as its level loss (per-level bins in the place of the NCC windows) on affine_pair with the fixed image
    remapped: (theta, history, expected fit, x, y)"""
    from pulpo_amd import affine
    x, y, want = AR.affine_pair(FIT_SIZE)
    y = M.remap(y)
    old = AR.level_loss
    AR.level_loss = lambda name, pred, true, pair, win: (M.loss(pred, true, win, 1.0) if pair is None
                                                         else M.loss_masked(pred, true, pair[0], pair[1], win, 1.0))
    try:
        theta, hist = AR.fit(x.to(dtype), y.to(dtype), loss="mi", win=affine.DEFAULT_MI_BINS)
    finally:
        AR.level_loss = old
    return theta, hist, want, x, y


def theta_voxels(theta, size):
    return torch.cat([theta[:, :, :3] * ((max(size) - 1) / 2), theta[:, :, 3:]], dim=2)


def hist_rel(h, h64):
    return (h[:, 0].double().cpu() - h64[:, 0]).abs() / h64[:, 0].abs()


def test_affine_fit_with_mi_vs_float64(ops):
    """affine.fit(loss="mi") with its defaults against the float64 reference fit on the same pair: theta (in voxels of edge displacement)
    and the history (row by row, relative) within 8 x the distance between the reference's own fp32 and float64 runs - the rule of
    test_gpu_affine.test_fit_vs_float64; the corner error falls from at least 4.4 voxels to at most 1.0; two fits give equal bits"""
    from pulpo_amd import affine
    th64, h64, want, x, y = _fit_reference(torch.float64)
    th32, h32, *_ = _fit_reference(torch.float32)
    own_t = float((theta_voxels(th32.double(), FIT_SIZE) - theta_voxels(th64, FIT_SIZE)).abs().max())
    own_h = float(hist_rel(h32, h64).max())
    ref_end = AR.corner_error(th64, want, FIT_SIZE)
    print(f"FIGURE fit mi: reference fp32 against float64 theta {own_t:.3g} voxels, history {own_h:.3g} relative; reference ends at {ref_end:.3f}")
    assert ref_end <= 0.8
    xd, yd = dev(x), dev(y)
    res = affine.fit(xd, yd, loss="mi")
    got, hist = res["theta"], res["history"]
    assert tuple(hist.shape) == tuple(h64.shape) and torch.equal(hist[:, 1].cpu().double(), h64[:, 1])
    rt = R.ratio(theta_voxels(got, FIT_SIZE).cpu(), theta_voxels(th64, FIT_SIZE), FACTOR * own_t)
    rh = float(hist_rel(hist, h64).max()) / (FACTOR * own_h)
    start, end = AR.corner_error(AR.identity(1), want, FIT_SIZE), float(affine.corner_error(got.cpu(), want, FIT_SIZE))
    print(f"RATIO fit mi theta {rt:.3g}")
    print(f"RATIO fit mi history {rh:.3g}")
    print(f"FIGURE fit mi: corner error {start:.3f} -> {end:.3f}")
    assert rt <= 1.0 and rh <= 1.0, (rt, rh)
    assert start >= START_MIN and end <= END_MAX
    again = affine.fit(xd, yd, loss="mi")
    assert torch.equal(again["theta"], got) and torch.equal(again["history"], hist)
    same = affine.fit(xd, yd, loss="mi", mi_bins=(16, 16, 32))
    assert torch.equal(same["theta"], got)
    other = affine.fit(xd, yd, loss="mi", mi_bins=16, levels=2, iters=(2, 2))
    assert tuple(other["history"].shape) == (5, 2) and bool(torch.isfinite(other["history"]).all())
