"""Instance-specific refinement on the MI355X against the float64 definition of tests/refine_ref.py: the anchored
Adam kernel element by element, one iteration's objective and gradient, the whole loop, and the behaviour of refine() / performance(refine=).

Bounds.  Kernel: the rule test_gpu_pyramid_metrics.test_adam_vs_float64 holds ops.adam_step to, max(4 x the fp32 reference's own deviation
from float64, 1e-6 max|ref|) per element (metrics_ref.bound); the anchor sum 1e-4 |ref|, the loss tests' bound.  Objective and gradient:
those of test_gpu_pyramid_ops.test_ncc_vs_float64, loss 1e-4 |ref|, gradient 5e-5 max|ref| per level with an upstream factor of 1.7.
Loop: FIELD_TOL and HIST_TOL below.  Each element-wise bound is shown to reject the reference with one element moved by 1e-3 max|ref|;
every comparison prints a RATIO line (pytest -s).  The float64 references run on the CPU, once per case (functools.lru_cache)."""
import functools

import pytest
import torch

import masked_ref as MK
import metrics_ref as M
import pyramid_ref as R
import refine_ref as RR
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)
UP = 1.7
# The loop's bounds: 8 x the largest error of an fp32 CPU run of refine_ref.loop against its float64 run over the two loop cases below (the
# rule of test_gpu_mind.DESC_TOL; the factor leaves room for another summation order and the device's atomics).  The two figures live in
# refine_ref (FIELD_OWN voxels, HIST_OWN relative to |history[0, 0]|); tests/test_host_refine.py re-measures them on the CPU.
FIELD_TOL, HIST_TOL = 8 * RR.FIELD_OWN, 8 * RR.HIST_OWN


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd import evaluation, ops, refine
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb, ops, refine, evaluation


def amax(t) -> float:
    return float(t.detach().abs().max())


def check(name, got, ref, tol, power=-1):
    """max |got - ref| <= tol element by element; and the bound rejects ref with element `power` moved by 1e-3 max|ref|"""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    ref = ref.to(got.device)
    r = R.ratio(got, ref, tol)
    print(f"RATIO {name} {r:.3g}")
    assert r <= 1.0, f"{name}: max error / tolerance = {r:.3g}"
    if power is not None:
        assert R.ratio(got, R.perturbed(ref, power), tol) > 1.0, f"{name}: the bound does not reject a 1e-3 max|ref| error"


def make_model(models, T, L, size, seed=0, **kw):
    torch.manual_seed(seed)
    return models.PULPo(T, L, 0.1, list(size), feedback=FB, n0=4, **kw).to(DEV).eval()


def pin_noise(model, nb, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    for l in range(model.latent_levels):
        shape = (B, model.ndims) + tuple(model.autoencoder.level_sizes[l + model.lk_offset])
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(shape, generator=g).to(DEV))


# ================================================================================================ the kernel
ADAM_TRIP = 4096 * 1024
# tail only (1, 3), body only (4), body + tail (1023, 4101), one size past the grid cap: the stride loop takes a second trip
KERNEL_SIZES = [1, 3, 4, 1023, 4101, ADAM_TRIP + 7]


@pytest.mark.parametrize("form", ["none", "mean", "mean+prec"])
@pytest.mark.parametrize("n", KERNEL_SIZES)
def test_kernel_vs_float64(api, n, form):
    """three consecutive ops.anchored_adam_step from zero moments: p, m and v element by element and the anchor sum against the float64
    update (RR.adam_update) on the same fp32 inputs, each chain carrying its own state, the bound from the fp32 evaluation of the same
    reference; without a mean the result is ops.adam_step's on copies, bit for bit."""
    ops = api[2]
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + len(form))
    lr = 0.03
    p = torch.randn(n, device=DEV, generator=g)
    mean = (p + 0.3 * torch.randn(n, device=DEV, generator=g)) if form != "none" else None
    prec = (0.05 + 3.0 * torch.rand(n, device=DEV, generator=g)) if form == "mean+prec" else None
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    twin = [p.clone(), m.clone(), v.clone()]
    state = {dt: [p.to(dt, copy=True), m.to(dt, copy=True), v.to(dt, copy=True)] for dt in (torch.float32, torch.float64)}
    val = torch.zeros(1, device=DEV)
    pw = ADAM_TRIP if n > ADAM_TRIP else n - 1
    for step in (1, 2, 3):
        gr = torch.randn(n, device=DEV, generator=g)
        ops.anchored_adam_step(p, gr, m, v, lr, step, mean=mean, prec=prec, loss_out=val if mean is not None else None)
        vals = {}
        for dt in state:
            *state[dt], vals[dt] = RR.adam_update(*state[dt][:1], gr.to(dt), *state[dt][1:], lr, step, None if mean is None else mean.to(dt),
                                                  None if prec is None else prec.to(dt))
        for k, (name, got) in enumerate((("p", p), ("m", m), ("v", v))):
            check(f"anchored adam n={n} {form} step {step} {name}", got, state[torch.float64][k],
                  M.bound(state[torch.float32][k], state[torch.float64][k], 1e-6), power=pw if k == 0 else n - 1)
        if mean is not None:
            ref = float(vals[torch.float64])
            dev = abs(float(val) - ref) / abs(ref)
            print(f"RATIO anchored adam n={n} {form} step {step} anchor sum {dev / 1e-4:.3g}")
            assert dev <= 1e-4, (float(val), ref)
        else:
            ops.adam_step(twin[0], gr, twin[1], twin[2], lr, step)
            assert torch.equal(p, twin[0]) and torch.equal(m, twin[1]) and torch.equal(v, twin[2])


def test_kernel_without_a_sum_and_argument_checks(api):
    """loss_out=None gives the same update; a misaligned view comes back as PulpoHipError from the argument check, nothing is launched"""
    ops = api[2]
    from pulpo_amd._lib import PulpoHipError
    g = torch.Generator(device=DEV).manual_seed(1)
    n = 4101
    base = [torch.randn(n, device=DEV, generator=g) for _ in range(4)]
    a = [base[0].clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [t.clone() for t in a]
    val = torch.zeros(1, device=DEV)
    ops.anchored_adam_step(a[0], base[1], a[1], a[2], 0.1, 1, mean=base[2], prec=base[3].abs(), loss_out=val)
    ops.anchored_adam_step(b[0], base[1], b[1], b[2], 0.1, 1, mean=base[2], prec=base[3].abs())
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and float(val) > 0.0
    arena = torch.zeros(n + 1, device=DEV)
    before = a[0].clone()
    for bad in range(6):
        args = [a[0], base[1], a[1], a[2], base[2], base[3]]
        args[bad] = arena[1:]
        with pytest.raises(PulpoHipError, match="16-byte"):
            ops.anchored_adam_step(args[0], args[1], args[2], args[3], 0.1, 2, mean=args[4], prec=args[5])
    with pytest.raises(ValueError):
        ops.anchored_adam_step(a[0], base[1], a[1], a[2], 0.1, 2, prec=base[3])
    for bad in range(6):                                 # every array is fp32: another dtype of the same element count is refused, not reinterpreted
        for dt in (torch.float64, torch.bfloat16):
            args = [a[0], base[1], a[1], a[2], base[2], base[3]]
            args[bad] = args[bad].to(dt)
            with pytest.raises(PulpoHipError, match="fp32"):
                ops.anchored_adam_step(args[0], args[1], args[2], args[3], 0.1, 2, mean=args[4], prec=args[5])
    with pytest.raises(PulpoHipError, match="fp32"):
        ops.anchored_adam_step(a[0], base[1], a[1], a[2], 0.1, 2, mean=base[2], loss_out=torch.zeros(1, device=DEV, dtype=torch.float64))
    assert torch.equal(a[0], before) and not bool(arena.any())


# ================================================================================================ one iteration: objective and gradient
# (T, L, size, B): the shapes that have goldens
CASES = [(3, 2, (16, 16, 16), 1), (3, 2, (16, 16, 16), 2), (4, 3, (16, 24, 16), 1), (3, 2, (32, 24), 1)]
# NCC, ["mind"] (3-D only: ops.mind_loss refuses slices), NCC with a ball x rand mask pair
OBJECTIVE_PARAMS = [c + (v,) for c in CASES for v in ("ncc", "mind", "masked") if not (v == "mind" and len(c[2]) == 2)]


def _case_inputs(T, L, size, B, variant):
    cfg = O.Cfg(T, L, list(size))
    x, y = RR.pair(size, B, 11 + len(size) + B)
    g = torch.Generator().manual_seed(5 + T)
    v = {l: 0.5 * torch.randn(s, dtype=torch.float64, generator=g) for l, s in RR.level_shapes(cfg, B).items()}
    kw = {}
    if variant == "mind":
        kw["recon"] = ("mind",)
    if variant == "masked":
        kw["mask_x"] = MK.ball(B, size).double()
        kw["mask_y"] = torch.rand(B, 1, *size, dtype=torch.float64, generator=g)
    return cfg, x, y, v, kw


@functools.lru_cache(maxsize=None)
def _objective_reference(T, L, size, B, variant):
    cfg, x, y, v, kw = _case_inputs(T, L, size, B, variant)
    leaves = {l: t.clone().requires_grad_(True) for l, t in v.items()}
    total, sim, reg, _ = RR.objective(leaves, x, y, cfg, **kw)
    grads = torch.autograd.grad(UP * total, [leaves[l] for l in sorted(leaves)])
    return sim.detach(), reg.detach(), {l: gr for l, gr in zip(sorted(leaves), grads)}


@pytest.mark.parametrize("T,L,size,B,variant", OBJECTIVE_PARAMS)
def test_objective_and_gradient_vs_float64(api, T, L, size, B, variant):
    """refine.Objective at random level fields: similarity and regulariser to 1e-4 |ref|, the gradient with respect to every level's field
    (upstream factor 1.7) to 5e-5 max|ref| element by element, against autograd through refine_ref.objective in float64"""
    models, _, _, refine, _ = api
    cfg, x, y, v, kw = _case_inputs(T, L, size, B, variant)
    model = make_model(models, T, L, size)
    obj = refine.Objective(model, x.float().to(DEV), y.float().to(DEV), recon_loss=["mind"] if variant == "mind" else None,
                           mask_x=kw["mask_x"].float().to(DEV) if variant == "masked" else None,
                           mask_y=kw["mask_y"].float().to(DEV) if variant == "masked" else None)
    leaves = {l: t.float().to(DEV).requires_grad_(True) for l, t in v.items()}
    with torch.enable_grad():
        rec, reg, _, _ = obj(leaves)
        grads = torch.autograd.grad(rec + reg, [leaves[l] for l in sorted(leaves)], grad_outputs=torch.tensor(UP, device=DEV))
    sim64, reg64, g64 = _objective_reference(T, L, size, B, variant)
    name = f"objective T{T}/L{L}/{size}/B{B}/{variant}"
    for tag, got, ref in (("similarity", rec, sim64), ("regulariser", reg, reg64)):
        dev = abs(float(got.detach()) - float(ref)) / abs(float(ref))
        print(f"RATIO {name} {tag} {dev / 1e-4:.3g}")
        assert dev <= 1e-4, (tag, float(got.detach()), float(ref))
    for l, got in zip(sorted(leaves), grads):
        check(f"{name} grad level {l}", got, g64[l], 5e-5 * amax(g64[l]))
    assert all(p.grad is None for p in model.parameters())


# ================================================================================================ the loop
LOOP_CFG = (3, 2, (16, 16, 16), 1)


class _GivenVariance:
    """stands in for the N-sample start of refine._start: zero fields with a given per-voxel variance"""

    def __init__(self, v0, var):
        self.v0, self.var = v0, var

    def __call__(self, model, x, y, individual_dfs, N):
        return self.v0, self.var


@pytest.mark.parametrize("anchor", [0.0, 0.1])
def test_loop_vs_float64(api, anchor, monkeypatch):
    """refine() from zero fields, lr 0.03, 20 iterations, without an anchor and with anchor 0.1 on a synthetic variance map (handed in where
    the N posterior samples' variance would come from): the final individual_dfs element by element within FIELD_TOL voxels, history row
    by row within HIST_TOL |history[0, 0]| of refine_ref.loop in float64.
    fp32 CPU run of refine_ref.loop against float64 over the two cases: fields FIELD_OWN voxels, history HIST_OWN (refine_ref); the bounds
    are 8 x those.  On the MI355X (profiles/refine_gpu_tests.txt, this file's pytest -s output): fields 0.16 of the bound (1.8e-6 voxels), history 0.13
    (2.8e-7)."""
    models, _, _, refine, _ = api
    T, L, size, B = LOOP_CFG
    cfg, x, y, v0, var, _ = RR.loop_inputs(LOOP_CFG, anchor, torch.float32)
    model = make_model(models, T, L, size)
    to = lambda d: {l: t.to(DEV) for l, t in d.items()}
    if anchor:
        monkeypatch.setattr(refine, "_start", _GivenVariance(to(v0), to(var)))
        res = refine.refine(model, x.to(DEV), y.to(DEV), N=2, iters=20, lr=0.03, anchor=anchor)
    else:
        res = refine.refine(model, x.to(DEV), y.to(DEV), individual_dfs=to(v0), iters=20, lr=0.03)
    f64, h64 = RR.loop_reference(LOOP_CFG, anchor)
    for l in f64:
        check(f"loop anchor={anchor} field level {l}", res["individual_dfs"][l], f64[l], FIELD_TOL)
    scale = abs(float(h64[0, 0]))
    assert res["history"].shape == (21, 4)
    for i in range(21):
        check(f"loop anchor={anchor} history row {i}", res["history"][i], h64[i], HIST_TOL * scale, power=None)
    assert R.ratio(res["history"].cpu(), R.perturbed(h64, 4 * 20), HIST_TOL * scale) > 1.0
    if anchor:
        assert float(res["history"][-1, 3]) > 0.0 and float(res["history"][0, 3]) == 0.0


# ================================================================================================ behaviour
@pytest.fixture(scope="module")
def setup(api):
    models, nb = api[0], api[1]
    size = (16, 16, 16)
    model = make_model(models, 3, 2, size, seed=4)
    pin_noise(model, nb, 1)
    x, y = RR.pair(size, 1, 21, dtype=torch.float32)
    return model, x.to(DEV), y.to(DEV)


def _same(a, b):
    return all(torch.equal(a[k][l], b[k][l]) for k in ("individual_dfs", "combined_dfs", "final_dfs", "outputs") for l in a[k]) \
        and torch.equal(a["history"], b["history"])


def test_refine_descends_and_leaves_the_model_alone(api, setup):
    """from the untrained model's predict_deterministic start the total objective drops; afterwards every parameter's .grad is None and the
    state dict (BatchNorm statistics included) is bitwise unchanged; the result is the same under an outer no_grad and - deterministic
    mode - from call to call"""
    ops = api[2]
    model, x, y = setup
    before = {k: t.clone() for k, t in model.state_dict().items()}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        res = model.refine(x, y, iters=8, lr=0.03)
        with torch.no_grad():
            res_ng = model.refine(x, y, iters=8, lr=0.03)
        res2 = model.refine(x, y, iters=8, lr=0.03)
    finally:
        ops.set_deterministic(prev)
    h = res["history"]
    print(f"FIGURE refine from the prediction: total {float(h[0, 0]):.4f} -> {float(h[-1, 0]):.4f}")
    assert float(h[-1, 0]) < float(h[0, 0]) and bool(torch.isfinite(h).all()) and bool((h[:, 3] == 0).all())
    assert all(p.grad is None for p in model.parameters())
    after = model.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert _same(res, res_ng), "refine under torch.no_grad() differs"
    assert _same(res, res2), "two deterministic calls differ"
    assert res["anchor_prec"] is None and sorted(res["outputs"]) == [0, 1] and tuple(res["outputs"][1].shape[2:]) == (4, 4, 4)
    start = model.predict_deterministic(x, y)[1]
    assert all(not torch.equal(start[l], res["individual_dfs"][l]) for l in start)


def cycling_noise(nb, eps_list):
    """a FixedNoiseSampler whose noise advances through eps_list with every draw"""
    class Cycling(nb.FixedNoiseSampler):
        def __init__(self, eps):
            self.eps_list, self.draws = eps, 0

        @property
        def fixed_eps(self):
            self.draws += 1
            return self.eps_list[(self.draws - 1) % len(self.eps_list)]
    return Cycling(eps_list)


def test_anchor_precision_from_posterior_samples(api):
    """N = 4 with the samplers pinned to four known draws: anchor_mean is the mean and anchor_prec = anchor * kl_w[l] / (var + floor) (B = 1)
    of the four individual_dfs drawn by hand with the same noise; with iters = 0 the fields returned are that mean"""
    models, nb, _, refine, _ = api
    size, N, anchor, floor = (16, 16, 16), 4, 0.1, 1e-4
    model = make_model(models, 3, 2, size, seed=6)
    g = torch.Generator().manual_seed(9)
    eps = {l: [torch.randn(1, 3, *model.autoencoder.level_sizes[l + 1], generator=g).to(DEV) for _ in range(N)] for l in range(2)}
    x, y = (t.to(DEV) for t in RR.pair(size, 1, 5, dtype=torch.float32))
    samples = []
    with torch.no_grad():
        for k in range(N):
            for l in range(2):
                model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l][k])
            samples.append(model.autoencoder(x, model.downpath(x, y))[4])
    for l in range(2):
        model.autoencoder.encoders[l].sampler = cycling_noise(nb, eps[l])
    res = refine.refine(model, x, y, N=N, iters=0, anchor=anchor, anchor_floor=floor)
    kl_w = model.hierarchical_kl_loss.weight_dict
    for l in range(2):
        stack = torch.stack([s[l] for s in samples]).double()
        mean, var = stack.mean(0), stack.var(0, unbiased=True)
        assert float(var.max()) > 1e-6, "the four draws do not differ"
        want = anchor * kl_w[l] / (var + floor)
        check(f"anchor mean level {l}", res["anchor_mean"][l], mean, 1e-6 * amax(mean))
        r = float(((res["anchor_prec"][l].double() - want).abs() / want).max())
        print(f"RATIO anchor prec level {l} {r / 1e-4:.3g}")
        assert r <= 1e-4
        assert torch.equal(res["individual_dfs"][l], res["anchor_mean"][l])
    assert res["history"].shape == (1, 4) and float(res["history"][0, 3]) == 0.0


def test_performance_scores_the_refined_fields(api, setup):
    """performance(refine={...}) = level_scores on refine(...)'s fields, bit for bit in deterministic mode, inverse rows included;
    refine=None is today's call"""
    _, _, ops, refine, evaluation = api
    model, x, y = setup
    kw = {"iters": 5, "lr": 0.03}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            got = evaluation.performance(model, x, y, refine=kw)
            got_inv = evaluation.performance(model, x, y, refine=kw, inverse=True)
            res = refine.refine(model, x, y, **kw)
            want = evaluation.level_scores(res["outputs"], res["final_dfs"], y)
            _, fin, inv = model.combine_dfs_bidirectional(res["individual_dfs"])
            want_inv = evaluation.level_scores(res["outputs"], fin, y, final_dfs_inv=inv)
            plain = evaluation.performance(model, x, y)
            outputs, ind = model.predict_deterministic(x, y)
            today = evaluation.level_scores(outputs, model.combine_dfs(ind)[1], y)
    finally:
        ops.set_deterministic(prev)
    for a, b in ((got, want), (got_inv, want_inv), (plain, today)):
        assert a.keys() == b.keys()
        for k in a:
            for l in a[k]:
                assert torch.equal(a[k][l], b[k][l]), (k, l, float(a[k][l]), float(b[k][l]))
    assert "InvCons" in got_inv and "InvCons" not in got
    assert float(got["RMSE"][0]) != float(plain["RMSE"][0])
