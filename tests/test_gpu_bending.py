"""The bending-energy regulariser on the device against the float64 definition of tests/bending_ref.py, evaluated with
plain torch ops on the GPU: value and gradient element by element at the shapes where bending.hip changes path, the vector and the scalar
kernels against each other, run-to-run bits, affine invariance, and the feature's way through the training step, refine() and the score table.

Bounds are the project's own for the L2 regulariser (tests/test_gpu_pyramid_ops.py): loss 1e-5 |ref|, gradient 1e-7 max(1, max|ref|) +
1e-4 |ref| per element.  torch's own float32 evaluation of the definition sits at <= 0.18 of the gradient bound on these inputs (measured on
the CPU for the listed shapes).  Every comparison is shown to have power: the same bound must reject the reference with one border-plane
element moved by 1e-3 max|ref|."""
import pytest
import torch

import bending_ref as BR
import pyramid_ref as R
import refine_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
FB = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
LAMB, UP = 0.025, 1.7


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd import evaluation, losses, ops, refine
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb, ops, refine, evaluation, losses


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


def _offset_copy(x):
    """x's values in a buffer that starts one float past an allocation: same shape, contiguous, 4-byte aligned only (the scalar kernels)"""
    buf = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    y = buf[1:1 + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.is_contiguous() and y.data_ptr() % 16 != 0
    return y


def _value_and_grad(ops, u):
    x = u.detach().requires_grad_(True)
    loss = ops.bending_reg(x, LAMB)
    g, = torch.autograd.grad(loss, [x], grad_outputs=torch.tensor(UP, device=DEV))
    return loss.detach(), g


def _reference(u):
    r64 = u.detach().double()
    return BR.bending_ref(r64, LAMB), BR.bending_grad_ref(r64, LAMB, UP)


def _grad_tol(rg):
    return 1e-7 * max(1.0, amax(rg)) + 1e-4 * rg.abs()


def _hold(name, loss, g, ref, rg):
    check(name + " loss", loss, ref, 1e-5 * abs(float(ref)))
    check(name + " grad", g, rg, _grad_tol(rg))                     # (power: the last element, a corner of three border planes)
    check(name + " grad (first plane)", g, rg, _grad_tol(rg), power=1)


# bending.hip's tile: kTX = 32 voxels of a row, kTY = 16 rows; a workgroup marches over 16, 8 or 4 planes - the longest march that leaves the
# grid 1024 workgroups, else 4 (so 4 at the small shapes, 8 and 16 only with many planes or a large volume).  (B, C, D, H, W)
SHAPES = [
    (1, 3, 3, 3, 3),                                      # the interior is one voxel
    (1, 3, 4, 4, 4),
    (2, 3, 5, 6, 7),                                      # scalar path, every voxel within 2 of a border
    (2, 3, 9, 10, 36),                                    # vector path, two tiles along x
    (1, 3, 20, 24, 20),
    (1, 3, 40, 40, 40),
    (1, 2, 1, 20, 24), (2, 2, 1, 5, 7),                   # the 2-D form
    (1, 1, 4, 5, 31), (1, 1, 4, 5, 33), (1, 1, 4, 5, 65), # W at kTX - 1, kTX + 1, 2 kTX + 1 (scalar path: W % 4 != 0)
    (1, 1, 3, 4, 28), (1, 1, 3, 4, 36), (1, 1, 3, 4, 68), # ... and the vector path's nearest: kTX - 4, kTX + 4, 2 kTX + 4
    (1, 2, 4, 15, 8), (1, 2, 4, 17, 8), (1, 2, 4, 33, 8), # H at kTY - 1, kTY + 1, 2 kTY + 1
    (1, 2, 3, 5, 8), (1, 2, 5, 5, 8), (1, 2, 9, 5, 8),    # D at 4 - 1, 4 + 1, 2 * 4 + 1: marches of 4
    (1, 2, 15, 5, 8), (1, 2, 17, 5, 8), (1, 2, 33, 5, 8), # ... of 4 still: 15 = 4 * 4 - 1, 17 = 4 * 4 + 1, 33 = 8 * 4 + 1
    (32, 4, 9, 17, 33), (32, 4, 15, 17, 33), (32, 3, 17, 17, 33),     # marches of 8 (512, 512, 384 tiles a plane slab): D at 8 + 1, 16 - 1, 16 + 1
    (32, 4, 15, 33, 65), (32, 4, 17, 33, 65), (32, 4, 33, 33, 65),    # marches of 16 (1152 tiles): D at 16 - 1, 16 + 1, 32 + 1
    (1, 3, 160, 160, 160),                                # the flagship's level 0: marches of 16, vector path
]


@pytest.mark.parametrize("shape", SHAPES)
def test_value_and_gradient_vs_float64(api, shape):
    ops = api[2]
    u = torch.randn(shape, device=DEV, generator=gen(sum(s * 7 ** i for i, s in enumerate(shape))))
    ref, rg = _reference(u)
    loss, g = _value_and_grad(ops, u)
    _hold(f"bending {shape}", loss, g, ref, rg)
    if shape[2] == 1:                                                    # the same slices as a 4-D (B,C,H,W) tensor
        loss4, g4 = _value_and_grad(ops, u[:, :, 0])
        ref4, rg4 = _reference(u[:, :, 0])
        assert g4.shape == u[:, :, 0].shape and abs(float(ref4) - float(ref)) <= 1e-12 * abs(float(ref))
        _hold(f"bending {shape} as 4-D", loss4, g4, ref4, rg4)


def test_smooth_field_of_large_amplitude(api):
    """a smoothed field of 4 voxels amplitude at 40^3 (second differences far below the values: the cancellation case)"""
    ops = api[2]
    u = torch.randn(1, 3, 40, 40, 40, device=DEV, generator=gen(5))
    for _ in range(4):
        u = torch.nn.functional.avg_pool3d(u, 5, stride=1, padding=2, count_include_pad=False)
    u = u * (4.0 / amax(u))
    ref, rg = _reference(u)
    loss, g = _value_and_grad(ops, u)
    _hold("bending smooth 40^3", loss, g, ref, rg)


@pytest.mark.parametrize("shape", [(2, 3, 9, 10, 36), (1, 3, 20, 24, 20), (1, 2, 1, 20, 24)])
def test_vector_and_scalar_kernels_agree(api, shape):
    """W % 4 == 0: the aligned tensor takes the 16-byte loads, its copy one float past an allocation the 4-byte loads; a view that starts at an
    odd x of a wider tensor is made planar first.  All three against float64 and against each other, to the same bounds"""
    ops = api[2]
    wide = torch.randn(shape[:-1] + (shape[-1] + 3,), device=DEV, generator=gen(shape[-1]))
    view = wide[..., 1:1 + shape[-1]]
    assert not view.is_contiguous()
    u = view.contiguous()
    ref, rg = _reference(u)
    got = {"aligned": _value_and_grad(ops, u), "offset": _value_and_grad(ops, _offset_copy(u)), "view": _value_and_grad(ops, view)}
    for path, (loss, g) in got.items():
        _hold(f"bending {shape} {path}", loss, g, ref, rg)
    tol = _grad_tol(rg)
    for path in ("offset", "view"):
        assert R.ratio(got[path][1], got["aligned"][1].double(), tol) <= 1.0, path
        assert abs(float(got[path][0]) - float(got["aligned"][0])) <= 1e-5 * abs(float(ref)), path
    assert torch.equal(got["view"][1], got["aligned"][1]) and torch.equal(got["view"][0], got["aligned"][0])


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_calls_give_the_same_bits(api, deterministic):
    """no atomics: value and gradient bit-identical from call to call, in deterministic mode and out of it"""
    ops = api[2]
    prev = ops.DETERMINISTIC
    ops.set_deterministic(deterministic)
    try:
        for shape in ((1, 3, 20, 24, 20), (2, 3, 9, 10, 11), (1, 2, 1, 20, 24)):
            u = torch.randn(shape, device=DEV, generator=gen(11))
            a, b = _value_and_grad(ops, u), _value_and_grad(ops, u)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), shape
            assert float(a[0]) > 0.0
    finally:
        ops.set_deterministic(prev)


def test_affine_field_costs_nothing_on_the_device(api):
    """a random affine displacement field of 12 x 14 x 16: float32 rounding only (about 1e-12 in torch), where L2_reg charges about 1"""
    ops = api[2]
    theta = (torch.eye(3, 4).unsqueeze(0) + 0.1 * torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(0))).to(DEV)
    u = ops.affine_field(theta, (12, 14, 16))
    bend, first = float(ops.bending_reg(u, LAMB)), float(ops.l2_reg(u, LAMB))
    print(f"FIGURE affine field 12x14x16: bending {bend:.3g}, L2 {first:.3g}")
    assert first > 0.1 and 0.0 <= bend <= 1e-6 * first


def test_argument_checks_on_the_device(api):
    ops, losses = api[2], api[5]
    for shape in ((1, 3, 2, 5, 6), (1, 3, 4, 2, 6), (1, 3, 4, 5, 2), (1, 2, 2, 6), (1, 2, 1, 5, 2)):
        with pytest.raises(ValueError, match=str(shape[-1]) + r"\)"):
            ops.bending_reg(torch.zeros(shape, device=DEV), 0.1)
    with pytest.raises(ValueError):
        losses.Bending_reg(torch.zeros(1, 3, 2, 5, 6, device=DEV), 0.1)
    assert float(ops.bending_reg(torch.zeros(1, 3, 3, 3, 3, device=DEV), 0.1)) == 0.0


# ================================================================================================ the model
def _model(models, **kw):
    torch.manual_seed(0)
    return models.PULPo(3, 3, 0.1, [16, 16, 16], feedback=FB, n0=2, regularizer="bending", **kw).to(DEV)


def _pin_noise(model, nb, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    for l in range(model.latent_levels):
        shape = (B, model.ndims) + tuple(model.autoencoder.level_sizes[l + model.lk_offset])
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(shape, generator=g).to(DEV))


def _pair():
    return tuple(t.to(DEV) for t in RR.pair((16, 16, 16), 1, 5, dtype=torch.float32))


def _reference_sum(model, final_dfs, lamb):
    w = model.hierarchical_regularization.weight_dict
    assert sorted(w) == sorted(final_dfs) == [0, 1, 2]
    return sum(w[l] * float(BR.bending_ref(final_dfs[l].detach().double(), lamb)) for l in w)


def test_training_step_with_the_bending_regulariser(api):
    """one step of a 16^3 / 3-level model: the logged regularisation term is sum_l reg_w[l] * ref(final_dfs[l]); every parameter gradient is
    finite; the regulariser's own gradient reaches the decoders (non-zero on the last VelocityField weights of every level)"""
    models = api[0]
    model = _model(models).train()
    x, y = _pair()
    seen = {}
    hook = model.hierarchical_regularization.register_forward_hook(lambda mod, args, out: seen.update(dfs=args[0]))
    total = model.training_step((x, y, None, None, None, None, None, None), 0)
    hook.remove()
    assert [tuple(seen["dfs"][l].shape[2:]) for l in (0, 1, 2)] == [(16, 16, 16), (8, 8, 8), (4, 4, 4)]
    want = _reference_sum(model, seen["dfs"], model.hparams.lamb)
    got = float(model.logged["train/regularization_loss"].detach())
    print(f"FIGURE training step: regularisation term {got:.6g}, reference {want:.6g}, ratio to 1e-5 {abs(got - want) / (1e-5 * abs(want)):.3g}")
    assert want > 0.0 and abs(got - want) <= 1e-5 * abs(want)
    total.backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}        # (parameters outside the step's graph have none)
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(any(k.startswith(f"autoencoder.decoders.{l}.velocity_field") and k.endswith("weight") for k in grads) for l in range(3))
    model.zero_grad(set_to_none=True)
    reg = model._forward_and_losses(x, y)[2][3]
    reg.backward()
    for l in range(3):
        w = model.autoencoder.decoders[l].velocity_field._op[-1].weight
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and amax(w.grad) > 0.0, l


def test_refine_descends_on_the_models_regulariser(api):
    models, nb, _, refine, _, _ = api
    model = _model(models).eval()
    _pin_noise(model, nb, 1)
    x, y = _pair()
    res = refine.refine(model, x, y, iters=0)
    want = _reference_sum(model, res["final_dfs"], model.hparams.lamb)
    got = float(res["history"][0, 2])
    print(f"FIGURE refine: regulariser {got:.6g}, reference {want:.6g}")
    assert want > 0.0 and abs(got - want) <= 1e-5 * abs(want)
    res = refine.refine(model, x, y, iters=3, lr=0.03)
    assert bool(torch.isfinite(res["history"]).all()) and float(res["history"][-1, 0]) < float(res["history"][0, 0])


def test_score_row(api):
    """performance(..., bending=True): BendingE[l] = ref(final_dfs[l], 1) / (D H W), of the affine-composed fields with affine=; without the
    flag the rows are what they were"""
    models, nb, ops, _, evaluation, _ = api
    model = _model(models).eval()
    _pin_noise(model, nb, 1)
    x, y = _pair()
    plain = evaluation.performance(model, x, y)
    got = evaluation.performance(model, x, y, bending=True)
    assert set(plain) == {"RMSE", "JDetStd", "JDetLeq0"} and set(got) == set(plain) | set(evaluation.BENDING_METRICS)
    assert all(torch.equal(plain[k][l], got[k][l]) for k in plain for l in plain[k])
    with torch.no_grad():
        final = model.combine_dfs(model.predict_deterministic(x, y)[1])[1]
    theta = (torch.eye(3, 4).unsqueeze(0) + 0.05 * torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(2))).to(DEV)
    got_aff = evaluation.performance(model, x, y, affine=theta, bending=True)
    with torch.no_grad():
        final_aff = model.combine_dfs(model.predict_deterministic(ops.affine_warp(theta, x), y)[1])[1]
        final_aff = {l: ops.affine_compose(theta, df, x.shape[2:]) for l, df in final_aff.items()}
    for name, scores, fields in (("plain", got, final), ("affine", got_aff, final_aff)):
        assert sorted(scores["BendingE"]) == [0, 1, 2]
        for l, df in fields.items():
            v = scores["BendingE"][l]
            assert v.is_cuda and v.dim() == 0
            want = float(BR.bending_ref(df.double(), 1.0)) / float(df[0, 0].numel())
            print(f"FIGURE BendingE {name} level {l}: {float(v):.6g}, reference {want:.6g}")
            assert want > 0.0 and abs(float(v) - want) <= 1e-5 * want, (name, l)
    table = evaluation.PerformanceTable(evaluation.METRICS + evaluation.BENDING_METRICS, 3, ["a"], 1)
    table.add(0, 0, got)
    assert table.mean()[0].shape == (3, len(evaluation.METRICS) + 1)
