"""CPU-side tests of instance-specific refinement: the float64 definition of tests/refine_ref.py (its Adam is
torch.optim.Adam's, its field operators the oracle's, its loop descends on the case measured for the issue) and the public surface of the
feature as far as it exists without a GPU (entry point, argument checks, arena layout, the refused 'dice' term)."""
import ctypes
import inspect

import pytest
import torch

import pyramid_ref as R
import refine_ref as RR
from oracle import pulpo_oracle as O

FB = list(O.FEEDBACK_DEFAULT)


# ================================================================================================ the reference's own properties
@pytest.mark.parametrize("n", [1, 5, 630])
@pytest.mark.parametrize("form", ["none", "mean", "mean+prec"])
def test_reference_update_is_torch_adam_with_the_anchor_gradient_added(n, form):
    """three steps from zero moments against torch.optim.Adam in float64, the anchor's gradient a (p - mean) added to g by hand; the value
    returned is 1/2 sum a (p - mean)^2 at the iterate before the update"""
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, dtype=torch.float64, generator=g)
    mean = torch.randn(n, dtype=torch.float64, generator=g) if form != "none" else None
    prec = torch.rand(n, dtype=torch.float64, generator=g) * 3 if form == "mean+prec" else None
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=0.03)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        gr = torch.randn(n, dtype=torch.float64, generator=g)
        a = 0.0 if mean is None else (prec if prec is not None else 1.0) * (tp.detach() - mean)
        want_val = 0.0 if mean is None else float(0.5 * torch.sum((prec if prec is not None else 1.0) * (tp.detach() - mean) ** 2))
        tp.grad = gr + a
        opt.step()
        p, m, v, val = RR.adam_update(p, gr, m, v, 0.03, step, mean, prec)
        torch.testing.assert_close(p, tp.detach(), rtol=1e-13, atol=1e-15)
        assert abs(float(val) - want_val) <= 1e-13 * max(1.0, abs(want_val))
    st = opt.state[tp]
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=0.0)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=0.0)


def test_reference_field_operators_are_the_oracles():
    """the rank-generic warp / vecint / resize / combine_dfs / level images of refine_ref equal oracle.pulpo_oracle's on volumes, bit for bit"""
    cfg = O.Cfg(4, 3, [16, 24, 16])
    g = torch.Generator().manual_seed(2)
    x = torch.rand(1, 1, 16, 24, 16, dtype=torch.float64, generator=g)
    v = {l: torch.randn(s, dtype=torch.float64, generator=g) for l, s in RR.level_shapes(cfg, 1).items()}
    assert [tuple(t.shape[2:]) for t in v.values()] == [(8, 12, 8), (4, 6, 4), (2, 3, 2)]
    assert torch.equal(RR.warp(v[0], x), O.warp(v[0], x)) and torch.equal(RR.vecint(v[1]), O.vecint(v[1]))
    assert torch.equal(RR.resize_field(v[1], 0.5), O.resize_field(v[1], 0.5)) and torch.equal(RR.pool2(x), O.pool2(x))
    (c0, f0), (c1, f1) = RR.combine_dfs(v, cfg), O.combine_dfs(v, cfg)
    for l in v:
        assert torch.equal(c0[l], c1[l]) and torch.equal(f0[l], f1[l])
    assert tuple(f0[0].shape[2:]) == (16, 24, 16) and tuple(f0[1].shape[2:]) == (4, 6, 4)
    lx = RR.level_images(x, cfg)
    assert torch.equal(lx[0], x) and torch.equal(lx[1], O.pool2(O.pool2(x))) and torch.equal(lx[2], O.pool2(lx[1]))


def test_reference_objective_is_the_training_steps_loss_block():
    """at the fields of an oracle forward pass, similarity + regulariser of refine_ref.objective are rec + reg of O.losses"""
    cfg = O.Cfg(3, 2, [16, 16, 16], n0=2)
    sd = O.init_state_dict(cfg, seed=1)
    x, y = RR.pair(cfg.input_size, 2, 3, dtype=torch.float32)
    with torch.no_grad():
        outs = O.forward(sd, cfg, x, y, eps=None, training=True)
        _, _, rec, reg, _, _, _ = O.losses(outs, y, cfg)
        total, sim, r, anc = RR.objective(outs[4], x, y, cfg)
    torch.testing.assert_close(sim, rec, rtol=1e-5, atol=0.0)
    torch.testing.assert_close(r, reg, rtol=1e-5, atol=0.0)
    assert float(anc) == 0.0 and float(total) == float(sim + r)


LOOP_CASE = (3, 2, (16, 16, 16), 1)


def test_reference_loop_descends_from_zero_fields():
    """T3 / L2 at 16^3, lr 0.03, 20 iterations from zero fields: the history's last total is below its first and no step rises"""
    fields, hist = RR.loop_reference(LOOP_CASE, 0.0)
    assert hist.shape == (21, 4) and bool((hist[:, 3] == 0).all())
    torch.testing.assert_close(hist[:, 0], hist[:, 1] + hist[:, 2], rtol=1e-14, atol=0.0)
    assert float(hist[-1, 0]) < float(hist[0, 0]) - 10.0
    assert float((hist[1:, 0] - hist[:-1, 0]).max()) < 0.0
    assert 0.1 < max(float(t.abs().max()) for t in fields.values()) < 2.0
    _, hist_a = RR.loop_reference(LOOP_CASE, 0.1)
    assert float(hist_a[0, 3]) == 0.0 and float(hist_a[-1, 3]) > 0.0 and float(hist_a[-1, 0]) < float(hist_a[0, 0])
    torch.testing.assert_close(hist_a[:, 0], hist_a[:, 1:].sum(1), rtol=1e-14, atol=0.0)


def test_loop_bounds_are_the_fp32_references_own_error():
    """refine_ref.FIELD_OWN / HIST_OWN, which the GPU test's bounds are 8 x, are what an fp32 CPU run of refine_ref.loop gives against
    float64 on the tests' inputs: re-measured, at most 25 % above the constants and not below a fifth of them"""
    worst_f = worst_h = 0.0
    for anchor in (0.0, 0.1):
        f64, h64 = RR.loop_reference(LOOP_CASE, anchor)
        f32, h32 = RR.loop_reference(LOOP_CASE, anchor, torch.float32)
        worst_f = max(worst_f, max(R.ratio(f32[l], f64[l], 1.0) for l in f64))
        worst_h = max(worst_h, R.ratio(h32, h64, abs(float(h64[0, 0]))))
    print(f"FIGURE fp32 reference: fields {worst_f:.3g} voxels, history {worst_h:.3g}")
    assert 0.2 * RR.FIELD_OWN <= worst_f <= 1.25 * RR.FIELD_OWN, worst_f
    assert 0.2 * RR.HIST_OWN <= worst_h <= 1.25 * RR.HIST_OWN, worst_h


# ================================================================================================ the public surface
def test_header_declares_the_entry_point_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    assert "pulpo_anchored_adam_step" in protos
    restype, args = protos["pulpo_anchored_adam_step"]
    P, F32, F64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    assert restype is ctypes.c_int
    assert args == [P, P, P, P, P, P, ctypes.c_int64, F32, F64, F64, F32, ctypes.c_int, P, P]
    assert header_abi_version() == 8


def test_names_and_signatures():
    from pulpo_amd import evaluation, ops, refine as refine_mod
    import src.models as models
    names = list(inspect.signature(ops.anchored_adam_step).parameters)
    assert names == ["p", "g", "m", "v", "lr", "step", "mean", "prec", "loss_out", "beta1", "beta2", "eps"]
    sig = inspect.signature(refine_mod.refine).parameters
    assert list(sig) == ["model", "x", "y", "individual_dfs", "N", "iters", "lr", "anchor", "anchor_floor", "recon_loss", "lamb", "gamma", "mask_x",
                         "mask_y"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    assert (sig["N"].default, sig["iters"].default, sig["anchor"].default, sig["anchor_floor"].default) == (1, 50, 0.0, 1e-4)
    assert sig["lr"].default == refine_mod.DEFAULT_LR and refine_mod.DEFAULT_LR in (0.01, 0.03, 0.1, 0.3)
    assert inspect.signature(evaluation.performance).parameters["refine"].default is None
    assert callable(models.PULPo.refine)
    from pulpo_amd.components.pulpo import Autoencoder
    assert callable(Autoencoder.level_images)


def test_cpu_tensors_are_refused():
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    p, g, m, v = (torch.zeros(8) for _ in range(4))
    with pytest.raises(PulpoHipError):
        ops.anchored_adam_step(p, g, m, v, 0.1, 1)
    with pytest.raises(PulpoHipError):
        ops.anchored_adam_step(p, g, m, v, 0.1, 1, mean=torch.zeros(8), prec=torch.ones(8), loss_out=torch.zeros(1))


def test_library_refuses_bad_arguments():
    """null arrays, n < 1, step < 1, prec without mean, an array that is not 16-byte aligned: the library's error code, no launch"""
    from pulpo_amd._lib import lib
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    f = lib.raw("pulpo_anchored_adam_step")
    tail = (0.1, 0.9, 0.999, 1e-8)
    assert f(None, p, p, p, None, None, 4, *tail, 1, None, None) != 0 and f(p, None, p, p, None, None, 4, *tail, 1, None, None) != 0
    assert f(p, p, None, p, None, None, 4, *tail, 1, None, None) != 0 and f(p, p, p, None, None, None, 4, *tail, 1, None, None) != 0
    assert f(p, p, p, p, None, None, 0, *tail, 1, None, None) != 0 and f(p, p, p, p, None, None, 4, *tail, 0, None, None) != 0
    assert f(p, p, p, p, None, p, 4, *tail, 1, None, None) != 0                                  # prec without mean
    assert b"prec needs mean" in lib.raw("pulpo_last_error")()
    for bad in range(6):
        args = [p] * 6
        args[bad] = off
        assert f(*args, 4, *tail, 1, None, None) != 0, bad
        assert b"16-byte aligned" in lib.raw("pulpo_last_error")()


def test_arena_layout_pads_levels_to_16_bytes():
    from pulpo_amd.refine import arena_layout
    offsets, total = arena_layout([(1, 3, 5, 6, 7), (1, 3, 10, 10, 10), (2, 2, 5, 3)])
    assert offsets == [0, 632, 632 + 3000] and total == 632 + 3000 + 60
    offsets, total = arena_layout([(1, 3, 10, 10, 10), (1, 3, 5, 6, 7), (1, 3, 3, 3, 3)])
    assert offsets == [0, 3000, 3632] and total == 3632 + 84
    assert all(o % 4 == 0 for o in offsets) and total % 4 == 0
    assert arena_layout([]) == ([], 0)


def test_dice_is_refused_before_the_device_is_touched():
    """a CPU model and CPU tensors: the ValueError comes before any operator (which would refuse the CPU tensors with PulpoHipError)"""
    import src.models as models
    from pulpo_amd.refine import refine
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2)
    x = torch.rand(1, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="dice"):
        refine(m, x, x, recon_loss=["dice"])
    with pytest.raises(ValueError, match="dice"):
        m.refine(x, x, recon_loss=["ncc", "dice"])
    with pytest.raises(ValueError, match="recon_loss"):
        refine(m, x, x, recon_loss=["nmi"])
    md = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2, recon_loss=["ncc", "dice"])
    with pytest.raises(ValueError, match="dice"):
        refine(md, x, x)
