"""The weight-gradient launches under a workgroup budget (pulpo_conv3d_k3_wgrad_wg / _det_wg / _kb_wg) and the stepper's coarse window that uses
them (ops.CoarseWindow, dp.DataParallelStepper(coarse_window=True)): weight gradients of the coarse pyramid levels, and the last ones produced
above them, on the side stream with a capped grid."""
import functools
import gc

import pytest
import torch
import torch.nn.functional as F

from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
FB = list(O.FEEDBACK_DEFAULT)

# (B, Cin, Cout, size): 32 -> 32 at 8x16x16 runs the F(2x2x2,3x3x3) kernel (one channel pair, 16 plane-pair steps: budgets 20, 100 and 128 exceed
# the step count); 96 -> 64 at 4x8x8 (six pairs) and 16 -> 96 at 8^3 lie below the Winograd kernels' 1000 voxels - the direct kernel, which must
# ignore the budget; 96 -> 64 at 4x16x16 is the six-pair case ON the budgeted kernel (budget 4 < six pairs -> 6 workgroups, 8 -> 6, 20 -> 6 x 3,
# 100 and 128 -> 6 x 16 = 96: a multiple of 8 needs a split count that is a multiple of 4).
SHAPES = [(1, 32, 32, (8, 16, 16)), (2, 96, 64, (4, 8, 8)), (1, 16, 96, (8, 8, 8)), (2, 96, 64, (4, 16, 16))]
BUDGETS = [0, 4, 8, 20, 100, 128]
TOL = 2e-6            # the per-operator relative-L2 bound of tests/test_gpu_ops.py


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@functools.lru_cache(maxsize=None)
def _case(B, Cin, Cout, size):
    """operands and the weight gradient of the fp64 CPU convolution (computed once per shape, never written to)"""
    gen = torch.Generator().manual_seed(B * 100 + Cin + Cout)
    x = torch.randn(B, Cin, *size, generator=gen)
    dy = torch.randn(B, Cout, *size, generator=gen)
    w = torch.zeros(Cout, Cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad((F.conv3d(x.double(), w, padding=1) * dy.double()).sum(), [w])
    return (x.cuda().contiguous(memory_format=torch.channels_last_3d), dy.cuda().contiguous(memory_format=torch.channels_last_3d), ref)


def _blocked(ops, t):
    B, C, D, H, W = t.shape
    g = ops._BlockedGrad(B, C, D, H, W, t.device)
    g.buf.copy_(t.permute(0, 2, 3, 4, 1).reshape(B, D, H, W, C // 8, 8).permute(4, 0, 1, 2, 3, 5).reshape(-1))
    return g


def _call(ops, entry, x, dy, budget=None, det=False):
    """one of the six C entry points directly: entry in ("", "_det", "_kb"), budget None = the entry point without the budget argument"""
    lib, p = ops.lib, ops._ptr
    B, Cin, D, H, W = x.shape
    Cout = dy.shape[1]
    dw = torch.empty(Cout, Cin, 3, 3, 3, device=x.device)
    nscr = lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", Cin, Cout)
    scratch = torch.empty(nscr, device=x.device)
    nslab = lib.query("pulpo_conv3d_k3_wgrad_det_slabs", Cin, Cout)
    slabs = torch.empty(nslab * nscr, device=x.device) if det else None
    xb, xp, xc = ops.grid_strides(x)
    tail = (B, D, H, W, Cin, Cout, ops._stream()) + (() if budget is None else (int(budget),))
    sfx = "" if budget is None else "_wg"
    if entry == "_kb":
        blk = isinstance(dy, ops._BlockedGrad)
        dyt, db, dp, dkb = (dy.buf, dy.bs, dy.ps, dy.kb) if blk else (dy, dy.stride(0), dy.stride(4), 8)
        lib.call("pulpo_conv3d_k3_wgrad_kb" + sfx, p(x), xb, xp, 8, p(dyt), db, dp, dkb, p(dw), 0, p(scratch), p(slabs), nslab if det else 0, *tail)
    elif det:
        lib.call("pulpo_conv3d_k3_wgrad_det" + sfx, p(x), xb, xp, xc, p(dy), *ops.grid_strides(dy), p(dw), 0, p(scratch), p(slabs), nslab, *tail)
    else:
        lib.call("pulpo_conv3d_k3_wgrad" + sfx, p(x), xb, xp, xc, p(dy), *ops.grid_strides(dy), p(dw), 0, p(scratch), *tail)
    return dw


@pytest.mark.parametrize("B,Cin,Cout,size", SHAPES)
def test_budgeted_weight_gradient_vs_fp64(ops, B, Cin, Cout, size):
    """every budget (0 = none, one below the pair count, one that is no multiple of 8, some above the step count) gives the fp64 gradient within the
    per-operator 2e-6, channels-last and - first shape - on a channel-blocked dy; the launch stays within the budget (never below one workgroup
    per channel pair) and is a multiple of 8 where the pair count allows.
    Budget 0 through the new entry points IS the old entry points: same grid, and the same bits wherever bits are defined - the deterministic forms
    (the atomic form adds its up to 16 splits in arrival order, so two runs of the SAME entry point already differ in the last bit; there it is
    held to the order-of-summation bound 1e-6 of test_deterministic_weight_gradient_is_bit_reproducible)."""
    x, dy, ref = _case(B, Cin, Cout, size)
    D, H, W = size
    q = ops.lib.query
    npair = -(-Cin // 32) * -(-Cout // 32)
    wino = q("pulpo_conv3d_k3_wgrad_algo", B, D, H, W, Cin, Cout, 1) >= 2
    assert wino == (D * H * W >= 1000)
    full = q("pulpo_conv3d_k3_wgrad_grid", B, D, H, W, Cin, Cout, 0)
    assert (full > 0) == wino
    blocked = _blocked(ops, dy) if (B, Cin, Cout, size) == SHAPES[0] else None
    for budget in BUDGETS:
        grid = q("pulpo_conv3d_k3_wgrad_grid", B, D, H, W, Cin, Cout, budget)
        if wino and budget:
            assert grid % npair == 0 and npair <= grid <= max(budget, npair) and grid <= full, (budget, grid)
            nsplit, m = grid // npair, 8 // max(g for g in (1, 2, 4, 8) if npair % g == 0)
            assert grid % 8 == 0 or nsplit < m, (budget, grid)
        got = _call(ops, "", x, dy, budget)
        err = rel_l2(got, ref)
        print(f"{Cin}->{Cout} {size} budget {budget}: grid {grid}, rel-L2 vs fp64 {err:.2e}")
        assert err < TOL, (budget, err)
        if blocked is not None:
            err = rel_l2(_call(ops, "_kb", x, blocked, budget), ref)
            print(f"   blocked dy: {err:.2e}")
            assert err < TOL, (budget, err)
    old = _call(ops, "", x, dy)
    assert rel_l2(_call(ops, "", x, dy, 0), old) < 1e-6
    assert torch.equal(_call(ops, "_det", x, dy, 0, det=True), _call(ops, "_det", x, dy, det=True))
    if blocked is not None:
        assert torch.equal(_call(ops, "_kb", x, blocked, 0, det=True), _call(ops, "_kb", x, blocked, det=True))
        assert rel_l2(_call(ops, "_kb", x, blocked, 0), old) < 1e-6


@pytest.mark.parametrize("B,Cin,Cout,size", [SHAPES[0], SHAPES[3]])
@pytest.mark.parametrize("budget", [8, 20, 128])
def test_deterministic_budgeted_weight_gradient_is_bit_reproducible(ops, B, Cin, Cout, size, budget):
    """the slab count follows the budgeted split count: three calls give the same bits, and the fp64 gradient within the same bound"""
    x, dy, ref = _case(B, Cin, Cout, size)
    a = _call(ops, "_det", x, dy, budget, det=True)
    for _ in range(2):
        assert torch.equal(_call(ops, "_det", x, dy, budget, det=True), a)
    assert rel_l2(a, ref) < TOL
    if (B, Cin, Cout, size) == SHAPES[0]:
        blk = _blocked(ops, dy)
        b = _call(ops, "_kb", x, blk, budget, det=True)
        assert torch.equal(_call(ops, "_kb", x, blk, budget, det=True), b) and torch.equal(b, a)


# ================================================================================================ the stepper's coarse window
def _make_step_case():
    """the T3 / L2, 32^3, n0 = 32 configuration of the step goldens: levels of 32^3, 16^3 and 8^3 voxels"""
    import src.models as models
    import src.network_blocks as nb
    gen = torch.Generator().manual_seed(9)
    x, y = torch.rand(1, 1, 32, 32, 32, generator=gen).cuda(), torch.rand(1, 1, 32, 32, 32, generator=gen).cuda()
    eps = [torch.randn(1, 3, 16, 16, 16, generator=gen).cuda(), torch.randn(1, 3, 8, 8, 8, generator=gen).cuda()]
    empty = torch.empty((0,))

    def make():
        torch.manual_seed(0)
        m = models.PULPo(3, 2, 0.1, [32, 32, 32], feedback=FB, n0=32).cuda().train()
        for l in range(2):
            m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        return m

    return make, (x, y, empty, empty, empty, empty, empty, empty)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_stepper_coarse_window_matches_the_inline_stepper(ops):
    """window mode forced on the small model: the 8^3 level is "coarse" (its weight gradients go to the side stream), every F(2x2x2) weight gradient
    of the 32^3 and 16^3 levels produced before it is held back for it (an unlimited FLOP budget).  Four steps with the weights kept (lr 0): losses
    and every parameter gradient as the in-line stepper's, within the bound of the in-line / side-stream comparison of
    test_unit_and_head_applied_twice_in_one_stepper_step (relative L2 2e-5; a bias in front of a BatchNorm - true gradient 0 - on the scale of its
    layer's weight gradient, 1e-4); nothing accumulates across steps.

    Memory: the live tensors after step 2 and after step 4 are the same in number and in the bytes they asked for (the allocator's
    requested_bytes).  torch.cuda.memory_allocated() itself is NOT compared: it counts every live tensor at the size of the cached block it
    happened to get (a block is left unsplit when less than 1 MiB would remain), and which block that is depends on where the tensors the previous
    step left behind lie.  The in-line stepper alone settles at once (108001792 bytes every step); in window mode the weight-gradient operands
    are freed later in the pass than in line, and the same bytes cycle between block sizes without growing - measured on MI355X, six steps of
    the window stepper alone: 108243968, 108245504, 108245504, 109294080, 108245504, 108245504 allocated with 107267172 bytes asked for and 179
    live tensors from the second step on (held back: none in the first step); with the two steppers interleaved as here 248677888, 248570368,
    247784960 after steps 2, 3, 4."""
    from pulpo_amd import dp
    make, batch = _make_step_case()
    a, b = make(), make()
    inline = dp.DataParallelStepper(a, lr=0.0, coarse_window=False)
    window = dp.DataParallelStepper(b, lr=0.0, coarse_window=True, coarse_voxels=8 ** 3, max_workgroups=64, defer_flop=1e30, exit_wait=True)
    assert not inline.coarse_window() and not inline.wgrad_on_side_stream() and inline.describe()["coarse_window"] is False
    assert window.coarse_window() and not window.wgrad_on_side_stream() and window.describe()["coarse_window"] is True
    mem = {}
    for step in range(1, 5):
        la, lb = inline.step(batch), window.step(batch)
        torch.cuda.synchronize()
        assert ops._PASS.window is None and not ops._PASS.jobs and not window._window.held and not window._window.keep
        assert abs(float(la) - float(lb)) <= 2e-5 * abs(float(la)), (step, float(la), float(lb))
        ga, gb = _grads(a), _grads(b)
        assert ga.keys() == gb.keys() and len(ga) > 60
        for k in ga:
            if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
                wmax = float(ga[k[:-4] + "weight"].abs().max())
                assert float((gb[k] - ga[k]).abs().max()) <= 1e-4 * max(wmax, 1e-6), (step, k)
                continue
            assert rel_l2(gb[k], ga[k]) < 2e-5, (step, k, rel_l2(gb[k], ga[k]))
        if step >= 2:                                  # (the first pass learns which jobs precede the window and holds none)
            assert window._window.deferred_last > 0 and window.describe()["coarse_window_settings"]["deferred_last_step"] > 0
        else:
            assert window._window.deferred_last == 0
        gc.collect()                                   # (tensors in reference cycles of the step's Python objects are no allocator state)
        st = torch.cuda.memory_stats()
        mem[step] = (st["requested_bytes.all.current"], st["allocation.all.current"])
        print(f"step {step}: loss {float(lb):.6f} (in line {float(la):.6f}), {window._window.deferred_last} weight gradients held back, live tensors "
              f"{mem[step][1]} with {mem[step][0]} bytes asked for, torch.cuda.memory_allocated() {torch.cuda.memory_allocated()}")
    assert mem[2] == mem[4], mem


@pytest.mark.parametrize("exit_wait", [False, True])
def test_coarse_window_exit_policies_and_tight_budgets(ops, exit_wait):
    """a FLOP budget that holds back only the last job before the window, and both exit policies: gradients as plain autograd's"""
    from pulpo_amd import dp
    make, batch = _make_step_case()
    ref = make()
    ref.training_step(batch, 0).backward()
    want = _grads(ref)
    probe = dp.DataParallelStepper(make(), lr=0.0, coarse_window=True, coarse_voxels=8 ** 3, defer_flop=1e30)
    probe.step(batch)
    last_flop = probe._window._plan_sig[-1][1]       # FLOP of the last weight gradient above the window
    net = make()
    stepper = dp.DataParallelStepper(net, lr=0.0, coarse_window=True, coarse_voxels=8 ** 3, max_workgroups=8, defer_flop=last_flop, exit_wait=exit_wait)
    for step in range(3):
        stepper.step(batch)
    torch.cuda.synchronize()
    assert 1 <= stepper._window.deferred_last < len(probe._window._plan_sig)
    for k, g in _grads(net).items():
        if k not in want:                               # (a parameter the loss does not reach: no gradient in plain autograd, zeros in the arena)
            assert not bool(g.any()), k
            continue
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            continue
        assert rel_l2(g, want[k]) < 2e-5, (k, rel_l2(g, want[k]))


def test_deterministic_mode_keeps_the_weight_gradients_in_line(ops):
    """deterministic mode with the window requested: the stepper reports it off (a budget would change the split count and with it the summation
    order) and gives the in-line deterministic stepper's gradients bit for bit"""
    from pulpo_amd import dp
    make, batch = _make_step_case()
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        a, b = make(), make()
        inline = dp.DataParallelStepper(a, lr=0.0, coarse_window=False)
        asked = dp.DataParallelStepper(b, lr=0.0, coarse_window=True, coarse_voxels=8 ** 3, defer_flop=1e30)
        assert not asked.coarse_window() and asked.describe()["coarse_window"] is False
        for _ in range(2):
            la, lb = inline.step(batch), asked.step(batch)
        torch.cuda.synchronize()
        assert float(la) == float(lb)
        ga, gb = _grads(a), _grads(b)
        assert ga.keys() == gb.keys()
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        assert asked._window.deferred_last == 0
    finally:
        ops.set_deterministic(was)
