"""Bidirectional training on the GPU.

  forward    pulpo_vecint_pair_fwd_work into a NaN-filled `work`: every stored field of both directions bit-equal to pulpo_vecint_fwd on v and
             on -v, and against the float64 chain with test_gpu_vecint's bounds, on both sides of the 2048-voxel switch.
  backward   pulpo_vecint_pair_bwd / _det step by step against float64 (test_gpu_vecint.StepRef: its bounds, its 1e-4-voxel boundary set and
             its +-2e-4 nudge), one size per step kernel, with both upstream gradients, the forward one alone and the inverse one alone (the
             skipped direction's fields and all scratch NaN); the chain is the composition of its steps - bit for bit in deterministic mode,
             where each direction also has pulpo_vecint_bwd_det's bits.
  autograd   ops.vecint_pair as one node: gradient against the two-call composition, memory, launch log, the 2-D form.
  the step   PULPo(bidirectional=True): the new outputs and loss terms against float64 on the device's own fields and images, parameter
             gradients against the same loss composed from public operators, flag off = today's step bit for bit, the symmetry the feature
             exists for, a captured step.
  refine and scores.
Every comparison prints a RATIO line (error / bound): pytest -s."""
import ctypes
import functools
import os

import pytest
import torch

import bidir_ref as BR
import label_dice_ref as LD
import masked_ref as MR
import mi_ref as MI
import pyramid_ref as R
import test_gpu_pyramid_ops as P
import test_gpu_vecint as V
from launch_log import LaunchLog
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
FB = list(O.FEEDBACK_DEFAULT)
check, amax, gen = P.check, P.amax, V.gen


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@pytest.fixture(scope="module")
def api(ops):
    import src.models as models
    import src.network_blocks as nb
    return models, nb


def _lib():
    from pulpo_amd._lib import lib
    return lib


_ptr, _stream = V._ptr, V._stream


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def deterministic(ops, on):
    """context: ops.set_deterministic(on), restored to the environment's default"""
    class _Ctx:
        def __enter__(self):
            ops.set_deterministic(on)

        def __exit__(self, *exc):
            ops.set_deterministic(P.det_default())
            return False
    return _Ctx()


# ------------------------------------------------------------------------------------------------ the entry points, through the C ABI
def run_pair_fwd(v, nsteps):
    """pulpo_vecint_pair_fwd_work into a NaN-filled work: (nsteps + 1, 2, B, 3, D, H, W)"""
    B, _, D, H, W = v.shape
    work = torch.full((nsteps + 1, 2, B, 3, D, H, W), NAN, device=DEV)
    _lib().call("pulpo_vecint_pair_fwd_work", _ptr(v), _ptr(work), B, D, H, W, nsteps, _stream())
    return work


def run_pair_bwd(det, work, gf, gi, nsteps, scratch=None):
    """pulpo_vecint_pair_bwd_det / pulpo_vecint_pair_bwd into a NaN-filled gin; the scratch has every byte 0xFF (NaN as floats, -1 as the
    fixed-point accumulators) unless one is handed in.  Returns (gin, scratch)"""
    assert work.is_contiguous() and work.shape[0] == nsteps + 1 and work.shape[1] == 2
    _, _, B, _, D, H, W = work.shape
    n = int(_lib().query("pulpo_vecint_pair_bwd_det_ws_bytes" if det else "pulpo_vecint_pair_bwd_tmp_floats", B, D, H, W, nsteps))
    if scratch is None and n:
        scratch = torch.full((n if det else 4 * n,), 0xFF, device=DEV, dtype=torch.uint8)
    gin = torch.full((B, 3, D, H, W), NAN, device=DEV)
    _lib().call("pulpo_vecint_pair_bwd_det" if det else "pulpo_vecint_pair_bwd", _ptr(work), _ptr(gf), _ptr(gi), _ptr(gin), _ptr(scratch), B, D, H, W,
                nsteps, _stream())
    return gin, scratch


def only(work, d):
    """work with the other direction's fields NaN: a call that has no gradient for a direction must not read that direction"""
    w = work.clone()
    w[:, 1 - d] = NAN
    return w


# ================================================================================================ 1. forward: every stored field
FWD_CASES = [(2, (8, 16, 16), 7, 12.0), (2, (8, 16, 17), 7, 12.0), (1, (9, 15, 15), 7, 6.0), (1, (1, 24, 20), 7, 9.0), (1, (12, 14, 10), 0, 5.0),
             (2, (10, 10, 10), 1, 3.0), (1, (66, 63, 65), 2, 4.0)]


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("B,size,nsteps,amp", FWD_CASES)
def test_forward_every_stored_field(ops, B, size, nsteps, amp, kind):
    """work[k][d] for every k and both directions (NaN on entry: every field must be written): the bits of pulpo_vecint_fwd on v and on -v,
    and the float64 chain within test_gpu_vecint's bound.  2048 voxels is the last size of the one-launch LDS kernel (2 B workgroups),
    8 x 16 x 17 the first of the step form; 2025 voxels is no multiple of the 1024 threads; a depth-1 grid; nsteps 0 and 1; 66 x 63 x 65 is
    more than one trip of the capped grid.  Smooth fields with peaks of 3 - 12 voxels, white noise of amplitude 3"""
    if kind == "noise":
        amp = 3.0
    v = R.vecint_field(kind, B, size, amp=amp, seed=size[2] + nsteps).to(DEV)
    name = f"vecint pair fwd {B}/{size}/n{nsteps}/{kind}"
    work = run_pair_fwd(v, nsteps)
    assert bool(torch.isfinite(work).all()), name
    for d, sign in ((0, 1.0), (1, -1.0)):
        single = V.run_fwd(sign * v, nsteps)
        for k in range(nsteps + 1):
            assert torch.equal(work[k, d], single[k]), f"{name}: work[{k}][{d}] differs from pulpo_vecint_fwd in {int((work[k, d] != single[k]).sum())} elements"
        ref = R.vecint_chain_ref(sign * v.double(), nsteps)
        r32 = R.vecint_chain_ref(sign * v, nsteps)
        tols = [max(1e-5 * max(1.0, amax(r)), 2 * R.ratio(s, r, 1.0)) for r, s in zip(ref, r32)]
        for k in range(nsteps + 1):
            check(f"{name} work[{k}][{d}]", work[k, d], ref[k], tols[k])
    if nsteps == 0:
        assert torch.equal(work[0, 0], v) and torch.equal(work[0, 1], -v)


# ================================================================================================ 2. backward
# (B, size, nsteps) -> the step kernel of pulpo_vecint_bwd's rules: the plain scatter below 8 voxels on an axis, the LDS tile with a one-voxel
# rim, and from 64^3 voxels on the two-voxel rim for the chain's last step (nsteps = 2: rim 2 at k = 1, rim 1 at k = 0)
BWD_CASES = [(1, (6, 12, 14), 1, "plain"), (1, (6, 12, 14), 3, "plain"), (2, (12, 10, 14), 2, "tile1"), (1, (9, 17, 23), 1, "tile1"),
             (1, (64, 64, 64), 1, "tile2"), (1, (64, 64, 64), 2, "tile2")]
BWD_SEED = 3          # seeds chosen so that the float64 boundary set of every step stays below 1 % of the voxels (checked on a CPU: the shares
#                       of every case are printed by the test: at most 0.07 %).  Nearest to its bound: 64^3, one step, 0.995 of it in the
#                       atomic and in the fixed-point kernel alike (profiles/bidir_gpu_tests.txt)


def _both_ref(srs, present):
    """float64 reference and bound of one backward squaring step of a paired call: gin = (ref+ - ref-) / 2 over the directions present"""
    ref, tol, off = 0.0, 0.0, None
    for d in present:
        ref = ref + (0.5 if d == 0 else -0.5) * srs[d].ref
        tol = tol + 0.5 * srs[d].tol_t
        off = srs[d].off if off is None else off & srs[d].off
    return ref, tol, int(torch.nonzero(off.reshape(-1)).reshape(-1)[-1])


@pytest.mark.parametrize("B,size,nsteps,kern", BWD_CASES)
def test_backward_steps_vs_float64_and_chain_is_their_composition(ops, B, size, nsteps, kern):
    """Every backward squaring step of the chain as a one-step call on (work[k], work[k + 1]) with the gradients the deterministic chain
    itself hands down: both directions, the forward one alone, the inverse one alone (other direction's fields NaN, scratch 0xFF), atomic
    and deterministic, each against float64 (StepRef) with the step tests' bounds and power check.  Then the nsteps-step call against the
    composition: torch.equal in deterministic mode, 1e-5 max|g| for the atomic one; two deterministic calls agree bit for bit; each
    direction alone has pulpo_vecint_bwd_det's bits."""
    assert V.kernel_of(size) == kern
    name = f"vecint pair bwd {B}/{size}/n{nsteps}"
    v = R.vecint_field("smooth", B, size, amp=3.0, seed=BWD_SEED + size[0]).to(DEV)
    work = run_pair_fwd(v, nsteps)
    n = v.numel()
    tiled = kern != "plain"
    assert int(_lib().query("pulpo_vecint_pair_bwd_tmp_floats", B, *size, nsteps)) == (2 * nsteps * n if tiled else 4 * n), name
    up = [torch.randn(B, 3, *size, device=DEV, generator=gen(7 + size[1] + d)) for d in (0, 1)]
    g = list(up)                                    # the gradients entering step k, per direction
    for k in range(nsteps - 1, -1, -1):
        pair = work[k:k + 2].contiguous()
        srs = [V.StepRef(pair[0, d], g[d]) for d in (0, 1)]
        for d in (0, 1):
            print(f"RATIO {name} k{k} dir{d} bnd share {srs[d].share:.3g} spread32 {srs[d].spread:.3g}")
            assert srs[d].share < 0.01, (name, k, d, srs[d].share)
        nxt = [None, None]
        for det in (False, True):
            for present in ((0, 1), (0,), (1,)):
                w = pair if len(present) == 2 else only(pair, present[0])
                gin, _ = run_pair_bwd(det, w, g[0] if 0 in present else None, g[1] if 1 in present else None, 1)
                ref, tol, last = _both_ref(srs, present)
                check(f"{name} k{k} {'fx' if det else kern} dirs{present}", gin, ref, tol, power=last)
                if det and len(present) == 1:
                    nxt[present[0]] = (2.0 if present[0] == 0 else -2.0) * gin
        g = nxt
    composed = (g[0] - g[1]) * (1.0 / 2 ** nsteps)
    d1, scratch = run_pair_bwd(True, work, up[0], up[1], nsteps)
    d2, _ = run_pair_bwd(True, work, up[0], up[1], nsteps, scratch=scratch)
    assert torch.equal(d1, d2), f"{name}: the deterministic call depends on what its workspace held"
    assert torch.equal(d1, composed), f"{name}: the deterministic chain is not the composition of its steps ({int((d1 != composed).sum())} elements differ)"
    a1, scratch = run_pair_bwd(False, work, up[0], up[1], nsteps)
    a2, _ = run_pair_bwd(False, work, up[0], up[1], nsteps, scratch=scratch)
    for tag, t in (("chain", a1), ("chain on its used scratch", a2)):
        check(f"{name} atomic {tag} vs deterministic", t, d1.double(), 1e-5 * amax(d1))
    for d, sign in ((0, 1.0), (1, -1.0)):
        single, _ = V.run_bwd(True, work[:, d].contiguous(), up[d], nsteps)
        alone, _ = run_pair_bwd(True, only(work, d), up[0] if d == 0 else None, up[1] if d == 1 else None, nsteps)
        assert torch.equal(alone, sign * single), f"{name}: direction {d} alone differs from pulpo_vecint_bwd_det"
        atomic, _ = run_pair_bwd(False, only(work, d), up[0] if d == 0 else None, up[1] if d == 1 else None, nsteps)
        check(f"{name} atomic direction {d} alone vs deterministic", atomic, alone.double(), 1e-5 * amax(alone))


def test_backward_nsteps_zero_and_depth_one(ops):
    """nsteps = 0: gin = gfwd - ginv exactly, no scratch; a depth-1 (2-D) field runs the plain scatter: against the per-direction calls"""
    size = (12, 14, 10)
    v = R.vecint_field("smooth", 1, size, amp=3.0, seed=1).to(DEV)
    gf, gi = (torch.randn(1, 3, *size, device=DEV, generator=gen(d)) for d in (1, 2))
    work = run_pair_fwd(v, 0)
    for det in (False, True):
        assert torch.equal(run_pair_bwd(det, work, gf, gi, 0)[0], gf - gi)
        assert torch.equal(run_pair_bwd(det, work, gf, None, 0)[0], gf) and torch.equal(run_pair_bwd(det, work, None, gi, 0)[0], -gi)
    size = (1, 24, 20)
    v = R.vecint_field("smooth", 2, size, amp=4.0, seed=2).to(DEV)
    gf, gi = (torch.randn(2, 3, *size, device=DEV, generator=gen(d)) for d in (3, 4))
    work = run_pair_fwd(v, 7)
    want = V.run_bwd(True, work[:, 0].contiguous(), gf, 7)[0] - V.run_bwd(True, work[:, 1].contiguous(), gi, 7)[0]
    assert torch.equal(run_pair_bwd(True, work, gf, gi, 7)[0], want)
    check("vecint pair bwd depth-1 atomic", run_pair_bwd(False, work, gf, gi, 7)[0], want.double(), 1e-5 * amax(want))


# ================================================================================================ 3. ops.vecint_pair as one autograd node
def _two_calls(ops, v, a, b, nsteps=7):
    v = v.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad((ops.vecint(v, nsteps) * a + ops.vecint(-v, nsteps) * b).sum(), [v])
    return g


@pytest.mark.parametrize("B,size", [(2, (12, 10, 14)), (1, (24, 20, 28)), (2, (6, 7, 5)), (2, (24, 20))])
def test_ops_vecint_pair_gradient_is_the_two_call_composition(ops, B, size):
    """the gradient of (fwd * a + inv * b).sum() through the paired node against (vecint(v), vecint(-v)): within twice the run-to-run rel_l2
    spread of that composition itself (floor 1e-6) with the float atomics, equal bits in deterministic mode.  Volumes on both sides of the
    LDS switch and of the tiled scatter, and the 2-D (B, 2, H, W) form; the outputs have the composition's bits"""
    nd = len(size)
    v = (torch.randn(B, nd, *size, device=DEV, generator=gen(size[0])) * 1.5)
    a, b = (torch.randn(B, nd, *size, device=DEV, generator=gen(size[-1] + d)) for d in (1, 2))
    for det in (False, True):
        with deterministic(ops, det):
            v1 = v.clone().requires_grad_(True)
            fwd, inv = ops.vecint_pair(v1)
            assert fwd.requires_grad and inv.requires_grad and fwd.shape == v.shape == inv.shape
            assert torch.equal(fwd, ops.vecint(v)) and torch.equal(inv, ops.vecint(-v))
            got, = torch.autograd.grad((fwd * a + inv * b).sum(), [v1])
            r1, r2 = _two_calls(ops, v, a, b), _two_calls(ops, v, a, b)
        if det:
            assert torch.equal(r1, r2) and torch.equal(got, r1), (size, int((got != r1).sum()))
        else:
            bound = max(1e-6, 2 * rel_l2(r1, r2))
            print(f"RATIO ops.vecint_pair grad {B}/{size} {rel_l2(got, r1) / bound:.3g} (spread of the composition {rel_l2(r1, r2):.3g})")
            assert rel_l2(got, r1) <= bound
            bad = r1.clone()
            bad.view(-1)[-1] += 1e-3 * amax(r1)
            assert rel_l2(bad, r1) > bound


def test_ops_vecint_pair_launches_and_memory(ops):
    """one forward and one backward lib.call, no pulpo_vecint_fwd / pulpo_vecint_bwd among them (tests/launch_log.py); at 40^3 the forward
    holds 2 (nsteps + 1) fields - the saved work, whose last pair is the result - and at most 3 more at its peak"""
    S, nsteps = 40, 7
    n = 3 * S ** 3 * 4
    v = torch.randn(1, 3, S, S, S, device=DEV, generator=gen(4)).requires_grad_(True)
    up = torch.randn(1, 3, S, S, S, device=DEV, generator=gen(5))
    for det, bwd in ((False, "pulpo_vecint_pair_bwd"), (True, "pulpo_vecint_pair_bwd_det")):
        with deterministic(ops, det), LaunchLog() as log:
            fwd, inv = ops.vecint_pair(v, nsteps)
            (fwd * up).sum().backward()
            (inv * up).sum().backward()                    # the second pass over the node: its buffer outlives the first
        names = [line.split(" ", 1)[0] for line in log.lines]
        assert names == ["pulpo_vecint_pair_fwd_work", bwd, bwd], names
        assert log.lines[1].split()[2:4] == ["p", "0"] and log.lines[2].split()[2:4] == ["0", "p"]          # the absent gradient arrives as NULL
    v.grad = None
    del fwd, inv
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fwd, inv = ops.vecint_pair(v, nsteps)
    torch.cuda.synchronize()
    peak, held = torch.cuda.max_memory_allocated() - before, torch.cuda.memory_allocated() - before
    print(f"FIGURE ops.vecint_pair at 40^3: peak {peak / n:.2f} fields above the input, {held / n:.2f} held")
    assert 2 * (nsteps + 1) * n <= held <= peak <= (2 * (nsteps + 1) + 3) * n
    assert fwd.untyped_storage().data_ptr() == inv.untyped_storage().data_ptr()          # both results are views of the one work buffer


# ================================================================================================ 4. the step
# 12 x 16 x 20: three different extents, none a power of two, odd at the coarsest level (3 x 4 x 5).  (An extent that is odd at a FINER latent
# level, as the 14 of 12 x 14 x 16 -> 6 x 7 x 8 -> 3 x 4 x 4, is outside the model with or without the flag: the decoder adds the level's
# own 7 voxels to the 2 * 4 = 8 of the up-scaled coarser field.  test_flag_off_is_todays_step_bit_for_bit shows it.)
SIZES = [(16, 16, 16), (12, 16, 20)]
C = 4


@functools.lru_cache(maxsize=None)
def _batch(size):
    g = torch.Generator().manual_seed(8 + size[0])
    x, y = torch.rand(1, 1, *size, generator=g).to(DEV), torch.rand(1, 1, *size, generator=g).to(DEV)
    seg_x = LD.make_labels(1, size, C, torch.uint8, g, False).to(DEV)
    seg_y = torch.roll(seg_x, shifts=1, dims=3).contiguous()
    box = torch.zeros(1, 1, *size, device=DEV)
    box[:, :, 2:size[0] - 2, 2:size[1] - 3, 3:size[2] - 2] = 1.0
    return x, y, seg_x, seg_y, box, MR.ball(1, size, device=DEV)


RECONS = {"ncc": dict(recon_loss=["ncc"]), "mse+dice": dict(recon_loss=["mse", "dice"], num_classes=C), "mi+masks": dict(recon_loss=["mi"], mask=True),
          "mse": dict(recon_loss=["mse"])}
STEP_CASES = ["ncc", "mse+dice", "mi+masks"]


def _inputs(size, case):
    x, y, seg_x, seg_y, box, ball = _batch(size)
    e = torch.empty((0,), device=DEV)
    return x, y, (seg_x if "dice" in case else e), (seg_y if "dice" in case else e), (box if "masks" in case else e), (ball if "masks" in case else e)


def _model(api, size, case, **kw):
    models, nb = api
    torch.manual_seed(0)
    m = models.PULPo(3, 2, 0.1, list(size), feedback=FB, n0=4, **RECONS[case], **kw).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    sizes = O.Cfg(3, 2, list(size)).level_sizes()
    for l in range(2):
        m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, *sizes[l + 1], generator=g).to(DEV))
    return m


def _step(model, inputs):
    model.zero_grad(set_to_none=True)
    outs, _, losses, levels = model._forward_and_losses(*inputs)
    losses[0].backward()
    return outs, [t.detach() for t in losses], levels, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _composed_loss(ops, model, inputs):
    """the bidirectional objective composed in the test from public operators on the unidirectional forward pass: ops.vecint(-combined),
    resize, warp, ops.similarity / label_dice_loss / soft_dice_loss, the model's regulariser, python arithmetic for the weights"""
    x, y, seg_x, seg_y, mask_x, mask_y = inputs
    outs = model.autoencoder(x, model.downpath(x, y, _needed=model._needed_levels))
    mus, sigmas, final, y_hat = outs[0], outs[1], outs[6], outs[7]
    kl, _ = model.hierarchical_kl_loss(*model.prior(mus, sigmas), mus, sigmas, scale=model.beta)
    level_y = model.autoencoder.level_images(y)
    final_inv = {l: model._resize_integrated(l, ops.vecint(-outs[5][l], 7)) for l in final}
    x_hat = {l: ops.warp3d(final_inv[l], level_y[l]) for l in final}
    rl = model.hierarchical_recon_loss
    recon = list(model.hparams.recon_loss)
    rec = reg = 0.0
    for l, w in rl.weight_dict.items():
        size = tuple(final[l].shape[2:])
        sides = 0.0
        for img_hat, img, df, sa, sb, ma, mb in ((y_hat, y, final, seg_x, seg_y, mask_x, mask_y), (x_hat, x, final_inv, seg_y, seg_x, mask_y, mask_x)):
            tgt = img if size == tuple(img.shape[2:]) else ops.resize_trilinear(img, size)
            wa = ops.warp_mask(df[l], ma) if ma.numel() else None
            wb = (mb if size == tuple(mb.shape[2:]) else ops.resize_trilinear(mb, size)) if mb.numel() else None
            for kind in recon:
                if kind == "dice":
                    sides = sides + model.label_dice_terms({l: df[l]}, sa, sb)[l]
                else:
                    sides = sides + ops.similarity(kind, img_hat[l], tgt, wa, wb, win=rl.window_size[l], gamma=model.hparams.gamma, bins=rl.mi_bins)
        rec = rec + (w / 2) * sides / len(recon)
        wr = model.hierarchical_regularization.weight_dict[l]
        reg = reg + (wr / 2) * (ops.l2_reg(final[l], model.hparams.lamb) + ops.l2_reg(final_inv[l], model.hparams.lamb))
    return kl + rec + reg


def _flat(grads):
    return torch.cat([grads[k].reshape(-1) for k in sorted(grads)])


def _ref_terms(model, case, outs, inputs):
    """rec and reg of the formula of DESIGN.md section 3u in float64, on the device's own fields and warped images"""
    x, y, seg_x, seg_y, mask_x, mask_y = (t.double() if t.is_floating_point() else t for t in inputs)
    cfg = O.Cfg(3, 2, list(x.shape[2:]), n0=4)
    final, y_hat, final_inv, x_hat = ({l: t.detach().double() for l, t in outs[i].items()} for i in (6, 7, 8, 9))
    rl = model.hierarchical_recon_loss
    sims, extra, extra_inv = {}, None, None
    if "mi" in case:
        def masked_mi(fields, ma, mb):
            def f(pred, true, l):
                wa = R.warp_ref(fields[l], ma)
                wb = R.resize_ref(mb, tuple(pred.shape[2:]))
                return MI.loss_masked(pred, true, wa, wb, rl.mi_bins, model.hparams.gamma)
            return f
        rec_f, _ = BR.rec_from_images(cfg, y_hat, y, None, None, ("mi",), {"mi": masked_mi(final, mask_x, mask_y)})
        rec_i, _ = BR.rec_from_images(cfg, x_hat, x, None, None, ("mi",), {"mi": masked_mi(final_inv, mask_y, mask_x)})
        rec = 0.5 * (rec_f + rec_i)
    else:
        recon = tuple(model.hparams.recon_loss)
        if "dice" in recon:
            def dice(fields, moving, target):
                warped = O.transform_segmentation(None, cfg, fields, LD.one_hot(moving, C, torch.float64))
                return {l: O.soft_dice(warped[l], R.resize_ref(LD.one_hot(target, C, torch.float64), tuple(warped[l].shape[2:]))) for l in fields}
            extra, extra_inv = dice(final, seg_x, seg_y), dice(final_inv, seg_y, seg_x)
        rec, _ = BR.rec_from_images(cfg, y_hat, y, x_hat, x, recon, extra=extra, extra_inv=extra_inv)
    reg, _ = BR.reg_from_fields(cfg, final, final_inv)
    return rec, reg


@pytest.mark.parametrize("case", STEP_CASES)
@pytest.mark.parametrize("size", SIZES)
def test_bidirectional_step_vs_float64_and_public_operators(ops, api, size, case):
    """T3 / L2 on 16^3 and 12 x 16 x 20.  outs gains final_dfs_inv and x_hat: float64 from the device's own combined_dfs and
    final_dfs_inv (the integration with test_gpu_vecint's forward bound, the warp with test_warp_vs_float64's); rec and reg are the float64
    formula on the device's own warped images (rtol 1e-4, tests/test_gpu_masks.py's bound for a loss value); the per-level dicts sum to
    them; every parameter gradient against the same loss composed from public operators, within twice the run-to-run rel_l2 spread of
    that composition (floor 1e-6) over all parameters"""
    inputs = _inputs(size, case)
    model = _model(api, size, case, bidirectional=True)
    outs, (total, kl, rec, reg), levels, grads = _step(model, inputs)
    assert len(outs) == 10 and sorted(outs[8]) == sorted(outs[9]) == [0, 1]
    cfg = O.Cfg(3, 2, list(size), n0=4)
    name = f"bidir step {size}/{case}"
    level_y = BR.level_images(cfg, inputs[1].double())
    for l in (0, 1):
        c = outs[5][l].detach()
        ratio = outs[6][l].shape[2] / c.shape[2]
        ref = O.resize_field(O.vecint(-c.double(), 7), 1.0 / ratio)
        r32 = O.resize_field(O.vecint(-c, 7), 1.0 / ratio)
        check(f"{name} final_dfs_inv[{l}]", outs[8][l], ref, max(1e-5 * max(1.0, amax(ref)), 2 * R.ratio(r32, ref, 1.0)))
        assert outs[8][l].shape == outs[6][l].shape and amax(outs[8][l] + outs[6][l]) > 0
        f = outs[8][l].detach()
        ref = R.warp_ref(f.double(), level_y[l])
        r32 = R.warp_ref(f, level_y[l].float())
        check(f"{name} x_hat[{l}]", outs[9][l], ref, max(1e-5 * max(1.0, amax(ref)), 2 * R.ratio(r32, ref, 1.0)))
    ref_rec, ref_reg = _ref_terms(model, case, outs, inputs)
    for what, got, ref in (("rec", rec, ref_rec), ("reg", reg, ref_reg)):
        print(f"RATIO {name} {what} {abs(float(got) - float(ref)) / (1e-4 * abs(float(ref))):.3g}")
        assert abs(float(got) - float(ref)) <= 1e-4 * abs(float(ref)), (what, float(got), float(ref))
        assert abs(float(got) * (1 + 1e-3) - float(ref)) > 1e-4 * abs(float(ref))          # (the bound rejects a 1e-3 relative error)
    torch.testing.assert_close(sum(levels[1].values()).reshape(()), rec.reshape(()), rtol=1e-5, atol=0)
    torch.testing.assert_close(sum(levels[2].values()).reshape(()), reg.reshape(()), rtol=1e-5, atol=0)
    torch.testing.assert_close(total, kl + rec + reg, rtol=1e-6, atol=0)

    def composed():
        model.zero_grad(set_to_none=True)
        loss = _composed_loss(ops, model, inputs)
        loss.backward()
        return loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    (l1, g1), (l2, g2) = composed(), composed()
    torch.testing.assert_close(total.reshape(()), l1.reshape(()), rtol=1e-5, atol=0)
    assert g1.keys() == grads.keys() and len(grads) > 20
    bound = max(1e-6, 2 * rel_l2(_flat(g2), _flat(g1)))
    err = rel_l2(_flat(grads), _flat(g1))
    print(f"RATIO {name} parameter gradients {err / bound:.3g} (spread of the composition {rel_l2(_flat(g2), _flat(g1)):.3g})")
    assert err <= bound
    # ... and the unidirectional step is another objective: the inverse terms reach the loss and the gradients
    _, (total0, _, rec0, reg0), _, grads0 = _step(_model(api, size, case), inputs)
    assert abs(float(rec0) - float(rec)) > 1e-4 * abs(float(rec)) and rel_l2(_flat(grads0), _flat(g1)) > 100 * bound


@pytest.mark.parametrize("case", ["ncc", "mse+dice"])
def test_flag_off_is_todays_step_bit_for_bit(ops, api, case):
    """bidirectional=False against a model built without the keyword, deterministic mode: total, every output, every parameter gradient
    and the launch log are equal"""
    size = SIZES[1]
    inputs = _inputs(size, case)
    with deterministic(ops, True):
        runs = []
        for kw in ({}, {"bidirectional": False}):
            model = _model(api, size, case, **kw)
            with LaunchLog() as log:
                runs.append(_step(model, inputs) + (log.lines,))
    (outs0, losses0, _, grads0, lines0), (outs1, losses1, _, grads1, lines1) = runs
    assert len(outs0) == len(outs1) == 8 and lines0 == lines1 and not any("vecint_pair" in line for line in lines1)
    assert all(torch.equal(a, b) for a, b in zip(losses0, losses1))
    assert all(torch.equal(outs0[i][l], outs1[i][l]) for i in range(8) for l in outs0[i])
    assert grads0.keys() == grads1.keys() and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
    # with the flag on the step integrates through the paired node only
    with LaunchLog() as log:
        _step(_model(api, size, case, bidirectional=True), inputs)
    names = [line.split(" ", 1)[0] for line in log.lines]
    assert names.count("pulpo_vecint_pair_fwd_work") == 2 == sum(n in ("pulpo_vecint_pair_bwd", "pulpo_vecint_pair_bwd_det") for n in names)
    assert "pulpo_vecint_fwd" not in names and "pulpo_vecint_bwd" not in names
    for kw in ({}, {"bidirectional": True}):
        with pytest.raises(ValueError, match="SpatialTransformer|size"):
            _step(_model(api, (12, 14, 16), "ncc", **kw), _inputs((12, 14, 16), "ncc"))


@pytest.mark.parametrize("size", SIZES)
def test_objective_symmetry(ops, api, size):
    """refinement objectives on given level fields, deterministic mode: Objective(x, y)(v) and Objective(y, x)(-v) exchange final <->
    final_inv and y_hat <-> x_hat bit for bit, agree in value to 1e-6 relative, and the gradients with respect to the fields are each
    other's negatives to the same bound; the unidirectional objective is not symmetric"""
    from pulpo_amd import refine
    x, y = _batch(size)[:2]
    model = _model(api, size, "ncc").eval()
    sizes = O.Cfg(3, 2, list(size)).level_sizes()
    v = {l: R.vecint_field("smooth", 1, sizes[l + 1], amp=2.0 / (l + 1), seed=5 + l).to(DEV) for l in (0, 1)}
    with deterministic(ops, True):
        res = []
        for a, b, sign in ((x, y, 1.0), (y, x, -1.0)):
            f = {l: (sign * t).clone().requires_grad_(True) for l, t in v.items()}
            t = refine.Objective(model, a, b, bidirectional=True).terms(f)
            grads = torch.autograd.grad(t["rec"] + t["reg"], [f[0], f[1]])
            res.append((t, grads))
        one = [refine.Objective(model, a, b, bidirectional=False)({l: sign * t for l, t in v.items()})[0] for a, b, sign in ((x, y, 1.0), (y, x, -1.0))]
    (ta, ga), (tb, gb) = res
    for l in (0, 1):
        assert torch.equal(ta["final"][l], tb["final_inv"][l]) and torch.equal(ta["final_inv"][l], tb["final"][l])
        assert torch.equal(ta["y_hat"][l], tb["x_hat"][l]) and torch.equal(ta["x_hat"][l], tb["y_hat"][l])
        assert rel_l2(ga[l], -gb[l]) <= 1e-6 and float(ga[l].abs().max()) > 0
    for key in ("rec", "reg"):
        assert abs(float(ta[key]) - float(tb[key])) <= 1e-6 * abs(float(ta[key])), (key, float(ta[key]), float(tb[key]))
    assert abs(float(one[0]) - float(one[1])) > 1e-4 * abs(float(one[0]))
    assert abs(float(ta["rec"]) - 0.5 * (float(one[0]) + float(one[1]))) <= 1e-5 * abs(float(ta["rec"]))


def test_graphed_bidirectional_step_equals_the_eager_step(ops, api):
    """dp.DataParallelStepper(graph=True) captures the step with the flag on (no host read on the new path) and replays it: the losses of
    five steps equal the eager stepper's (lr = 0: the same weights throughout)"""
    from pulpo_amd import dp
    size = SIZES[0]
    x, y = _batch(size)[:2]
    e = torch.empty((0,), device=DEV)

    def run(graph):
        st = dp.DataParallelStepper(_model(api, size, "ncc", bidirectional=True), lr=0.0, graph=graph)
        losses = [float(st.step((x, y, e, e, e, e, e, e))) for _ in range(5)]
        assert (st._graph is not None) == graph
        return losses
    eager, graphed = run(False), run(True)
    outs, (total, _, _, _), _, _ = _step(_model(api, size, "ncc", bidirectional=True), (x, y, e, e, e, e))
    assert abs(eager[0] - float(total)) <= 1e-5 * abs(float(total))
    for a, b in zip(graphed, eager):
        assert abs(a - b) <= 1e-5 * abs(b), (graphed, eager)


# ================================================================================================ 5. refinement and scores
def test_refine_bidirectional_lowers_both_rmse(ops, api):
    """model.refine(..., bidirectional=True, iters=10) on a synthetic pair: RMSE (x warped forward against y) and RMSE_inv (y warped by
    the inverse fields against x) at level 0 both end below where the prediction starts; the model's flag is followed when the keyword is
    not given; refine with the flag off returns no inverse items"""
    from pulpo_amd import synthetic
    size = (32, 32, 32)
    x, y = synthetic.oasis_like_pair(list(size), 1, 3, DEV, max_disp=2.0)
    model = _model(api, size, "mse").eval()
    start = model.refine(x, y, bidirectional=True, iters=0)
    res = model.refine(x, y, bidirectional=True, iters=10)
    assert sorted(res["final_dfs_inv"]) == sorted(res["outputs_inv"]) == [0, 1] and res["outputs_inv"][0].shape == x.shape
    for key, target in (("outputs", y), ("outputs_inv", x)):
        before, after = float(ops.rmse(start[key][0], target)), float(ops.rmse(res[key][0], target))
        print(f"FIGURE refine bidirectional {key}: RMSE {before:.5f} -> {after:.5f}")
        assert after < before, key
    assert bool((res["history"][-1, 0] < res["history"][0, 0]).item())
    assert "final_dfs_inv" not in model.refine(x, y, iters=1)
    model.bidirectional = True
    assert "final_dfs_inv" in model.refine(x, y, iters=1) and "final_dfs_inv" not in model.refine(x, y, iters=1, bidirectional=False)



def test_performance_inverse_image_rows(ops, api):
    """performance(..., inverse_image=True) returns the rows of the plain call, unchanged, plus exactly RMSE_inv and Dice_inv: ops.rmse of
    outputs_inv against x at the level, and the Dice of ops.warp_labels_soft_dice with the label maps exchanged under the inverse fields"""
    from pulpo_amd import evaluation
    size = SIZES[1]
    x, y, seg_x, seg_y, _, _ = _batch(size)
    model = _model(api, size, "ncc").eval()
    plain = evaluation.performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C)
    both = evaluation.performance(model, x, y, seg_x=seg_x, seg_y=seg_y, num_classes=C, inverse_image=True)
    assert set(plain) == {"RMSE", "JDetStd", "JDetLeq0", "Dice"} and set(both) == set(plain) | set(evaluation.INVERSE_IMAGE_METRICS)
    for m in plain:
        for l in plain[m]:
            assert torch.equal(plain[m][l], both[m][l]), (m, l)
    res = model.predict_bidirectional(x, y, deterministic=True)
    for l in (0, 1):
        out = res["outputs_inv"][l]
        tgt = x if tuple(out.shape[2:]) == tuple(x.shape[2:]) else ops.resize_trilinear(x, tuple(out.shape[2:]))
        assert torch.equal(both["RMSE_inv"][l], ops.rmse(out, tgt))
        assert torch.equal(both["Dice_inv"][l], ops.warp_labels_soft_dice(res["final_dfs_inv"][l], seg_y, C, seg_x)[1])
        assert 0.0 < float(both["Dice_inv"][l]) <= 1.0 and float(both["RMSE_inv"][l]) > 0
    assert set(evaluation.performance(model, x, y, inverse_image=True)) == {"RMSE", "JDetStd", "JDetLeq0", "RMSE_inv"}
    with pytest.raises(NotImplementedError):
        evaluation.performance(model, x, y, inverse_image=True, affine={})
