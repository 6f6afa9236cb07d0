"""The 1x1x1 heads on the PRE-NORM tensor of the ConvUnit in front of them (pulpo_heads_fwd_bn_t, pulpo_heads_bwd_bn_t,
pulpo_bn_lrelu_bwd_apply_heads_t / _kb_t): the unit's activation z = lrelu(scale y + shift) and the gradient dz the head returns are formed
per element and never written.

Through the C ABI, fused against the separate passes of the same build (pulpo_bn_lrelu_apply -> pulpo_heads_fwd, pulpo_heads_bwd):
  * head outputs and the head's partial rows (dW | db per block: same block partition, same order) bit for bit;
  * sum dbn, sum dbn (y - m32), dbeta, dgamma and dy element by element against the float64 references of tests/pyramid_ref.py, with
    bounds T = m max(1, rho32) 2^-24 A built from the float64 values alone (rho32: the same plain-ops reference evaluated in fp32):
      dpre (mu rows)    = g0 + g2: one rounding, u (|g0| + |g2|)
      dpre (sigma rows) = (g1 + g2 eps) s, s = 1 - exp(-sigma): 3 u of the product's magnitude, and s itself - expf within 2 ulp, the
                          subtraction one more, sigma the forward's fp32 output whose error T_sigma = (C + 2) u (sum |z| |W| + |b|) sigmoid' + 4 u sigma
                          enters through exp(-sigma): (e (T_sigma + 3 u) + u s) (|g1| + |g2 eps|)
      dz = sum_j dpre_j W_jc: nout fused multiply-adds, m = nout + 1 on A = sum_j |dpre_j| |W_jc|, plus the dpre bounds carried through |W|
      sums, dbeta, dgamma, dy: the formulae of test_batchnorm_chain_vs_float64 (tests/test_gpu_pyramid_convunit.py) with dz's bound as the
      gradient's own error and the coefficient block rounded from the float64 statistics (one rounding per entry); voxels whose
      y scale + shift lies within its bound of the LeakyReLU kink get that test's allowance, 0.8 |dz|;
    every comparison also rejects the reference with one element moved by 1e-3 max|ref| (check());
  * two evaluations give the same bits.
Through the modules at 16^3 (PULPoEncoder: ConvSequence -> MuSigmaBlock; VelocityField): outputs equal to the unfused path, gradients within
the ConvUnit golden test's tolerance (test_conv_unit_golden), every fallback condition on the separate passes, both modes deterministic."""
import ctypes

import pytest
import torch

import pyramid_ref as R
from test_gpu_pyramid_convunit import U, _chan, _csum, bound, coef_block, held, vp
from test_gpu_pyramid_ops import gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE, EPS = 0.2, 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


def _lib():
    from pulpo_amd._lib import lib
    return lib


def _like(B, C, size, off, fill=float("nan")):
    """(B, C, D, H, W) channels-last fp32 tensor, NaN-filled; off: channels [off, off + C) of a tensor eight channels wider (a slice that is
    4-byte but - for off % 4 != 0 - not 16-byte aligned)"""
    wide = torch.full((B, *size, C + (8 if off is not None else 0)), fill, device=DEV)
    t = wide if off is None else wide[..., off:off + C]
    return t.permute(0, 4, 1, 2, 3)


# (B, C, size, nout, eps?, slice offset): 5x6x7 (tail trips, rows that do not fill a block) and 8^3, B = 1 and 2, C = 32 / 96 (groups of four), C = 6
# (single channels), a 32-channel slice at channel 1 of a 40-channel tensor (single channels), both heads, with and without noise
CASES = [(1, 32, (5, 6, 7), 6, True, None), (2, 32, (8, 8, 8), 3, False, None), (2, 96, (5, 6, 7), 6, False, None), (1, 96, (8, 8, 8), 3, False, None),
         (2, 96, (8, 8, 8), 6, True, None), (1, 6, (5, 6, 7), 6, True, None), (2, 6, (8, 8, 8), 3, False, None), (2, 6, (8, 8, 8), 6, False, None),
         (2, 32, (5, 6, 7), 6, True, 1), (1, 32, (8, 8, 8), 3, False, 1), (2, 32, (5, 6, 7), 3, False, None), (1, 32, (8, 8, 8), 6, False, None)]


@pytest.mark.parametrize("B,C,size,nout,with_eps,off", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_heads_on_prenorm_tensor_vs_separate_passes_and_float64(ops, B, C, size, nout, with_eps, off):
    lib, st = _lib(), ops._stream()
    D, H, W = size
    V, npix = D * H * W, B * D * H * W
    g = gen(7 * C + 3 * D + B + nout)
    name = f"heads_bn B{B} C{C} {size} nout{nout} eps{int(with_eps)} off{off}"
    y = _like(B, C, size, off)
    y.copy_(torch.randn(B, C, *size, device=DEV, generator=g) * 1.5 + 0.3)
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.3
    Wt = torch.randn(nout, C, device=DEV, generator=g) / C ** 0.5
    hb = torch.randn(nout, device=DEV, generator=g)
    eps = torch.randn(B, 3, *size, device=DEV, generator=g) if with_eps else None
    gs = [torch.randn(B, 3, *size, device=DEV, generator=g) for _ in range(3 if nout == 6 else 1)] + [None] * (0 if nout == 6 else 2)
    y64 = y.double()
    r = R.bn_train_ref(y64, gamma.double(), beta.double(), EPS, 0.1, None, None, SLOPE)
    coef = coef_block(r["mean"], r["rstd"], gamma.double(), beta.double()).contiguous()
    assert coef.data_ptr() % 16 == 0
    cf = coef[:4 * C].reshape(4, C)
    yps = y.stride(4)
    v4 = C % 4 == 0 and off is None
    assert (y.data_ptr() % 16 == 0) == (off is None)

    # ---------------- forward: separate passes, then the head on y
    z = _like(B, C, size, off)
    lib.call("pulpo_bn_lrelu_apply", vp(y), yps, vp(z), z.stride(4), vp(coef), npix, C, SLOPE, st)
    nan = lambda: torch.full((B, 3, *size), float("nan"), device=DEV)
    o_sep, o_fus = [nan() for _ in range(3)], [nan() for _ in range(3)]
    lib.call("pulpo_heads_fwd", vp(z), z.stride(4), vp(Wt), vp(hb), vp(eps), *(vp(t) for t in o_sep), nout, B, V, C, st)
    lib.call("pulpo_heads_fwd_bn_t", vp(y), yps, vp(coef), SLOPE, vp(Wt), vp(hb), vp(eps), *(vp(t) for t in o_fus), nout, B, V, C, st)
    for k in range(3 if nout == 6 else 1):
        assert bool(torch.isfinite(o_sep[k]).all())
        assert torch.equal(o_fus[k], o_sep[k]), f"{name}: head output {k} differs from the separate passes"
    sigma = o_sep[1] if nout == 6 else None

    # ---------------- backward of the head: partial rows equal to pulpo_heads_bwd's (same blocks), sums against float64
    hblk = lib.query("pulpo_heads_bwd_blocks", B, V, C)
    rowlen = nout * C + nout
    dz = _like(B, C, size, off)
    p_sep = torch.full((hblk * rowlen,), float("nan"), device=DEV)
    lib.call("pulpo_heads_bwd", vp(z), z.stride(4), vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma), vp(dz), dz.stride(4), vp(p_sep), nout, B, V, C, st)
    runs = []
    for _ in range(2):
        p_fus = torch.full((hblk * rowlen,), float("nan"), device=DEV)
        bnpart = torch.full((hblk * 2 * C,), float("nan"), device=DEV)
        lib.call("pulpo_heads_bwd_bn_t", vp(y), yps, vp(coef), SLOPE, vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma), vp(p_fus), vp(bnpart),
                 nout, B, V, C, st)
        runs.append((p_fus, bnpart))
    p_fus, bnpart = runs[0]
    assert bool(torch.isfinite(p_sep).all()) and torch.equal(p_fus, p_sep), f"{name}: the head's dW / db rows differ from pulpo_heads_bwd's"
    assert torch.equal(runs[1][0], p_fus) and torch.equal(runs[1][1], bnpart), f"{name}: two evaluations of the backward differ"
    print(f"{name}: {hblk} head blocks, groups of {4 if v4 else 1}")

    # float64: dz from the heads reference on the float64 activation, then the BatchNorm / LeakyReLU backward
    W64, b64 = Wt.double(), hb.double()
    z64 = r["z"]
    g64 = [t.double() for t in gs if t is not None]
    if nout == 6:
        pre_s = R._mix(z64, W64[3:], b64[3:])
        sg64 = torch.nn.functional.softplus(pre_s)
        e64 = torch.exp(-sg64)
        s64 = 1 - e64
        gsum = g64[1] + (g64[2] * eps.double() if with_eps else 0)
        a_gs = g64[1].abs() + ((g64[2] * eps.double()).abs() if with_eps else 0)
        dpre = torch.cat([g64[0] + g64[2], gsum * s64], 1)
        # (softplus' = sigmoid = 1 - exp(-sigma); log1pf(expf(.)): four more roundings of sigma itself)
        t_sigma = (C + 2) * U * (R._mix(z64.abs(), W64[3:].abs(), b64[3:].abs())) * s64 + 4 * U * sg64
        t_dpre = torch.cat([U * (g64[0].abs() + g64[2].abs()), 3 * U * a_gs * s64 + (e64 * (t_sigma + 3 * U) + U * s64) * a_gs], 1)
    else:
        dpre, t_dpre = g64[0], torch.zeros_like(g64[0])
    mixT = lambda d, w: torch.einsum("bj...,jc->bc...", d, w)
    dz64 = mixT(dpre, W64)
    a_dz = mixT(dpre.abs(), W64.abs())
    t_dz = bound(name + " dz", mixT(dpre.float(), Wt), dz64, a_dz, nout + 1.0) + mixT(t_dpre, W64.abs())
    held(name + " dz (separate pass)", dz, dz64, t_dz)           # (the bound itself, on the tensor the old kernel writes)
    bw = R.bn_lrelu_bwd_ref(dz64, y64, r["mean"], r["rstd"], r["scale"], r["shift"], SLOPE)
    # coefficient block: the float64 statistics rounded once per entry
    t_mean, t_rstd, t_scale = U * r["mean"].abs(), U * r["rstd"], U * r["scale"].abs()
    tiny = 1e-30
    t_bn = ((y64 - _chan(r["mean"])).abs() * _chan(t_scale) + _chan(r["scale"].abs() * t_mean + 2 * U * (beta.double().abs() + (r["mean"] * r["scale"]).abs()))
            + 2 * U * ((y64 * _chan(r["scale"])).abs() + _chan(r["shift"].abs())))
    near = (r["bn"].abs() <= t_bn) & (r["bn"] != 0)
    print(f"{name}: {int(near.sum())} of {near.numel()} voxels within the bound of the LeakyReLU kink")
    m32 = cf[0].double()
    yc32 = y64 - _chan(m32)
    flip = 0.8 * dz64.abs() * near + t_dz
    mblk = (npix + hblk - 1) // hblk + 2
    prow = bnpart.reshape(hblk, 2, C)
    assert bool(torch.isfinite(prow).all()), f"{name}: {int((~torch.isfinite(prow)).sum())} BatchNorm row entries were not written"
    t_s = mblk * U * _csum(bw["dbn"].abs()) + _csum(flip)
    t_q = mblk * U * _csum((bw["dbn"] * yc32).abs()) + _csum(flip * yc32.abs())
    got = prow.double().sum(0)
    held(name + " rows sum dbn", got[0], bw["sum_dbn"], t_s)
    held(name + " rows sum dbn (y - m32)", got[1], _csum(bw["dbn"] * yc32), t_q)
    tot = torch.full((2 * C,), float("nan"), device=DEV)
    totd = torch.full((2 * C,), float("nan"), device=DEV, dtype=torch.float64)
    assert lib.query("pulpo_bn_bwd_finalize_scratch_doubles", hblk, C) == 0
    lib.call("pulpo_bn_bwd_finalize", vp(bnpart), hblk, C, vp(coef), float(npix), 1, vp(tot), ctypes.c_void_p(tot.data_ptr() + 4 * C), 0, vp(totd), None, st)
    t_x = t_q + t_mean * bw["sum_dbn"].abs() + U * r["mean"].abs() * t_s
    t_dgamma = r["rstd"] * t_x + bw["sum_dbn_c"].abs() * t_rstd + 2 * U * bw["dgamma"].abs()
    held(name + " dbeta", tot[:C], bw["dbeta"], t_s + U * bw["dbeta"].abs())
    held(name + " dgamma", tot[C:], bw["dgamma"], t_dgamma)

    # ---------------- second pass: dy (channels-last and, C % 8 == 0, channel-blocked) and the bias-gradient rows
    sc, rs = _chan(r["scale"]), _chan(r["rstd"])
    yc = y64 - _chan(r["mean"])
    a_dy = sc.abs() * (bw["dbn"].abs() + _chan(bw["sum_dbn"].abs()) / npix + yc.abs() * rs * rs * _chan(bw["sum_dbn_c"].abs()) / npix)
    t_dy = (8 * U * a_dy + sc.abs() * (flip + _chan(t_s) / npix + yc.abs() * (rs * rs * _chan(t_x) + 2 * rs * _chan(t_rstd * bw["sum_dbn_c"].abs())) / npix
                                       + _chan(t_mean + tiny) * rs * rs * _chan(bw["sum_dbn_c"].abs()) / npix) + _chan(t_scale / r["scale"].abs()) * a_dy)
    nblk = lib.query("pulpo_bn_bwd_blocks", npix, C)
    hargs = (vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma))
    for blocked in ([False, True] if C % 8 == 0 else [False]):
        outs = []
        for _ in range(2):
            part2 = torch.full((nblk * C,), float("nan"), device=DEV)
            if blocked:
                dyk = torch.full((C // 8, B, *size, 8), float("nan"), device=DEV)
                lib.call("pulpo_bn_lrelu_bwd_apply_heads_kb_t", vp(y), yps, vp(coef), vp(totd), SLOPE, *hargs, vp(dyk), 8, npix * 8, vp(part2), nout, B, V, C, st)
                dyt = ops.blocked_to_cl(dyk)
            else:
                dyt = _like(B, C, size, off)
                lib.call("pulpo_bn_lrelu_bwd_apply_heads_t", vp(y), yps, vp(coef), vp(totd), SLOPE, *hargs, vp(dyt), dyt.stride(4), vp(part2), nout, B, V, C, st)
            outs.append((dyt, part2))
        dyt, part2 = outs[0]
        sfx = "_kb" if blocked else ""
        assert torch.equal(outs[1][0], dyt) and torch.equal(outs[1][1], part2), f"{name}{sfx}: two evaluations of the second pass differ"
        held(f"{name}{sfx} dy", dyt, bw["dy"], t_dy)
        p2 = part2.reshape(nblk, C)
        assert bool(torch.isfinite(p2).all()), f"{name}{sfx}: {int((~torch.isfinite(p2)).sum())} bias-gradient row entries were not written"
        # (bias-gradient rows: the column sums of the STORED dy, as in the BatchNorm-chain test)
        t_b = ((npix + nblk - 1) // nblk + 2) * U * _csum(dyt.double().abs())
        held(f"{name}{sfx} bias rows", p2.double().sum(0), _csum(dyt.double()), t_b, power=None)
        assert float(t_b[-1]) < 1e-3 * float(_csum(dyt.double().abs())[-1])


# ================================================================================================ through the modules
def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _grads_close(name, got, ref, wscale):
    """the ConvUnit golden test's tolerance (test_conv_unit_golden): relative L2 error below 1e-4; a conv bias in front of a BatchNorm has a
    true gradient of 0 and holds rounding noise - held to 1e-4 of the weight gradient's scale"""
    for k in ref:
        if ref[k] is None:
            assert got[k] is None, (name, k)
        elif k.endswith("_op.0.bias") and "_op." in k[:-10]:
            assert float((got[k] - ref[k]).abs().max()) <= 1e-4 * max(1.0, wscale), (name, k)
        else:
            assert rel_l2(got[k], ref[k]) < 1e-4, (name, k, rel_l2(got[k], ref[k]))


def _run(ops, module, inputs, ups, fuse, call=None):
    """forward + backward of a fresh copy of the inputs; returns (outputs, gradients by name, heads that ran on the pre-norm tensor)"""
    old, hits = ops.FUSE_HEAD_BN, ops.HEAD_BN_HITS
    ops.FUSE_HEAD_BN = fuse
    try:
        module.zero_grad(set_to_none=True)
        xs = [t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in inputs]
        outs = (call or module)(*xs)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in module.named_parameters()}
        grads.update({f"input{k}": x.grad.clone() for k, x in enumerate(xs)})
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], grads, ops.HEAD_BN_HITS - hits
    finally:
        ops.FUSE_HEAD_BN = old


def _bn_buffers(module):
    return {n: b.clone() for n, b in module.named_buffers()}


def _restore(module, buffers):
    for n, b in module.named_buffers():
        b.copy_(buffers[n])


def _encoder(ops, g, sampler="fixed", B=2, S=16):
    from pulpo_amd.components.pulpo import PULPoEncoder
    from pulpo_amd.network_blocks import FixedNoiseSampler, gauss_sampler
    eps = torch.randn(B, 3, S, S, S, device=DEV, generator=g)
    torch.manual_seed(11)
    enc = PULPoEncoder(FixedNoiseSampler(eps) if sampler == "fixed" else (gauss_sampler if sampler == "gauss" else sampler), 32, 3, (S, S, S), n0=8).to(DEV).train()
    CL = torch.channels_last_3d
    act = torch.randn(B, 32, S, S, S, device=DEV, generator=g).contiguous(memory_format=CL)
    fb = torch.randn(B, 24, S, S, S, device=DEV, generator=g).contiguous(memory_format=CL)
    ups = [torch.randn(B, 3, S, S, S, device=DEV, generator=g) for _ in range(3)]
    return enc, [act, fb], ups


def _compare(ops, name, module, inputs, ups, call=None, expect_hits=1):
    buf = _bn_buffers(module)
    o_ref, g_ref, h_ref = _run(ops, module, inputs, ups, False, call)
    b_ref = _bn_buffers(module)
    _restore(module, buf)
    o_fus, g_fus, h_fus = _run(ops, module, inputs, ups, True, call)
    assert h_ref == 0 and h_fus == expect_hits, (name, h_ref, h_fus)
    for a, b in zip(o_fus, o_ref):
        assert torch.equal(a, b), f"{name}: outputs differ from the separate passes"
    for n, b in module.named_buffers():
        assert torch.equal(b, b_ref[n]), f"{name}: buffer {n} differs"
    wscale = max([float(v.abs().max()) for k, v in g_ref.items() if v is not None and k.endswith("_op.0.weight")], default=1.0)
    _grads_close(name, g_fus, g_ref, wscale)
    return o_fus, g_fus


def test_conv_sequence_to_mu_sigma_block_equals_the_separate_passes(ops):
    enc, inputs, ups = _encoder(ops, gen(5))
    call = lambda a, f: enc(a, feedback=f)
    _, g1 = _compare(ops, "encoder", enc, inputs, ups, call)
    assert all(v is not None for v in g1.values())
    # two evaluations: the same bits, in the default and in the deterministic mode
    for det in (ops.DETERMINISTIC, not ops.DETERMINISTIC):
        was = ops.DETERMINISTIC
        ops.set_deterministic(det)
        try:
            buf = _bn_buffers(enc)
            _, ga, ha = _run(ops, enc, inputs, ups, True, call)
            _restore(enc, buf)
            _, gb, hb = _run(ops, enc, inputs, ups, True, call)
            _restore(enc, buf)
        finally:
            ops.set_deterministic(was)
        assert ha == 1 and hb == 1
        # (the BatchNorm backward of the unit in front of the head and the head's own gradients are order-fixed in both modes; the weight gradients
        #  of the convolutions add with atomics outside the deterministic mode)
        keys = list(ga) if det else [k for k in ga if "mu_sigma" in k or k.endswith("sample_merge_block._op.1._op.1.weight") or k.endswith("sample_merge_block._op.1._op.1.bias")]
        assert keys
        for k in keys:
            assert torch.equal(ga[k], gb[k]), (det, k)


def test_velocity_field_equals_the_separate_passes(ops):
    from pulpo_amd.network_blocks import VelocityField
    g = gen(9)
    torch.manual_seed(3)
    vf = VelocityField((16, 16, 16), 3, 8, 3).to(DEV).train()
    zs = torch.randn(2, 3, 16, 16, 16, device=DEV, generator=g)
    ups = [torch.randn(2, 3, 16, 16, 16, device=DEV, generator=g)]
    _compare(ops, "velocity field", vf, [zs], ups)


@pytest.mark.parametrize("why", ["hook-unit", "hook-bn", "hook-lrelu", "hook-sequence", "eval", "user-sampler", "zdim", "2d", "no-feedback", "twice"])
def test_fallback_conditions_keep_the_separate_passes(ops, why):
    """each condition under which the activation has (or may have) another reader: the separate passes run (no head on a pre-norm tensor is
    counted) and give the numbers of the switched-off path"""
    from pulpo_amd.components.pulpo import PULPoEncoder
    from pulpo_amd.network_blocks import FixedNoiseSampler
    g = gen(21)
    if why == "2d":
        torch.manual_seed(11)
        eps = torch.randn(2, 2, 16, 16, device=DEV, generator=g)
        enc = PULPoEncoder(FixedNoiseSampler(eps), 32, 2, (16, 16), n0=8).to(DEV).train()
        inputs = [torch.randn(2, 32, 16, 16, device=DEV, generator=g), torch.randn(2, 16, 16, 16, device=DEV, generator=g)]
        ups = [torch.randn(2, 2, 16, 16, device=DEV, generator=g) for _ in range(3)]
        _compare(ops, why, enc, inputs, ups, lambda a, f: enc(a, feedback=f), expect_hits=0)
        return
    if why == "zdim":
        torch.manual_seed(11)
        eps = torch.randn(2, 4, 16, 16, 16, device=DEV, generator=g)
        enc = PULPoEncoder(FixedNoiseSampler(eps), 32, 4, (16, 16, 16), n0=8).to(DEV).train()
        CL = torch.channels_last_3d
        inputs = [torch.randn(2, 32, 16, 16, 16, device=DEV, generator=g).contiguous(memory_format=CL),
                  torch.randn(2, 32, 16, 16, 16, device=DEV, generator=g).contiguous(memory_format=CL)]
        ups = [torch.randn(2, 4, 16, 16, 16, device=DEV, generator=g) for _ in range(3)]
        _compare(ops, why, enc, inputs, ups, lambda a, f: enc(a, feedback=f), expect_hits=0)
        return
    sampler = (lambda mu, sigma: mu + 0.5 * sigma) if why == "user-sampler" else "fixed"
    enc, inputs, ups = _encoder(ops, g, sampler)
    call = lambda a, f: enc(a, feedback=f)
    seen = []
    hook = lambda m, i, o: seen.append(tuple(o.shape))
    blk = enc.sample_merge_block
    target = {"hook-unit": blk._op[-1], "hook-bn": blk._op[-1]._op[1], "hook-lrelu": blk._op[-1]._op[2], "hook-sequence": blk}.get(why)
    handle = target.register_forward_hook(hook) if target is not None else None
    try:
        if why == "eval":
            enc.eval()
            with torch.no_grad():
                hits = ops.HEAD_BN_HITS
                a = enc(*[t.clone() for t in inputs[:1]], feedback=inputs[1])
                ops.FUSE_HEAD_BN, old = False, ops.FUSE_HEAD_BN
                try:
                    b = enc(inputs[0], feedback=inputs[1])
                finally:
                    ops.FUSE_HEAD_BN = old
                assert ops.HEAD_BN_HITS == hits and all(torch.equal(p, q) for p, q in zip(a, b))
        elif why == "no-feedback":               # (the coarsest level: the head reads a DownPath activation, a skip tensor with other readers)
            _compare(ops, why, enc, inputs[:1], ups, lambda a: enc(a), expect_hits=0)
        elif why == "twice":
            # a second differentiable pass over the same tensors before the first one's backward: both fuse (each pass owns its pre-norm tensor), and the
            # summed gradients are those of the separate passes
            both = lambda a, f: tuple(p + q for p, q in zip(enc(a, feedback=f), enc(a, feedback=f)))
            _compare(ops, why, enc, inputs, ups, both, expect_hits=2)
        else:
            _compare(ops, why, enc, inputs, ups, call, expect_hits=0)
            if why in ("hook-unit", "hook-sequence"):
                assert seen and all(s == (2, 32, 16, 16, 16) for s in seen)        # (the hook saw the activation itself)
    finally:
        if handle is not None:
            handle.remove()
