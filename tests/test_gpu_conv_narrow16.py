"""The 16-channel forms of the F(2x2x2,3x3x3) kernels (v_mfma_f32_16x16x4_f32 tiles): the forward / data-gradient kernel with 16 output
channels - the feedback layers' data gradient 96 -> 16 - and the weight-gradient kernel on a 16-channel ci tile (Cin = 16, or the last tile of
Cin = 48).  Every case first asserts the route through pulpo_conv3d_k3_narrow16, then holds the FULL result tensor - all six border faces are
among the compared elements - to the float64 reference with the bounds tests/test_gpu_pyramid_convunit.py derives for these kernel families
(T = m max(1, rho32) 2^-24 A, m = 54 for F(2x2x2,3x3x3); the 16x16x4 instruction sums k in another grouping, the bound does not care).

Shapes: the smallest whole-tile volumes pulpo_conv3d_k3_algo routes to the kernel (4-deep statistics tiles need 64 000 voxels, the kernel
256 work items): 32x32x64 = exactly 256 tiles (one tile per workgroup, no next tile, deferred statistics flush after the loop, tiles walked in
4x4x4 bricks) and 36x32x64 = 288 tiles (32 workgroups take a second tile, linear tile order); B = 2 at 32x32x64 gives every workgroup a second
tile in the OTHER batch element.  257 tiles - exactly one workgroup with a second tile - is prime and no whole-tile volume has it.
Weight gradient: 4x16x16 (two plane pairs per column: the segment warm-up is as long as the segment) and 12x16x16 (several segments per split)."""
import pytest
import torch

import pyramid_ref as R
from test_gpu_pyramid_convunit import CL, DEV, M_FWD, M_WGRAD, bound, coef_block, conv_data, held, rows_vs_stored, vp
from test_gpu_pyramid_ops import gen

pytestmark = pytest.mark.gpu

S256, S288 = (32, 32, 64), (36, 32, 64)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    assert torch.backends.cuda.matmul.allow_tf32 is False
    return _ops


def _blocked(ops, t):
    """t (B, C, D, H, W) as the channel-blocked operand [C / 8][B][D][H][W][8]"""
    B, C, D, H, W = t.shape
    g = ops._BlockedGrad(B, C, D, H, W, t.device)
    g.buf.copy_(t.permute(0, 2, 3, 4, 1).reshape(B, D, H, W, C // 8, 8).permute(4, 0, 1, 2, 3, 5).reshape(-1))
    return g


# ================================================================================================ data gradient, N = 16
def _dgrad_route(lib, B, size, K, N=16):
    assert lib.query("pulpo_conv3d_k3_narrow16", 0, K, N) == 1
    assert lib.query("pulpo_conv3d_k3_narrow16", 0, K, 32) == 0 and lib.query("pulpo_conv3d_k3_narrow16", 2, K, N) == 0
    assert lib.query("pulpo_conv3d_k3_algo", B, *size, K, N) == 3


def _dgrad_case(g, B, K, size, N=16):
    """dy (B, K, size), the unit's weight wt (Cout = K, Cin = N), its dgrad pack - operands with a mean of their own, as the BNRED cases of
    test_gpu_pyramid_convunit.py use them (row sums then grow like the magnitude sums of their bound)"""
    dy, w, _, _ = conv_data(g, B, K, N, size, False)
    dy, w = dy + 1.0, w + 1.0 / (27 * K)
    wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()
    return dy, wt


def _pack_dgrad(ops, wt, K, N):
    lib = ops.lib
    wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_wino3_floats", K, N), device=DEV)
    lib.call("pulpo_conv3d_k3_pack_weight_wino3", vp(wt), vp(wp), N, K, 1, ops._stream())
    return wp


def _hold_dx(name, dx, dy, wt):
    assert bool(torch.isfinite(dx).all()), f"{name}: {int((~torch.isfinite(dx)).sum())} elements of dx were not written"
    ref = R.conv3_dgrad_ref(dy.double(), wt.double())
    held(name + " dx", dx, ref, bound(name + " dx", R.conv3_dgrad_ref(dy, wt), ref, R.conv3_dgrad_mag(dy.double(), wt.double()), M_FWD["z"]))


# (B, K, size, blocked dy): 96 -> 16 on 256 and on 288 tiles; two chunks (the least the staging allows); three chunks - the image parity
# differs from tile to tile - at B = 2; the channel-blocked gradient operand of the step's 80^3 level (ops._blocked_dy_ok takes this layer)
DGRAD_CASES = [(1, 96, S256, False), (1, 96, S288, False), (1, 16, S256, False), (2, 24, S256, False), (1, 96, S256, True)]


@pytest.mark.parametrize("B,K,size,kb", DGRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dgrad_16_channels_vs_float64(ops, B, K, size, kb):
    """dx and the statistics rows (NaN-filled on entry) of the plain entry points: every row written, rows summed in float64 = the channel
    sums of the stored dx"""
    lib, N = ops.lib, 16
    _dgrad_route(lib, B, size, K)
    dy, wt = _dgrad_case(gen(K + B + size[0]), B, K, size)
    wp = _pack_dgrad(ops, wt, K, N)
    dx = torch.full((B, *size, N), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
    nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
    stats = torch.full((nrow * 2 * N,), float("nan"), device=DEV)
    xs, st = ops.grid_strides(dx), ops._stream()
    if kb:
        blk = _blocked(ops, dy)
        lib.call("pulpo_conv3d_k3_fwd_wino3_kb", vp(blk.buf), blk.bs, blk.ps, blk.kb, vp(wp), None, None, 0.2, vp(dx), xs[0], xs[1], 8, vp(stats),
                 B, *size, K, N, st)
    else:
        dyc = dy.contiguous(memory_format=CL)
        lib.call("pulpo_conv3d_k3_fwd_wino3", vp(dyc), *ops.grid_strides(dyc), vp(wp), None, None, 0.2, vp(dx), *xs, vp(stats), B, *size, K, N, st)
    name = f"narrow16 dgrad B{B} {K}to{N} {size} kb={kb}"
    _hold_dx(name, dx, dy, wt)
    d64 = dx.double()
    rows_vs_stored(name, stats, nrow, N, d64.sum(dim=(0, 2, 3, 4)), (d64 * d64).sum(dim=(0, 2, 3, 4)), d64.abs().sum(dim=(0, 2, 3, 4)),
                   (d64 * d64).sum(dim=(0, 2, 3, 4)), d64.numel() // N)


def test_dgrad_16_channels_with_batchnorm_backward_rows(ops):
    """the _bnred entry (the C ABI takes N = 16 there too): rows = sum(dbn), sum(dbn (y - mean)) formed from the kernel's own stored dx"""
    lib, B, K, N, size = ops.lib, 1, 32, 16, S288
    _dgrad_route(lib, B, size, K)
    g = gen(K + N + size[0])
    dy, wt = _dgrad_case(g, B, K, size)
    ybn = (torch.randn(B, N, *size, device=DEV, generator=g) * 1.5 + 0.3).contiguous(memory_format=CL)
    mean = ybn.double().mean(dim=(0, 2, 3, 4))
    rstd = (ybn.double().var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5).rsqrt()
    coef = coef_block(mean, rstd, torch.rand(N, device=DEV, generator=g).double() + 0.5, torch.randn(N, device=DEV, generator=g).double() * 0.5)
    wp = _pack_dgrad(ops, wt, K, N)
    dyc = dy.contiguous(memory_format=CL)
    dx = torch.full((B, *size, N), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
    nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
    part = torch.full((nrow * 2 * N,), float("nan"), device=DEV)
    xs, ys = ops.grid_strides(dx), ops.grid_strides(ybn)
    lib.call("pulpo_conv3d_k3_dgrad_wino3_bnred", vp(dyc), *ops.grid_strides(dyc), vp(wp), vp(dx), xs[0], xs[1], vp(ybn), ys[0], ys[1], vp(coef), 0.2,
             vp(part), B, *size, K, N, ops._stream())
    name = f"narrow16 bnred {K}to{N} {size}"
    _hold_dx(name, dx, dy, wt)
    v = lambda t: t.reshape(1, -1, 1, 1, 1)
    bn = ybn * v(coef[2 * N:3 * N]) + v(coef[3 * N:4 * N])
    dbn = torch.where(bn > 0, dx, 0.2 * dx).double()
    yc = ybn.double() - v(coef[:N].double())
    rows_vs_stored(name, part, nrow, N, dbn.sum(dim=(0, 2, 3, 4)), (dbn * yc).sum(dim=(0, 2, 3, 4)), dbn.abs().sum(dim=(0, 2, 3, 4)),
                   (dbn * yc).abs().sum(dim=(0, 2, 3, 4)), dbn.numel() // N)


# ================================================================================================ weight gradient, ci tile of 16
def _wgrad_call(ops, x, dy, budget=None, det=False, kb=False):
    """one of the C entry points: atomic / deterministic (slabs), with (budget) or without the workgroup budget, dy channels-last or blocked"""
    lib = ops.lib
    B, Cin, D, H, W = x.shape
    Cout = dy.shape[1]
    dw = torch.full((Cout, Cin, 3, 3, 3), float("nan"), device=DEV)
    nscr = lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", Cin, Cout)
    scratch = torch.empty(nscr, device=DEV)
    nslab = lib.query("pulpo_conv3d_k3_wgrad_det_slabs", Cin, Cout)
    slabs = torch.empty(nslab * nscr, device=DEV) if det else None
    xb, xp, xc = ops.grid_strides(x)
    tail = (B, D, H, W, Cin, Cout, ops._stream()) + (() if budget is None else (int(budget),))
    sfx = "" if budget is None else "_wg"
    if kb:
        blk = _blocked(ops, dy)
        lib.call("pulpo_conv3d_k3_wgrad_kb" + sfx, vp(x), xb, xp, 8, vp(blk.buf), blk.bs, blk.ps, blk.kb, vp(dw), 0, vp(scratch), vp(slabs),
                 nslab if det else 0, *tail)
    elif det:
        lib.call("pulpo_conv3d_k3_wgrad_det" + sfx, vp(x), xb, xp, xc, vp(dy), *ops.grid_strides(dy), vp(dw), 0, vp(scratch), vp(slabs), nslab, *tail)
    else:
        lib.call("pulpo_conv3d_k3_wgrad" + sfx, vp(x), xb, xp, xc, vp(dy), *ops.grid_strides(dy), vp(dw), 0, vp(scratch), *tail)
    return dw


# (B, Cin, Cout, size): one and three cout tiles at the two depths; ci tiles 32 + 16 (only the last one narrow, one packed gradient); B = 2
WGRAD_CASES = [(1, 16, 32, (4, 16, 16)), (1, 16, 96, (4, 16, 16)), (1, 16, 32, (12, 16, 16)), (1, 16, 96, (12, 16, 16)), (1, 48, 32, (12, 16, 16)),
               (2, 16, 32, (4, 16, 16))]


@pytest.mark.parametrize("B,Cin,Cout,size", WGRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_wgrad_16_channel_tile_vs_float64(ops, B, Cin, Cout, size):
    """one split per channel pair, the launcher's own split, a forced other split through the budgeted entry, the deterministic slabs (two
    runs bit-equal) and the channel-blocked dy - all against the float64 weight gradient"""
    lib = ops.lib
    assert lib.query("pulpo_conv3d_k3_narrow16", 1, Cin, Cout) == 1 and lib.query("pulpo_conv3d_k3_narrow16", 1, 32, Cout) == 0
    assert lib.query("pulpo_conv3d_k3_wgrad_algo", B, *size, Cin, Cout, 1) == 3
    npair = -(-Cin // 32) * -(-Cout // 32)
    full = lib.query("pulpo_conv3d_k3_wgrad_grid", B, *size, Cin, Cout, 0)
    assert lib.query("pulpo_conv3d_k3_wgrad_grid", B, *size, Cin, Cout, npair) == npair                 # nsplit = 1
    assert lib.query("pulpo_conv3d_k3_wgrad_grid", B, *size, Cin, Cout, 3 * npair) == 3 * npair < full  # a split the launcher would not pick
    g = gen(B * 1000 + Cin * 10 + Cout + size[0])
    x, _, _, dy = conv_data(g, B, Cin, Cout, size, False)
    x, dy = x.contiguous(memory_format=CL), dy.contiguous(memory_format=CL)
    x64, dy64 = x.double(), dy.double()
    ref = R.conv3_wgrad_ref(x64, dy64)
    name = f"narrow16 wgrad B{B} {Cin}to{Cout} {size}"
    tol = bound(name, R.conv3_wgrad_ref(x, dy), ref, R.conv3_wgrad_mag(x64, dy64), M_WGRAD[3])
    held(name + " nsplit=1", _wgrad_call(ops, x, dy, budget=npair), ref, tol)
    held(name + " default split", _wgrad_call(ops, x, dy), ref, tol)
    held(name + " nsplit=3", _wgrad_call(ops, x, dy, budget=3 * npair), ref, tol)
    d0, d1 = _wgrad_call(ops, x, dy, det=True), _wgrad_call(ops, x, dy, det=True)
    assert torch.equal(d0, d1), f"{name}: two deterministic runs differ"
    held(name + " slabs", d0, ref, tol)
    held(name + " blocked dy", _wgrad_call(ops, x, dy, kb=True), ref, tol)
