"""The bf16 ACTIVATION-STORAGE kernels (BASELINE configs 4 - 5, set_conv_precision("bf16", activations="bf16")) - the bf16-stored
instantiations of the bf16-operand convolution (staged, split-K + splitk_reduce, the persistent pw<NN,TPB>), the weight gradient's
transposing-read and register-prefetch paths, and the typed `*_t` forms of the BatchNorm / pooling / up-2 passes called with dtype code 1 -
each held ALONE, through the C ABI, to a float64 reference element by element.

The criterion (pyramid_ref.held_bf16).  A bf16-storing kernel computes an fp32 value v and stores RNE_bf16(v).  With r the float64 reference
and T the fp32 bound of the same operation, built exactly as the fp32 tests build it (test_gpu_pyramid_convunit: bound(), M_FWD, M_WGRAD and the
BatchNorm / pool / up-2 formulas; rho32 from the plain-ops fp32 reference, never from the kernel), |v - r| <= T and so, for every element:
  1. got is finite and |got - r| <= T + 2^-8 (|r| + T) - half a bf16 ulp at the far end of the interval;
  2. wherever r lies farther than T from every midpoint between two adjacent bf16 values, got == RNE_bf16(r) bit for bit.
Rule 2 rejects truncation, a swapped pair of a packed store, a stale lane of an exchange and any one-ulp error anywhere; the share of elements
it does not cover (NEARMID) is printed and capped - 5 % for convolution outputs and data gradients, 2 % for everything elementwise: a
condition on the inputs, not a tolerance - and every comparison is shown to have power: the reference with ONE element of the last voxel
moved by one bf16 ulp of that element must be rejected.

Inputs.  Activations are drawn as fp32, rounded to bf16 ONCE, and the kernel gets those bits; the reference reads the same bits decoded.
Coefficient blocks are built in float64 (coef_block), so every kernel is held alone and T carries no propagated terms.  Every output is
poisoned before its call (NaN).  In the elementwise tests channels 0 and 1 carry data whose fp32 arithmetic is exact - small integers, and
bf16 values with 8-bit mantissas from one binade, power-of-two scale and integer shift in the coefficient block: there T = 0, nothing is
exempt and got == RNE_bf16(r) everywhere, ties included (an average of bf16 values lands exactly on a bf16 midpoint in ~13 % of the outputs,
and RNE must break the tie to even).  The one inexact step on those lanes is the LeakyReLU slope (0.2 is no fp32 number): where the
negative branch is taken T is one rounding of the product, 2^-24 |r|.

Every convolution and weight-gradient case first asserts which kernel runs (pulpo_conv3d_k3_fwd_bf16_kernel / _wgrad_bf16_kernel)."""
import ctypes
import struct

import pytest
import torch

import pyramid_ref as R
from pulpo_amd._lib import PulpoHipError
from test_gpu_pyramid_ops import det_default, gen
from test_gpu_pyramid_convunit import (CL, DEV, M_FWD, M_WGRAD, U, _chan, _csum, _lib, bound, coef_block, conv_data, held, ops, rows_vs_stored,  # noqa: F401
                                       vp)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CAP_CONV, CAP_ELT = 0.05, 0.02
SLOPE = 0.2
SLOPE32 = float(torch.tensor(SLOPE, dtype=torch.float32).double())          # the slope as the kernels multiply by it
NAN = float("nan")


# ================================================================================================ helpers
def bf_buffer(B, size, C, width=None, off=0, fill=NAN):
    """a (B, C, D, H, W) channels-last bf16 view - the whole of a NaN-filled buffer, or channels off .. off + C of a buffer `width` channels
    wide whose other channels hold a recognisable pattern; returns (view, whole buffer)"""
    width = C if width is None else width
    buf = torch.full((B, *size, width), fill, device=DEV, dtype=BF)
    if width != C:
        buf[..., :off] = 7.0
        buf[..., off + C:] = -3.0
    return buf.permute(0, 4, 1, 2, 3)[:, off:off + C], buf


def as_bf(t, width=None, off=0):
    """t's values (already bf16-representable) as a channels-last bf16 operand, optionally a channel slice of a wider buffer"""
    B, C = t.shape[:2]
    v, _ = bf_buffer(B, t.shape[2:], C, width, off, fill=1.0)
    v.copy_(t)
    assert bool((v.double() == t.double()).all())
    return v


def untouched(buf, C, off):
    """the channels around a slice still hold bf_buffer's pattern, bit for bit"""
    return bool((buf[..., :off] == 7.0).all()) and bool((buf[..., off + C:] == -3.0).all())


def rnd(t):
    return t.bfloat16().float()


def ulp_of(r):
    return R.bf16_grid(r)[0]


def exact_lanes(g, shape):
    """(lane 0, lane 1) of shape (B, D, H, W): small integers in -2 .. 2, and +-(128 + k) / 128 - bf16 values with 8-bit mantissas from the
    binade [1, 2)"""
    a = torch.randint(-2, 3, shape, device=DEV, generator=g).float()
    k = torch.randint(0, 128, shape, device=DEV, generator=g).float()
    s = torch.randint(0, 2, shape, device=DEV, generator=g).float() * 2 - 1
    return a, s * (128 + k) / 128


def act(g, B, C, size, mean=0.0, std=1.0):
    """a bf16-representable fp32 activation (B, C, *size) with the two exact lanes in channels 0 and 1"""
    t = rnd(torch.randn(B, C, *size, device=DEV, generator=g) * std + mean)
    t[:, 0], t[:, 1] = exact_lanes(g, (B, *size))
    return t


def grid_of(v):
    """the power of two a bf16 value is a multiple of: its own ulp (inf for 0, a multiple of everything)"""
    return torch.where(v == 0, torch.full_like(v, float("inf")), ulp_of(v))


def pool_sum_exact(x64):
    """pooled windows of a tensor of bf16 values whose fp32 sum is exact IN ANY ORDER: every addend is a multiple of q = the smallest ulp in
    the window and sum |x| < 2^24 q, so every partial sum is a multiple of q below 2^24 q - an fp32 number; the product with 1 / count (a
    power of two) is exact as well.  There the kernel's fp32 value IS the reference: T = 0, ties included"""
    q = -torch.nn.functional.max_pool3d(-grid_of(x64), 2, 2, ceil_mode=True)
    return 8 * R.avgpool2_ref(x64.abs()) < 2.0 ** 24 * q


def pair_sum_exact(a64, b64):
    """the same for a + b of two bf16 values"""
    return a64.abs() + b64.abs() < 2.0 ** 24 * torch.minimum(grid_of(a64), grid_of(b64))


def lane_mask(ref):
    m = torch.zeros_like(ref, dtype=torch.bool)
    m[:, :2] = True
    return m


# ================================================================================================ a / b / c. convolutions
FWD_KERNEL = {"staged2": 0, "staged4": 1, "pw19": 2, "pw23": 3}
SPLITK = 16


def fwd_kernel(B, size, K, N, in_ps=None, out_ps=None, dt=1):
    return _lib().query("pulpo_conv3d_k3_fwd_bf16_kernel", B, *size, K, N, dt, in_ps or K, out_ps or N)


def call_conv(ops, xb, w, bias, out, stats, dgrad=False, coef=None):
    """pulpo_conv3d_k3_fwd_bf16_t / _fwd_bn_lrelu_bf16_t with dt = 1 on the bf16 operand xb, NaN-filled split-K scratch"""
    lib, st = _lib(), ops._stream()
    B, K, D, H, W = xb.shape
    N = out.shape[1]
    wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_bf16_elems", K, N), device=DEV, dtype=torch.int16)
    lib.call("pulpo_conv3d_k3_pack_weight_bf16", vp(w.contiguous()), vp(wp), w.shape[1], w.shape[0], int(dgrad), st)
    n = lib.query("pulpo_conv3d_k3_fwd_bf16_scratch_floats", B, D, H, W, K, N)
    scr = torch.full((n,), NAN, device=DEV) if n else None
    xs, ys = ops.grid_strides(xb), ops.grid_strides(out)
    if coef is None:
        lib.call("pulpo_conv3d_k3_fwd_bf16_t", vp(xb), *xs, vp(wp), vp(bias), vp(out), *ys, 1, vp(stats), vp(scr), B, D, H, W, K, N, st)
    else:
        lib.call("pulpo_conv3d_k3_fwd_bn_lrelu_bf16_t", vp(xb), *xs, vp(wp), vp(bias), vp(coef), SLOPE, vp(out), *ys, 1, vp(scr), B, D, H, W, K, N, st)
    return scr is not None


# (B, Cin, Cout, size, out width, out offset, expected kernel code): the paths of conv_fwd_bf16_impl with dt = 1
#   32 -> 32 @40^3            pw<1,9>, one chunk, 250 work items: every persistent workgroup takes one
#   32 -> 96 @48^3            pw<1,9>, 1296 items over 512 workgroups: first, steady-state and last tile of a walk, three cout tiles
#   64 -> 192 @40^3           pw<2,3>, two chunks, 750 items
#   B = 2, 96 -> 128 @40^3    pw<2,3>, three chunks, the batch stride
#   32 -> 32 @40^3 into channels 8 .. 40 of a 56-channel bf16 buffer (16-byte aligned): pw; the channels around it stay untouched
#   64 -> 64 @16^3            staged + split-K: splitk_reduce with dt = 1 writes the rows and the rounded output
#   B = 2, 40 -> 24 @9x7x10   staged 2x8x8 (+ split-K: 20 tiles, two chunks), ragged in every axis, K % 32 != 0, a partly empty cout tile
#   32 -> 32 @40x40x44        W % 8 != 0: not the persistent kernel (staged, 4x8x8)
FWD_CASES = [
    (1, 32, 32, (40, 40, 40), None, 0, FWD_KERNEL["pw19"]), (1, 32, 96, (48, 48, 48), None, 0, FWD_KERNEL["pw19"]),
    (1, 64, 192, (40, 40, 40), None, 0, FWD_KERNEL["pw23"]), (2, 96, 128, (40, 40, 40), None, 0, FWD_KERNEL["pw23"]),
    (1, 32, 32, (40, 40, 40), 56, 8, FWD_KERNEL["pw19"]), (1, 64, 64, (16, 16, 16), None, 0, FWD_KERNEL["staged2"] + SPLITK),
    (2, 40, 24, (9, 7, 10), None, 0, FWD_KERNEL["staged2"] + SPLITK), (1, 32, 32, (40, 40, 44), None, 0, FWD_KERNEL["staged4"]),
]


def _fid(c):
    return f"B{c[0]}-{c[1]}to{c[2]}-{'x'.join(map(str, c[3]))}" + (f"-ps{c[4]}" if len(c) > 4 and c[4] else "")


def conv_bound(name, x, w, b, dgrad=False):
    """(float64 reference, T = 8 max(1, rho32) 2^-24 A) of the forward convolution or the data gradient on bf16-representable operands"""
    if dgrad:
        ref = R.conv3_dgrad_ref(x.double(), w.double())
        return ref, bound(name, R.conv3_dgrad_ref(x, w), ref, R.conv3_dgrad_mag(x.double(), w.double()), M_FWD["b"])
    ref = R.conv3_ref(x.double(), w.double(), b.double())
    return ref, bound(name, R.conv3_ref(x, w, b), ref, R.conv3_mag(x.double(), w.double(), b.double()), M_FWD["b"])


@pytest.mark.parametrize("case", FWD_CASES, ids=_fid)
def test_conv_forward_bf16_stored_vs_float64(ops, case):
    """a: output by held_bf16, statistics rows against the STORED tensor decoded to float64"""
    B, Cin, Cout, size, width, off, code = case
    lib = _lib()
    assert fwd_kernel(B, size, Cin, Cout, out_ps=width) == code
    assert (lib.query("pulpo_conv3d_k3_fwd_bf16_scratch_floats", B, *size, Cin, Cout) > 0) == (code >= SPLITK)
    if size == (40, 40, 44):
        assert fwd_kernel(B, (40, 40, 40), Cin, Cout) == FWD_KERNEL["pw19"]          # (the same layer with whole tiles in x would be)
    g = gen(B * 1000 + Cin * 10 + Cout + size[2] + (width or 0))
    x, w, b, _ = conv_data(g, B, Cin, Cout, size, True)
    xb = as_bf(x)
    y, buf = bf_buffer(B, size, Cout, width, off)
    assert y.data_ptr() % 16 == 0
    nrow = lib.query("pulpo_conv3d_k3_fwd_bf16_stat_tiles", B, *size)
    stats = torch.full((nrow * 2 * Cout,), NAN, device=DEV)
    assert call_conv(ops, xb, w, b, y, stats) == (code >= SPLITK)
    name = f"bf16-store fwd {_fid(case)}"
    ref, T = conv_bound(name, x, w, b)
    R.held_bf16(name, y, ref, T, CAP_CONV)
    if width is not None:
        assert untouched(buf, Cout, off), f"{name}: channels outside the slice were written"
    y64 = y.double()
    rows_vs_stored(name, stats, nrow, Cout, _csum(y64), _csum(y64 * y64), _csum(y64.abs()), _csum(y64 * y64), y64.numel() // Cout)


@pytest.mark.parametrize("case", [(1, 32, 32, (40, 40, 40), FWD_KERNEL["pw19"]), (2, 40, 24, (9, 7, 10), FWD_KERNEL["staged2"] + SPLITK)],
                         ids=lambda c: _fid(c[:4]))
def test_conv_fused_eval_store_bf16_vs_float64(ops, case):
    """b: the eval-mode store rounds y as the unfused path would have stored it: RNE_bf16(lrelu(bn(RNE_bf16(conv)))).  Rule 2 where BOTH
    roundings are covered; where the first is not, y may sit one ulp away and z moves by |scale| ulp(y): that much is added to T there"""
    B, Cin, Cout, size, code = case
    assert fwd_kernel(B, size, Cin, Cout) == code
    g = gen(77 + Cin + Cout)
    x, w, b, _ = conv_data(g, B, Cin, Cout, size, True)
    mean = torch.randn(Cout, device=DEV, generator=g).double() * 0.3
    rstd = torch.rand(Cout, device=DEV, generator=g).double() + 0.7
    gamma = torch.rand(Cout, device=DEV, generator=g).double() + 0.5
    beta = torch.randn(Cout, device=DEV, generator=g).double() * 0.5
    coef = coef_block(mean, rstd, gamma, beta)
    sc, sh = _chan(coef[2 * Cout:3 * Cout].double()), _chan(coef[3 * Cout:4 * Cout].double())
    z, _ = bf_buffer(B, size, Cout)
    call_conv(ops, as_bf(x), w, b, z, None, coef=coef)
    name = f"bf16-store fused eval {_fid(case[:4])}"
    r1, T1 = conv_bound(name + " (y)", x, w, b)
    y1 = R.rne_bf16(r1)
    loose = ~(R.bf16_midpoint_distance(r1) > T1)
    bn = y1 * sc + sh
    ref = torch.where(bn > 0, bn, SLOPE32 * bn)
    T = 4 * U * ((y1 * sc).abs() + sh.abs()) + loose * sc.abs() * ulp_of(y1)
    R.held_bf16(name, z, ref, T, CAP_CONV, exempt=loose)


# (B, K = channels of dy, N = channels of dx, size, expected kernel): the same entry with the data-gradient pack
#   96 -> 32 @40^3: three chunks on 250 tiles - split-K on 4x8x8 tiles (conv_ksplit_bf16: fewer than 512 workgroups, more than one chunk)
#   96 -> 96 @40^3: the persistent kernel with three chunks (750 work items)
#   B = 2, 24 -> 40 @9x7x10: staged 2x8x8, one ragged chunk, ragged tiles, a partly empty cout tile
DGRAD_CASES = [(1, 96, 32, (40, 40, 40), FWD_KERNEL["staged4"] + SPLITK), (1, 96, 96, (40, 40, 40), FWD_KERNEL["pw19"]),
               (2, 24, 40, (9, 7, 10), FWD_KERNEL["staged2"])]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: _fid(c[:4]))
def test_conv_data_gradient_bf16_stored_vs_float64(ops, case):
    """c: dx = conv(dy, flipped transposed w) through pulpo_conv3d_k3_fwd_bf16_t with the dgrad pack, no bias, no statistics"""
    B, K, N, size, code = case
    assert fwd_kernel(B, size, K, N) == code
    g = gen(B + K + 3 * N)
    dy, wt, _, _ = conv_data(g, B, K, N, size, True)                 # (wt: (N, K, 3, 3, 3))
    w = wt.transpose(0, 1).flip(2, 3, 4).contiguous()                 # the unit's weight (Cout = K, Cin = N)
    assert tuple(w.shape[:2]) == (K, N)
    dx, _ = bf_buffer(B, size, N)
    call_conv(ops, as_bf(dy), w, None, dx, None, dgrad=True)
    name = f"bf16-store dgrad {_fid(case[:4])}"
    ref, T = conv_bound(name, dy, w, None, dgrad=True)
    R.held_bf16(name, dx, ref, T, CAP_CONV)


# ================================================================================================ d. weight gradient, bf16-stored x and dy
# (B, Cin, Cout, size, expected code = ntw + 16 tr + 32 pf).  ntw = row tiles per wave, ceil(ceil(27 min(Cin, 32) / 32) / 4) rounded up to
# 1 / 2 / 4 / 7: 7 from Cin = 24 up (so on every multi-channel layer of the model), 4 at Cin = 16, 2 at Cin = 8
#   32 -> 32 @8x16x16          tr + pf
#   B = 2, 32 -> 64 @6x16x24   pf with 36 splits, three tiles in z and in x
#   32 -> 32 @8x12x16          tr without pf (H % 8 != 0)
#   24 -> 40 @9x7x10           the gathers (Cin % 16 != 0), ragged in every axis
#   160 -> 64 @8x16x16         five cin chunks, two cout tiles
#   16 -> 32, 8 -> 32 @8x16x16 ntw = 4 (tr + pf) and ntw = 2 (gathers)
WGRAD_CASES = [(1, 32, 32, (8, 16, 16), 7 + 16 + 32), (2, 32, 64, (6, 16, 24), 7 + 16 + 32), (1, 32, 32, (8, 12, 16), 7 + 16), (1, 24, 40, (9, 7, 10), 7),
               (1, 160, 64, (8, 16, 16), 7 + 16 + 32), (1, 16, 32, (8, 16, 16), 4 + 16 + 32), (1, 8, 32, (8, 16, 16), 2)]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: _fid(c[:4]))
def test_weight_gradient_bf16_stored_operands_vs_float64(ops, case):
    """d: pulpo_conv3d_k3_wgrad_bf16_t and _det_t with dt = 1, accumulate 0 / 1 / 2 (deferred + pulpo_grad_finish_multi).  fp32 results: held()
    with the direct weight gradient's m = 2; adding into a non-zero dw rounds once more: 2 u (|dw0| + |ref|)"""
    B, Cin, Cout, size, code = case
    lib, st = _lib(), ops._stream()
    assert lib.query("pulpo_conv3d_k3_wgrad_bf16_kernel", B, *size, Cin, Cout, 1, Cin, Cout) == code
    g = gen(B + 7 * Cin + Cout + size[1])
    x, _, _, dy = conv_data(g, B, Cin, Cout, size, True)
    xb, dyb = as_bf(x), as_bf(dy)
    name = f"bf16-store wgrad {_fid(case[:4])}"
    ref = R.conv3_wgrad_ref(x.double(), dy.double())
    tol = bound(name, R.conv3_wgrad_ref(x, dy), ref, R.conv3_wgrad_mag(x.double(), dy.double()), M_WGRAD[0])
    nscr = lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", Cin, Cout)
    nslab = lib.query("pulpo_conv3d_k3_wgrad_det_slabs", Cin, Cout)
    dw0 = torch.randn(Cout, Cin, 3, 3, 3, device=DEV, generator=g)
    tol_acc = tol + 2 * U * (dw0.double().abs() + ref.abs())

    def run(det, accumulate, scratch=None):
        dw = torch.full((Cout, Cin, 3, 3, 3), NAN, device=DEV) if accumulate == 0 else dw0.clone()
        scr = torch.full((nscr,), NAN, device=DEV) if scratch is None else scratch
        args = (vp(xb), *ops.grid_strides(xb), vp(dyb), *ops.grid_strides(dyb), 1, vp(dw) if accumulate != 2 else None, accumulate, vp(scr))
        if det:
            slabs = torch.full((nslab * nscr,), NAN, device=DEV)
            lib.call("pulpo_conv3d_k3_wgrad_bf16_det_t", *args, vp(slabs), nslab, B, *size, Cin, Cout, st)
        else:
            lib.call("pulpo_conv3d_k3_wgrad_bf16_t", *args, B, *size, Cin, Cout, st)
        return dw

    atomic = run(False, 0)
    held(name + " dw", atomic, ref, tol)
    held(name + " dw += ", run(False, 1), dw0.double() + ref, tol_acc)
    det = run(True, 0)
    held(name + " dw det", det, ref, tol)
    assert torch.equal(det, run(True, 0)), f"{name}: the deterministic form differs between two calls"
    held(name + " dw det vs atomic", det, atomic.double(), tol)
    held(name + " dw det += ", run(True, 1), dw0.double() + ref, tol_acc)
    # deferred: the packed sums stay in a scratch that arrives all zero; one pulpo_grad_finish_multi job (kind 0) adds them into dw and
    # returns the scratch to all zero
    scr = torch.zeros(nscr, device=DEV)
    run(False, 2, scr)
    assert bool(torch.isfinite(scr).all()) and float(scr.abs().max()) > 0
    dw = dw0.clone()
    table = torch.frombuffer(bytearray(struct.pack("<QQiiii", scr.data_ptr(), dw.data_ptr(), 0, Cin, Cout, nscr // (27 * Cin))), dtype=torch.uint8).to(DEV)
    lib.call("pulpo_grad_finish_multi", vp(table), 1, st)
    held(name + " dw deferred", dw, dw0.double() + ref, tol_acc)
    assert not bool(scr.any()), f"{name}: the packed scratch is not all zero after pulpo_grad_finish_multi"


# ================================================================================================ the BatchNorm data of e and f
class BnData:
    """One ConvUnit's BatchNorm operands for a (B, C, *size) volume, all bf16-representable, exact lanes in channels 0 and 1:
    y ~ N(0.3, 1.5^2), dz ~ N(m_c, 1), a pooled gradient gpool ~ N(0, 1); a coefficient block built in float64 from y's own statistics
    (lanes 0 / 1: mean 0, scale 1 / 0.5, shift -1 / 0: y scale + shift is exact, takes both signs and, on lane 0, the value 0) and the
    float64 references of every pass formed from the block's own fp32 entries, as the kernels read them"""

    def __init__(self, g, B, C, size):
        self.B, self.C, self.size, self.npix = B, C, size, B * size[0] * size[1] * size[2]
        self.y = act(g, B, C, size, 0.3, 1.5)
        self.dz = rnd(torch.randn(B, C, *size, device=DEV, generator=g) + _chan(torch.randn(C, device=DEV, generator=g)))
        self.dz[:, 0], self.dz[:, 1] = exact_lanes(g, (B, *size))
        psize = tuple((n + 1) // 2 for n in size)
        self.gpool = act(g, B, C, psize)
        y64 = self.y.double()
        mean = y64.mean(dim=(0, 2, 3, 4))
        rstd = (y64.var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5).rsqrt()
        gamma = torch.rand(C, device=DEV, generator=g).double() + 0.5
        beta = torch.randn(C, device=DEV, generator=g).double() * 0.3
        mean[:2], rstd[0], rstd[1], gamma[0], gamma[1], beta[0], beta[1] = 0.0, 1.0, 2.0, 1.0, 0.25, -1.0, 0.0
        self.coef = coef_block(mean, rstd, gamma, beta)
        c32 = self.coef[:4 * C].reshape(4, C).double()
        self.m32, self.scale, self.shift = c32[0], c32[2], c32[3]
        self.mean, self.rstd = mean, rstd                                # (the block's doubles)
        assert float(self.scale[0]) == 1.0 and float(self.scale[1]) == 0.5 and float(self.shift[0]) == -1.0 and float(self.shift[1]) == 0.0
        self.lanes = lane_mask(y64)
        # ---- forward
        self.bn = y64 * _chan(self.scale) + _chan(self.shift)
        self.z = torch.where(self.bn > 0, self.bn, SLOPE32 * self.bn)
        # T = 4 u (|y scale| + |shift|) (product, sum, slope); exact lanes: nothing but the slope's product on the negative branch
        self.t_z = torch.where(self.lanes, (self.bn < 0) * U * self.z.abs(), 4 * U * ((y64 * _chan(self.scale)).abs() + _chan(self.shift).abs()))
        assert bool((self.bn[:, 0] == 0).any()) and all(bool((self.bn[:, k] > 0).any()) and bool((self.bn[:, k] < 0).any()) for k in (0, 1))
        # ---- the LeakyReLU kink: where |bn| is below its own fp32 bound (and not exactly 0) the fp32 branch may differ
        t_bn = 2 * U * ((y64 * _chan(self.scale)).abs() + _chan(self.shift).abs())
        self.near = (self.bn.abs() <= t_bn) & (self.bn != 0) & ~self.lanes
        self.yc = y64 - _chan(self.m32)

    def dz_pooled(self, add):
        """(reference, T, slack) of dz = (add +) avgpool2_bwd(gpool) as a bf16 tensor the kernels form per element and round: the product with
        1 / count is exact, the sum rounds once (T = 0 without `add` and wherever the sum is exact, pair_sum_exact); slack: one ulp where the rounding of the
        stored value is not decided by rule 2 - what a sum over the stored gradient may differ by"""
        p = self.y.double().requires_grad_(True)
        up, = torch.autograd.grad((R.avgpool2_ref(p) * self.gpool.double()).sum(), [p])
        if add is None:
            return R.rne_bf16(up), up, torch.zeros_like(up), torch.zeros_like(up)
        r = add.double() + up
        T = torch.where(pair_sum_exact(add.double(), up), torch.zeros_like(r), 2 * U * (add.double().abs() + up.abs()))
        assert bool(pair_sum_exact(add.double(), up)[:, :2].all())
        covered = (R.bf16_midpoint_distance(r) > T) | (T == 0)
        return R.rne_bf16(r), r, T, (~covered) * ulp_of(r)

    def backward(self, dz64, slack=None):
        """float64 reference of both backward passes for the gradient dz64 (a stored tensor, decoded): dbn, the two sums, totd as
        pulpo_bn_bwd_finalize would hand it on (lanes 0 / 1: 0.5 and 0.25, so that the second pass stays exact there), dy and the bounds"""
        s = type("bw", (), {})()
        slack = torch.zeros_like(dz64) if slack is None else slack
        s.dbn = torch.where(self.bn > 0, dz64, SLOPE32 * dz64)
        s.flip = 0.8 * dz64.abs() * self.near + slack
        s.sum_dbn, s.sum_dbn_c = _csum(s.dbn), _csum(s.dbn * self.yc)
        c1 = s.sum_dbn / self.npix
        c2 = self.rstd * (s.sum_dbn_c - (self.mean - self.m32) * s.sum_dbn) / self.npix
        c1[:2], c2[0], c2[1] = 0.5, 0.25, 0.25
        s.totd = torch.cat([c1, c2]).contiguous()
        sc, rs = _chan(self.scale), _chan(self.rstd)
        ycm = self.y.double() - _chan(self.mean)
        s.dy = sc * (s.dbn - _chan(c1) - ycm * rs * _chan(c2))
        a_dy = sc.abs() * (s.dbn.abs() + _chan(c1.abs()) + ycm.abs() * rs * _chan(c2.abs()))
        # 8 u of the terms (as the fp32 chain's test) + the kink; exact lanes: scale, B = -scale c2 rstd and C = -scale c1 are powers of two
        # and every term a small multiple of 2^-10: nothing rounds on the positive branch; on the other one the slope's product does, and
        # the two sums behind it: 4 u of the terms
        s.t_dy = torch.where(self.lanes, (self.bn <= 0) * 4 * U * a_dy, 8 * U * a_dy) + sc.abs() * s.flip
        return s


def bn_case(g, B, C, size, width=None, off=0):
    d = BnData(g, B, C, size)
    d.width, d.off = width, off
    d.yb, d.dzb, d.gpb = as_bf(d.y, width, off), as_bf(d.dz, width, off), as_bf(d.gpool, width, off)
    d.yf, d.dzf = d.y.contiguous(memory_format=CL), d.dz.contiguous(memory_format=CL)
    return d


def out_bf(d, pooled=False):
    size = tuple((n + 1) // 2 for n in d.size) if pooled else d.size
    return bf_buffer(d.B, size, d.C, d.width, d.off)


def out_f32(d):
    return torch.full((d.B, *d.size, d.C), NAN, device=DEV).permute(0, 4, 1, 2, 3)


def check_rows(name, part, nblk, d, bw, mblk):
    prow = part.reshape(nblk, 2, d.C)
    assert bool(torch.isfinite(prow).all()), f"{name}: {int((~torch.isfinite(prow)).sum())} row entries were not written"
    got = prow.double().sum(0)
    held(name + " rows sum dbn", got[0], bw.sum_dbn, mblk * U * _csum(bw.dbn.abs()) + _csum(bw.flip) + 1e-30)
    held(name + " rows sum dbn (y - m32)", got[1], bw.sum_dbn_c, mblk * U * _csum((bw.dbn * d.yc).abs()) + _csum(bw.flip * d.yc.abs()) + 1e-30)


def check_bias_rows(name, part2, nblk, C, dy_stored, mblk):
    """the conv-bias gradient partials are the column sums of dy AS STORED (decoded), as in the fp32 chain's test"""
    p2 = part2.reshape(nblk, C)
    assert bool(torch.isfinite(p2).all()), f"{name}: {int((~torch.isfinite(p2)).sum())} bias-gradient row entries were not written"
    sdy, ady = _csum(dy_stored.double()), _csum(dy_stored.double().abs())
    t_b = mblk * U * ady
    held(name + " bias rows", p2.double().sum(0), sdy, t_b, power=None)
    assert float(t_b[-1]) < 1e-3 * float(ady[-1])


# ================================================================================================ e. input-layer weight gradient + BatchNorm backward
@pytest.mark.parametrize("B,Cin,size", [(1, 3, (12, 8, 16)), (1, 2, (9, 7, 10))], ids=lambda v: str(v).replace(" ", ""))
def test_wgrad_bn_with_bf16_dz_vs_float64(ops, B, Cin, size):
    """e: pulpo_conv3d_k3_wgrad_bn with dz_dt = 1 (y fp32): dy = batch_norm_backward(leaky_relu_backward(dz)) is formed per element in fp32
    and never stored.  dw against the float64 weight gradient of the float64 dy: the direct kernel's bound plus dy's own bound carried
    through the sum, sum |x| T_dy; the bias-gradient rows against sum dy"""
    lib, st = _lib(), ops._stream()
    C = 32
    g = gen(Cin * 100 + size[0])
    d = bn_case(g, B, C, size)
    bw = d.backward(d.dz.double())
    x = torch.randn(B, Cin, *size, device=DEV, generator=g)
    dw = torch.full((C, Cin, 3, 3, 3), NAN, device=DEV)
    wscr = torch.full((lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", Cin, C),), NAN, device=DEV)
    nrow = lib.query("pulpo_conv3d_k3_wgrad_bn_rows", B, *size, C)
    prt = torch.full((nrow * C,), NAN, device=DEV)
    lib.call("pulpo_conv3d_k3_wgrad_bn", vp(x), *ops.grid_strides(x), vp(d.dzb), 1, d.dzb.stride(0), d.dzb.stride(4), vp(d.yf), d.yf.stride(0), d.yf.stride(4),
             vp(d.coef), vp(bw.totd), SLOPE, vp(dw), 0, vp(wscr), vp(prt), B, *size, Cin, C, st)
    name = f"bf16-dz wgrad_bn B{B} {Cin}to{C} {size}"
    wref = R.conv3_wgrad_ref(x.double(), bw.dy)
    t_w = bound(name, R.conv3_wgrad_ref(x, bw.dy.float()), wref, R.conv3_wgrad_mag(x.double(), bw.dy), M_WGRAD[0]) + R.conv3_wgrad_ref(x.double().abs(), bw.t_dy)
    held(name + " dw", dw, wref, t_w)
    p2 = prt.reshape(nrow, C)
    assert bool(torch.isfinite(p2).all()), f"{name}: {int((~torch.isfinite(p2)).sum())} bias-gradient row entries were not written"
    t_b = ((d.npix + nrow - 1) // nrow + 2) * U * _csum(bw.dy.abs()) + _csum(bw.t_dy)
    held(name + " bias rows", p2.double().sum(0), _csum(bw.dy), t_b, power=None)
    assert float(t_b[-1]) < 1e-3 * float(_csum(bw.dy.abs())[-1])


# ================================================================================================ f. the BatchNorm chain, typed
# (B, size, C, buffer width, channel offset): groups of 8 (C = 40), of 4 (C = 12), scalar (C = 6), and C = 40 as a channel slice 4 channels
# into a 48-channel bf16 buffer - 8-byte but not 16-byte aligned, so GroupProbe falls to groups of 4.  B = 2, 5x7x9: odd in every axis (pooled
# edge windows of 4, 2 and 1 voxels); 6x7x5: config 5's coarsest level
BN_T_CASES = [(B, size, C, w, o) for B, size in [(2, (5, 7, 9)), (1, (6, 7, 5))] for C, w, o in [(40, None, 0), (12, None, 0), (6, None, 0), (40, 48, 4)]]


def _bid(c):
    return f"B{c[0]}-{'x'.join(map(str, c[1]))}-C{c[2]}" + (f"-slice{c[4]}of{c[3]}" if c[3] else "")


@pytest.mark.parametrize("case", BN_T_CASES, ids=_bid)
def test_bn_apply_typed_vs_float64(ops, case):
    """f: pulpo_bn_lrelu_apply_t for (y, z) dtypes (0, 1), (1, 1), (1, 0) and pulpo_bn_lrelu_apply_pool2_t for (0, 1), (1, 1), with and
    without z.  The pooled tensor averages z AS STORED: its reference is the average of RNE_bf16(z), rounded; where a window holds a z that
    rule 2 does not decide, the average may move by ulp(z) / count and the element is exempt"""
    B, size, C, width, off = case
    lib, st = _lib(), ops._stream()
    d = bn_case(gen(C * 3 + size[0] + B), B, C, size, width, off)
    name = f"bf16 bn apply {_bid(case)}"
    for ydt, zdt in ((0, 1), (1, 1), (1, 0)):
        y = d.yb if ydt else d.yf
        z, zbuf = out_bf(d) if zdt else (out_f32(d), None)
        lib.call("pulpo_bn_lrelu_apply_t", vp(y), ydt, y.stride(4), vp(z), zdt, z.stride(4), vp(d.coef), d.npix, C, SLOPE, st)
        if zdt:
            R.held_bf16(f"{name} z({ydt},{zdt})", z, d.z, d.t_z, CAP_ELT)
            assert width is None or untouched(zbuf, C, off)
        else:
            held(f"{name} z({ydt},{zdt})", z, d.z, d.t_z + 1e-30)
            assert bool((z[:, 0].double() == d.z[:, 0])[d.bn[:, 0] >= 0].all())
    if not lib.query("pulpo_bn_lrelu_apply_pool2_ok", C, d.yb.stride(4), d.yb.stride(4), d.yb.stride(4)):
        assert C % 4 != 0
        return
    zs = R.rne_bf16(d.z)
    z_loose = ~((R.bf16_midpoint_distance(d.z) > d.t_z) | (d.t_z == 0))
    pref = R.avgpool2_ref(zs)
    # the sum of <= 8 stored values and the product with 1 / count: 8 u of the average of |z| - and nothing where the sum is exact in any
    # order (pool_sum_exact: the exact lanes, and most other windows as well)
    t_p = torch.where(pool_sum_exact(zs), torch.zeros_like(pref), 8 * U * R.avgpool2_ref(zs.abs()))
    assert bool(pool_sum_exact(zs)[:, :2].all())
    p_loose = R.avgpool2_ref(z_loose.double()) > 0
    t_p = t_p + p_loose * R.avgpool2_ref(z_loose * ulp_of(zs))
    for ydt, with_z in ((0, True), (1, True), (1, False)):
        y = d.yb if ydt else d.yf
        z, zbuf = out_bf(d)
        pooled, pbuf = out_bf(d, pooled=True)
        lib.call("pulpo_bn_lrelu_apply_pool2_t", vp(y), ydt, y.stride(4), vp(z) if with_z else None, 1, z.stride(4), vp(pooled), pooled.stride(4), vp(d.coef),
                 B, *size, C, SLOPE, st)
        tag = f"{name} pool2({ydt},1{'' if with_z else ',z=NULL'})"
        if with_z:
            R.held_bf16(tag + " z", z, d.z, d.t_z, CAP_ELT)
        else:
            assert bool(torch.isnan(zbuf).all() if width is None else torch.isnan(z).all()), f"{tag}: z was written"
        R.held_bf16(tag + " pooled", pooled, pref, t_p, CAP_ELT, exempt=p_loose)
        assert width is None or (untouched(zbuf, C, off) and untouched(pbuf, C, off))


@pytest.mark.parametrize("case", BN_T_CASES, ids=_bid)
def test_bn_backward_typed_vs_float64(ops, case):
    """f: both backward passes on a bf16 gradient - pulpo_bn_lrelu_bwd_reduce_t / _bwd_apply_t for (dz, y) dtypes (1, 1), (1, 0), the pooled
    forms pulpo_avgpool2_bwd_bnred_t / pulpo_bn_lrelu_bwd_apply_pooled_t with g_dt = 1, y_dt 1 / 0, with and without the skip gradient `add`,
    and for C = 40 the channel-blocked second passes _kb_t / _pooled_kb_t (bf16 gradient in, fp32 dy out).  Partial rows by the fp32 chain's row
    bounds against sums over the decoded stored operands; stored outputs by held_bf16"""
    B, size, C, width, off = case
    lib, st = _lib(), ops._stream()
    g = gen(C * 5 + size[1] + B)
    d = bn_case(g, B, C, size, width, off)
    name = f"bf16 bn backward {_bid(case)}"
    nblk = lib.query("pulpo_bn_bwd_blocks", d.npix, C)
    mblk = (d.npix + nblk - 1) // nblk + 2
    kb = C % 8 == 0 and width is None

    def blocked_dy():
        t = torch.full((C // 8, B, *size, 8), NAN, device=DEV)
        return t, (8, d.npix * 8)

    # ---- plain: dz a stored tensor
    bw = d.backward(d.dz.double())
    for ydt in (1, 0):
        y = d.yb if ydt else d.yf
        tag = f"{name} plain(1,{ydt})"
        part = torch.full((nblk * 2 * C,), NAN, device=DEV)
        lib.call("pulpo_bn_lrelu_bwd_reduce_t", vp(d.dzb), 1, d.dzb.stride(4), vp(y), ydt, y.stride(4), vp(d.coef), d.npix, C, SLOPE, vp(part), st)
        check_rows(tag, part, nblk, d, bw, mblk)
        dy, dbuf = out_bf(d) if ydt else (out_f32(d), None)
        part2 = torch.full((nblk * C,), NAN, device=DEV)
        lib.call("pulpo_bn_lrelu_bwd_apply_t", vp(d.dzb), 1, d.dzb.stride(4), vp(y), ydt, y.stride(4), vp(d.coef), vp(bw.totd), vp(dy), dy.stride(4), d.npix, C,
                 SLOPE, vp(part2), st)
        if ydt:
            R.held_bf16(tag + " dy", dy, bw.dy, bw.t_dy, CAP_ELT)
            assert width is None or untouched(dbuf, C, off)
        else:
            held(tag + " dy", dy, bw.dy, bw.t_dy + 1e-30)
        check_bias_rows(tag, part2, nblk, C, dy, mblk)
    if kb:
        dyk, dys = blocked_dy()
        part2 = torch.full((nblk * C,), NAN, device=DEV)
        lib.call("pulpo_bn_lrelu_bwd_apply_kb_t", vp(d.dzb), 1, d.dzb.stride(4), 8, vp(d.yf), d.yf.stride(4), vp(d.coef), vp(bw.totd), vp(dyk), *dys, d.npix, C,
                 SLOPE, vp(part2), st)
        dyt = ops.blocked_to_cl(dyk)
        held(f"{name} plain kb dy", dyt, bw.dy, bw.t_dy + 1e-30)
        check_bias_rows(f"{name} plain kb", part2, nblk, C, dyt, mblk)
    if C % 4 != 0:
        return                                                     # (the pooled forms take groups of four channels only)
    # ---- pooled: dz = (add +) avgpool2_bwd(gpool), formed per element, rounded to bf16 and - first pass, gin given - stored
    for with_add in (True, False):
        add = d.dzb if with_add else None
        dzs, dz_ref, t_dzp, slack = d.dz_pooled(d.dz if with_add else None)
        bw = d.backward(dzs, slack)
        for ydt in (1, 0):
            y = d.yb if ydt else d.yf
            tag = f"{name} pooled(1,{ydt}{',add' if with_add else ''})"
            for with_gin in (True, False):
                gin, gbuf = out_bf(d)
                part = torch.full((nblk * 2 * C,), NAN, device=DEV)
                lib.call("pulpo_avgpool2_bwd_bnred_t", vp(d.gpb), d.gpb.stride(4), vp(add), add.stride(4) if with_add else 0, vp(gin) if with_gin else None,
                         gin.stride(4), 1, vp(y), ydt, y.stride(4), vp(d.coef), SLOPE, vp(part), B, *size, C, st)
                if with_gin:
                    R.held_bf16(tag + " gin", gin, dz_ref, t_dzp, CAP_ELT)
                    assert width is None or untouched(gbuf, C, off)
                check_rows(tag + ("" if with_gin else " gin=NULL"), part, nblk, d, bw, mblk)
            dy, dbuf = out_bf(d) if ydt else (out_f32(d), None)
            part2 = torch.full((nblk * C,), NAN, device=DEV)
            lib.call("pulpo_bn_lrelu_bwd_apply_pooled_t", vp(d.gpb), d.gpb.stride(4), vp(add), add.stride(4) if with_add else 0, 1, vp(y), ydt, y.stride(4),
                     vp(d.coef), vp(bw.totd), vp(dy), dy.stride(4), SLOPE, vp(part2), B, *size, C, st)
            if ydt:
                R.held_bf16(tag + " dy", dy, bw.dy, bw.t_dy, CAP_ELT, exempt=slack > 0)
                assert width is None or untouched(dbuf, C, off)
            else:
                held(tag + " dy", dy, bw.dy, bw.t_dy + 1e-30)
            check_bias_rows(tag, part2, nblk, C, dy, mblk)
        if kb:
            dyk, dys = blocked_dy()
            part2 = torch.full((nblk * C,), NAN, device=DEV)
            lib.call("pulpo_bn_lrelu_bwd_apply_pooled_kb_t", vp(d.gpb), d.gpb.stride(4), vp(add), add.stride(4) if with_add else 0, 1, vp(d.yf), d.yf.stride(4),
                     vp(d.coef), vp(bw.totd), vp(dyk), *dys, SLOPE, vp(part2), B, *size, C, st)
            dyt = ops.blocked_to_cl(dyk)
            held(f"{name} pooled kb{' add' if with_add else ''} dy", dyt, bw.dy, bw.t_dy + 1e-30)
            check_bias_rows(f"{name} pooled kb{' add' if with_add else ''}", part2, nblk, C, dyt, mblk)


def test_bn_typed_misaligned_slice(ops):
    """f: a slice that starts ONE channel into a wider bf16 buffer, C % 4 == 0: 2-byte aligned.  The backward entries refuse it with the
    documented error and write nowhere; pulpo_bn_lrelu_apply_t computes it on its scalar path"""
    B, size, C, width, off = 2, (5, 7, 9), 12, 16, 1
    lib, st = _lib(), ops._stream()
    d = bn_case(gen(1234), B, C, size, width, off)
    assert d.yb.data_ptr() % 4 == 2
    z, zbuf = out_bf(d)
    lib.call("pulpo_bn_lrelu_apply_t", vp(d.yb), 1, d.yb.stride(4), vp(z), 1, z.stride(4), vp(d.coef), d.npix, C, SLOPE, st)
    R.held_bf16("bf16 bn apply misaligned z", z, d.z, d.t_z, CAP_ELT)
    assert untouched(zbuf, C, off)
    bw = d.backward(d.dz.double())
    nblk = lib.query("pulpo_bn_bwd_blocks", d.npix, C)
    part = torch.full((nblk * 2 * C,), NAN, device=DEV)
    with pytest.raises(PulpoHipError, match="bn_lrelu_bwd_reduce: operands must be aligned to four elements when C % 4 == 0"):
        lib.call("pulpo_bn_lrelu_bwd_reduce_t", vp(d.dzb), 1, d.dzb.stride(4), vp(d.yb), 1, d.yb.stride(4), vp(d.coef), d.npix, C, SLOPE, vp(part), st)
    dy, dbuf = out_bf(d)
    part2 = torch.full((nblk * C,), NAN, device=DEV)
    with pytest.raises(PulpoHipError, match="bn_lrelu_bwd_apply: operands must be aligned to four elements when C % 4 == 0"):
        lib.call("pulpo_bn_lrelu_bwd_apply_t", vp(d.dzb), 1, d.dzb.stride(4), vp(d.yb), 1, d.yb.stride(4), vp(d.coef), vp(bw.totd), vp(dy), dy.stride(4), d.npix, C,
                 SLOPE, vp(part2), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(part2).all()) and bool(torch.isnan(dy).all()) and untouched(dbuf, C, off)


# ================================================================================================ g. pooling and up-2, typed
@pytest.mark.parametrize("B,C,size", [(2, 16, (5, 7, 9)), (1, 6, (7, 5, 3))], ids=lambda v: str(v).replace(" ", ""))
def test_avgpool2_typed_vs_float64(ops, B, C, size):
    """g: pulpo_avgpool2_fwd_t / _bwd_t with dt = 1, the backward with and without `add`.  Forward: 7 additions and the product with
    1 / count, m = 8; backward: g / count is exact, the sum with `add` rounds once (m = 2), and without `add` nothing rounds at all: T = 0,
    every element bit-identical.  Sums of bf16 values are exact in fp32 wherever their exponents lie within 13 binades of each other
    (pool_sum_exact, pair_sum_exact): T = 0 there too, which is what puts the ~13 % of averages that are exact ties under rule 2.
    Divisors 8, 4, 2 and 1 (the all-odd volume's far corner)"""
    lib, st = _lib(), ops._stream()
    g = gen(C + size[0] + B)
    x = act(g, B, C, size)
    xb = as_bf(x)
    name = f"bf16 pool B{B} C{C} {size}"
    x64 = x.double()
    ref = R.avgpool2_ref(x64)
    T = bound(name + " out", R.avgpool2_ref(x), ref, R.avgpool2_ref(x64.abs()), 8.0) * ~pool_sum_exact(x64)
    assert bool(pool_sum_exact(x64)[:, :2].all())
    psize = tuple(ref.shape[2:])
    out, _ = bf_buffer(B, psize, C)
    lib.call("pulpo_avgpool2_fwd_t", vp(xb), xb.stride(4), vp(out), out.stride(4), 1, B, *size, C, st)
    R.held_bf16(name + " out", out, ref, T, CAP_ELT)
    ties = R.bf16_midpoint_distance(ref[:, :2]) == 0
    print(f"TIES {name} {float(ties.double().mean()):.3g}")
    assert bool(ties.any())                                         # (the exact lanes do put RNE's tie rule to the test)
    up = act(g, B, C, psize)
    upb = as_bf(up)
    p = x64.clone().requires_grad_(True)
    rg, = torch.autograd.grad((R.avgpool2_ref(p) * up.double()).sum(), [p])
    skip = act(g, B, C, size)
    skb = as_bf(skip)
    for add in (None, skb):
        gin, _ = bf_buffer(B, size, C)
        lib.call("pulpo_avgpool2_bwd_t", vp(upb), upb.stride(4), vp(add), add.stride(4) if add is not None else 0, vp(gin), gin.stride(4), 1, B, *size, C, st)
        if add is None:
            R.held_bf16(name + " gin", gin, rg, 0.0, CAP_ELT)
        else:
            r = rg + skip.double()
            exact = pair_sum_exact(rg, skip.double())
            assert bool(exact[:, :2].all())
            R.held_bf16(name + " gin+add", gin, r, 2 * U * (rg.abs() + skip.double().abs()) * ~exact, CAP_ELT)


@pytest.mark.parametrize("B,size,need", [(1, (3, 4, 3), (1, 0, 1, 1, 0, 1)), (2, (6, 7, 5), (1, 1, 0, 1, 1, 1))], ids=lambda v: str(v).replace(" ", ""))
def test_feedback_up2_typed_vs_float64(ops, B, size, need):
    """g: pulpo_feedback_up2_fwd_t / _bwd_t with dt = 1: planar fp32 sources (the first one small integers: weights are products of 1/4 and
    3/4, every product and sum exact, T = 0 on its channels) up-sampled and concatenated into a bf16 tensor; the backward gathers a bf16
    gradient into planar fp32 source gradients, NULL entries for the sources that ask for none (held(), m = 64)"""
    lib, st = _lib(), ops._stream()
    chans = [3, 3, 3, 3, 3, 1]
    g = gen(size[0] + size[2] + B)
    srcs = [torch.randn(B, c, *size, device=DEV, generator=g) for c in chans]
    srcs[0] = torch.randint(-8, 9, (B, 3, *size), device=DEV, generator=g).float()
    name = f"bf16 up2 B{B} {size}"
    s64 = [s.double().requires_grad_(bool(n)) for s, n in zip(srcs, need)]
    ref = R.up2_cat_ref(s64)
    refa = R.up2_cat_ref([s.double().abs() for s in srcs])
    T = bound(name + " out", R.up2_cat_ref(srcs), ref.detach(), refa, 8.0)
    T[:, :3] = 0.0
    n = len(srcs)
    osize = tuple(2 * k for k in size)
    out, _ = bf_buffer(B, osize, 16)
    ch = (ctypes.c_int * n)(*chans)
    lib.call("pulpo_feedback_up2_fwd_t", (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs]), ch, n, vp(out), 1, out.stride(4), B, *size, st)
    R.held_bf16(name + " out", out, ref.detach(), T, CAP_ELT)
    up = rnd(torch.randn(B, 16, *osize, device=DEV, generator=g))
    upb = as_bf(up)
    want = [s for s, k in zip(s64, need) if k]
    rg = torch.autograd.grad((ref * up.double()).sum(), want)
    sa = [s.double().abs().requires_grad_(bool(k)) for s, k in zip(srcs, need)]
    ag = torch.autograd.grad((R.up2_cat_ref(sa) * up.double().abs()).sum(), [s for s, k in zip(sa, need) if k])
    s32 = [s.clone().requires_grad_(bool(k)) for s, k in zip(srcs, need)]
    g32 = torch.autograd.grad((R.up2_cat_ref(s32) * up).sum(), [s for s, k in zip(s32, need) if k])
    gs = [torch.full((B, c, *size), NAN, device=DEV) if k else None for c, k in zip(chans, need)]
    lib.call("pulpo_feedback_up2_bwd_t", vp(upb), 1, upb.stride(4), (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in gs]), ch, n, B, *size, st)
    for k, (a, r, r32, A) in enumerate(zip([t for t in gs if t is not None], rg, g32, ag)):
        held(f"{name} gsrc{k}", a, r, bound(f"{name} gsrc{k}", r32, r, A, 64.0))


# ================================================================================================ h. routing
def test_conv_unit_routes_to_the_bf16_storage_entries(ops):
    """h: one ConvUnit 32 -> 32 @40^3, pool_after, forward and backward under set_conv_precision("bf16", activations="bf16"): the entry points
    of a, c, d and f are the ones called, with dtype code 1 for every activation operand"""
    import src.network_blocks as nb
    from launch_log import LaunchLog
    size, C = (40, 40, 40), 32
    torch.manual_seed(11)
    unit = nb.ConvUnit(list(size), C, C).cuda().train()
    g = gen(5)
    x = rnd(torch.randn(1, C, *size, device=DEV, generator=g)).bfloat16().contiguous(memory_format=CL).requires_grad_(True)
    ops.set_conv_precision("bf16", activations="bf16")
    try:
        with LaunchLog() as log:
            z = unit(x, pool_after=True)
            skip, pooled = ops.avg_pool2_skip(z)                    # (as DownPath does: the activation is pooled AND handed on as a skip connection)
            assert skip.dtype == BF and pooled.dtype == BF
            ups = [rnd(torch.randn(t.shape, device=DEV, generator=g)).bfloat16().contiguous(memory_format=CL) for t in (skip, pooled)]
            torch.autograd.grad([skip, pooled], [x] + list(unit.parameters()), grad_outputs=ups)
            torch.cuda.synchronize()
    finally:
        ops.set_conv_precision("fp32")
    calls = [line.split() for line in log.lines]
    print("\n".join(log.lines))

    def args_of(entry):
        hit = [c[1:] for c in calls if c[0] == entry]
        assert hit, f"{entry} was not called: {sorted({c[0] for c in calls})}"
        return hit

    convs = args_of("pulpo_conv3d_k3_fwd_bf16_t")
    assert len(convs) == 2 and all(a[10] == "1" for a in convs)                                    # forward and data gradient, dt = 1
    assert fwd_kernel(1, size, C, C) == FWD_KERNEL["pw19"]
    wg = args_of("pulpo_conv3d_k3_wgrad_bf16_det_t" if det_default() else "pulpo_conv3d_k3_wgrad_bf16_t")
    assert all(a[8] == "1" for a in wg)
    assert all(a[1] == "1" and a[4] == "1" for a in args_of("pulpo_bn_lrelu_apply_pool2_t"))       # y_dt, z_dt
    assert all(a[6] == "1" and a[8] == "1" for a in args_of("pulpo_avgpool2_bwd_bnred_t"))         # g_dt, y_dt
    assert all(a[4] == "1" and a[6] == "1" for a in args_of("pulpo_bn_lrelu_bwd_apply_pooled_t"))  # g_dt, y_dt
    assert not any(c[0] in ("pulpo_conv3d_k3_fwd_bf16", "pulpo_conv3d_k3_wgrad_bf16", "pulpo_bn_lrelu_apply", "pulpo_bn_lrelu_bwd_apply") for c in calls)
