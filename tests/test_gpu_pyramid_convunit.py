"""The ConvUnit kernels - the 3x3x3 convolution families with their data and weight gradients, the statistics rows their stores write, the
BatchNorm / LeakyReLU chain, pooling and the x2 up-sampling - against float64 references (tests/pyramid_ref.py, evaluated with plain torch
ops on the GPU) at the layer shapes of the training step: config 3's 160^3 pyramid, config 2's 96^3 pyramid at B = 2 and config 5's ragged
levels (96x112x80 ... 6x7x5).

Every tensor is compared element by element and every comparison is shown to have power: the same bound must reject the reference with its
LAST element moved by 1e-3 max|ref| - the far border planes, the last voxel tile of the last batch element and the last real channel of a
partly empty output-channel tile at once.

Bounds.  A convolution output is a sum of products; any fp32 evaluation of it errs by at most (number of roundings) * 2^-24 * A per element,
A = sum |a_i| |b_i| the magnitude sum (pyramid_ref.conv3_mag).  The bound is the tensor T = m * max(1, rho32) * 2^-24 * A:
  * rho32 is the largest |err| / (2^-24 A) of the SAME plain-ops reference evaluated in fp32 on the same data (never of the code under test);
  * m is the worst-case growth of the magnitude sums under the Winograd transforms, (|B^T|_inf |G|_inf)^d = 3^d - 9 for F(2x2,3x3) in (y, x),
    27 for F(2x2x2,3x3x3) - doubled once for the output transform and the bias: 18 and 54.
  * the direct kernels (fp32 and bf16 operands, with and without split-K) have no transform, and m = 2 would hold them to twice the error
    of the plain-ops reference, whose 27 short per-tap matmuls are summed in another order.  They keep ONE fp32 accumulator per output
    through all 27 K products (MFMA steps chained through the taps and channel chunks; split-K adds the slabs' ordered sum).  Each update
    rounds the running sum s_k by at most u |s_k|, independently and without bias: the error's variance is u^2 sum s_k^2 / 3, and for
    zero-mean terms t (s_k^2 ~ k rms(t)^2) that is u^2 n^2 rms(t)^2 / 6 - against A = n E|t| an rms error of rms(t) / (sqrt(6) E|t|) u A =
    0.64 u A for products of two normal variates (E|t| = 2 / pi), whatever n.  The largest of N = 1.3e8 such errors (32 x 160^3) lies at
    sqrt(2 ln N) = 6.1 standard deviations: 3.9 u A.  Doubled once like the others for the bias and the slabs: m = 8.  This is reasoning
    about the accumulation order, not a fit: round 6 measured at most 3.3 u A (16 -> 96 @12x14x10) with the worst elements scattered over
    interior voxels and channels, no tile, border or channel-tile pattern.
Weight gradients over 4e6 voxels and more (160^3): A is ~300 max|dw| there and T would no longer reject the perturbation, so A is replaced
by the random-walk magnitude R = sqrt(sum x^2 dy^2) and the margin is 4 * the fp32 plain-ops reference's own max |err| / (2^-24 R).
BatchNorm, pooling and up-sampling use the same construction with A the sum of the absolute values of the terms the formula adds."""
import ctypes

import pytest
import torch

import pyramid_ref as R
from test_gpu_pyramid_ops import amax, check, det_default, gen

pytestmark = pytest.mark.gpu

CL = torch.channels_last_3d
DEV = "cuda"
U = 2.0 ** -24
M_FWD = {"d": 8.0, "y": 18.0, "z": 54.0, "b": 8.0}     # direct, F(2x2,3x3), F(2x2x2,3x3x3), bf16 operands (direct): module docstring
M_WGRAD = {0: 2.0, 2: 18.0, 3: 54.0}                     # (the direct weight gradient keeps the issue's m = 2)
RANDOM_WALK_VOXELS = 4_000_000                            # weight gradients summed over this many voxels and more use R (module docstring)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    assert torch.backends.cuda.matmul.allow_tf32 is False          # rho32 measures a true fp32 evaluation
    return _ops


def _lib():
    from pulpo_amd._lib import lib
    return lib


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def worst(name, got, ref, tol):
    """where the largest |got - ref| / tol sits (printed before a comparison asserts): flat index -> the tensor's own coordinates"""
    r = (got.detach().to(ref.dtype) - ref.detach()).abs() / tol
    i = int(torch.nan_to_num(r, nan=float("inf")).reshape(-1).argmax()) if r.numel() else 0
    idx = []
    for n in reversed(ref.shape):
        idx.append(i % n)
        i //= n
    print(f"WORST {name} index {tuple(reversed(idx))} of {tuple(ref.shape)}")


def held(name, got, ref, tol, power=-1):
    if R.ratio(got, ref, tol) > 1.0:
        worst(name, got, ref, tol if isinstance(tol, torch.Tensor) else torch.full_like(ref, float(tol)))
    check(name, got, ref, tol, power)


def bound(name, ref32, ref64, A, m):
    """T = m max(1, rho32) 2^-24 A"""
    A = A.clamp_min(1e-200)                         # (an operand that is exactly 0 - one normal variate in ~1e8 is - gives 0 / 0 otherwise)
    rho = R.ratio(ref32, ref64, U * A)
    print(f"RHO32 {name} {rho:.3g}")
    return m * max(1.0, rho) * U * A


# ================================================================================================ a / b. convolution layers
# (B, Cin, Cout, size, forward family, data-gradient family, weight-gradient algo), as pulpo_conv3d_k3_algo / _wino2_pipelined / the scratch
# queries / pulpo_conv3d_k3_wgrad_algo answer for channels-last fp32 operands:  d direct, y F(2x2,3x3) in (y, x) - p pipelined, r round-2 -,
# z F(2x2x2,3x3x3); a trailing s = split-K (scratch query > 0)
def _s(a, b=None, c=None):
    return (a, a, a) if b is None else (a, b, c)


# config 3 (160^3, B = 1): the 15 layers of profiles/r5_conv_bench.txt and the input layers 2 -> 32 @160^3, 3 -> 32 @80^3
C3 = [
    (1, 2, 32, _s(160), "d", "yp", 0), (1, 32, 32, _s(160), "z", "z", 3), (1, 3, 32, _s(80), "d", "yp", 0), (1, 32, 64, _s(80), "z", "z", 3),
    (1, 64, 64, _s(80), "z", "z", 3), (1, 96, 96, _s(80), "z", "z", 3), (1, 160, 64, _s(80), "z", "z", 3), (1, 16, 96, _s(80), "z", "z", 3),
    (1, 32, 32, _s(80), "z", "z", 3), (1, 64, 128, _s(40), "z", "z", 3), (1, 128, 128, _s(40), "z", "z", 3), (1, 96, 96, _s(40), "z", "z", 3),
    (1, 224, 128, _s(40), "z", "z", 3), (1, 128, 192, _s(20), "yp", "yps", 3), (1, 192, 192, _s(20), "yps", "yps", 3),
    (1, 288, 192, _s(20), "yps", "yp", 3), (1, 192, 192, _s(10), "yps", "yps", 3),
]
# config 2 (96^3, B = 2): every distinct layer of its four levels
C2 = [
    (2, 2, 32, _s(96), "d", "yp", 0), (2, 32, 32, _s(96), "z", "z", 3),
    (2, 3, 32, _s(48), "d", "yp", 0), (2, 16, 96, _s(48), "z", "z", 3), (2, 32, 64, _s(48), "z", "z", 3), (2, 32, 32, _s(48), "z", "z", 3),
    (2, 64, 64, _s(48), "z", "z", 3), (2, 96, 96, _s(48), "z", "z", 3), (2, 160, 64, _s(48), "z", "z", 3),
    (2, 3, 32, _s(24), "d", "yp", 0), (2, 16, 96, _s(24), "z", "yp", 3), (2, 32, 32, _s(24), "yp", "yp", 3), (2, 64, 128, _s(24), "z", "yp", 3),
    (2, 96, 96, _s(24), "z", "z", 3), (2, 128, 128, _s(24), "z", "z", 3), (2, 224, 128, _s(24), "z", "z", 3),
    (2, 3, 32, _s(12), "d", "ds", 0), (2, 32, 32, _s(12), "ds", "ds", 3), (2, 128, 192, _s(12), "ds", "yps", 3), (2, 192, 192, _s(12), "yps", "yps", 3),
]
# config 5 (192x224x160): its five levels below full resolution, every distinct layer the model runs there
_L5 = [(96, 112, 80), (48, 56, 40), (24, 28, 20), (12, 14, 10), (6, 7, 5)]
C5 = [
    (1, 3, 32, _L5[0], "d", "yp", 0), (1, 16, 96, _L5[0], "z", "z", 3), (1, 32, 64, _L5[0], "z", "z", 3), (1, 32, 32, _L5[0], "z", "z", 3),
    (1, 64, 64, _L5[0], "z", "z", 3), (1, 96, 96, _L5[0], "z", "z", 3), (1, 160, 64, _L5[0], "z", "z", 3),
    (1, 3, 32, _L5[1], "d", "yp", 0), (1, 16, 96, _L5[1], "z", "z", 3), (1, 32, 32, _L5[1], "z", "z", 3), (1, 64, 128, _L5[1], "z", "z", 3),
    (1, 96, 96, _L5[1], "z", "z", 3), (1, 128, 128, _L5[1], "z", "z", 3), (1, 224, 128, _L5[1], "z", "z", 3),
    (1, 3, 32, _L5[2], "d", "yp", 0), (1, 16, 96, _L5[2], "yp", "yps", 3), (1, 32, 32, _L5[2], "yp", "yp", 3), (1, 96, 96, _L5[2], "yp", "yp", 3),
    (1, 128, 192, _L5[2], "yp", "yps", 3), (1, 192, 192, _L5[2], "yp", "yp", 3), (1, 288, 192, _L5[2], "yp", "yp", 3),
    (1, 3, 32, _L5[3], "d", "ds", 0), (1, 16, 96, _L5[3], "d", "yps", 3), (1, 32, 32, _L5[3], "ds", "ds", 3), (1, 96, 96, _L5[3], "yps", "yps", 3),
    (1, 192, 192, _L5[3], "yps", "yps", 3), (1, 288, 192, _L5[3], "yps", "yps", 3),
    (1, 3, 32, _L5[4], "d", "ds", 0), (1, 32, 32, _L5[4], "ds", "ds", 0), (1, 192, 192, _L5[4], "ds", "ds", 0),
]


def _cid(c):
    return f"B{c[0]}-{c[1]}to{c[2]}-{'x'.join(map(str, c[3]))}"


def family(B, size, K, N, in_ps=None):
    """the kernel family the default selection runs for a 16-byte-aligned channels-last fp32 operand of K channels with voxel stride in_ps"""
    lib = _lib()
    a = lib.query("pulpo_conv3d_k3_algo", B, *size, K, N)
    s = {0: "d", 2: "y", 3: "z"}[a]
    if a == 2:
        s += "p" if lib.query("pulpo_conv3d_k3_wino2_pipelined", *size, K, in_ps or K) else "r"
        if lib.query("pulpo_conv3d_k3_fwd_wino2_scratch_floats", B, *size, K, N) > 0:
            s += "s"
    elif a == 0 and lib.query("pulpo_conv3d_k3_fwd_scratch_floats", B, *size, K, N) > 0:
        s += "s"
    return s


def operand(t, form, g):
    """t's values as the operand the step would pass: cl - contiguous channels-last; planar; aligned / unaligned - a channel slice of a wider
    channels-last buffer (random elsewhere) at a 16-byte-aligned / an unaligned channel offset; ("ps", n) - a slice of a buffer n channels wide"""
    B, C, D, H, W = t.shape
    if form == "cl":
        return t.contiguous(memory_format=CL)
    if form == "planar":
        return t.contiguous()
    width, off = {"aligned": (C + 24, 8), "unaligned": (C + 11, 3)}[form] if isinstance(form, str) else (form[1], 16)
    buf = torch.empty(B, D, H, W, width, device=DEV)
    if width <= 1024:
        buf.normal_(generator=g)
    else:                                            # (a very wide buffer: only the channels next to the slice are filled)
        buf[..., :off + C + 16].normal_(generator=g)
    v = buf.permute(0, 4, 1, 2, 3)[:, off:off + C]
    v.copy_(t)
    assert v.stride(1) == 1 and v.stride(4) == width and (v.data_ptr() % 16 == 0) == (form != "unaligned")
    return v


def conv_data(g, B, Cin, Cout, size, bf16_values):
    x = torch.randn(B, Cin, *size, device=DEV, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, device=DEV, generator=g) / (27 * Cin) ** 0.5
    b = torch.randn(Cout, device=DEV, generator=g)
    dy = torch.randn(B, Cout, *size, device=DEV, generator=g)
    if bf16_values:                                  # bf16-representable fp32 values: the kernel's operand rounding is the identity
        x, w, dy = (t.bfloat16().float() for t in (x, w, dy))
    return x, w, b, dy


def run_conv_case(ops, name, B, Cin, Cout, size, fam_f, fam_d, walgo, form="cl", bf16=False, wgrad_forms=None):
    """forward and data gradient through ops.conv3d_k3, weight gradient through ops._wgrad_raw (atomic and deterministic), against float64"""
    g = gen(B * 1000 + Cin * 10 + Cout + size[0] + size[2])
    x, w, b, dy = conv_data(g, B, Cin, Cout, size, bf16)
    xo, dyo = operand(x, form, g), operand(dy, "cl" if form == "planar" else form, g)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    mf = M_FWD["b" if (bf16 and Cin > 4) else fam_f[0]]
    md = M_FWD["b" if bf16 else fam_d[0]]
    mw = M_WGRAD[0 if (bf16 and Cin > 4) else walgo]
    ops.set_conv_precision("bf16" if bf16 else "fp32")
    try:
        xg = xo.requires_grad_(True)
        out = ops.conv3d_k3(xg, w, b)
        gx, = torch.autograd.grad(out, [xg], grad_outputs=dyo)
        ref = R.conv3_ref(x64, w64, b64)
        held(f"{name} out", out, ref, bound(f"{name} out", R.conv3_ref(x, w, b), ref, R.conv3_mag(x64, w64, b64), mf))
        del out, ref
        ref = R.conv3_dgrad_ref(dy64, w64)
        held(f"{name} dx", gx, ref, bound(f"{name} dx", R.conv3_dgrad_ref(dy, w), ref, R.conv3_dgrad_mag(dy64, w64), md))
        del gx, ref
        ref = R.conv3_wgrad_ref(x64, dy64)
        r32 = R.conv3_wgrad_ref(x, dy)
        if B * size[0] * size[1] * size[2] >= RANDOM_WALK_VOXELS:
            Rw = R.conv3_wgrad_mag(x64, dy64, random_walk=True)
            rho = R.ratio(r32, ref, U * Rw)
            print(f"RHO32 {name} dw(random walk) {rho:.3g}")
            tol = 4.0 * rho * U * Rw
        else:
            tol = bound(f"{name} dw", r32, ref, R.conv3_wgrad_mag(x64, dy64), mw)
        for det in (False, True):
            ops.set_deterministic(det)
            held(f"{name} dw det={det}", ops._wgrad_raw(xo.detach(), dyo, Cin, Cout), ref, tol)
    finally:
        ops.set_deterministic(det_default())
        ops.set_conv_precision("fp32")


def assert_families(B, Cin, Cout, size, fam_f, fam_d, walgo, ps_x=None, ps_dy=None, vec=None):
    lib = _lib()
    assert family(B, size, Cin, Cout, ps_x) == fam_f, (family(B, size, Cin, Cout, ps_x), fam_f)
    assert family(B, size, Cout, Cin, ps_dy) == fam_d, (family(B, size, Cout, Cin, ps_dy), fam_d)
    vec = int(Cin % 4 == 0 and Cout % 4 == 0) if vec is None else vec
    assert lib.query("pulpo_conv3d_k3_wgrad_algo", B, *size, Cin, Cout, vec) == walgo


@pytest.mark.parametrize("case", C3 + C2 + C5, ids=_cid)
def test_conv_layer_fp32_vs_float64(ops, case):
    """a (config 3, config 2 at B = 2, config 5's levels): the <= 4-channel input layers take their image planar, as the step passes it"""
    B, Cin, Cout, size, ff, fd, wa = case
    assert_families(*case)
    run_conv_case(ops, f"conv {_cid(case)}", B, Cin, Cout, size, ff, fd, wa, form="planar" if Cin <= 4 else "cl")


@pytest.mark.parametrize("case", C3 + C5, ids=_cid)
def test_conv_layer_bf16_operands_vs_float64(ops, case):
    """b (configs 4 - 5): x, w and dy are bf16-representable, so the operand rounding of the bf16-operand kernels (every GEMM with more than 4
    reduction channels) is the identity, bf16 x bf16 products are exact in fp32 and the float64 reference of a) is the exact definition: the
    fp32 bound of the direct kernel applies.  (The <= 4-channel forward and weight gradient stay on the fp32 kernels of a.)"""
    B, Cin, Cout, size, ff, fd, wa = case
    ops.set_conv_precision("bf16")
    try:
        assert ops._use_bf16(Cout) and ops._use_bf16(Cin) == (Cin > 4)
    finally:
        ops.set_conv_precision("fp32")
    run_conv_case(ops, f"conv-bf16 {_cid(case)}", B, Cin, Cout, size, ff, fd, wa, form="planar" if Cin <= 4 else "cl", bf16=True)


# operand forms, one layer per kernel family: (B, Cin, Cout, size, form, forward, data gradient, weight gradient algo)
#   64 -> 64 @40^3 F(2x2x2,3x3x3) (an unaligned slice is copied to channels-last by ops._conv_raw; the weight gradient then runs the direct kernel)
#   32 -> 32 @40^3 F(2x2,3x3) pipelined; an unaligned slice takes the round-2 kernel's scalar path
#   32 -> 32 @10^3 direct with split-K; 192 -> 192 @20^3 F(2x2,3x3) with split-K; 32 -> 64 @9x16x16 the (y, x) weight gradient (odd depth)
#   3 -> 32 @80^3 and 2 -> 32 @64^3 (persistent input-layer kernel) channels-last instead of planar
#   32 -> 32 @40^3 as a slice of a buffer 8384 / 8392 channels wide: D H W in_ps 4 bytes just below / above 2^31 - the pipelined kernel's gate
FORMS = [
    (1, 64, 64, _s(40), "aligned", "z", "z", 3, 1), (1, 64, 64, _s(40), "unaligned", "z", "z", 0, 0),
    (1, 32, 32, _s(40), "aligned", "yp", "yp", 3, 1), (1, 32, 32, _s(40), "unaligned", "yr", "yr", 0, 0),
    (1, 32, 32, _s(10), "aligned", "ds", "ds", 3, 1), (1, 32, 32, _s(10), "unaligned", "ds", "ds", 0, 0),
    (1, 192, 192, _s(20), "aligned", "yps", "yps", 3, 1), (1, 192, 192, _s(20), "unaligned", "yrs", "yrs", 0, 0),
    (1, 32, 64, (9, 16, 16), "cl", "ds", "yps", 2, 1), (1, 32, 64, (9, 16, 16), "aligned", "ds", "yps", 2, 1),
    (1, 3, 32, _s(80), "cl", "d", "yp", 0, 0), (1, 2, 32, _s(64), "cl", "d", "yp", 0, 0), (2, 3, 32, _s(20), "unaligned", "d", "yr", 0, 0),
    (1, 32, 32, _s(40), ("ps", 8384), "yp", "yp", 3, 1), (1, 32, 32, _s(40), ("ps", 8392), "yr", "yr", 3, 1),
]


@pytest.mark.parametrize("case", FORMS, ids=lambda c: f"{_cid(c)}-{c[4] if isinstance(c[4], str) else c[4][1]}")
def test_conv_operand_forms_vs_float64(ops, case):
    B, Cin, Cout, size, form, ff, fd, wa, vec = case
    lib = _lib()
    nvox = size[0] * size[1] * size[2]
    ps_x = ps_dy = None
    if not isinstance(form, str):
        ps_x = ps_dy = form[1]
        assert (nvox * form[1] * 4 < 2 ** 31) == (form[1] == 8384) and abs(nvox * form[1] * 4 - 2 ** 31) < 2 ** 21
    # (an unaligned operand never runs the pipelined kernel: the round-2 kernel's scalar loads, or a channels-last copy in front of F(2x2x2,3x3x3))
    fam = lambda K, N, ps: family(B, size, K, N, ps).replace("p", "r") if form == "unaligned" else family(B, size, K, N, ps)
    assert fam(Cin, Cout, ps_x) == ff and fam(Cout, Cin, ps_dy) == fd
    assert lib.query("pulpo_conv3d_k3_wgrad_algo", B, *size, Cin, Cout, vec) == wa
    run_conv_case(ops, f"conv-form {_cid(case)} {form}", B, Cin, Cout, size, ff, fd, wa, form=form)


@pytest.mark.parametrize("Cin,Cout,size,algo", [(64, 64, _s(40), 3), (192, 192, _s(10), 2)])
def test_winograd_paths_copy_an_unaligned_channel_slice(ops, Cin, Cout, size, algo):
    """regression: ops._conv_raw promised to copy an operand the vector-load kernels cannot take - F(2x2x2,3x3x3) anywhere, F(2x2,3x3) on volumes
    that only its pipelined kernel runs (depth % 4 != 0 or fewer than 20^3 voxels) - but made that copy with to_cl(), which hands a channel
    slice of a wider channels-last buffer back unchanged: at an unaligned channel offset the entry point then refused the call
    (PulpoHipError).  The slice now gives the bits of its packed copy, forward and data gradient"""
    assert _lib().query("pulpo_conv3d_k3_algo", 1, *size, Cin, Cout) == algo and _lib().query("pulpo_conv3d_k3_algo", 1, *size, Cout, Cin) == algo
    g = gen(Cin + size[0])
    x, w, b, dy = conv_data(g, 1, Cin, Cout, size, False)
    outs = []
    for form in ("unaligned", "cl"):
        xo, dyo = operand(x, form, g).requires_grad_(True), operand(dy, form, g)
        out = ops.conv3d_k3(xo, w, b)
        outs.append((out, torch.autograd.grad(out, [xo], grad_outputs=dyo)[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_conv_bf16_storage_vs_float64(ops):
    """b: activations stored as bf16 (set_conv_precision("bf16", activations="bf16")): the bf16-operand kernel reads a bf16 x and stores a bf16
    y.  The stored value is the fp32 result rounded to 8 significant bits: half a bf16 ulp of the reference, 2^-9 |ref| at most... taken as
    2^-8 |ref| like the heads' bf16 dh, plus the fp32 bound.  Power: the channel of the last voxel with the smallest |ref|"""
    B, Cin, Cout, size = 1, 64, 96, (40, 40, 40)
    g = gen(4096)
    x, w, b, _ = conv_data(g, B, Cin, Cout, size, True)
    ops.set_conv_precision("bf16", activations="bf16")
    try:
        assert ops.act_dtype() == torch.bfloat16
        xb = x.bfloat16().contiguous(memory_format=CL)
        y = ops.new_cl(B, Cout, *size, DEV, torch.bfloat16)
        wp = ops._pack_weight_now(w, False, (B, *size), register=False)
        assert wp._pulpo_algo == "bf16"
        ops._conv_raw(xb, wp, b, y, Cin, Cout, None)
    finally:
        ops.set_conv_precision("fp32")
    ref = R.conv3_ref(x.double(), w.double(), b.double())
    tol = 2.0 ** -8 * ref.abs() + bound("conv bf16-storage out", R.conv3_ref(x, w, b), ref, R.conv3_mag(x.double(), w.double(), b.double()), M_FWD["b"])
    c = int(ref[-1, :, -1, -1, -1].abs().argmin())
    D, H, W = size
    held("conv bf16-storage out", y, ref, tol, power=((((B - 1) * Cout + c) * D + D - 1) * H + H - 1) * W + W - 1)


# ================================================================================================ c. statistics and reduction rows
def _call_fwd(ops, fam, x, w, bias, stats, poison=True):
    """one forward convolution through the C ABI of the given family with NaN-filled scratch; returns the stored output"""
    lib = _lib()
    B, K, D, H, W = x.shape
    N = w.shape[0]
    st = ops._stream()
    y = torch.full((B, D, H, W, N), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
    pack, nwp, wdt = {"d": ("pulpo_conv3d_k3_pack_weight", "pulpo_conv3d_k3_packed_floats", torch.float32),
                      "y": ("pulpo_conv3d_k3_pack_weight_wino2", "pulpo_conv3d_k3_packed_wino2_floats", torch.float32),
                      "z": ("pulpo_conv3d_k3_pack_weight_wino3", "pulpo_conv3d_k3_packed_wino3_floats", torch.float32),
                      "b": ("pulpo_conv3d_k3_pack_weight_bf16", "pulpo_conv3d_k3_packed_bf16_elems", torch.int16)}[fam]
    wp = torch.empty(lib.query(nwp, K, N), device=DEV, dtype=wdt)
    lib.call(pack, vp(w.contiguous()), vp(wp), K, N, 0, st)
    nscr = {"d": "pulpo_conv3d_k3_fwd_scratch_floats", "y": "pulpo_conv3d_k3_fwd_wino2_scratch_floats", "b": "pulpo_conv3d_k3_fwd_bf16_scratch_floats"}.get(fam)
    scr = None
    if nscr is not None:
        n = lib.query(nscr, B, D, H, W, K, N)
        scr = torch.full((n,), float("nan"), device=DEV) if n else None
    xs, ys = ops.grid_strides(x), ops.grid_strides(y)
    if fam == "z":
        lib.call("pulpo_conv3d_k3_fwd_wino3", vp(x), *xs, vp(wp), vp(bias), None, 0.2, vp(y), *ys, vp(stats), B, D, H, W, K, N, st)
    elif fam == "y":
        lib.call("pulpo_conv3d_k3_fwd_wino2", vp(x), *xs, vp(wp), vp(bias), None, 0.2, vp(y), *ys, vp(stats), vp(scr), B, D, H, W, K, N, st)
    else:
        lib.call("pulpo_conv3d_k3_fwd_bf16" if fam == "b" else "pulpo_conv3d_k3_fwd", vp(x), *xs, vp(wp), vp(bias), vp(y), *ys, vp(stats), vp(scr),
                 B, D, H, W, K, N, st)
    return y, scr is not None


def rows_vs_stored(name, rows, nrow, C, s1, s2, a1, a2, nvox):
    """rows [nrow][2][C] hold fp32 sums over disjoint voxel tiles: every row finite, and their float64 sums equal the two given channel sums
    of the STORED tensor.  Bound: a row is an fp32 sum of nvox / nrow terms in some order - at most (terms - 1) roundings of at most 2^-24 of
    the running magnitude each, plus one for the product inside the second sum: (nvox / nrow + 1) 2^-24 A, A = the sum of |terms|"""
    rows = rows.reshape(nrow, 2, C)
    assert bool(torch.isfinite(rows).all()), f"{name}: {int((~torch.isfinite(rows)).sum())} of {rows.numel()} promised row entries were not written"
    m = (nvox + nrow - 1) // nrow + 1
    got = rows.double().sum(0)
    held(f"{name} row sum 0", got[0], s1, m * U * a1)
    held(f"{name} row sum 1", got[1], s2, m * U * a2)


# (family, B, Cin, Cout, size, expected default family): direct with and without split-K, the persistent input-layer kernel (whole 4x8x8 tiles
# from 64^3 up, <= 4 channels), (y, x) Winograd pipelined / round-2 (K % 8 != 0) / split-K, xyz Winograd with a partly empty cout tile, bf16
STAT_CASES = [("d", 1, 3, 32, _s(20), "d"), ("d", 1, 32, 32, _s(10), "ds"), ("d", 1, 2, 32, _s(64), "d"), ("y", 1, 32, 32, _s(40), "yp"),
              ("y", 1, 20, 32, _s(40), "yr"), ("y", 1, 192, 192, _s(20), "yps"), ("y", 2, 32, 32, (24, 28, 20), "yp"), ("z", 1, 64, 48, _s(40), "z"),
              ("z", 2, 32, 32, _s(48), "z"), ("b", 1, 64, 64, _s(40), None), ("b", 1, 192, 192, _s(20), None)]


@pytest.mark.parametrize("fam,B,Cin,Cout,size,expect", STAT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_statistics_rows_describe_the_stored_output(ops, fam, B, Cin, Cout, size, expect):
    """c: stats and scratch arrive NaN-filled; every promised row is written, the output is fully written, and the rows summed in float64
    are sum(y) and sum(y^2) of the kernel's own stored output - the statistics arithmetic on its own, whatever the convolution's"""
    lib = _lib()
    if expect is not None:
        assert family(B, size, Cin, Cout) == expect
    g = gen(Cin + Cout + size[0])
    x, w, b, _ = conv_data(g, B, Cin, Cout, size, fam == "b")
    x = x.contiguous(memory_format=CL) if Cin > 4 else x
    nrow = lib.query("pulpo_conv3d_k3_fwd_bf16_stat_tiles" if fam == "b" else "pulpo_conv3d_k3_stat_tiles", B, *size)
    stats = torch.full((nrow * 2 * Cout,), float("nan"), device=DEV)
    y, split = _call_fwd(ops, fam, x, w, b, stats)
    assert split == (expect is not None and expect.endswith("s")) or fam == "b"
    assert bool(torch.isfinite(y).all())
    y64 = y.double()
    name = f"stats {fam} B{B} {Cin}to{Cout} {size}"
    rows_vs_stored(name, stats, nrow, Cout, y64.sum(dim=(0, 2, 3, 4)), (y64 * y64).sum(dim=(0, 2, 3, 4)), y64.abs().sum(dim=(0, 2, 3, 4)),
                   (y64 * y64).sum(dim=(0, 2, 3, 4)), y64.numel() // Cout)
    ref = R.conv3_ref(x.double(), w.double(), b.double())
    held(name + " out", y, ref, bound(name + " out", R.conv3_ref(x, w, b), ref, R.conv3_mag(x.double(), w.double(), b.double()), M_FWD[fam]))


def coef_block(mean64, rstd64, gamma64, beta64):
    """the coefficient block of pulpo_bn_fwd_finalize: [4][C] floats (mean, rstd, scale, shift) then [2][C] doubles (mean, rstd)"""
    scale = gamma64 * rstd64
    f = torch.stack([mean64, rstd64, scale, beta64 - mean64 * scale]).float().reshape(-1)
    return torch.cat([f.view(torch.uint8), torch.stack([mean64, rstd64]).reshape(-1).contiguous().view(torch.uint8)]).view(torch.float32)


# (entry, B, K = channels of dy, N = channels of dx, size): the (y, x) and the xyz data-gradient forms with the BatchNorm-backward reduction
BNRED_CASES = [("wino2", 1, 32, 32, _s(40)), ("wino2", 2, 32, 32, _s(24)), ("wino3", 1, 64, 64, _s(40)), ("wino3", 1, 128, 96, _s(40)), ("wino3_kb", 1, 64, 64, _s(40))]


@pytest.mark.parametrize("entry,B,K,N,size", BNRED_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dgrad_bnred_rows_describe_the_stored_gradient(ops, entry, B, K, N, size):
    """c: part arrives NaN-filled; the rows summed in float64 are sum(dbn) and sum(dbn (y - fp32 mean)) with dbn = dx lrelu'(y scale + shift)
    formed from the kernel's own stored dx, the given pre-norm tensor y and coefficient block; dx itself against the float64 data gradient"""
    lib = _lib()
    assert lib.query("pulpo_conv3d_k3_dgrad_wino2_bnred_ok", B, *size, K, N) == 1
    assert lib.query("pulpo_conv3d_k3_algo", B, *size, K, N) == (2 if entry == "wino2" else 3)
    g = gen(K + N + size[0] + B)
    dy, w, _, _ = conv_data(g, B, K, N, size, False)                 # (w: (N, K, 3, 3, 3) of the data-gradient GEMM = flipped transpose below)
    # (a mean of its own for dy and w: dx then has mean ~1 per channel, the row sums grow with the voxel count like the magnitude sums their
    #  bound is made of, and the power check keeps its meaning)
    dy, w = dy + 1.0, w + 1.0 / (27 * K)
    wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()                  # the unit's weight (Cout = K, Cin = N)
    ybn = (torch.randn(B, N, *size, device=DEV, generator=g) * 1.5 + 0.3).contiguous(memory_format=CL)
    mean = ybn.double().mean(dim=(0, 2, 3, 4))
    rstd = (ybn.double().var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5).rsqrt()
    gamma = torch.rand(N, device=DEV, generator=g).double() + 0.5
    beta = torch.randn(N, device=DEV, generator=g).double() * 0.5
    coef = coef_block(mean, rstd, gamma, beta)
    st = ops._stream()
    kind = "wino2" if entry == "wino2" else "wino3"
    wp = torch.empty(lib.query(f"pulpo_conv3d_k3_packed_{kind}_floats", K, N), device=DEV)
    lib.call(f"pulpo_conv3d_k3_pack_weight_{kind}", vp(wt), vp(wp), N, K, 1, st)
    dyc = dy.contiguous(memory_format=CL)
    dx = torch.full((B, *size, N), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
    nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
    part = torch.full((nrow * 2 * N,), float("nan"), device=DEV)
    ds, xs, ys = ops.grid_strides(dyc), ops.grid_strides(dx), ops.grid_strides(ybn)
    if entry == "wino3_kb":
        # channel-blocked gradient operand [K / 8][B][D][H][W][8]: voxel stride 8, block stride B V 8
        V = size[0] * size[1] * size[2]
        dkb = dy.reshape(B, K // 8, 8, *size).permute(1, 0, 3, 4, 5, 2).contiguous()
        lib.call("pulpo_conv3d_k3_dgrad_wino3_bnred_kb", vp(dkb), V * 8, 8, B * V * 8, vp(wp), vp(dx), xs[0], xs[1], 8, vp(ybn), ys[0], ys[1], vp(coef), 0.2,
                 vp(part), B, *size, K, N, st)
    else:
        lib.call(f"pulpo_conv3d_k3_dgrad_{entry}_bnred", vp(dyc), *ds, vp(wp), vp(dx), xs[0], xs[1], vp(ybn), ys[0], ys[1], vp(coef), 0.2, vp(part),
                 B, *size, K, N, st)
    assert bool(torch.isfinite(dx).all())
    name = f"bnred {entry} B{B} {K}to{N} {size}"
    c32 = coef[:4 * N].reshape(4, N).double()
    v = lambda t: t.reshape(1, -1, 1, 1, 1)
    bn = (ybn * v(coef[2 * N:3 * N]) + v(coef[3 * N:4 * N]))                   # fp32, as the kernel forms the LeakyReLU branch
    dbn = torch.where(bn > 0, dx, 0.2 * dx).double()
    yc = ybn.double() - v(c32[0])
    rows_vs_stored(name, part, nrow, N, dbn.sum(dim=(0, 2, 3, 4)), (dbn * yc).sum(dim=(0, 2, 3, 4)), dbn.abs().sum(dim=(0, 2, 3, 4)),
                   (dbn * yc).abs().sum(dim=(0, 2, 3, 4)), dbn.numel() // N)
    ref = R.conv3_dgrad_ref(dy.double(), wt.double())
    held(name + " dx", dx, ref, bound(name + " dx", R.conv3_dgrad_ref(dy, wt), ref, R.conv3_dgrad_mag(dy.double(), wt.double()), M_FWD["y" if entry == "wino2" else "z"]))


# ================================================================================================ e. pooling and x2 up-sampling
def _pool_bound(name, x, m):
    x64 = x.double()
    ref = R.avgpool2_ref(x64)
    return ref, bound(name, R.avgpool2_ref(x), ref, R.avgpool2_ref(x64.abs()), m)


# (B, C, size): the step's pooled activations (32 @160^3, 64 @80^3, 128 @40^3, 192 @20^3) and images (C = 1, planar), config 2 at B = 2,
# config 5's levels down to 6x7x5 -> 3x4x3 (divisors 8, 4, 2) and an all-odd volume (divisor 1 in the far corner)
POOL_CASES = [(1, 32, _s(160)), (1, 64, _s(80)), (1, 128, _s(40)), (1, 192, _s(20)), (1, 1, _s(160)), (1, 1, _s(20)), (2, 32, _s(96)), (2, 1, _s(48)),
              (1, 64, (96, 112, 80)), (1, 192, (12, 14, 10)), (1, 192, (6, 7, 5)), (1, 1, (6, 7, 5)), (2, 32, (5, 7, 9)), (1, 6, (7, 5, 3))]


@pytest.mark.parametrize("B,C,size", POOL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_avg_pool2_and_skip_vs_float64(ops, B, C, size):
    """e: avg_pool2 and avg_pool2_skip, forward and backward (the skip form with both gradients, with the pooled one only and with the skip
    one only).  An average of at most 8 terms: 7 additions and the division, m = 8; backward g / divisor (+ skip gradient): m = 2"""
    g = gen(C + size[0] + B)
    x = torch.randn(B, C, *size, device=DEV, generator=g)
    x = x.contiguous(memory_format=CL) if C > 1 else x
    name = f"pool B{B} C{C} {size}"
    ref, tol = _pool_bound(name + " out", x, 8.0)
    up = torch.randn(ref.shape, device=DEV, generator=g)
    gskip = torch.randn(B, C, *size, device=DEV, generator=g)
    gskip = gskip.contiguous(memory_format=CL) if C > 1 else gskip
    x64 = x.double().requires_grad_(True)
    rg, = torch.autograd.grad((R.avgpool2_ref(x64) * up.double()).sum(), [x64])
    xa = x.double().requires_grad_(True)
    ag, = torch.autograd.grad((R.avgpool2_ref(xa) * up.double().abs()).sum(), [xa])
    x32 = x.clone().requires_grad_(True)
    g32, = torch.autograd.grad((R.avgpool2_ref(x32) * up).sum(), [x32])
    tol_g = bound(name + " gin", g32, rg, ag, 2.0)
    tol_gs = bound(name + " gin+skip", g32 + gskip, rg + gskip.double(), ag + gskip.double().abs(), 2.0)
    xg = x.clone().requires_grad_(True)
    out = ops.avg_pool2(xg)
    held(name + " out", out, ref, tol)
    gin, = torch.autograd.grad(out, [xg], grad_outputs=up.contiguous(memory_format=CL) if C > 1 else up)
    held(name + " gin", gin, rg, tol_g)
    for both in ("pool+skip", "pool", "skip"):
        xg = x.clone().requires_grad_(True)
        alias, pooled = ops.avg_pool2_skip(xg)
        assert torch.equal(alias, x)
        held(name + " skip-form out", pooled, ref, tol)
        loss = (pooled * up).sum() if both != "skip" else 0
        loss = loss + ((alias * gskip).sum() if both != "pool" else 0)
        gin, = torch.autograd.grad(loss, [xg])
        if both == "skip":
            assert torch.equal(gin, gskip)
        else:
            held(f"{name} {both} gin", gin, rg + gskip.double() if both == "pool+skip" else rg, tol_gs if both == "pool+skip" else tol_g)


# (B, source size, which sources ask for a gradient): the feedback list of the step - samples, velocity fields, individual, combined and final
# displacement fields (3 channels each) and the transformed image (1) = 16 channels - at 80 -> 160, 40 -> 80, 20 -> 40, 10 -> 20, config 2 at
# B = 2 and config 5's odd 6x7x5 -> 12x14x10; a single source; sources without a gradient (NULL entries of the backward's pointer table)
UP2_CHANS = [3, 3, 3, 3, 3, 1]
UP2_CASES = [(1, _s(80), (1, 1, 1, 1, 1, 1)), (1, _s(40), (1, 1, 0, 1, 0, 1)), (1, _s(20), (1, 1, 1, 1, 1, 0)), (1, _s(10), (0, 1, 1, 0, 1, 1)),
             (2, _s(24), (1, 0, 1, 1, 1, 1)), (1, (6, 7, 5), (1, 1, 1, 0, 1, 1)), (2, (6, 7, 5), (0, 0, 0, 0, 0, 1)), (1, (3, 4, 3), (1,))]


@pytest.mark.parametrize("B,size,need", UP2_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_feedback_up2_vs_float64(ops, B, size, need):
    """e: x2 trilinear up-sampling of every source + channel concatenation.  Weights are products of 1/4 and 3/4, exact in fp32: an output is
    a sum of 8 rounded products (m = 8); a source gradient gathers at most 4 outputs per axis, 64 terms (m = 64)"""
    g = gen(size[0] + size[2] + B + len(need))
    chans = UP2_CHANS[:len(need)]
    srcs = [torch.randn(B, c, *size, device=DEV, generator=g) for c in chans]
    name = f"up2 B{B} {size} {need}"
    s64 = [s.double().requires_grad_(bool(n)) for s, n in zip(srcs, need)]
    ref = R.up2_cat_ref(s64)
    up = torch.randn(ref.shape, device=DEV, generator=g).contiguous(memory_format=CL)
    want = [s for s, n in zip(s64, need) if n]
    rg = torch.autograd.grad((ref * up.double()).sum(), want)
    sa = [s.double().abs().requires_grad_(bool(n)) for s, n in zip(srcs, need)]
    refa = R.up2_cat_ref(sa)
    ag = torch.autograd.grad((refa * up.double().abs()).sum(), [s for s, n in zip(sa, need) if n])
    s32 = [s.clone().requires_grad_(bool(n)) for s, n in zip(srcs, need)]
    ref32 = R.up2_cat_ref(s32)
    g32 = torch.autograd.grad((ref32 * up).sum(), [s for s, n in zip(s32, need) if n])
    sg = [s.clone().requires_grad_(bool(n)) for s, n in zip(srcs, need)]
    out = ops.feedback_up2(sg)
    assert ops.is_cl(out)
    held(name + " out", out, ref.detach(), bound(name + " out", ref32.detach(), ref.detach(), refa.detach(), 8.0))
    got = torch.autograd.grad(out, [s for s, n in zip(sg, need) if n], grad_outputs=up)
    for k, (a, r, r32, A) in enumerate(zip(got, rg, g32, ag)):
        held(f"{name} gsrc{k}", a, r, bound(f"{name} gsrc{k}", r32, r, A, 64.0))


# ================================================================================================ d. the BatchNorm / LeakyReLU chain
def _tile_rows(y, tile=256):
    """statistics rows as a convolution store writes them: (sum y, sum y^2) over consecutive 256-voxel tiles, formed in float64 and rounded to
    fp32 once - each entry is within 2^-24 of its value, so the chain's own arithmetic is what the comparison sees"""
    B, C = y.shape[:2]
    yl = y.permute(0, 2, 3, 4, 1).reshape(-1, C).double()
    n = yl.shape[0]
    ntile = (n + tile - 1) // tile
    yl = torch.cat([yl, yl.new_zeros(ntile * tile - n, C)]).reshape(ntile, tile, C)
    return torch.stack([yl.sum(1), (yl * yl).sum(1)], 1).float().contiguous(), ntile


def _chan(t):
    return t.reshape(1, -1, 1, 1, 1)


def _csum(t):
    return t.sum(dim=(0, 2, 3, 4))


# (B, C, size): the step's units C = 32 @160^3, 64 and 96 @80^3, 128 @40^3, 192 @20^3 and 10^3; config 2 at B = 2; config 5's ragged 6x7x5
# (pooled edge windows of 4 and 2 voxels) and an all-odd volume (a corner window of 1 voxel)
BN_CASES = [(1, 32, _s(160)), (1, 64, _s(80)), (1, 96, _s(80)), (1, 128, _s(40)), (1, 192, _s(20)), (1, 192, _s(10)), (2, 32, _s(96)), (2, 64, _s(48)),
            (2, 192, _s(12)), (1, 192, (6, 7, 5)), (2, 32, (5, 7, 9))]


@pytest.mark.parametrize("B,C,size", BN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_batchnorm_chain_vs_float64(ops, B, C, size):
    """d: pulpo_bn_fwd_finalize, pulpo_bn_lrelu_apply (+ _pool2, _kb), pulpo_bn_lrelu_bwd_reduce, pulpo_avgpool2_bwd_bnred, pulpo_bn_bwd_finalize,
    pulpo_bn_lrelu_bwd_apply (+ _pooled_t, _kb_t, _pooled_kb_t) and, for C = 32, pulpo_conv3d_k3_wgrad_bn through the C ABI, every output buffer
    NaN-filled before its call.

    Channel 0 holds small integers in antisymmetric halves with beta = 0: every partial sum is exact in any order, so mean = shift = 0 exactly,
    y scale + shift is exactly 0 where y is, and both LeakyReLU branches occur (at 0: z = 0 and the gradient takes the slope, as ATen does).
    Channel 1 is 0.5 + 1e-4 N(0, 1): its variance 1e-8 is far below eps, rstd is near 1 / sqrt(eps).

    Bounds (u = 2^-24), each the sum of |terms| the formula adds times the roundings it makes, plus the bounds of its inputs propagated:
      mean: rows carry one rounding each, the kernel adds them in double, the float row of coef one more: 2 u mean|y|
      var = q / n - mean^2: 2 u (mean(y^2) + 2 |mean| mean|y|);  rstd: |d rstd / d var| = rstd^3 / 2 times that, + 2 u rstd
      scale = gamma rstd, shift = beta - mean scale, running statistics: the product rule on those, + 2 u (4 u: three roundings) of the terms
      z: |y - mean| T_scale + |scale| T_mean + 2 u (|beta| + |mean scale|) + 2 u (|y scale| + |shift|);  pooled: the average of T_z + 8 u the average of |z|
      sum dbn, sum dbn (y - m32): block partials in fp32, (voxels per block + 2) u of the magnitude sums; where |y scale + shift| is below its
      own bound (and not exactly 0) the fp32 sign may differ from the float64 one: 0.8 |dz| more there
      dy = A dbn + B (y - m32) + C: 8 u (|A dbn| + |B (y - m32)| + |C|) + the bounds of scale, both means and rstd propagated"""
    lib = _lib()
    st = ops._stream()
    D, H, W = size
    npix, eps, slope = B * D * H * W, 1e-5, 0.2
    g = gen(C * 3 + D + B)
    y = torch.randn(B, C, *size, device=DEV, generator=g) * 1.5 + 0.3
    half = torch.randint(-2, 3, (npix // 2,), device=DEV, generator=g).float()
    assert npix % 2 == 0
    y[:, 0] = torch.cat([half, -half])[torch.randperm(npix, device=DEV, generator=g)].reshape(B, *size)
    y[:, 1] = 0.5 + 1e-4 * torch.randn(B, *size, device=DEV, generator=g)
    y = y.contiguous(memory_format=CL)
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.3
    beta[0] = 0.0
    rm, rv = torch.randn(C, device=DEV, generator=g), torch.rand(C, device=DEV, generator=g) + 0.5
    name = f"bn B{B} C{C} {size}"
    y64 = y.double()
    r = R.bn_train_ref(y64, gamma.double(), beta.double(), eps, 0.1, rm.double(), rv.double(), slope)
    assert float(r["mean"][0]) == 0.0 and float(r["rstd"][1]) > 0.99 / eps ** 0.5 * 0.999 and bool((r["bn"][:, 0] == 0).any())
    assert bool((r["bn"][:, 0] > 0).any()) and bool((r["bn"][:, 0] < 0).any())

    # ---- forward finalize
    rows, ntile = _tile_rows(y)
    coef = torch.full((8 * C,), float("nan"), device=DEV)
    rmk, rvk, nbt = rm.clone(), rv.clone(), torch.zeros(1, dtype=torch.int64, device=DEV)
    nsd = lib.query("pulpo_bn_fwd_finalize_scratch_doubles", ntile, C)
    assert (nsd > 0) == (ntile > 2048)
    scr = torch.full((nsd,), float("nan"), device=DEV, dtype=torch.float64) if nsd else None
    lib.call("pulpo_bn_fwd_finalize", vp(rows), ntile, C, float(npix), vp(gamma), vp(beta), vp(rmk), vp(rvk), vp(nbt), 0.1, eps, vp(coef), vp(scr), st)
    assert int(nbt) == 1
    cf = coef[:4 * C].reshape(4, C)
    cd = coef[4 * C:].view(torch.float64).reshape(2, C)
    a_mean = _csum(y64.abs()) / npix
    t_mean = 2 * U * a_mean
    t_var = 2 * U * (_csum(y64 * y64) / npix + 2 * r["mean"].abs() * a_mean)
    t_rstd = 0.5 * r["rstd"] ** 3 * t_var * 1.01 + 2 * U * r["rstd"]
    t_scale = gamma.double() * t_rstd + 2 * U * r["scale"].abs()
    t_shift = r["mean"].abs() * t_scale + r["scale"].abs() * t_mean + 2 * U * (beta.double().abs() + (r["mean"] * r["scale"]).abs())
    tiny = 1e-30                                       # (channel 0: mean and shift are exactly 0 and so are their bounds' leading terms)
    held(name + " coef mean", cf[0], r["mean"], t_mean + tiny)
    held(name + " coef rstd", cf[1], r["rstd"], t_rstd)
    held(name + " coef scale", cf[2], r["scale"], t_scale)
    held(name + " coef shift", cf[3], r["shift"], t_shift + tiny)
    held(name + " coef mean(double)", cd[0], r["mean"], t_mean + tiny)
    held(name + " coef rstd(double)", cd[1], r["rstd"], t_rstd)
    assert float(cf[0, 0]) == 0.0 and float(cf[3, 0]) == 0.0 and float(cd[0, 0]) == 0.0
    held(name + " running_mean", rmk, r["running_mean"], 0.1 * t_mean + 4 * U * (0.9 * rm.double().abs() + 0.1 * r["mean"].abs()))
    held(name + " running_var", rvk, r["running_var"], 0.1 * npix / (npix - 1) * t_var + 4 * U * (0.9 * rv.double() + 0.1 * r["var"] * npix / (npix - 1)))

    # ---- apply: z, z + pooled, blocked z
    # (the kernel's shift is beta - mean' scale' with ITS mean and scale: y scale' + shift' = (y - mean') scale' + beta, so the errors of scale and
    #  shift enter through (y - mean), not through y)
    t_bn = ((y64 - _chan(r["mean"])).abs() * _chan(t_scale) + _chan(r["scale"].abs() * t_mean + 2 * U * (beta.double().abs() + (r["mean"] * r["scale"]).abs()))
            + 2 * U * ((y64 * _chan(r["scale"])).abs() + _chan(r["shift"].abs())))
    t_z = t_bn + tiny
    yps = y.stride(4)
    z = torch.full((B, *size, C), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
    lib.call("pulpo_bn_lrelu_apply", vp(y), yps, vp(z), z.stride(4), vp(coef), npix, C, slope, st)
    held(name + " z", z, r["z"], t_z)
    assert bool((z[:, 0][y[:, 0] == 0] == 0).all())
    pooled_ref = R.avgpool2_ref(r["z"])
    t_pool = R.avgpool2_ref(t_z) + 8 * U * R.avgpool2_ref(r["z"].abs())
    if lib.query("pulpo_bn_lrelu_apply_pool2_ok", C, yps, C, C):
        z2 = torch.full((B, *size, C), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
        pooled = torch.full((B, *pooled_ref.shape[2:], C), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
        lib.call("pulpo_bn_lrelu_apply_pool2", vp(y), yps, vp(z2), z2.stride(4), vp(pooled), pooled.stride(4), vp(coef), B, D, H, W, C, slope, st)
        held(name + " z(pool2)", z2, r["z"], t_z)
        held(name + " pooled", pooled, pooled_ref, t_pool)
    else:
        assert C % 4 != 0
    if C % 8 == 0:
        zkb = torch.full((C // 8, B, *size, 8), float("nan"), device=DEV)
        lib.call("pulpo_bn_lrelu_apply_kb", vp(y), yps, vp(zkb), 8, npix * 8, vp(coef), npix, C, slope, st)
        held(name + " z(blocked)", ops.blocked_to_cl(zkb), r["z"], t_z)

    # ---- backward: plain (dz a tensor) and pooled (dz = gskip + avg_pool_backward(gpool), never written) forms
    # (a mean of its own per channel: sum dbn then grows with the voxel count like the magnitude sum its bound is made of, and the power
    #  check keeps its meaning at 160^3)
    dz = (torch.randn(B, C, *size, device=DEV, generator=g) + _chan(torch.randn(C, device=DEV, generator=g))).contiguous(memory_format=CL)
    gpool = torch.randn(pooled_ref.shape, device=DEV, generator=g).contiguous(memory_format=CL)
    p64 = y64.clone().requires_grad_(True)
    dzp64 = dz.double() + torch.autograd.grad((R.avgpool2_ref(p64) * gpool.double()).sum(), [p64])[0]
    pa = y64.clone().requires_grad_(True)
    t_dzp = 2 * U * (dz.double().abs() + torch.autograd.grad((R.avgpool2_ref(pa) * gpool.double().abs()).sum(), [pa])[0])
    near = (r["bn"].abs() <= t_bn) & (r["bn"] != 0)
    print(f"{name}: {int(near.sum())} of {near.numel()} voxels within the bound of the LeakyReLU kink")
    nblk = lib.query("pulpo_bn_bwd_blocks", npix, C)
    m32 = cf[0].double()
    mblk = (npix + nblk - 1) // nblk + 2
    for form in ("plain", "pooled"):
        dz64 = dz.double() if form == "plain" else dzp64
        t_dz = torch.zeros_like(dz64) if form == "plain" else t_dzp
        bw = R.bn_lrelu_bwd_ref(dz64, y64, r["mean"], r["rstd"], r["scale"], r["shift"], slope)
        yc32 = y64 - _chan(m32)
        flip = 0.8 * dz64.abs() * near + t_dz
        part = torch.full((nblk * 2 * C,), float("nan"), device=DEV)
        gin = None
        if form == "plain":
            lib.call("pulpo_bn_lrelu_bwd_reduce", vp(dz), dz.stride(4), vp(y), yps, vp(coef), npix, C, slope, vp(part), st)
        else:
            gin = torch.full((B, *size, C), float("nan"), device=DEV).permute(0, 4, 1, 2, 3)
            lib.call("pulpo_avgpool2_bwd_bnred", vp(gpool), gpool.stride(4), vp(dz), dz.stride(4), vp(gin), gin.stride(4), vp(y), yps, vp(coef), slope, vp(part),
                     B, D, H, W, C, st)
            held(f"{name} {form} gin", gin, dzp64, t_dzp)
        prow = part.reshape(nblk, 2, C)
        assert bool(torch.isfinite(prow).all()), f"{name} {form}: {int((~torch.isfinite(prow)).sum())} row entries were not written"
        t_s = mblk * U * _csum(bw["dbn"].abs()) + _csum(flip)
        t_q = mblk * U * _csum((bw["dbn"] * yc32).abs()) + _csum(flip * yc32.abs())
        got = prow.double().sum(0)
        held(f"{name} {form} rows sum dbn", got[0], bw["sum_dbn"], t_s)
        held(f"{name} {form} rows sum dbn (y - m32)", got[1], _csum(bw["dbn"] * yc32), t_q)
        tot = torch.full((2 * C,), float("nan"), device=DEV)
        totd = torch.full((2 * C,), float("nan"), device=DEV, dtype=torch.float64)
        nsd = lib.query("pulpo_bn_bwd_finalize_scratch_doubles", nblk, C)
        scr = torch.full((nsd,), float("nan"), device=DEV, dtype=torch.float64) if nsd else None
        lib.call("pulpo_bn_bwd_finalize", vp(part), nblk, C, vp(coef), float(npix), 1, vp(tot), ctypes.c_void_p(tot.data_ptr() + 4 * C), 0, vp(totd), vp(scr), st)
        t_x = t_q + t_mean * bw["sum_dbn"].abs() + U * r["mean"].abs() * t_s
        t_dgamma = r["rstd"] * t_x + bw["sum_dbn_c"].abs() * t_rstd + 2 * U * bw["dgamma"].abs()
        held(f"{name} {form} dbeta", tot[:C], bw["dbeta"], t_s + U * bw["dbeta"].abs())
        held(f"{name} {form} dgamma", tot[C:], bw["dgamma"], t_dgamma)
        held(f"{name} {form} mean dbn", totd[:C], bw["sum_dbn"] / npix, t_s / npix)
        held(f"{name} {form} mean dbn xhat", totd[C:], bw["dgamma"] / npix, t_dgamma / npix)
        # second pass
        sc, rs = _chan(r["scale"]), _chan(r["rstd"])
        yc = y64 - _chan(r["mean"])
        a_dy = sc.abs() * (bw["dbn"].abs() + _chan(bw["sum_dbn"].abs()) / npix + yc.abs() * rs * rs * _chan(bw["sum_dbn_c"].abs()) / npix)
        t_dy = (8 * U * a_dy + sc.abs() * (flip + _chan(t_s) / npix + yc.abs() * (rs * rs * _chan(t_x) + 2 * rs * _chan(t_rstd * bw["sum_dbn_c"].abs())) / npix
                                           + _chan(t_mean) * rs * rs * _chan(bw["sum_dbn_c"].abs()) / npix) + _chan(t_scale / r["scale"].abs()) * a_dy)
        if form == "plain" and C == 32:
            # pulpo_conv3d_k3_wgrad_bn (the image pair's unit, 2 -> 32): dy is formed per element while the weight gradient stages it and never
            # stored.  dw against the float64 weight gradient of the float64 dy: the direct kernel's convolution bound (random-walk form from
            # 4e6 voxels up, as for the plain weight gradient) plus dy's own bound carried through the sum, sum |x| T_dy
            x2 = torch.randn(B, 2, *size, device=DEV, generator=g)
            dwk = torch.full((C, 2, 3, 3, 3), float("nan"), device=DEV)
            wscr = torch.full((lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", 2, C),), float("nan"), device=DEV)
            nrow2 = lib.query("pulpo_conv3d_k3_wgrad_bn_rows", B, D, H, W, C)
            prt = torch.full((nrow2 * C,), float("nan"), device=DEV)
            lib.call("pulpo_conv3d_k3_wgrad_bn", vp(x2), *ops.grid_strides(x2), vp(dz), 0, dz.stride(0), dz.stride(4), vp(y), y.stride(0), yps, vp(coef), vp(totd),
                     slope, vp(dwk), 0, vp(wscr), vp(prt), B, D, H, W, 2, C, st)
            wref = R.conv3_wgrad_ref(x2.double(), bw["dy"])
            w32 = R.conv3_wgrad_ref(x2, bw["dy"].float())
            carried = R.conv3_wgrad_ref(x2.double().abs(), t_dy)
            if npix >= RANDOM_WALK_VOXELS:
                Rw = R.conv3_wgrad_mag(x2.double(), bw["dy"], random_walk=True)
                rho = R.ratio(w32, wref, U * Rw)
                print(f"RHO32 {name} wgrad_bn dw(random walk) {rho:.3g}")
                t_w = 4.0 * rho * U * Rw + carried
            else:
                t_w = bound(f"{name} wgrad_bn dw", w32, wref, R.conv3_wgrad_mag(x2.double(), bw["dy"]), M_WGRAD[0]) + carried
            held(f"{name} wgrad_bn dw", dwk, wref, t_w)
            p2 = prt.reshape(nrow2, C)
            assert bool(torch.isfinite(p2).all()), f"{name} wgrad_bn: {int((~torch.isfinite(p2)).sum())} bias-gradient row entries were not written"
            t_b = ((npix + nrow2 - 1) // nrow2 + 2) * U * _csum(bw["dy"].abs()) + _csum(t_dy)
            held(f"{name} wgrad_bn bias rows", p2.double().sum(0), _csum(bw["dy"]), t_b, power=None)
            assert float(t_b[-1]) < 1e-3 * float(_csum(bw["dy"].abs())[-1])
        variants = [("", False)] + ([("_kb", True)] if C % 8 == 0 else [])
        for sfx, blocked in variants:
            dyk = torch.full((C // 8, B, *size, 8) if blocked else (B, *size, C), float("nan"), device=DEV)
            dyv = dyk if blocked else dyk.permute(0, 4, 1, 2, 3)
            dys = (8, npix * 8) if blocked else (dyv.stride(4),)
            part2 = torch.full((nblk * C,), float("nan"), device=DEV)
            if form == "plain" and not blocked:
                lib.call("pulpo_bn_lrelu_bwd_apply", vp(dz), dz.stride(4), vp(y), yps, vp(coef), vp(totd), vp(dyk), *dys, npix, C, slope, vp(part2), st)
            elif form == "plain":
                lib.call("pulpo_bn_lrelu_bwd_apply_kb_t", vp(dz), 0, dz.stride(4), 8, vp(y), yps, vp(coef), vp(totd), vp(dyk), *dys, npix, C, slope, vp(part2), st)
            elif not blocked:
                lib.call("pulpo_bn_lrelu_bwd_apply_pooled_t", vp(gpool), gpool.stride(4), vp(dz), dz.stride(4), 0, vp(y), 0, yps, vp(coef), vp(totd), vp(dyk), *dys,
                         slope, vp(part2), B, D, H, W, C, st)
            else:
                lib.call("pulpo_bn_lrelu_bwd_apply_pooled_kb_t", vp(gpool), gpool.stride(4), vp(dz), dz.stride(4), 0, vp(y), yps, vp(coef), vp(totd), vp(dyk), *dys,
                         slope, vp(part2), B, D, H, W, C, st)
            dyt = ops.blocked_to_cl(dyk) if blocked else dyv
            held(f"{name} {form}{sfx} dy", dyt, bw["dy"], t_dy)
            # bias-gradient rows: the column sums of the STORED dy.  In exact arithmetic they vanish, so the perturbation of the power check is
            # taken on the scale of what is summed: the bound rejects an error of 1e-3 of the last channel's sum |dy|
            p2 = part2.reshape(nblk, C)
            assert bool(torch.isfinite(p2).all()), f"{name} {form}{sfx}: {int((~torch.isfinite(p2)).sum())} bias-gradient row entries were not written"
            sdy, ady = _csum(dyt.double()), _csum(dyt.double().abs())
            t_b = mblk * U * ady
            held(f"{name} {form}{sfx} bias rows", p2.double().sum(0), sdy, t_b, power=None)
            assert float(t_b[-1]) < 1e-3 * float(ady[-1])
