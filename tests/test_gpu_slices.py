"""The 2-D (slice) mode (train.py --ndims 2) at real slice sizes: every kernel a slice runs, element by element against float64.

A slice runs as a depth-1 volume through the 3-D kernels (pulpo_amd/ops.py, "2-D mode").  Which kernels that selects is asserted from the
library's own queries before anything runs: the forward and the data gradient are always the direct kernel (conv_tz(1, H, W) == 2: tiles of
two planes, one of them empty), with split-K wherever a layer has fewer than 512 tiles and more than one channel chunk; the weight gradient
is F(2x2,3x3) in (y, x) (algorithm 2: a depth of 1 is never an even depth of at least 4) wherever the operands are vectorisable, Cin >= 8
and H W >= 1000, else the direct kernel - the z-streaming (y, x) kernel then does ONE plane step per (y, x) tile with both halo planes
outside the volume.

  a  the convolution layers of the model on three slice pyramids, ragged slices and both sides of the selection gates, as 5-D operands of
     depth 1 through test_gpu_pyramid_convunit.run_conv_case (its bounds: M_FWD / M_WGRAD with the rho32 construction);
  b  the 4-D entries (conv3d_k3, conv_bn_lrelu, avg_pool2 / avg_pool2_skip) against tests/slice_ref.py, which is written with torch's native
     2-D operators and never lifts - so the lifting (_lift_w3, _lift_field, padded head rows, the identity depth mapping) is under test;
  c  the 1x1 heads with two latent channels;  d  the bilinear resize and the ragged feedback path;  e  warp, warp_mask and VecInt;
  f  a training step of the REAL reference at 80x96 (tests/golden/make_golden.py slices) replayed, and on the same model deterministic
     mode, the data-parallel stepper against autograd + Adam, and the bf16-operand mode.

Every comparison goes through check / held (tests/test_gpu_pyramid_ops.py, test_gpu_pyramid_convunit.py): max |got - ref| against a bound,
and the same bound must reject the reference with one element moved by 1e-3 max|ref|.  No bound is fitted to the code under test: each is a
project constant, a bound built from the float32 evaluation of the same plain reference (rho32), or twice torch's own float32 spread.

Section b's ConvUnit bound.  The unit is z = lrelu(scale (y - mean) + beta), y the convolution, and its backward the formulas of
slice_ref.bn_lrelu_bwd_ref followed by the convolution's two gradients.  The bound of each tensor is T = m max(1, rho32) 2^-24 A + F:
  * A is the first-order propagated magnitude: every stage adds the sum of the absolute values of the terms it adds (its own roundings) and
    the magnitudes of its inputs times the absolute partial derivatives (A_y = sum |x| |w| + |b| for the convolution; mean: the channel
    mean of A_y and of |y|; var: 2 mean(|y - mean| (A_y + A_mean)) + mean((y - mean)^2); rstd: rstd^3 / 2 A_var + rstd; and so on down to
    dx and dw, whose A is the convolution's own magnitude sum plus the magnitude of dy carried through the same sum);
  * m is the project constant of the kernel family that forms the tensor: M_FWD["d"] = 8 for everything the direct forward / data
    gradient produce, M_WGRAD[algorithm] for dw;
  * rho32 is the largest (|err| - F) / (2^-24 A) of the float32 evaluation of the same slice_ref function on the same data;
  * F covers the LeakyReLU kink: where |bn| is below its own bound (and not exactly 0) the fp32 sign may differ from the float64 one and the
    gradient takes the other slope, 0.8 |dz| there, carried through the same sums without a factor (test_batchnorm_chain_vs_float64)."""
import types

import numpy as np
import pytest
import torch

import pyramid_ref as R
import slice_ref as S
from test_gpu_pyramid_convunit import M_FWD, M_WGRAD, U, _cid, assert_families, bound, conv_data, family, held, operand, run_conv_case
from test_gpu_pyramid_ops import amax, check, det_default, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL2 = torch.channels_last
T = torch.from_numpy
FB = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
OUT = ("mus", "sigmas", "samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    assert torch.backends.cuda.matmul.allow_tf32 is False
    return _ops


def _lib():
    from pulpo_amd._lib import lib
    return lib


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ================================================================================================ a. convolution layers at depth 1
# (B, Cin, Cout, (1, H, W), forward family, data-gradient family, weight-gradient algorithm) as the library's queries answer for channels-last
# fp32 operands: d direct, ds direct with split-K; 2 F(2x2,3x3) in (y, x), 0 direct.  The 17 layers of the model (channel pairs of
# test_gpu_pyramid_convunit.C3 / C5) on a 160x192 slice at B = 1, the same at B = 8 (the top levels leave split-K) and 192x224 at B = 2
def _lv(H, W, l):
    return (1, H >> l, W >> l)


P1 = [
    (1, 2, 32, _lv(160, 192, 0), "d", "ds", 0), (1, 32, 32, _lv(160, 192, 0), "ds", "ds", 2), (1, 3, 32, _lv(160, 192, 1), "d", "ds", 0),
    (1, 32, 64, _lv(160, 192, 1), "ds", "ds", 2), (1, 64, 64, _lv(160, 192, 1), "ds", "ds", 2), (1, 96, 96, _lv(160, 192, 1), "ds", "ds", 2),
    (1, 160, 64, _lv(160, 192, 1), "ds", "d", 2), (1, 16, 96, _lv(160, 192, 1), "d", "ds", 2), (1, 32, 32, _lv(160, 192, 1), "ds", "ds", 2),
    (1, 64, 128, _lv(160, 192, 2), "ds", "ds", 2), (1, 128, 128, _lv(160, 192, 2), "ds", "ds", 2), (1, 96, 96, _lv(160, 192, 2), "ds", "ds", 2),
    (1, 224, 128, _lv(160, 192, 2), "ds", "ds", 2), (1, 128, 192, _lv(160, 192, 3), "ds", "ds", 0), (1, 192, 192, _lv(160, 192, 3), "ds", "ds", 0),
    (1, 288, 192, _lv(160, 192, 3), "ds", "ds", 0), (1, 192, 192, _lv(160, 192, 4), "ds", "ds", 0),
]
P8 = [
    (8, 2, 32, _lv(160, 192, 0), "d", "d", 0), (8, 32, 32, _lv(160, 192, 0), "d", "d", 2), (8, 3, 32, _lv(160, 192, 1), "d", "d", 0),
    (8, 32, 64, _lv(160, 192, 1), "d", "d", 2), (8, 64, 64, _lv(160, 192, 1), "d", "d", 2), (8, 96, 96, _lv(160, 192, 1), "d", "d", 2),
    (8, 160, 64, _lv(160, 192, 1), "d", "d", 2), (8, 16, 96, _lv(160, 192, 1), "d", "d", 2), (8, 32, 32, _lv(160, 192, 1), "d", "d", 2),
    (8, 64, 128, _lv(160, 192, 2), "ds", "ds", 2), (8, 128, 128, _lv(160, 192, 2), "ds", "ds", 2), (8, 96, 96, _lv(160, 192, 2), "d", "d", 2),
    (8, 224, 128, _lv(160, 192, 2), "ds", "d", 2), (8, 128, 192, _lv(160, 192, 3), "ds", "ds", 0), (8, 192, 192, _lv(160, 192, 3), "ds", "ds", 0),
    (8, 288, 192, _lv(160, 192, 3), "ds", "d", 0), (8, 192, 192, _lv(160, 192, 4), "ds", "ds", 0),
]
P2 = [
    (2, 2, 32, _lv(192, 224, 0), "d", "d", 0), (2, 32, 32, _lv(192, 224, 0), "d", "d", 2), (2, 3, 32, _lv(192, 224, 1), "d", "ds", 0),
    (2, 32, 64, _lv(192, 224, 1), "ds", "ds", 2), (2, 64, 64, _lv(192, 224, 1), "ds", "ds", 2), (2, 96, 96, _lv(192, 224, 1), "d", "d", 2),
    (2, 160, 64, _lv(192, 224, 1), "ds", "d", 2), (2, 16, 96, _lv(192, 224, 1), "d", "ds", 2), (2, 32, 32, _lv(192, 224, 1), "ds", "ds", 2),
    (2, 64, 128, _lv(192, 224, 2), "ds", "ds", 2), (2, 128, 128, _lv(192, 224, 2), "ds", "ds", 2), (2, 96, 96, _lv(192, 224, 2), "ds", "ds", 2),
    (2, 224, 128, _lv(192, 224, 2), "ds", "d", 2), (2, 128, 192, _lv(192, 224, 3), "ds", "ds", 0), (2, 192, 192, _lv(192, 224, 3), "ds", "ds", 0),
    (2, 288, 192, _lv(192, 224, 3), "ds", "ds", 0), (2, 192, 192, _lv(192, 224, 4), "ds", "ds", 0),
]
# ragged slices: sizes that are no multiple of the 8x8 tile (a last tile row / column of 1 pixel), a strip 9 pixels high; 6 -> 10 channels
# (no multiple of 4: scalar staging, the direct weight gradient)
RAGGED = [
    (1, 3, 32, (1, 97, 113), "d", "ds", 0), (1, 32, 32, (1, 97, 113), "ds", "ds", 2), (1, 16, 96, (1, 97, 113), "d", "ds", 2),
    (1, 192, 192, (1, 97, 113), "d", "d", 2), (1, 3, 32, (1, 33, 47), "d", "ds", 0), (1, 32, 32, (1, 33, 47), "ds", "ds", 2),
    (1, 16, 96, (1, 33, 47), "d", "ds", 2), (1, 192, 192, (1, 33, 47), "ds", "ds", 2), (1, 3, 32, (1, 9, 200), "d", "ds", 0),
    (1, 32, 32, (1, 9, 200), "ds", "ds", 2), (1, 16, 96, (1, 9, 200), "d", "ds", 2), (1, 192, 192, (1, 9, 200), "ds", "ds", 2),
    (2, 6, 10, (1, 33, 47), "d", "d", 0),
]
# both sides of the gates: 24x41 = 984 and 25x40 = 1000 pixels (WGRAD_WINO_MIN_VOXELS); 32 -> 32 with 7 x 73 = 511 and 16 x 32 = 512 tiles
# (conv_ksplit: the last shape at which split-K decides), and 8 -> 8 (one channel chunk: never split)
GATES = [
    (1, 32, 32, (1, 24, 41), "ds", "ds", 0), (1, 32, 32, (1, 25, 40), "ds", "ds", 2), (1, 8, 8, (1, 24, 41), "d", "d", 0), (1, 8, 8, (1, 25, 40), "d", "d", 2),
    (1, 32, 32, (1, 56, 584), "ds", "ds", 2), (1, 32, 32, (1, 128, 256), "d", "d", 2),
]
CONV_CASES = P1 + P8 + P2 + RAGGED + GATES


def test_slice_selection_gates_sit_where_the_cases_assume():
    """the gate cases really straddle the gates: pixel counts 984 / 1000, tile counts 511 / 512 of the direct kernel's 8x8 (y, x) tiles"""
    lib = _lib()
    assert 24 * 41 == 984 and 25 * 40 == 1000
    assert lib.query("pulpo_conv3d_k3_stat_tiles", 1, 1, 56, 584) == 511 and lib.query("pulpo_conv3d_k3_stat_tiles", 1, 1, 128, 256) == 512
    assert lib.query("pulpo_conv3d_k3_tile_config", 32, 32) % 1000 == 32          # one 32-wide output-channel tile: nblk = the tile count
    for case in CONV_CASES:                                                       # a slice never runs a Winograd forward / data gradient
        assert lib.query("pulpo_conv3d_k3_algo", case[0], *case[3], case[1], case[2]) == 0


@pytest.mark.parametrize("case", CONV_CASES, ids=_cid)
def test_slice_conv_layer_fp32_vs_float64(ops, case):
    """a: the <= 4-channel input layers take their image planar, as the step passes it"""
    B, Cin, Cout, size, ff, fd, wa = case
    assert size[0] == 1
    assert_families(*case)
    run_conv_case(ops, f"slice-conv {_cid(case)}", B, Cin, Cout, size, ff, fd, wa, form="planar" if Cin <= 4 else "cl")


@pytest.mark.parametrize("case", CONV_CASES[::3], ids=_cid)
def test_slice_conv_layer_bf16_operands_vs_float64(ops, case):
    """a: one case in three with bf16-representable operands through the bf16-operand kernels (test_conv_layer_bf16_operands_vs_float64)"""
    B, Cin, Cout, size, ff, fd, wa = case
    ops.set_conv_precision("bf16")
    try:
        assert ops._use_bf16(Cout) and ops._use_bf16(Cin) == (Cin > 4)
    finally:
        ops.set_conv_precision("fp32")
    run_conv_case(ops, f"slice-conv-bf16 {_cid(case)}", B, Cin, Cout, size, ff, fd, wa, form="planar" if Cin <= 4 else "cl", bf16=True)


# one layer per family as a channel slice of a wider channels-last buffer: (B, Cin, Cout, size, form, forward, data gradient, weight gradient
# algorithm, vec).  An unaligned slice is read with scalar loads and its weight gradient runs the direct kernel
SLICE_FORMS = [
    (1, 32, 32, (1, 40, 48), "aligned", "ds", "ds", 2, 1), (1, 32, 32, (1, 40, 48), "unaligned", "ds", "ds", 0, 0),
    (1, 32, 32, (1, 128, 256), "aligned", "d", "d", 2, 1), (1, 32, 32, (1, 128, 256), "unaligned", "d", "d", 0, 0),
]


@pytest.mark.parametrize("case", SLICE_FORMS, ids=lambda c: f"{_cid(c)}-{c[4]}")
def test_slice_conv_operand_forms_vs_float64(ops, case):
    B, Cin, Cout, size, form, ff, fd, wa, vec = case
    assert family(B, size, Cin, Cout) == ff and family(B, size, Cout, Cin) == fd
    assert _lib().query("pulpo_conv3d_k3_wgrad_algo", B, *size, Cin, Cout, vec) == wa
    run_conv_case(ops, f"slice-conv-form {_cid(case)} {form}", B, Cin, Cout, size, ff, fd, wa, form=form)


# ================================================================================================ b. the 4-D entries against slice_ref
# (B, Cin, Cout, H, W)
UNIT_CASES = [(2, 32, 32, 80, 96), (1, 2, 32, 160, 192), (3, 16, 96, 40, 48), (1, 192, 192, 10, 12), (2, 6, 10, 33, 47)]
_UNIT_DATA = {}


def _unit_data(case):
    """operands and upstream gradients of one case, on the CPU in float32 (made once per case and left unchanged)"""
    if case not in _UNIT_DATA:
        B, Cin, Cout, H, W = case
        g = torch.Generator().manual_seed(Cin * 100 + Cout + H)
        d = dict(x=torch.randn(B, Cin, H, W, generator=g), w=torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, b=torch.randn(Cout, generator=g),
                 gamma=torch.rand(Cout, generator=g) + 0.5, beta=torch.randn(Cout, generator=g) * 0.3, rm=torch.randn(Cout, generator=g) * 0.1,
                 rv=torch.rand(Cout, generator=g) + 0.5, up=torch.randn(B, Cout, H, W, generator=g))
        _UNIT_DATA[case] = d
    return _UNIT_DATA[case]


def _as_operand(t):
    """a (B, C, H, W) activation as the model passes it: channels-last from 5 channels up, the image pair planar"""
    t = t.to(DEV)
    return t.contiguous(memory_format=CL2) if t.shape[1] > 4 else t.contiguous()


def _walgo(B, Cin, Cout, H, W):
    return _lib().query("pulpo_conv3d_k3_wgrad_algo", B, 1, H, W, Cin, Cout, int(Cin % 4 == 0 and Cout % 4 == 0))


def _bound2(name, ref32, ref64, A, m, F=None):
    """T = m max(1, rho32) 2^-24 A (+ F), rho32 from the float32 evaluation (module docstring); all on the CPU, returned on the GPU"""
    A = A.clamp_min(1e-200)
    e = (ref32.double() - ref64).abs()
    if F is not None:
        e = (e - F).clamp_min(0)
    rho = float((e / (U * A)).max())
    print(f"RHO32 {name} {rho:.3g}")
    t = m * max(1.0, rho) * U * A
    return (t if F is None else t + F).to(DEV)


@pytest.mark.parametrize("case", UNIT_CASES, ids=lambda c: "B%d-%dto%d-%dx%d" % c)
def test_conv3d_k3_on_slices_vs_native_conv2d(ops, case):
    """b: ops.conv3d_k3 on (B, C, H, W) with a (Cout, Cin, 3, 3) weight - output, dx, dW (atomic and deterministic) and db against F.conv2d in
    float64.  The weight gradient comes back through _lift_w3's backward: the middle depth slice of the 3x3x3 gradient"""
    B, Cin, Cout, H, W = case
    d = _unit_data(case)
    x, w, b, dy = d["x"], d["w"], d["b"], d["up"]
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    name = "conv2d B%d %d->%d %dx%d" % case
    ref = S.conv2_ref(x64, w64, b64)
    t_out = _bound2(name + " out", S.conv2_ref(x, w, b), ref, S.conv2_mag(x64, w64, b64), M_FWD["d"])
    rdx, rdw = S.conv2_grads_ref(x64, w64, dy64)
    dx32, dw32 = S.conv2_grads_ref(x, w, dy)
    adx, adw = S.conv2_grads_mag(x64, w64, dy64)
    t_dx = _bound2(name + " dx", dx32, rdx, adx, M_FWD["d"])
    t_dw = _bound2(name + " dw", dw32, rdw, adw, M_WGRAD[_walgo(*case)])
    # db is torch's own channel sum of dy (no kernel of the library): twice the rho32 construction on sum |dy|
    rdb = dy64.sum(dim=(0, 2, 3))
    t_db = _bound2(name + " db", dy.sum(dim=(0, 2, 3)), rdb, dy64.abs().sum(dim=(0, 2, 3)), 2.0)
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            xg, wg, bg = _as_operand(x).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
            out = ops.conv3d_k3(xg, wg, bg)
            assert tuple(out.shape) == (B, Cout, H, W)
            gx, gw, gb = torch.autograd.grad(out, [xg, wg, bg], grad_outputs=_as_operand(dy))
        finally:
            ops.set_deterministic(det_default())
        assert tuple(gw.shape) == (Cout, Cin, 3, 3) and tuple(gx.shape) == (B, Cin, H, W)
        held(f"{name} det={det} out", out, ref.to(DEV), t_out)
        held(f"{name} det={det} dx", gx, rdx.to(DEV), t_dx)
        held(f"{name} det={det} dw", gw, rdw.to(DEV), t_dw)
        held(f"{name} det={det} db", gb, rdb.to(DEV), t_db)


def _unit_bounds(case, d, walgo):
    """float64 reference of the training-mode ConvUnit with the bound of every tensor (module docstring, 'Section b's ConvUnit bound')"""
    B, Cin, Cout, H, W = case
    n = B * H * W
    c = S._ch
    cs = lambda t: t.sum(dim=(0, 2, 3))
    cm = lambda t: t.mean(dim=(0, 2, 3))
    p64 = {k: v.double() for k, v in d.items()}
    args = lambda p: (p["x"], p["w"], p["b"], p["gamma"], p["beta"], p["rm"], p["rv"], p["up"])
    r, r32 = S.conv_unit_train_ref(*args(p64)), S.conv_unit_train_ref(*args(d))
    x, w, up, gamma, beta = p64["x"], p64["w"], p64["up"], p64["gamma"], p64["beta"]
    f = S.bn_train_ref(r["y"], gamma, beta)
    mean, var, rstd, scale = f["mean"], f["var"], f["rstd"], f["scale"]
    y, yc = r["y"], r["y"] - c(f["mean"])
    # ---- forward
    A_y = S.conv2_mag(x, w, p64["b"])
    a_mean = cm(A_y) + cm(y.abs())
    Ayc = A_y + c(a_mean)                                            # of y - mean
    a_var = 2 * cm(yc.abs() * Ayc) + cm(yc * yc)
    a_rstd = 0.5 * rstd ** 3 * a_var + rstd
    a_scale = gamma.abs() * a_rstd
    A_z = c(scale.abs()) * Ayc + yc.abs() * c(a_scale) + c(beta.abs()) + r["out"].abs()
    A = dict(out=A_z, running_mean=0.1 * a_mean + 0.9 * p64["rm"].abs() + 0.1 * mean.abs(),
             running_var=0.1 * n / (n - 1) * a_var + 0.9 * p64["rv"] + 0.1 * var * n / (n - 1))
    # ---- the LeakyReLU kink (F) and the backward
    m = M_FWD["d"]
    e_z = (r32["out"].double() - r["out"]).abs()
    rho_z = max(1.0, float((e_z / (U * A_z)).max()))
    near = (r["bn"].abs() <= m * rho_z * U * A_z) & (r["bn"] != 0)
    print(f"unit {case}: {int(near.sum())} of {near.numel()} pixels within the bound of the LeakyReLU kink")
    flip = 0.8 * up.abs() * near
    dbn = torch.where(r["bn"] > 0, up, 0.2 * up)
    s1, s2 = cs(dbn), cs(dbn * yc)
    A_s1, F_s1 = cs(dbn.abs()), cs(flip)
    A_s2, F_s2 = cs(dbn.abs() * (yc.abs() + Ayc)), cs(flip * yc.abs())
    r2 = rstd * rstd
    inner = dbn.abs() + c(s1.abs() + A_s1) / n + (Ayc * c(r2 * s2.abs()) + yc.abs() * c(2 * rstd * a_rstd * s2.abs() + r2 * A_s2) + yc.abs() * c(r2 * s2.abs())) / n
    A_dy = c(scale.abs()) * inner + c(a_scale / scale.abs()) * r["dy"].abs()
    F_dy = c(scale.abs()) * (flip + c(F_s1) / n + yc.abs() * c(r2 * F_s2) / n)
    mag_dx, mag_dw = S.conv2_grads_mag(x, w, r["dy"])
    car_dx, car_dw = S.conv2_grads_ref(x.abs(), w.abs(), A_dy)
    F_dx, F_dw = S.conv2_grads_ref(x.abs(), w.abs(), F_dy)
    A.update(dx=mag_dx + car_dx, dw=mag_dw + car_dw, dgamma=a_rstd * s2.abs() + rstd * A_s2, dbeta=A_s1)
    Fk = dict(dx=F_dx, dw=F_dw, dgamma=rstd * F_s2, dbeta=F_s1)
    ms = dict(dw=max(M_WGRAD[walgo], m))
    name = "unit B%d %d->%d %dx%d" % case
    tol = {k: _bound2(f"{name} {k}", r32[k], r[k], A[k], ms.get(k, m), Fk.get(k)) for k in A}
    return r, tol


@pytest.mark.parametrize("case", UNIT_CASES, ids=lambda c: "B%d-%dto%d-%dx%d" % c)
def test_conv_unit_on_slices_vs_slice_ref(ops, case):
    """b: ops.conv_bn_lrelu on (B, C, H, W) in training mode - output, running statistics and num_batches_tracked, dx, dW, dgamma, dbeta (the
    convolution's bias gradient to 1e-3 of the weight gradient's scale: its true value is 0) - and in eval mode, where convolution,
    BatchNorm and LeakyReLU run as one kernel, against the native 2-D definitions in float64"""
    B, Cin, Cout, H, W = case
    d = _unit_data(case)
    name = "unit B%d %d->%d %dx%d" % case
    r, tol = _unit_bounds(case, d, _walgo(*case))
    P = lambda k: d[k].to(DEV).clone().requires_grad_(True)
    xg, wg, bg, gg, btg = _as_operand(d["x"]).requires_grad_(True), P("w"), P("b"), P("gamma"), P("beta")
    rm, rv, nbt = d["rm"].to(DEV).clone(), d["rv"].to(DEV).clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    out = ops.conv_bn_lrelu(xg, wg, bg, gg, btg, rm, rv, True, 0.1, 1e-5, nbt)
    assert tuple(out.shape) == (B, Cout, H, W) and int(nbt) == 1
    grads = torch.autograd.grad(out, [xg, wg, bg, gg, btg], grad_outputs=_as_operand(d["up"]))
    assert [tuple(t.shape) for t in grads] == [(B, Cin, H, W), (Cout, Cin, 3, 3), (Cout,), (Cout,), (Cout,)]
    held(name + " out", out, r["out"].to(DEV), tol["out"])
    held(name + " running_mean", rm, r["running_mean"].to(DEV), tol["running_mean"])
    held(name + " running_var", rv, r["running_var"].to(DEV), tol["running_var"])
    for k, got in zip(("dx", "dw", "dgamma", "dbeta"), (grads[0], grads[1], grads[3], grads[4])):
        held(f"{name} {k}", got, r[k].to(DEV), tol[k])
    assert amax(grads[2]) <= 1e-3 * max(1e-3, amax(r["dw"]))
    # ---- eval mode with the updated running statistics: one kernel; z = lrelu((y - rm) s + beta), s = gamma / sqrt(rv + eps)
    p64 = {k: v.double() for k, v in d.items()}
    rm64, rv64 = r["running_mean"], r["running_var"]
    e64 = S.conv_unit_eval_ref(p64["x"], p64["w"], p64["b"], p64["gamma"], p64["beta"], rm64, rv64)
    e32 = S.conv_unit_eval_ref(d["x"], d["w"], d["b"], d["gamma"], d["beta"], rm64.float(), rv64.float())
    s = (p64["gamma"] * (rv64 + 1e-5).rsqrt()).abs()
    A_e = S._ch(s) * (S.conv2_mag(p64["x"], p64["w"], p64["b"]) + S._ch(rm64.abs())) + S._ch(p64["beta"].abs()) + e64.abs()
    rmk, rvk = rm64.float().to(DEV), rv64.float().to(DEV)
    with torch.no_grad():
        oe = ops.conv_bn_lrelu(_as_operand(d["x"]), wg.detach(), bg.detach(), gg.detach(), btg.detach(), rmk, rvk, False)
    assert torch.equal(rmk, rm64.float().to(DEV)) and torch.equal(rvk, rv64.float().to(DEV))
    held(name + " eval out", oe, e64.to(DEV), _bound2(name + " eval out", e32, e64, A_e, M_FWD["d"]))


# (B, C, H, W): the pooled activations and images of a slice pyramid, odd heights and widths (edge windows of 2 pixels, a corner of 1), H = 1
POOL_CASES = [(2, 32, 80, 96), (1, 1, 160, 192), (3, 96, 40, 48), (1, 192, 10, 12), (2, 6, 33, 47), (1, 1, 33, 47), (2, 32, 5, 7), (1, 8, 1, 9)]


@pytest.mark.parametrize("B,C,H,W", POOL_CASES, ids=lambda v: str(v))
def test_avg_pool2_on_slices_vs_native_avg_pool2d(ops, B, C, H, W):
    """b: avg_pool2 / avg_pool2_skip on (B, C, H, W) against F.avg_pool2d(2, 2, ceil_mode=True): the lifted depth is a ceil-mode window of one
    plane, (D + 1) // 2 == 1.  An average of at most 4 terms: m = 8 as in 3-D (test_avg_pool2_and_skip_vs_float64); backward m = 2"""
    g = torch.Generator().manual_seed(C + H + B)
    x = torch.randn(B, C, H, W, generator=g)
    name = f"pool2d B{B} C{C} {H}x{W}"
    x64 = x.double().requires_grad_(True)
    ref = S.avgpool2_ref(x64)
    up = torch.randn(ref.shape, generator=g)
    gskip = torch.randn(B, C, H, W, generator=g)
    rg, = torch.autograd.grad((ref * up.double()).sum(), [x64])
    xa = x.double().abs().requires_grad_(True)
    refa = S.avgpool2_ref(xa)
    ag, = torch.autograd.grad((refa * up.double().abs()).sum(), [xa])
    x32 = x.clone().requires_grad_(True)
    ref32 = S.avgpool2_ref(x32)
    g32, = torch.autograd.grad((ref32 * up).sum(), [x32])
    tol = _bound2(name + " out", ref32.detach(), ref.detach(), refa.detach(), 8.0)
    tol_g = _bound2(name + " gin", g32, rg, ag, 2.0)
    tol_gs = _bound2(name + " gin+skip", g32 + gskip, rg + gskip.double(), ag + gskip.double().abs(), 2.0)
    ref, rg = ref.detach().to(DEV), rg.to(DEV)
    xo, upo, gso = _as_operand(x), _as_operand(up), _as_operand(gskip)
    xg = xo.clone().requires_grad_(True)
    out = ops.avg_pool2(xg)
    assert tuple(out.shape) == (B, C, (H + 1) // 2, (W + 1) // 2)
    held(name + " out", out, ref, tol)
    gin, = torch.autograd.grad(out, [xg], grad_outputs=upo)
    held(name + " gin", gin, rg, tol_g)
    for both in ("pool+skip", "pool", "skip"):
        xg = xo.clone().requires_grad_(True)
        alias, pooled = ops.avg_pool2_skip(xg)
        assert torch.equal(alias, xo) and tuple(pooled.shape) == tuple(ref.shape)
        held(name + " skip-form out", pooled, ref, tol)
        loss = (pooled * upo).sum() if both != "skip" else 0
        loss = loss + ((alias * gso).sum() if both != "pool" else 0)
        gin, = torch.autograd.grad(loss, [xg])
        if both == "skip":
            assert torch.equal(gin, gso)
        else:
            held(f"{name} {both} gin", gin, rg + gso.double() if both == "pool+skip" else rg, tol_gs if both == "pool+skip" else tol_g)


# ================================================================================================ c. heads with two latent channels
def _heads2d_vs_ref(ops, name, h, params, nout, eps, g):
    """outputs, dh, dW and db of the 2-D heads against the float64 evaluation, at the 1e-5 scale bounds of test_gpu_pyramid_ops._heads_vs_ref;
    the padded zero row of the three-row kernel never leaks: two output channels, parameter gradients of the parameters' own shapes"""
    B, C, H, W = h.shape
    ups = [torch.randn(B, 2, H, W, device=DEV, generator=g) for _ in range(1 if nout == 3 else 3)]
    hg = h.detach().requires_grad_(True)
    pg = [p.detach().clone().requires_grad_(True) for p in params]
    outs = (ops.conv1x1_to3(hg, *pg),) if nout == 3 else ops.mu_sigma_sample(hg, *pg, eps)
    assert len(outs) == len(ups) and all(tuple(o.shape) == (B, 2, H, W) for o in outs)
    grads = torch.autograd.grad(sum((o * u).sum() for o, u in zip(outs, ups)), [hg] + pg)
    assert tuple(grads[0].shape) == (B, C, H, W) and [tuple(t.shape) for t in grads[1:]] == [tuple(p.shape) for p in params]
    h64 = h.detach().double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    routs = (S.conv1x1_ref(h64, *p64),) if nout == 3 else S.mu_sigma_ref(h64, *p64, eps.double() if eps is not None else None)
    rgrads = torch.autograd.grad(sum((o * u.double()).sum() for o, u in zip(routs, ups)), [h64] + p64)
    for k, (o, ro) in enumerate(zip(outs, routs)):
        check(f"heads2d {name} out{k}", o, ro.detach(), 1e-5 * max(1.0, amax(ro)))
    if nout == 6 and eps is None:
        assert torch.equal(outs[2], outs[0])
    check(f"heads2d {name} dh", grads[0], rgrads[0], 1e-5 * max(1.0, amax(rgrads[0])))
    for k, (gp, rp) in enumerate(zip(grads[1:], rgrads[1:])):
        check(f"heads2d {name} {'dW' if k % 2 == 0 else 'db'}{k // 2}", gp, rp, 1e-5 * max(1.0, amax(rp)))


@pytest.mark.parametrize("B,H,W", [(1, 80, 96), (2, 17, 23)])
@pytest.mark.parametrize("C", [32, 96, 10, 3])
@pytest.mark.parametrize("nout,noise", [(6, True), (6, False), (3, False)], ids=["musigma-eps", "musigma-eps_none", "to3"])
def test_heads_on_slices_vs_float64(ops, nout, noise, C, B, H, W):
    """c: mu_sigma_sample with zdim = 2 (rows (0, mu_y, mu_x, 0, sigma_y, sigma_x) of the three-component kernel), with noise and with eps = None,
    and the 2-D conv1x1_to3; vector (C % 4 == 0) and scalar channel counts; 17x23 at B = 2: a pixel count that is no multiple of the block's trip"""
    g = gen(C * 7 + B + H + nout)
    h = torch.randn(B, C, H, W, device=DEV, generator=g)
    h = h.contiguous(memory_format=CL2) if C > 4 else h
    w = lambda: torch.randn(2, C, 1, 1, device=DEV, generator=g) / C ** 0.5
    b = lambda: torch.randn(2, device=DEV, generator=g)
    params = [w(), b()] if nout == 3 else [w(), b(), w(), b()]
    eps = torch.randn(B, 2, H, W, device=DEV, generator=g) if (nout == 6 and noise) else None
    _heads2d_vs_ref(ops, f"{nout}/B{B}/{H}x{W}/C{C}/{'eps' if noise else 'none'}", h, params, nout, eps, g)


# ================================================================================================ d. resize
def _resize2d_vs_ref(ops, name, x, size, mult, add, sf, det, exact):
    g = torch.randn(x.shape[0], x.shape[1], *size, device=DEV, generator=gen(sum(size) + det))
    ops.set_deterministic(det)
    try:
        xg = x.clone().requires_grad_(True)
        out = ops.resize_trilinear(xg, size, mult, add, sf)
        gx, = torch.autograd.grad((out * g).sum(), [xg])
    finally:
        ops.set_deterministic(det_default())
    assert tuple(out.shape) == tuple(x.shape[:2]) + tuple(size)

    def ref_of(t):
        tg = t.clone().requires_grad_(True)
        o = mult * (S.resize_ref(tg, size=size) if sf is None else S.resize_ref(tg, scale_factor=sf))
        assert tuple(o.shape[2:]) == tuple(size)
        if add is not None:
            o = o + add.to(o.dtype)
        return o.detach(), torch.autograd.grad((o * g.to(o.dtype)).sum(), [tg])[0]

    ro, rg = ref_of(x.double())
    so, sgx = ref_of(x)                       # torch's own fp32 operator: the spread fp32 source coordinates give
    base_o, base_g = 1e-5 * max(1.0, amax(ro)), 1e-5 * max(1.0, amax(rg))
    print(f"RATIO resize2d {name} spread32 out {R.ratio(so, ro, 1.0):.3g} grad {R.ratio(sgx, rg, 1.0):.3g}")
    tol_o = base_o if exact else max(base_o, 2 * R.ratio(so, ro, 1.0))
    tol_g = base_g if exact else max(base_g, 2 * R.ratio(sgx, rg, 1.0))
    check(f"resize2d {name} det={det} out", out, ro, tol_o)
    check(f"resize2d {name} det={det} grad", gx, rg, tol_g)


# (B, C, in, out, mult, add, scale_factor, exact coordinates): the exact x2 80x96 -> 160x192 with mult and the fused add, scale_factor 0.5 from
# odd sizes (159x191, 97x113: 1 / scale is the step, not in / out), a generic ratio up and down
RESIZE2D = [(1, 2, (80, 96), (160, 192), 2.0, True, None, True), (2, 2, (80, 96), (160, 192), 1.0, False, None, True),
            (1, 2, (159, 191), (79, 95), 0.5, False, 0.5, True), (2, 2, (97, 113), (48, 56), 0.5, True, 0.5, True),
            (2, 2, (24, 28), (40, 33), 1.5, True, None, False), (1, 3, (24, 28), (40, 33), 1.0, False, None, False)]


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,C,isz,osz,mult,with_add,sf,exact", RESIZE2D)
def test_resize_on_slices_vs_native_bilinear(ops, B, C, isz, osz, mult, with_add, sf, exact, det):
    """d: resize_trilinear on (B, C, H, W) against bilinear F.interpolate in float64, the size= and the scale_factor= form; backward by float
    atomics and by the deterministic gather.  Bounds as test_resize_vs_float64: x2 and x0.5 coordinates are exact in fp32 (its fixed
    bound), other ratios are held to twice torch's fp32 spread on the same data"""
    g = gen(sum(isz) + B + C)
    x = torch.randn(B, C, *isz, device=DEV, generator=g)
    add = torch.randn(B, C, *osz, device=DEV, generator=g) if with_add else None
    _resize2d_vs_ref(ops, f"B{B}/C{C}/{isz}->{osz}/sf{sf}/m{mult}", x, osz, mult, add, sf, det, exact)


@pytest.mark.parametrize("B,isz,osz,exact", [(1, (40, 48), (80, 96), True), (2, (17, 24), (33, 47), False)])
def test_slice_feedback_path_resizes_and_concatenates(ops, B, isz, osz, exact):
    """d: Autoencoder._gather_feedback on slices always takes the resize-and-concatenate branch (feedback_up2 is the volumes' kernel): two
    sources (a 2-channel sample, the 1-channel transformed image) against cat(bilinear resize) in float64, values and both source gradients"""
    from pulpo_amd.components.pulpo import Autoencoder
    g = gen(isz[0] + osz[1] + B)
    srcs = [torch.randn(B, c, *isz, device=DEV, generator=g) for c in (2, 1)]
    up = torch.randn(B, 3, *osz, device=DEV, generator=g)
    sg = [s.clone().requires_grad_(True) for s in srcs]
    me = types.SimpleNamespace(feedback=["samples", "transformed"])
    fb = Autoencoder._gather_feedback(me, {"samples": {1: sg[0]}, "transformed": {1: sg[1]}}, 1, osz)
    assert tuple(fb.shape) == (B, 3, *osz) and fb.is_contiguous(memory_format=CL2)
    got = torch.autograd.grad((fb * up).sum(), sg)

    def ref_of(ts):
        tg = [t.clone().requires_grad_(True) for t in ts]
        o = torch.cat([S.resize_ref(t, size=osz) for t in tg], dim=1)
        return (o.detach(),) + torch.autograd.grad((o * up.to(o.dtype)).sum(), tg)

    r64, r32 = ref_of([s.double() for s in srcs]), ref_of(srcs)
    for k, (a, r, s32) in enumerate(zip((fb,) + got, r64, r32)):
        base = 1e-5 * max(1.0, amax(r))
        check(f"feedback2d B{B} {isz}->{osz} {'out' if k == 0 else 'gsrc%d' % (k - 1)}", a, r, base if exact else max(base, 2 * R.ratio(s32, r, 1.0)))


# ================================================================================================ e. warp, warp_mask, VecInt
def _warp_field2d(g, B, grid, img, amp, kind):
    """test_gpu_pyramid_ops._warp_field in 2-D: 'faces' pushes the samples of all four edges out of the image (clamped: border padding) and
    puts slabs of samples exactly on the border indices 0 and S - 1 and on an interior integer:
    c = (p + d) S_i / (S_g - 1) - 0.5 = k  <=>  d = (k + 0.5) (S_g - 1) / S_i - p"""
    df = torch.randn(B, 2, *grid, device=DEV, generator=g) * amp
    if kind == "faces":
        for a in range(2):
            n = grid[a]
            sl = [slice(None)] * 4
            sl[1] = a
            sl[2 + a] = slice(0, 3)
            df[tuple(sl)] -= 2.5 * amp
            sl[2 + a] = slice(n - 3, n)
            df[tuple(sl)] += 2.5 * amp
        for a in range(2):
            pos = torch.arange(grid[a], device=DEV, dtype=torch.float64)
            shape = [1, 1]
            shape[a] = -1
            for j, kk in enumerate((0.0, img[a] - 1.0, float(img[a] // 2))):
                d = ((kk + 0.5) * (grid[a] - 1) / img[a] - pos).reshape(shape).expand(*grid).float()
                slab = [slice(None)] * 2
                slab[(a + 1) % 2] = slice(4 * j, 4 * j + 2)
                df[(slice(None), a) + tuple(slab)] = d[tuple(slab)]
    return df


def _warp2d_ref_grads(df, img, up):
    d, i = df.clone().requires_grad_(True), img.clone().requires_grad_(True)
    out = S.warp_ref(d, i)
    return (out.detach(),) + torch.autograd.grad((out * up).sum(), [d, i])


# (B, grid, image, C, amplitude, field): grid = image at 160x192, an image larger than the grid (40x48 grid, 160x192 image), C = 2 (the
# self-warp of a field), samples clamped at all four edges with slabs exactly on the border indices, ragged 33x47
WARP2D = [(1, (160, 192), (160, 192), 1, 2.0, "rand"), (1, (40, 48), (160, 192), 1, 2.0, "rand"), (2, (80, 96), (80, 96), 2, 3.0, "rand"),
          (1, (40, 48), (40, 48), 1, 4.0, "faces"), (2, (33, 47), (33, 47), 2, 3.0, "faces")]


@pytest.mark.parametrize("B,grid,isize,C,amp,kind", WARP2D)
def test_warp_on_slices_vs_native_grid_sample(ops, B, grid, isize, C, amp, kind):
    """e: ops.warp3d on (B, 2, H, W) fields - forward, gdf, gimg through the atomic and the deterministic kernel - and warp_mask, against the
    2-D SpatialTransformer of slice_ref in float64.  The construction of test_warp_vs_float64: outputs and the image gradient at twice the
    spread of torch's fp32 grid_sample on the same data (at least 1e-5); pixels whose float64 sample coordinate lies within 1e-4 of a cell
    boundary or a clamp may take the other cell, where gdf jumps: there gdf is bounded by what a displacement 2e-4 pixel to either side
    gives in float64.  Random fields must keep that set under 1 % of the elements"""
    g = gen(grid[0] + 7 * C + B)
    df = _warp_field2d(g, B, grid, isize, amp, kind)
    img = torch.rand(B, C, *isize, device=DEV, generator=g)
    up = torch.randn(B, C, *grid, device=DEV, generator=g)
    ref = _warp2d_ref_grads(df.double(), img.double(), up.double())
    r32 = _warp2d_ref_grads(df, img, up)
    c = S.warp_coords(df.double(), isize)
    his = torch.tensor(isize, device=DEV, dtype=torch.float64).reshape(2, 1, 1, 1) - 1
    near = ((c - c.round()).abs() < 1e-4) | ((c - his).abs() < 1e-4) | (c.abs() < 1e-4)
    bnd = near.any(0).unsqueeze(1).expand(B, 2, *grid)
    if kind == "faces":          # samples beyond both edges of every axis, and on the border indices
        assert bool((c < 0).flatten(1).any(1).all()) and bool((c > his).flatten(1).any(1).all()) and int(bnd.sum()) > 0
    else:
        assert int(bnd.sum()) < 0.01 * bnd.numel()
    nudge = torch.zeros_like(ref[1])
    for a in range(2):
        for sgn in (1.0, -1.0):
            d = df.double().clone()
            d[:, a] += sgn * 2e-4 * (grid[a] - 1) / isize[a]
            nudge = torch.maximum(nudge, (_warp2d_ref_grads(d, img.double(), up.double())[1] - ref[1]).abs())
    tol_out = max(1e-5 * max(1.0, amax(ref[0])), 2 * R.ratio(r32[0], ref[0], 1.0))
    tol_img = max(1e-5 * max(1.0, amax(ref[2])), 2 * R.ratio(r32[2], ref[2], 1.0))
    tol_df = max(1e-5 * max(1.0, amax(ref[1])), 2 * float((r32[1] - ref[1]).abs()[~bnd].max()))
    tol_df_t = torch.where(bnd, tol_df + nudge, torch.full_like(nudge, tol_df))
    last_inner = int(torch.nonzero(~bnd.reshape(-1)).reshape(-1)[-1])
    tag = f"warp2d B{B}/{grid}/{isize}/C{C}/{kind}"
    print(f"RATIO {tag} spread32 out {R.ratio(r32[0], ref[0], 1.0):.3g} gdf {tol_df:.3g} gimg {tol_img:.3g} boundary pixels {int(bnd[:, 0].sum())}")
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dfg, imgg = df.clone().requires_grad_(True), img.clone().requires_grad_(True)
            out = ops.warp3d(dfg, imgg)
            gdf, gimg = torch.autograd.grad((out * up).sum(), [dfg, imgg])
        finally:
            ops.set_deterministic(det_default())
        assert tuple(out.shape) == (B, C, *grid) and tuple(gdf.shape) == (B, 2, *grid)
        check(f"{tag} det={det} out", out, ref[0], tol_out)
        print(f"RATIO {tag} det={det} gdf(off the boundaries) {R.ratio(gdf[~bnd], ref[1][~bnd], tol_df):.3g}")
        check(f"{tag} det={det} gdf", gdf, ref[1], tol_df_t, power=last_inner)
        check(f"{tag} det={det} gimg", gimg, ref[2], tol_img)
    # warp_mask: the same sample positions; a mask of ones stays exactly ones, any other mask is the warp of that mask
    ones = ops.warp_mask(df, torch.ones(B, 1, *isize, device=DEV))
    assert tuple(ones.shape) == (B, 1, *grid) and bool((ones == 1).all())
    mask = torch.rand(B, 1, *isize, device=DEV, generator=g)
    rm = S.warp_ref(df.double(), mask.double())
    check(f"{tag} mask", ops.warp_mask(df, mask), rm, max(1e-5, 2 * R.ratio(S.warp_ref(df, mask), rm, 1.0)))


@pytest.mark.parametrize("B,H,W,amp", [(1, 80, 96, 3.0), (2, 33, 47, 2.0)])
def test_vecint_on_slices_vs_float64(ops, B, H, W, amp):
    """e: VecInt (7 squaring steps) on (B, 2, H, W), forward and backward (atomic and deterministic), and vecint_pair under no_grad, against
    scaling and squaring through the 2-D SpatialTransformer in float64.  The output element by element at twice the spread of the same
    definition evaluated in fp32 (at least 1e-5); the bounds of test_vecint_backward_lds_tiled_scatter_vs_oracle: output relative L2 1e-5,
    gradient relative L2 max(1e-4, 3 x the fp32 evaluation's) - a rough field puts sample coordinates within rounding of a cell boundary,
    where the gradient jumps, and the fp32 evaluation of the same operator sets the scale of that effect"""
    g = gen(H + W + B)
    v = torch.randn(B, 2, H, W, device=DEV, generator=g) * amp
    up = torch.randn(B, 2, H, W, device=DEV, generator=g)
    vr = v.double().requires_grad_(True)
    ref = S.vecint_ref(vr, 7)
    gr, = torch.autograd.grad((ref * up.double()).sum(), [vr])
    v32 = v.clone().requires_grad_(True)
    ref32 = S.vecint_ref(v32, 7)
    g32, = torch.autograd.grad((ref32 * up).sum(), [v32])
    ref = ref.detach()
    tol = max(1e-5 * max(1.0, amax(ref)), 2 * R.ratio(ref32.detach(), ref, 1.0))
    name = f"vecint2d B{B} {H}x{W}"
    print(f"RATIO {name} spread32 out {R.ratio(ref32.detach(), ref, 1.0):.3g} grad rel-L2 of fp32 {rel_l2(g32, gr):.3g}")
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            vg = v.clone().requires_grad_(True)
            out = ops.vecint(vg, 7)
            gv, = torch.autograd.grad((out * up).sum(), [vg])
        finally:
            ops.set_deterministic(det_default())
        assert tuple(out.shape) == (B, 2, H, W) and tuple(gv.shape) == (B, 2, H, W)
        check(f"{name} det={det} out", out, ref, tol)
        assert rel_l2(out, ref) < 1e-5
        e = rel_l2(gv, gr)
        print(f"RATIO {name} det={det} grad rel-L2 {e:.3g}")
        assert e < max(1e-4, 3.0 * rel_l2(g32, gr))
    with torch.no_grad():
        fwd, inv = ops.vecint_pair(v, 7)
        rinv = S.vecint_ref(-v.double(), 7)
        tol_i = max(1e-5 * max(1.0, amax(rinv)), 2 * R.ratio(S.vecint_ref(-v, 7), rinv, 1.0))
    check(f"{name} pair fwd", fwd, ref, tol)
    check(f"{name} pair inv", inv, rinv, tol_i)


# ================================================================================================ f. a reference step at 80x96
STEP = "step2d_T4L3_n4_80x96"


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb


def _golden_model(api, g, **kw):
    """the fixture's model with its weights and noise, in training mode"""
    models, nb = api
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    assert len(size) == 2
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0, **kw)
    sd = model.state_dict()
    loaded = 0
    for k, v in g.items():
        if k.startswith("sd0."):
            assert k[4:] in sd and tuple(sd[k[4:]].shape) == v.shape, k
            sd[k[4:]] = T(v.copy())
            loaded += 1
    assert loaded > 50
    model.load_state_dict(sd)
    model = model.cuda().train()
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(T(g[f"eps.{l}"]).cuda())
    return model, T(g["x"]).cuda(), T(g["y"]).cuda()


def _is_noise_bias(k):
    """a convolution bias in front of a BatchNorm: its true gradient is zero"""
    return k.endswith("_op.0.bias") and "velocity_field._op.2" not in k


def test_slice_step_fixture_reaches_the_slice_kernels(golden):
    """the fixture is large enough: from the library's queries for this model's own layer shapes (n0 = 4 on 80x96, B = 1: 8 -> 8 and 16 -> 8 at
    40x48 - latent level 0 -, 24 -> 16 at 20x24 - latent level 1 -, the image pair's 2 -> 4 at 80x96) it runs the (y, x) Winograd weight
    gradient, the split-K direct forward and the narrow-input weight gradient.  Otherwise the fixture has the wrong size"""
    g = golden(STEP)
    lib = _lib()
    Tl, L, n0, B, H, W = [int(v) for v in g["cfg"]]
    assert (Tl, L, n0, B, H, W) == (4, 3, 4, 1, 80, 96)
    shp = lambda k: tuple(g["sd0." + k + "._op.0.weight"].shape[:2])
    assert shp("downpath.down_blocks.1._op.1") == (8, 8) and shp("autoencoder.encoders.0.sample_merge_block._op.0") == (8, 16)
    assert lib.query("pulpo_conv3d_k3_wgrad_algo", B, 1, H // 2, W // 2, 8, 8, 1) == 2 and lib.query("pulpo_conv3d_k3_wgrad_algo", B, 1, H // 2, W // 2, 16, 8, 1) == 2
    assert shp("autoencoder.encoders.1.sample_merge_block._op.0") == (16, 24)
    assert family(B, (1, H // 4, W // 4), 24, 16) == "ds"
    # (conv3d_wgrad.hip: up to 4 input channels with a vectorisable gradient operand - Cout a multiple of 4 - take the kernel of the input layers)
    cout, cin = shp("downpath.down_blocks.0._op.0")
    assert (cout, cin) == (4, 2) and cin <= 4 and cout % 4 == 0 and lib.query("pulpo_conv3d_k3_wgrad_algo", B, 1, H, W, cin, cout, 0) == 0


def test_slice_training_step_matches_reference_golden(api, golden):
    """f: the reference's training step on 80x96 slices (T = 4, L = 3) replayed at the tolerances of
    test_gpu_2d.test_training_step_2d_matches_reference_golden: outputs 1e-4 max(1, |ref|), losses rtol 1e-4, parameter gradients relative L2
    1e-3, running statistics 1e-5, the eval and deterministic forwards 1e-4"""
    g = golden(STEP)
    model, x, y = _golden_model(api, g)
    L = int(g["cfg"][1])
    outs, _, (total, kl, rec, reg), levels = model._forward_and_losses(x, y)
    for name, d in zip(OUT, outs):
        for l, v in d.items():
            ref = g[f"train.{name}.{l}"]
            assert tuple(v.shape) == ref.shape, (name, l, v.shape, ref.shape)
            err = np.abs(v.detach().cpu().numpy() - ref).max()
            print(f"RATIO slice-step train.{name}.{l} {err / (1e-4 * max(1.0, np.abs(ref).max())):.3g}")
            assert err <= 1e-4 * max(1.0, np.abs(ref).max()), (name, l, err)
    for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
        np.testing.assert_allclose(float(val), float(g["train." + key]), rtol=1e-4)
    total.backward()
    checked, worst = 0, 0.0
    for k, p in model.named_parameters():
        if "grad." + k in g:
            ref = g["grad." + k]
            if _is_noise_bias(k):
                wref = np.abs(g["grad." + k[:-4] + "weight"]).max()
                assert np.abs(p.grad.cpu().numpy()).max() <= 1e-3 * max(wref, 1e-3), k
                continue
            assert tuple(p.grad.shape) == ref.shape
            worst = max(worst, rel_l2(p.grad, ref))
            assert rel_l2(p.grad, ref) < 1e-3, (k, rel_l2(p.grad, ref))
            checked += 1
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    print(f"RATIO slice-step parameter gradients rel-L2 {worst / 1e-3:.3g}")
    assert checked > 60
    sd1 = model.state_dict()
    nstat = 0
    for k, v in g.items():
        if k.startswith("sd1."):
            np.testing.assert_allclose(sd1[k[4:]].cpu().numpy(), v, atol=1e-5, rtol=1e-5)
            nstat += 1
    assert nstat > 60
    model.eval()
    with torch.no_grad():
        outs_e, _, (tot_e, kl_e, rec_e, reg_e), _ = model._forward_and_losses(x, y)
        for key, val in zip(("total", "kl", "rec", "reg"), (tot_e, kl_e, rec_e, reg_e)):
            np.testing.assert_allclose(float(val), float(g["eval." + key]), rtol=1e-4)
        for name in ("transformed", "individual_dfs"):
            for l, v in outs_e[OUT.index(name)].items():
                np.testing.assert_allclose(v.cpu().numpy(), g[f"eval.{name}.{l}"], atol=1e-4)
        det_out, det_ind = model.predict_deterministic(x, y)
        assert len(det_out) == L
        for l in det_out:
            np.testing.assert_allclose(det_out[l].cpu().numpy(), g[f"det.transformed.{l}"], atol=1e-4)
            np.testing.assert_allclose(det_ind[l].cpu().numpy(), g[f"det.individual_dfs.{l}"], atol=1e-4)


def _grads_of_one_step(model, x, y):
    for p in model.parameters():
        p.grad = None
    _, _, (total, _, _, _), _ = model._forward_and_losses(x, y)
    total.backward()
    torch.cuda.synchronize()
    return float(total), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_slice_step_deterministic_mode_gives_bit_identical_gradients(api, golden):
    """f (test_deterministic_mode_gives_bit_identical_gradients on slices): two evaluations of the step in deterministic mode give bit-identical
    losses and parameter gradients - the (y, x) weight gradient's ordered slabs at depth 1, the warp / VecInt fixed-point scatter and the resize
    gather of the feedback path; the plain mode is held to it at 1e-5 relative L2 (atomic order only)"""
    from pulpo_amd import ops
    g = golden(STEP)
    model, x, y = _golden_model(api, g)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        ops.set_deterministic(True)
        runs = []
        for _ in range(2):
            model.load_state_dict(state)                # (BatchNorm running statistics move with every training forward)
            runs.append(_grads_of_one_step(model, x, y))
        assert runs[1][0] == runs[0][0] and runs[1][1].keys() == runs[0][1].keys() and len(runs[0][1]) > 60
        for k, gk in runs[1][1].items():
            assert torch.equal(gk, runs[0][1][k]), (k, float((gk - runs[0][1][k]).abs().max()))
        ops.set_deterministic(False)
        model.load_state_dict(state)
        loss_p, grads_p = _grads_of_one_step(model, x, y)
        assert loss_p == runs[0][0]                      # (the forward pass has no atomics in either mode)
        for k, gk in grads_p.items():
            if not _is_noise_bias(k):
                assert rel_l2(gk, runs[0][1][k]) < 1e-5, (k, rel_l2(gk, runs[0][1][k]))
    finally:
        ops.set_deterministic(det_default())


def test_slice_step_stepper_equals_autograd_and_adam(api, golden):
    """f (test_fused_adam_arena_step_matches_torch_adam on slices): two steps of dp.DataParallelStepper equal two steps of plain autograd +
    torch.optim.Adam, parameter for parameter, at that test's tolerance.  The lifted 3x3 weights are non-leaf tensors: their gradients reach
    the parameter arena through autograd's accumulation instead of the direct slots, and their packs are rebuilt on every call"""
    from pulpo_amd.dp import DataParallelStepper
    g = golden(STEP)
    a, x, y = _golden_model(api, g, lr=1e-3)
    b, _, _ = _golden_model(api, g, lr=1e-3)
    empty = torch.empty((0,))
    batch = (x, y, empty, empty, empty, empty, empty, empty)
    before = {k: p.detach().clone() for k, p in a.named_parameters()}
    stepper = DataParallelStepper(a)
    opt = b.configure_optimizers()
    for _ in range(2):
        stepper.step(batch)
        opt.zero_grad()
        b.training_step(batch, 0).backward()
        opt.step()
    moved = 0
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if _is_noise_bias(k):
            continue      # Adam normalises pure rounding noise on these: not comparable element-wise
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), atol=2e-4, rtol=0, err_msg=k)
        moved += int(float((pa.detach() - before[k]).abs().max()) > 1e-3)
    assert moved > 40                                   # (Adam's first steps move a parameter by about lr each: the comparison is of moved values)


def test_slice_step_bf16_operand_mode_stays_near_fp32(api, golden):
    """f: the bf16-operand mode on slices, held to the reference's fp32 step (the fixture) at the stated cost of the mode in
    test_bf16_operand_mode_step_vs_oracle_definition: loss terms rtol 5e-2, the final displacement field 5e-2 of its maximum, parameter
    gradients relative L2 <= 0.5"""
    from pulpo_amd import ops
    g = golden(STEP)
    model, x, y = _golden_model(api, g)
    ops.set_conv_precision("bf16")
    try:
        assert ops._use_bf16(8) and not ops._use_bf16(4)
        outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y)
        total.backward()
    finally:
        ops.set_conv_precision("fp32")
    for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
        np.testing.assert_allclose(float(val), float(g["train." + key]), rtol=5e-2)
    ref = g["train.final_dfs.0"]
    dfe = float(np.abs(outs[OUT.index("final_dfs")][0].detach().cpu().numpy() - ref).max() / np.abs(ref).max())
    assert dfe < 5e-2, dfe
    checked, worst = 0, 0.0
    for k, p in model.named_parameters():
        if "grad." + k not in g or _is_noise_bias(k):
            continue
        e = rel_l2(p.grad, g["grad." + k])
        worst = max(worst, e)
        assert e <= 0.5, (k, e)
        checked += 1
    assert checked > 60
    print(f"RATIO slice-step bf16 operands: final field {dfe / 5e-2:.3g} worst gradient rel-L2 {worst / 0.5:.3g}")
