"""F(2x2x2,3x3x3) as batched Winograd-domain GEMMs (pulpo_conv3d_k3_fwd_wino3g, conv3d_wino3g.hip): the forward and data-gradient convolution of
the coarse pyramid levels.  Reference: float64 torch.nn.functional.conv3d and its autograd; bound: tests/test_gpu_ops.py's per-operator 2e-6
relative L2.  Shapes are the smallest that take every path of the three kernels: 125 blocks (three padding rows of the 128-row GEMM tile),
210 blocks (a partial second row tile) with K = 136 (17 chunks: the last GEMM step holds one of four) and N = 160 (64-wide column tiles, the
last half empty) / 136 (data gradient: a partly filled 32-channel group of the output transform), two batch elements, N = 192 (96-wide column tiles).

Selection.  pulpo_conv3d_k3_algo keeps answering 2 for the shapes that run here: the existing suite pins that answer for exactly these layers
(tests/test_host.py, the family tables of tests/test_gpu_pyramid_convunit.py, tests/test_gpu_ops.py), so the default route is asked of
pulpo_conv3d_k3_wino3g_ok and of the pack ops._pack_weight_now hands out, on the same shapes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last_3d
BOUND = 2e-6                                     # tests/test_gpu_ops.py: relative L2 of a convolution against float64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@pytest.fixture(scope="module", autouse=True)
def leave_no_cached_blocks():
    """the blocks this module frees go back to the driver when it ends: later tests that compare torch.cuda.memory_allocated() count a live
    tensor at the size of the cached block it was given (tests/test_gpu_wgrad_budget.py says so), and a 2.3 MB block left here became
    tests/test_gpu_inverse.py's 1.5 MB scratch"""
    yield
    _REF.clear()
    torch.cuda.empty_cache()


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def call_entry(ops, x, w, bias, out, dgrad, stats=None):
    """the entry point on operand x (B, K, D, H, W view, any strides) with w packed for the forward (dgrad False) or data-gradient convolution;
    scratch arrives NaN-filled"""
    lib = ops.lib
    Cout, Cin = w.shape[0], w.shape[1]
    K, N = (Cout, Cin) if dgrad else (Cin, Cout)
    B, _, D, H, W = x.shape
    wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_wino3_floats", K, N), device=DEV)
    lib.call("pulpo_conv3d_k3_pack_weight_wino3", vp(w.contiguous()), vp(wp), Cin, Cout, int(dgrad), ops._stream())
    nscr = lib.query("pulpo_conv3d_k3_fwd_wino3g_scratch_floats", B, D, H, W, K, N)
    assert nscr == 64 * ((B * D * H * W // 8 + 127) // 128 * 128) * (K + N)
    scr = torch.full((nscr,), float("nan"), device=DEV)
    lib.call("pulpo_conv3d_k3_fwd_wino3g", vp(x), *ops.grid_strides(x), vp(wp), vp(bias), None, 0.2, vp(out), *ops.grid_strides(out), vp(stats), vp(scr),
             B, D, H, W, K, N, ops._stream())
    return out


_REF = {}


def case_data(B, Cin, Cout, size):
    """inputs and float64 references of a case, computed once and shared"""
    key = (B, Cin, Cout, size)
    if key not in _REF:
        g = torch.Generator(device=DEV).manual_seed(B * 1000 + Cin * 10 + Cout + size[1])
        x = torch.randn(B, Cin, *size, device=DEV, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, 3, device=DEV, generator=g) / (27 * Cin) ** 0.5
        b = torch.randn(Cout, device=DEV, generator=g)
        dy = torch.randn(B, Cout, *size, device=DEV, generator=g)
        x64 = x.double().requires_grad_(True)
        ref = F.conv3d(x64, w.double(), b.double(), padding=1)
        ref_nb = (ref - b.double().view(1, -1, 1, 1, 1)).detach()
        gx, = torch.autograd.grad(ref, [x64], grad_outputs=dy.double())
        _REF[key] = (x, w, b, dy, ref.detach(), ref_nb, gx)
    return _REF[key]


CASES = [(1, 128, 128, (10, 10, 10)), (1, 136, 160, (10, 12, 14)), (2, 128, 192, (8, 10, 10))]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,Cin,Cout,size", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_and_data_gradient_vs_float64(ops, B, Cin, Cout, size, with_bias):
    x, w, b, dy, ref, ref_nb, gx = case_data(B, Cin, Cout, size)
    out = call_entry(ops, x.contiguous(memory_format=CL), w, b if with_bias else None, torch.full_like(ref, float("nan"), dtype=torch.float32).contiguous(memory_format=CL), False)
    e = rel_l2(out, ref if with_bias else ref_nb)
    print(f"wino3g fwd B{B} {Cin}->{Cout} {size} bias={with_bias}: rel L2 {e:.3g}")
    assert bool(torch.isfinite(out).all()) and e < BOUND
    # data gradient: K = Cout, N = Cin, no bias in the reference's data gradient; `with_bias` adds one to the kernel's result and to the reference
    bz = torch.randn(Cin, device=DEV, generator=torch.Generator(device=DEV).manual_seed(Cin)) if with_bias else None
    dx = call_entry(ops, dy.contiguous(memory_format=CL), w, bz, torch.full_like(gx, float("nan"), dtype=torch.float32).contiguous(memory_format=CL), True)
    gref = gx + bz.double().view(1, -1, 1, 1, 1) if with_bias else gx
    e = rel_l2(dx, gref)
    print(f"wino3g dgrad B{B} {Cout}->{Cin} {size} bias={with_bias}: rel L2 {e:.3g}")
    assert bool(torch.isfinite(dx).all()) and e < BOUND


def test_operand_and_result_as_slices_of_wider_buffers(ops):
    """the operand a channel slice of a wider channels-last buffer, the result a slot of a concatenation buffer: strides, not shapes, address
    both, and nothing outside the slot is written"""
    B, Cin, Cout, size = 1, 136, 160, (10, 12, 14)
    x, w, b, dy, ref, _, gx = case_data(B, Cin, Cout, size)
    g = torch.Generator(device=DEV).manual_seed(7)
    xbuf = torch.randn(B, *size, Cin + 24, device=DEV, generator=g)
    xs = xbuf.permute(0, 4, 1, 2, 3)[:, 8:8 + Cin]
    xs.copy_(x)
    obuf = torch.full((B, *size, Cout + 40), 7.0, device=DEV)
    os_ = obuf.permute(0, 4, 1, 2, 3)[:, 16:16 + Cout]
    call_entry(ops, xs, w, b, os_, False)
    assert rel_l2(os_, ref) < BOUND
    assert bool((obuf[..., :16] == 7.0).all()) and bool((obuf[..., 16 + Cout:] == 7.0).all())
    dbuf = torch.randn(B, *size, Cout + 12, device=DEV, generator=g)
    ds = dbuf.permute(0, 4, 1, 2, 3)[:, 3:3 + Cout]          # (an unaligned channel offset: the input transform reads scalars)
    ds.copy_(dy)
    gbuf = torch.full((B, *size, Cin + 8), 7.0, device=DEV)
    gs = gbuf.permute(0, 4, 1, 2, 3)[:, 4:4 + Cin]
    call_entry(ops, ds, w, None, gs, True)
    assert rel_l2(gs, gx) < BOUND
    assert bool((gbuf[..., :4] == 7.0).all()) and bool((gbuf[..., 4 + Cin:] == 7.0).all())


def test_all_ones_is_exact(ops):
    """all-ones operand and weights at 10^3, 128 -> 128: the transformed operand holds small integers, the transformed weights multiples of 1/8,
    every product and sum is exact: each output equals 128 x (taps inside the volume), so a wrong halo or padding row shows without a tolerance"""
    C, S = 128, 10
    x = torch.ones(1, C, S, S, S, device=DEV).contiguous(memory_format=CL)
    w = torch.ones(C, C, 3, 3, 3, device=DEV)
    out = call_entry(ops, x, w, None, torch.full((1, C, S, S, S), float("nan"), device=DEV).contiguous(memory_format=CL), False)
    n1 = torch.full((S,), 3.0, device=DEV)
    n1[0] = n1[-1] = 2.0
    taps = n1.view(S, 1, 1) * n1.view(1, S, 1) * n1.view(1, 1, S)
    assert torch.equal(out, (C * taps).view(1, 1, S, S, S).expand_as(out))
    dx = call_entry(ops, x, w, None, torch.full((1, C, S, S, S), float("nan"), device=DEV).contiguous(memory_format=CL), True)
    assert torch.equal(dx, out)


@pytest.mark.parametrize("B,Cin,Cout,size", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_statistics_rows_describe_the_stored_output(ops, B, Cin, Cout, size):
    """rows arrive NaN-filled: every one of pulpo_conv3d_k3_stat_tiles() rows is written, and their float64 column sums are sum(y), sum(y^2) of the
    STORED output within the existing statistics tests' bound (tests/test_gpu_pyramid_convunit.py rows_vs_stored): a row is an fp32 sum of
    nvox / nrow terms, (terms - 1) roundings of 2^-24 of the running magnitude plus one for the square: (nvox / nrow + 1) 2^-24 sum |terms|"""
    x, w, b, _, ref, _, _ = case_data(B, Cin, Cout, size)
    nrow = ops.lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
    stats = torch.full((nrow * 2 * Cout,), float("nan"), device=DEV)
    y = call_entry(ops, x.contiguous(memory_format=CL), w, b, torch.full_like(ref, float("nan"), dtype=torch.float32).contiguous(memory_format=CL), False, stats)
    rows = stats.reshape(nrow, 2, Cout)
    assert bool(torch.isfinite(rows).all()), f"{int((~torch.isfinite(rows)).sum())} of {rows.numel()} row entries were not written"
    y64 = y.double()
    nvox = y64.numel() // Cout
    m = (nvox + nrow - 1) // nrow + 1
    got = rows.double().sum(0)
    s1, s2, a1 = y64.sum(dim=(0, 2, 3, 4)), (y64 * y64).sum(dim=(0, 2, 3, 4)), y64.abs().sum(dim=(0, 2, 3, 4))
    r1, r2 = float(((got[0] - s1).abs() / (m * U * a1)).max()), float(((got[1] - s2).abs() / (m * U * s2)).max())
    print(f"wino3g stats B{B} {Cin}->{Cout} {size}: |err| / bound {r1:.3g} (sum) {r2:.3g} (sum of squares)")
    assert r1 <= 1.0 and r2 <= 1.0


def test_selection(ops):
    """the default route takes the 160^3 pyramid's wide layers at 20^3 and 10^3 and nothing the launch-log fixture or the 32^3 golden pins;
    pulpo_conv3d_k3_algo answers what it answered before for all of them (module docstring)"""
    q = ops.lib.query
    takes = [(1, 20, 20, 20, 128, 192), (1, 20, 20, 20, 192, 192), (1, 20, 20, 20, 288, 192), (1, 10, 10, 10, 192, 192)]
    leaves = {(1, 16, 16, 16, 96, 96): 2, (1, 8, 8, 8, 128, 128): 0, (1, 20, 20, 20, 96, 96): 2, (1, 21, 20, 20, 192, 192): 0, (1, 160, 160, 160, 32, 32): 3}
    for s in takes:
        assert q("pulpo_conv3d_k3_wino3g_ok", *s) == 1 and q("pulpo_conv3d_k3_algo", *s) == 2, s
        w = torch.zeros(s[5], s[4], 3, 3, 3, device=DEV)
        assert ops._pack_weight_now(w, False, s[:4], register=False)._pulpo_algo == "wino3g"
    for s, algo in leaves.items():
        assert q("pulpo_conv3d_k3_wino3g_ok", *s) == 0 and q("pulpo_conv3d_k3_algo", *s) == algo, s
        w = torch.zeros(s[5], s[4], 3, 3, 3, device=DEV)
        assert ops._pack_weight_now(w, False, s[:4], register=False)._pulpo_algo == {0: "direct", 2: "wino2", 3: "wino3"}[algo]


def test_conv_sequence_vs_oracle(ops):
    """one ConvSequence (128 -> 128, depth 2) at 10^3, training mode, forward and backward through the modules - both units' forward and the second
    unit's data gradient run here - against oracle/pulpo_oracle.py's conv_sequence in float64.  tests/test_gpu_pyramid_convunit.py bounds kernels,
    not modules; the bounds here are the project's stated fp32 tolerances for module outputs and gradients (tests/test_gpu_ops.py's docstring,
    smoke()): outputs 1e-4 max(1, max|ref|) per element, gradients 1e-3 relative L2; a conv bias in front of a BatchNorm has a true gradient of
    zero and is held to 1e-4 of the largest gradient element"""
    from oracle import pulpo_oracle as O
    from pulpo_amd.network_blocks import ConvSequence
    C, size = 128, (10, 10, 10)
    assert ops.lib.query("pulpo_conv3d_k3_wino3g_ok", 1, *size, C, C) == 1
    torch.manual_seed(17)
    seq = ConvSequence(list(size), C, C, 2)
    params = {n for n, _ in seq.named_parameters()}
    sd = {}
    for k, v in seq.state_dict().items():
        t = v.detach().clone()
        sd["s." + k] = t.double().requires_grad_(k in params) if t.dtype.is_floating_point else t
    g = torch.Generator().manual_seed(23)
    x, up = torch.randn(1, C, *size, generator=g), torch.randn(1, C, *size, generator=g)
    x64 = x.double().requires_grad_(True)
    ref = O.conv_sequence(x64, sd, "s", 2, True)
    names = [n for n, _ in seq.named_parameters()]
    gref = torch.autograd.grad((ref * up.double()).sum(), [x64] + [sd["s." + n] for n in names])
    seq = seq.to(DEV).train()
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    z = seq(xd)
    got = torch.autograd.grad((z * up.to(DEV)).sum(), [xd] + list(seq.parameters()))
    err = float((z.detach().cpu().double() - ref.detach()).abs().max())
    print(f"wino3g ConvSequence out: max |err| {err:.3g} (max |ref| {float(ref.detach().abs().max()):.3g})")
    assert err <= 1e-4 * max(1.0, float(ref.abs().max()))
    scale = max(float(r.abs().max()) for r in gref)
    for n, a, r in zip(["x"] + names, got, gref):
        a = a.detach().cpu().double()
        if n.endswith("_op.0.bias"):
            print(f"wino3g ConvSequence d{n}: max |err| {float((a - r).abs().max()):.3g} of {scale:.3g}")
            assert float((a - r).abs().max()) <= 1e-4 * scale, n
        else:
            e = rel_l2(a, r)
            print(f"wino3g ConvSequence d{n}: rel L2 {e:.3g}")
            assert e < 1e-3, (n, e)
