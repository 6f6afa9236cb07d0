"""The training step's 1x1x1 heads, NCC, gradient-L2 regulariser, KL, warp and trilinear resize against float64 references
(tests/pyramid_ref.py, evaluated with plain torch ops on the GPU) at the sizes the pyramid runs them: 160^3 and its 80/40/20 levels, config
2's 96^3 pyramid at B = 2, config 5's 192x224x160 levels, and the edges where these kernels change path (tail trips, batch boundaries, row
segments, border planes, clamped samples).

Every tensor is compared element by element (max |got - ref| against a bound), and every comparison is shown to have power: the same bound
must reject the reference with one element - in the last pixel block or on a border plane - moved by 1e-3 max|ref|.  Bounds start from the
per-operator tests of test_gpu_ops.py; where fp32 coordinate arithmetic makes a kernel's error grow with the volume (warp, non-integer
resize) the bound is twice the spread of torch's own fp32 evaluation of the same operator on the same data."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import pyramid_ref as R
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

CL = torch.channels_last_3d
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def check(name, got, ref, tol, power=-1):
    """max |got - ref| <= tol element by element; and the bound rejects ref with element `power` (flat index) moved by 1e-3 max|ref|"""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    r = R.ratio(got, ref, tol)
    print(f"RATIO {name} {r:.3g}")
    assert r <= 1.0, f"{name}: max error / tolerance = {r:.3g}"
    if power is not None:
        assert R.ratio(got, R.perturbed(ref, power), tol) > 1.0, f"{name}: the bound does not reject a 1e-3 max|ref| error in element {power}"


def amax(t) -> float:
    return float(t.detach().abs().max())


def det_default() -> bool:
    return os.environ.get("PULPO_DETERMINISTIC", "0") == "1"


# ================================================================================================ heads
def _head_params(g, nout, zdim, C, sigma_bias=None, sigma_rows=None):
    w = lambda n: torch.randn(n, C, 1, 1, 1, device=DEV, generator=g) / C ** 0.5
    b = lambda n: torch.randn(n, device=DEV, generator=g)
    if nout == 3:
        return [w(3), b(3)]
    ws, bs = w(zdim), b(zdim)
    if sigma_bias is not None:
        bs = torch.tensor(sigma_bias, device=DEV, dtype=torch.float32)
        ws = ws * torch.tensor(sigma_rows, device=DEV, dtype=torch.float32).reshape(-1, 1, 1, 1, 1)
    return [w(zdim), b(zdim), ws, bs]


def _heads_vs_ref(ops, name, h, params, nout, eps, g, bf16_dh=False, tiny_sigma=False):
    """run the op forward and backward with random upstream gradients, compare outputs, dh, dW and db with the float64 evaluation.
    tiny_sigma: every sigma is below 1e-13 - held to 1e-5 of its own value, and the sigma rows' dW / db (the float64 values are ~1e-11: fp32's
    1 - exp(-sigma) is 0 below 6e-8) to 1e-5 of the mu rows' scale, without a power check of their own"""
    B, C, D, H, W = h.shape
    n = 3 if nout == 3 else params[0].shape[0]
    ups = [torch.randn(B, n, D, H, W, device=DEV, generator=g) for _ in range(1 if nout == 3 else 3)]
    hg = h.detach().requires_grad_(True)
    pg = [p.detach().clone().requires_grad_(True) for p in params]
    outs = (ops.conv1x1_to3(hg, *pg),) if nout == 3 else ops.mu_sigma_sample(hg, *pg, eps)
    grads = torch.autograd.grad(sum((o * u).sum() for o, u in zip(outs, ups)), [hg] + pg)
    h64 = h.detach().double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    e64 = eps.double() if eps is not None else None
    routs = (R.conv1x1_ref(h64, *p64),) if nout == 3 else R.mu_sigma_ref(h64, *p64, e64)
    rgrads = torch.autograd.grad(sum((o * u.double()).sum() for o, u in zip(routs, ups)), [h64] + p64)
    for k, (o, ro) in enumerate(zip(outs, routs)):
        check(f"heads {name} out{k}", o, ro.detach(), 1e-5 * ro.detach().abs() if tiny_sigma and k == 1 else 1e-5 * max(1.0, amax(ro)))
    dh, rdh = grads[0], rgrads[0]
    if bf16_dh:
        # dh is stored as bf16: the fp32 value rounded to 8 significant bits.  Power: the element of the last pixel with the smallest |ref|
        tol = 2.0 ** -8 * rdh.abs() + 1e-5 * max(1.0, amax(rdh))
        c = int(rdh[-1, :, -1, -1, -1].abs().argmin())
        check(f"heads {name} dh", dh, rdh, tol, power=((((B - 1) * C + c) * D + D - 1) * H + H - 1) * W + W - 1)
    else:
        check(f"heads {name} dh", dh, rdh, 1e-5 * max(1.0, amax(rdh)))
    for k, (gp, rp) in enumerate(zip(grads[1:], rgrads[1:])):
        if tiny_sigma and k >= 2:
            check(f"heads {name} {'dW' if k % 2 == 0 else 'db'}1", gp, rp, 1e-5 * max(1.0, amax(rgrads[k - 1])), power=None)
        else:
            check(f"heads {name} {'dW' if k % 2 == 0 else 'db'}{k // 2}", gp, rp, 1e-5 * max(1.0, amax(rp)))


# vector paths (C % 4 == 0): C = 96 leaves 16 idle threads per backward block (RB = 10); 80^3 runs 16-100 trips per block (both LDS buffers
# of the nout-6 backward alternate); 17x19x23 at B = 2 is a pixel count that is no multiple of RB or 32, so trips straddle the batch boundary.
# Scalar paths: C in {1, 3, 6, 10}.
HEAD_CASES = [(6, 1, (80, 80, 80), 32), (6, 1, (80, 80, 80), 96), (6, 2, (17, 19, 23), 192), (6, 2, (48, 48, 48), 64), (6, 1, (40, 40, 40), 16),
              (6, 2, (9, 7, 5), 4), (6, 2, (17, 19, 23), 1), (6, 1, (40, 40, 40), 3), (6, 2, (20, 20, 20), 6), (6, 1, (33, 20, 17), 10),
              (3, 1, (160, 160, 160), 16), (3, 1, (80, 80, 80), 64), (3, 2, (17, 19, 23), 96), (3, 1, (40, 40, 40), 4), (3, 2, (17, 19, 23), 10),
              (3, 1, (40, 40, 40), 3), (3, 2, (48, 48, 48), 32), (6, 1, (96, 112, 80), 32)]


@pytest.mark.parametrize("nout,B,size,C", HEAD_CASES)
def test_heads_vs_float64(ops, nout, B, size, C):
    g = gen(C * 7 + B + size[0])
    h = torch.randn(B, C, *size, device=DEV, generator=g).contiguous(memory_format=CL)
    eps = torch.randn(B, 3, *size, device=DEV, generator=g) if nout == 6 else None
    _heads_vs_ref(ops, f"{nout}/{B}/{size}/C{C}", h, _head_params(g, nout, 3, C), nout, eps, g)


HEAD_EDGES = ["eps_none", "zdim5", "zdim1", "softplus_high", "softplus_low", "bf16", "slice_aligned", "slice_unaligned"]


@pytest.mark.parametrize("case", HEAD_EDGES)
def test_heads_edges_vs_float64(ops, case):
    """eps=None (z = mu); zdim 5 and 1 (grouped launches of three latent rows); sigma pre-activations above 20, at 20 +- 1e-3 and below -30
    (softplus threshold, 1 - exp(-sigma)); bf16 h (bf16 dh); channel slices of a wider channels-last buffer at a 16-byte aligned offset
    (vector kernels, pixel stride 104) and at an unaligned one (scalar forward and the VEC = 1 backward)"""
    g = gen(100 + HEAD_EDGES.index(case))
    B, size, C = 2, (21, 18, 25), 96
    h = torch.randn(B, C, *size, device=DEV, generator=g).contiguous(memory_format=CL)
    eps = torch.randn(B, 3, *size, device=DEV, generator=g)
    zdim, sb, sr, bf16 = 3, None, None, False
    if case == "eps_none":
        eps = None
    elif case in ("zdim5", "zdim1"):
        zdim = int(case[-1])
        eps = torch.randn(B, zdim, *size, device=DEV, generator=g)
    elif case == "softplus_high":
        sb, sr = [25.0, 20.0 + 1e-3, 20.0 - 1e-3], [0.5, 0.0, 0.0]
    elif case == "softplus_low":
        sb, sr = [-35.0, -30.5, -40.0], [0.5, 0.0, 1.0]
    elif case == "bf16":
        h, bf16 = h.bfloat16(), True
    else:
        off = 4 if case == "slice_aligned" else 2
        buf = torch.randn(B, C + 8, *size, device=DEV, generator=g).contiguous(memory_format=CL)
        h = buf[:, off:off + C]
        assert h.stride(4) == C + 8 and (h.data_ptr() % 16 == 0) == (case == "slice_aligned")
    params = _head_params(g, 6, zdim, C, sb, sr)
    if sb is not None:
        pre = R._mix(h.double(), params[2].double(), params[3].double())
        if case == "softplus_high":
            assert bool((pre[:, 0] > 20).all()) and bool((pre[:, 1] > 20).all()) and bool((pre[:, 2] < 20).all())
        else:
            assert bool((pre < -30).all())
    _heads_vs_ref(ops, case, h, params, 6, eps, g, bf16_dh=bf16, tiny_sigma=case == "softplus_low")


def test_heads_backward_takes_an_unaligned_slice_its_forward_took(ops):
    """regression: the backward refused (PulpoHipError "heads_bwd: unaligned operands") a channel slice at a non-16-byte offset that the forward
    ran with its scalar loads; the plain head too, and the result equals the same head on a packed copy of the slice"""
    g = gen(77)
    buf = torch.randn(2, 100, 9, 10, 11, device=DEV, generator=g).contiguous(memory_format=CL)
    w, b = torch.randn(3, 96, 1, 1, 1, device=DEV, generator=g), torch.randn(3, device=DEV, generator=g)
    up = torch.randn(2, 3, 9, 10, 11, device=DEV, generator=g)
    outs = []
    for h in (buf[:, 2:98], buf[:, 2:98].contiguous(memory_format=CL)):
        hg, wg, bg = h.detach().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        o = ops.conv1x1_to3(hg, wg, bg)
        outs.append((o,) + torch.autograd.grad((o * up).sum(), [hg, wg, bg]))
    for a, c in zip(*outs):
        assert float((a - c).abs().max()) <= 1e-5 * max(1.0, amax(c))


# ================================================================================================ NCC
def _images(g, B, size, kind):
    if kind == "rand":
        t = torch.rand(B, 1, *size, device=DEV, generator=g)
        return torch.rand(B, 1, *size, device=DEV, generator=g), t

    def smooth():
        lo = torch.rand(B, 1, *(max(2, s // 4) for s in size), device=DEV, generator=g)
        return F.interpolate(lo, size=size, mode="trilinear", align_corners=False)
    t = smooth()
    p = 0.7 * smooth() + 0.3 * t
    if kind == "zerobg":                       # smooth blob with zero background, like a skull-stripped scan (tests/golden/make_golden.py)
        zz, yy, xx = torch.meshgrid(*[torch.linspace(-1, 1, s, device=DEV) for s in size], indexing="ij")
        mask = ((zz ** 2 + yy ** 2 + xx ** 2) < 0.8).float()
        t, p = t * mask, p * mask
    return p, t


# (B, size, window, images): the pyramid's windows 9/7/5/3 at 160/80/40/20, config 2 (96^3, B = 2) and config 5 (192x224x160) levels;
# W = k (64 - 2 pad) and one either side (several wave segments per row, forward and backward W passes); H = 1 (no march for the H pass);
# D = 1 (2-D window count); an extent below the pad (D = 3, w = 11); w = 13 (the non-marching box_axis / ncc_final kernels)
NCC_CASES = [(1, (160, 160, 160), 9, "rand"), (1, (80, 80, 80), 7, "smooth"), (1, (40, 40, 40), 5, "rand"), (1, (20, 20, 20), 3, "smooth"),
             (2, (96, 96, 96), 9, "smooth"), (2, (48, 48, 48), 7, "rand"), (1, (96, 112, 80), 7, "rand"), (1, (24, 28, 20), 3, "rand"),
             (2, (4, 5, 111), 9, "rand"), (2, (4, 5, 112), 9, "rand"), (2, (4, 5, 113), 9, "rand"),
             (1, (3, 4, 123), 3, "rand"), (1, (3, 4, 124), 3, "rand"), (1, (3, 4, 125), 3, "smooth"), (1, (5, 3, 180), 7, "rand"),
             (2, (6, 1, 70), 5, "rand"), (2, (1, 20, 130), 7, "rand"), (1, (3, 12, 70), 11, "rand"), (1, (10, 12, 40), 13, "smooth")]


@pytest.mark.parametrize("B,size,win,kind", NCC_CASES)
def test_ncc_vs_float64(ops, B, size, win, kind):
    g = gen(win * 1000 + size[2] + B)
    p, t = _images(g, B, size, kind)
    pg = p.clone().requires_grad_(True)
    loss = ops.ncc_loss(pg, t, win, 0.05)
    gp, = torch.autograd.grad(loss, [pg], grad_outputs=torch.tensor(1.7, device=DEV))
    ref = R.ncc_ref(p.double(), t.double(), win, 0.05)
    check(f"ncc {B}/{size}/w{win}/{kind} loss", loss, ref, 1e-4 * abs(float(ref)))
    rg = 1.7 * R.ncc_grad_ref(p.double(), t.double(), win, 0.05)
    # smooth images: nearly constant windows cancel in Iv = S_II - S_I^2 / n; measured fp32 error 2.3e-4 max|ref| at 20^3 (w 3, 5^3
    # control points), below 2e-5 on random images (test_ncc_golden: 2e-3 with zero background)
    check(f"ncc {B}/{size}/w{win}/{kind} grad", gp, rg, (5e-4 if kind == "smooth" else 5e-5) * amax(rg))


def test_ncc_zero_background_vs_float64(ops):
    """zero background: where both window variances nearly vanish the fp32 box sums' rounding is amplified (test_ncc_golden's argument,
    2e-3 max|ref|); that bound holds only on voxels whose window reaches such a voxel, the rest keep the bound of the other images"""
    B, size, win = 1, (40, 40, 40), 9
    p, t = _images(gen(5), B, size, "zerobg")
    pg = p.clone().requires_grad_(True)
    loss = ops.ncc_loss(pg, t, win, 0.05)
    gp, = torch.autograd.grad(loss, [pg], grad_outputs=torch.tensor(1.7, device=DEV))
    ref = R.ncc_ref(p.double(), t.double(), win, 0.05)
    check("ncc zerobg loss", loss, ref, 1e-4 * abs(float(ref)))
    rg = 1.7 * R.ncc_grad_ref(p.double(), t.double(), win, 0.05)
    loose = R.ncc_degenerate(p.double(), t.double(), win)
    assert 0 < int(loose.sum()) < loose.numel()
    tol = torch.where(loose, 2e-3 * amax(rg) + 1e-7, 2e-4 * amax(rg))
    tight = torch.nonzero(~loose.reshape(-1)).reshape(-1)
    check("ncc zerobg grad", gp, rg, tol, power=int(tight[-1]))
    print(f"RATIO ncc zerobg grad(tight part) {R.ratio(gp[~loose], rg[~loose], 2e-4 * amax(rg)):.3g}")


# ================================================================================================ L2 regulariser
def _offset_copy(x):
    """x's values in a buffer that starts one float past an allocation: same shape, contiguous, 4-byte aligned only (the scalar kernels)"""
    buf = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    y = buf[1:1 + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.is_contiguous() and y.data_ptr() % 16 != 0
    return y


# (B, size): 3 and 6 planes; W % 4 == 0 takes the vector kernels when aligned; W = 4 (a single group per row), H = 2, D = 1 (the 2-D form)
L2_CASES = [(1, (160, 160, 160)), (2, (80, 80, 80)), (2, (96, 96, 96)), (1, (96, 112, 80)), (1, (20, 20, 20)), (1, (5, 6, 4)), (2, (7, 2, 8)),
            (2, (1, 9, 12)), (1, (1, 2, 4)), (2, (9, 10, 11)), (1, (13, 11, 20))]


@pytest.mark.parametrize("B,size", L2_CASES)
def test_l2reg_vector_and_scalar_kernels_vs_float64(ops, B, size):
    g = gen(size[0] * 31 + size[2] + B)
    df = torch.randn(B, 3, *size, device=DEV, generator=g)
    r64 = df.double().requires_grad_(True)
    ref = R.l2reg_ref(r64, 0.025)
    rg, = torch.autograd.grad(ref, [r64], grad_outputs=torch.tensor(1.7, dtype=torch.float64, device=DEV))
    got = {}
    for path, x in (("aligned", df), ("offset", _offset_copy(df))):
        xg = x.detach().requires_grad_(True)
        loss = ops.l2_reg(xg, 0.025)
        gdf, = torch.autograd.grad(loss, [xg], grad_outputs=torch.tensor(1.7, device=DEV))
        got[path] = gdf
        name = f"l2reg {B}/{size} {path}"
        check(name + " loss", loss, ref.detach(), 1e-5 * abs(float(ref)))
        tol = 1e-7 * max(1.0, amax(rg)) + 1e-4 * rg.abs()
        check(name + " grad", gdf, rg, tol)
        # every voxel of the first and last planes along each axis, on their own (the border terms of the backward)
        for d in (2, 3, 4):
            for i in (0, size[d - 2] - 1):
                assert R.ratio(gdf.narrow(d, i, 1), rg.narrow(d, i, 1), tol.narrow(d, i, 1)) <= 1.0, (name, d, i)
    # losses.hip: the vector backward evaluates the scalar kernel's four terms in its order - the same bits
    assert torch.equal(got["aligned"], got["offset"])


# ================================================================================================ KL
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("second", [False, True])
def test_kl_vs_float64(ops, B, second):
    """sigma from 1e-4 to 1e2 (log-uniform), 3 x 80^3 per batch element, against N(0, 1) and against a second diagonal Gaussian"""
    g = gen(B * 10 + second)
    shp = (B, 3, 80, 80, 80)
    mu = torch.randn(shp, device=DEV, generator=g)
    sg = 10.0 ** (torch.rand(shp, device=DEV, generator=g) * 6 - 4)
    mu1 = torch.randn(shp, device=DEV, generator=g) if second else None
    sg1 = 10.0 ** (torch.rand(shp, device=DEV, generator=g) * 2 - 1) if second else None
    mg, sgg = mu.clone().requires_grad_(True), sg.clone().requires_grad_(True)
    kl = ops.kl_diag(mg, sgg, mu1, sg1)
    gm, gs = torch.autograd.grad(kl, [mg, sgg], grad_outputs=torch.tensor(1.7, device=DEV))
    m64, s64 = mu.double().requires_grad_(True), sg.double().requires_grad_(True)
    ref = R.kl_ref(m64, s64, mu1.double() if second else None, sg1.double() if second else None)
    rm, rs = torch.autograd.grad(ref, [m64, s64], grad_outputs=torch.tensor(1.7, dtype=torch.float64, device=DEV))
    name = f"kl B{B} second={second}"
    check(name + " loss", kl, ref.detach(), 1e-5 * abs(float(ref)))
    check(name + " gmu", gm, rm, 1e-6 * amax(rm) + 1e-5 * rm.abs())
    check(name + " gsigma", gs, rs, 1e-6 * amax(rs) + 1e-5 * rs.abs())
    if not second:
        kl2 = ops.kl_std_normal(mu, sg)
        assert torch.equal(kl2, ops.kl_diag(mu, sg))


# ================================================================================================ warp
def _warp_field(g, B, grid, img, amp, kind):
    df = torch.randn(B, 3, *grid, device=DEV, generator=g) * amp
    if kind == "faces":
        # push every face's samples out of the volume (clamped: border padding) and put one slab of samples exactly on the border indices
        # 0 and S - 1 and on interior integers: c = (p + d) S_i / (S_g - 1) - 0.5 = k  <=>  d = (k + 0.5) (S_g - 1) / S_i - p
        for a in range(3):
            n = grid[a]
            sl = [slice(None)] * 5
            sl[1] = a
            sl[2 + a] = slice(0, 3)
            df[tuple(sl)] -= 2.5 * amp
            sl[2 + a] = slice(n - 3, n)
            df[tuple(sl)] += 2.5 * amp
        Si = img
        for a in range(3):
            pos = torch.arange(grid[a], device=DEV, dtype=torch.float64)
            k = torch.tensor([0.0, Si[a] - 1.0, float(Si[a] // 2)], device=DEV, dtype=torch.float64)
            shape = [1] * 3
            shape[a] = -1
            for j, kk in enumerate(k):
                d = ((kk + 0.5) * (grid[a] - 1) / Si[a] - pos).reshape(shape).expand(*grid).float()
                slab = [slice(None)] * 3
                slab[(a + 1) % 3] = slice(4 * j, 4 * j + 2)
                df[(slice(None), a) + tuple(slab)] = d[tuple(slab)]
    return df


def _warp_grads(ops, df, img, up, det):
    ops.set_deterministic(det)
    try:
        dfg, imgg = df.clone().requires_grad_(True), img.clone().requires_grad_(True)
        out = ops.warp3d(dfg, imgg)
        return (out,) + torch.autograd.grad((out * up).sum(), [dfg, imgg])
    finally:
        ops.set_deterministic(det_default())


def _ref_grads(df, img, up):
    d, i = df.clone().requires_grad_(True), img.clone().requires_grad_(True)
    out = R.warp_ref(d, i)
    return (out.detach(),) + torch.autograd.grad((out * up).sum(), [d, i])


# (B, grid, image, C, amplitude, field): a 1-channel image at 160^3 / 80^3 (the step's image warps), a 3-channel field (self warp of a
# velocity-sized field), an image larger than the grid (full_res: 40^3 grid, 160^3 image), config 2 (B = 2, 96^3), config 5's 96x112x80 level,
# and samples clamped at all six faces with slabs exactly on the border index
WARP_CASES = [(1, (160, 160, 160), (160, 160, 160), 1, 2.0, "rand"), (1, (80, 80, 80), (80, 80, 80), 3, 3.0, "rand"),
              (1, (40, 40, 40), (160, 160, 160), 1, 2.0, "rand"), (2, (96, 96, 96), (96, 96, 96), 1, 1.5, "rand"),
              (1, (96, 112, 80), (96, 112, 80), 1, 2.0, "rand"), (1, (40, 40, 40), (40, 40, 40), 1, 4.0, "faces"),
              (2, (40, 44, 36), (40, 44, 36), 3, 3.0, "faces")]


@pytest.mark.parametrize("B,grid,isize,C,amp,kind", WARP_CASES)
def test_warp_vs_float64(ops, B, grid, isize, C, amp, kind):
    """forward, gdf and gimg through the atomic and the deterministic (fixed-point) kernels.  fp32 sample coordinates carry a rounding that
    grows with the extent (about 1e-5 voxel at 160): outputs and gradients are held to twice the spread of torch's fp32 grid_sample on the
    same data (at least the 1e-5 of test_warp_golden).  Voxels whose float64 sample coordinate lies within 1e-4 voxel of a cell boundary (or
    of a clamp) may take the other cell, where the displacement gradient jumps: there gdf is bounded by the float64 gradient a displacement
    2e-4 voxel to either side gives"""
    g = gen(grid[0] + 7 * C + B)
    df = _warp_field(g, B, grid, isize, amp, kind)
    img = torch.rand(B, C, *isize, device=DEV, generator=g)
    up = torch.randn(B, C, *grid, device=DEV, generator=g)
    ref = _ref_grads(df.double(), img.double(), up.double())
    r32 = _ref_grads(df, img, up)
    c = R.warp_coords(df.double(), isize)
    his = torch.tensor(isize, device=DEV, dtype=torch.float64).reshape(3, 1, 1, 1, 1) - 1
    near = ((c - c.round()).abs() < 1e-4) | ((c - his).abs() < 1e-4) | (c.abs() < 1e-4)
    bnd = near.any(0).unsqueeze(1).expand(B, 3, *grid)
    if kind == "faces":          # samples beyond both faces of every axis, and on the border indices
        assert bool((c < 0).flatten(1).any(1).all()) and bool((c > his).flatten(1).any(1).all()) and int(bnd.sum()) > 0
    else:
        assert int(bnd.sum()) < 0.01 * bnd.numel()
    nudge = torch.zeros_like(ref[1])
    for a in range(3):           # one axis at a time: along its own axis the gradient is constant within a cell, so the jump is all it sees
        for sgn in (1.0, -1.0):
            d = df.double().clone()
            d[:, a] += sgn * 2e-4 * (grid[a] - 1) / isize[a]
            nudge = torch.maximum(nudge, (_ref_grads(d, img.double(), up.double())[1] - ref[1]).abs())
    tol_out = max(1e-5 * max(1.0, amax(ref[0])), 2 * R.ratio(r32[0], ref[0], 1.0))
    tol_img = max(1e-5 * max(1.0, amax(ref[2])), 2 * R.ratio(r32[2], ref[2], 1.0))
    tol_df = max(1e-5 * max(1.0, amax(ref[1])), 2 * float((r32[1] - ref[1]).abs()[~bnd].max()))
    tol_df_t = torch.where(bnd, tol_df + nudge, torch.full_like(nudge, tol_df))
    last_inner = int(torch.nonzero(~bnd.reshape(-1)).reshape(-1)[-1])
    print(f"RATIO warp {B}/{grid}/{isize}/C{C}/{kind} spread32 out {R.ratio(r32[0], ref[0], 1.0):.3g} gdf {tol_df:.3g} gimg {tol_img:.3g} "
          f"boundary voxels {int(bnd[:, 0].sum())}")
    for det in (False, True):
        out, gdf, gimg = _warp_grads(ops, df, img, up, det)
        name = f"warp {B}/{grid}/{isize}/C{C}/{kind} det={det}"
        check(name + " out", out, ref[0], tol_out)
        print(f"RATIO {name} gdf(off the boundaries) {R.ratio(gdf[~bnd], ref[1][~bnd], tol_df):.3g}")
        check(name + " gdf", gdf, ref[1], tol_df_t, power=last_inner)
        check(name + " gimg", gimg, ref[2], tol_img)


def test_warp_bwd_det_without_image_gradient_or_workspace(ops):
    """regression: pulpo_warp3d_bwd_det with gimg = NULL and ws = NULL (the header allows it: ws is 'nullable when gimg is') read its scale slot
    from the null workspace.  The displacement gradient of that call is the plain kernel's, bit for bit, with a workspace or without"""
    from pulpo_amd._lib import lib
    g = gen(91)
    B, C, grid, isize = 2, 1, (24, 20, 28), (30, 26, 22)
    df = torch.randn(B, 3, *grid, device=DEV, generator=g) * 3.0
    img = torch.rand(B, C, *isize, device=DEV, generator=g)
    up = torch.randn(B, C, *grid, device=DEV, generator=g)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    plain, det, det_ws = (torch.full_like(df, float("nan")) for _ in range(3))
    lib.call("pulpo_warp3d_bwd", p(df), p(img), p(up), p(plain), None, B, C, *grid, *isize, st)
    lib.call("pulpo_warp3d_bwd_det", p(df), p(img), p(up), p(det), None, None, B, C, *grid, *isize, st)
    ws = torch.full((lib.query("pulpo_warp3d_bwd_det_ws_bytes", B, C, *isize),), 0xA5, device=DEV, dtype=torch.uint8)
    lib.call("pulpo_warp3d_bwd_det", p(df), p(img), p(up), p(det_ws), None, p(ws), B, C, *grid, *isize, st)
    torch.cuda.synchronize()
    assert torch.equal(det, plain) and torch.equal(det_ws, plain)
    ref = _ref_grads(df.double(), img.double(), up.double())[1]
    assert float((det - ref).abs().max()) <= 1e-3 * amax(ref)


# ================================================================================================ resize
def _resize_vs_ref(ops, name, x, size, mult, add, scale_factor, det, exact):
    g = torch.randn(x.shape[0], x.shape[1], *size, device=DEV, generator=gen(sum(size) + det))
    ops.set_deterministic(det)
    try:
        xg = x.clone().requires_grad_(True)
        out = ops.resize_trilinear(xg, size, mult, add, scale_factor)
        gx, = torch.autograd.grad((out * g).sum(), [xg])
    finally:
        ops.set_deterministic(det_default())
    steps = None if scale_factor is None else (1.0 / scale_factor,) * 3

    def ref_of(t, fp32):
        tg = t.clone().requires_grad_(True)
        if fp32:          # torch's own fp32 operator: the spread fp32 source coordinates give at these sizes
            o = mult * (F.interpolate(tg, size=tuple(size), mode="trilinear", align_corners=False) if scale_factor is None else
                        F.interpolate(tg, scale_factor=scale_factor, mode="trilinear", align_corners=False))
        else:
            o = mult * R.resize_ref(tg, size, steps)
        if add is not None:
            o = o + add.to(o.dtype)
        return o.detach(), torch.autograd.grad((o * g.to(o.dtype)).sum(), [tg])[0]

    ro, rg = ref_of(x.double(), False)
    so, sgx = ref_of(x, True)
    base_o, base_g = 1e-5 * max(1.0, amax(ro)), 1e-5 * max(1.0, amax(rg))
    tol_o = base_o if exact else max(base_o, 2 * R.ratio(so, ro, 1.0))
    tol_g = base_g if exact else max(base_g, 2 * R.ratio(sgx, rg, 1.0))
    check(f"resize {name} det={det} out", out, ro, tol_o)
    check(f"resize {name} det={det} grad", gx, rg, tol_g)


# (B, C, in, out, mult, add, scale_factor, exact coordinates): the exact x2 path 3 x 80^3 -> 160^3 with mult and the fused add, config 2's
# 48^3 -> 96^3 at B = 2; scale_factor = 0.5 at 160^3 and from odd sizes (159^3, 97x113x81); non-integer size ratios down and up
RESIZE_CASES = [(1, 3, (80, 80, 80), (160, 160, 160), 2.0, True, None, True), (2, 3, (48, 48, 48), (96, 96, 96), 2.0, False, None, True),
                (1, 3, (160, 160, 160), (80, 80, 80), 0.5, False, 0.5, True), (1, 3, (159, 159, 159), (79, 79, 79), 0.5, False, 0.5, True),
                (1, 3, (97, 113, 81), (48, 56, 40), 0.5, False, 0.5, True), (1, 3, (97, 113, 81), (40, 48, 33), 1.0, False, None, False),
                (2, 3, (24, 28, 20), (40, 48, 33), 1.5, True, None, False), (1, 3, (48, 56, 40), (96, 112, 80), 2.0, True, None, True)]


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,C,isz,osz,mult,with_add,sf,exact", RESIZE_CASES)
def test_resize_vs_float64(ops, B, C, isz, osz, mult, with_add, sf, exact, det):
    """exact x2 (resize_up2_fwd / resize_up2_bwd), the scale_factor form and generic ratios (resize_fwd; backward by float atomics, or by the
    gather in deterministic mode).  Coordinates of x2 and x0.5 are exact in fp32; other ratios are held to twice torch's fp32 spread"""
    g = gen(sum(isz) + B)
    x = torch.randn(B, C, *isz, device=DEV, generator=g)
    add = torch.randn(B, C, *osz, device=DEV, generator=g) if with_add else None
    _resize_vs_ref(ops, f"{B}/{isz}->{osz}/sf{sf}", x, osz, mult, add, sf, det, exact)
