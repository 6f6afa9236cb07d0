"""float64 references of the training step's head, loss, field and ConvUnit operators, written with plain torch ops (matmul, einsum,
softplus, cumsum, index_select, grid_sample) so that they also run on the GPU at the pyramid's sizes, and the element-wise comparison the
pyramid tests use.  tests/test_oracle_golden.py pins every helper to oracle/pulpo_oracle.py and torch.nn.functional at small shapes;
tests/test_gpu_pyramid_ops.py, tests/test_gpu_pyramid_convunit.py and tests/test_gpu_vecint.py (the VecInt helpers and field generators) hold
the HIP kernels to them; tests/test_gpu_bf16_storage.py holds the bf16-storing kernels to the ROUNDED reference (held_bf16, at the end)."""
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import pulpo_oracle as O
from inverse_ref import smooth_field
from slice_ref import warp_ref as _warp2d_ref


# ------------------------------------------------------------------------------------------------ 1x1x1 heads
def _mix(h, w, b):
    """(B, C, ...) x (n, C) + (n,) -> (B, n, ...)"""
    C = h.shape[1]
    return torch.einsum("bc...,jc->bj...", h, w.reshape(w.shape[0], C)) + b.reshape(1, -1, *([1] * (h.dim() - 2)))


def mu_sigma_ref(h, w_mu, b_mu, w_sigma, b_sigma, eps: Optional[torch.Tensor]):
    """MuSigmaBlock + sampler: mu = W_mu h + b_mu, sigma = softplus(W_sigma h + b_sigma), z = mu + sigma eps (eps None: z = mu)"""
    mu = _mix(h, w_mu, b_mu)
    sigma = F.softplus(_mix(h, w_sigma, b_sigma))
    return mu, sigma, (mu if eps is None else mu + sigma * eps)


def conv1x1_ref(h, w, b):
    """VelocityField's last layer: Conv3d(C, n, kernel_size=1)"""
    return _mix(h, w, b)


# ------------------------------------------------------------------------------------------------ NCC
def box1(v, pad: int, dim: int):
    """zero-padded sum over positions i - pad .. i + pad along one axis, from a prefix sum"""
    n = v.shape[dim]
    c = torch.cumsum(v, dim)
    c = torch.cat([torch.zeros_like(c.narrow(dim, 0, 1)), c], dim)
    i = torch.arange(n, device=v.device)
    return c.index_select(dim, (i + pad + 1).clamp(max=n)) - c.index_select(dim, (i - pad).clamp(min=0))


def box_sum(v, win: int):
    """zero-padded win^3 box sum over the last three axes (the reference's ones-kernel conv3d), as three separable passes"""
    for d in (-3, -2, -1):
        v = box1(v, win // 2, d)
    return v


def ncc_window_count(win: int, D: int) -> float:
    """win^ndims: a depth-1 volume is the reference's 2-D case"""
    return float(win ** 3 if D > 1 else win ** 2)


def _ncc_terms(pred, true, win: int):
    I, J = true, pred
    n = ncc_window_count(win, I.shape[2])
    SI, SJ, SII, SJJ, SIJ = (box_sum(t, win) for t in (I, J, I * I, J * J, I * J))
    return I, J, n, SI, SJ, SII, SJJ, SIJ


def ncc_ref(pred, true, win: int, gamma: float):
    """local normalised cross-correlation loss (src/losses.py NCC_loss): -gamma / B * sum of cc"""
    I, J, n, SI, SJ, SII, SJJ, SIJ = _ncc_terms(pred, true, win)
    uI, uJ = SI / n, SJ / n
    cross = SIJ - uJ * SI - uI * SJ + uI * uJ * n
    Iv = SII - 2 * uI * SI + uI * uI * n
    Jv = SJJ - 2 * uJ * SJ + uJ * uJ * n
    return -(gamma / I.shape[0]) * torch.sum(cross * cross / (Iv * Jv + 1e-8))


def ncc_grad_ref(pred, true, win: int, gamma: float):
    """d ncc_ref / d pred in closed form (the expression of O.ncc_grad_closed_form, with the 2-D window count at depth 1)"""
    I, J, n, SI, SJ, SII, SJJ, SIJ = _ncc_terms(pred, true, win)
    cross = SIJ - SI * SJ / n
    Iv = SII - SI * SI / n
    Jv = SJJ - SJ * SJ / n
    Dn = Iv * Jv + 1e-8
    a = -2 * cross * SI / (n * Dn) + 2 * cross * cross * Iv * SJ / (n * Dn * Dn)
    b = -cross * cross * Iv / (Dn * Dn)
    c = 2 * cross / Dn
    return -(gamma / I.shape[0]) * (box_sum(a, win) + 2 * J * box_sum(b, win) + I * box_sum(c, win))


def ncc_degenerate(pred, true, win: int, thr: float = 1e-4):
    """voxels whose window overlaps one where Iv * Jv is below thr (the 1e-8 of the denominator dominates): there the fp32 box sums' rounding
    is amplified, as the golden test (test_ncc_golden) argues for zero background"""
    _, _, n, SI, SJ, SII, SJJ, _ = _ncc_terms(pred, true, win)
    small = ((SII - SI * SI / n) * (SJJ - SJ * SJ / n) < thr).to(SI.dtype)
    return box_sum(small, win) > 0


# ------------------------------------------------------------------------------------------------ KL, L2 regulariser
def kl_ref(mu, sigma, mu1=None, sigma1=None, eps: float = 1e-10):
    """KL[N(mu, sigma^2) || N(mu1, sigma1^2)] summed over features, mean over the batch; None = N(0, 1)"""
    s0 = sigma * sigma
    s1 = sigma1 * sigma1 if sigma1 is not None else torch.ones_like(s0)
    dm = (mu1 if mu1 is not None else torch.zeros_like(mu)) - mu
    term = (s0 + dm * dm) / (s1 + eps) + torch.log(s1 + eps) - torch.log(s0 + eps) - 1
    return 0.5 * term.sum() / mu.shape[0]


def l2reg_ref(df, lamb: float):
    """squared forward differences on the [1:, 1:, 1:] block, mean, times lamb * D * H * W; depth 1: the 2-D form (no depth term)"""
    D, H, W = df.shape[-3:]
    if D == 1:
        c = df[:, :, :, 1:, 1:]
        d = (c - df[:, :, :, :-1, 1:]) ** 2 + (c - df[:, :, :, 1:, :-1]) ** 2
    else:
        c = df[:, :, 1:, 1:, 1:]
        d = (c - df[:, :, :-1, 1:, 1:]) ** 2 + (c - df[:, :, 1:, :-1, 1:]) ** 2 + (c - df[:, :, 1:, 1:, :-1]) ** 2
    return d.mean() * lamb * D * H * W


# ------------------------------------------------------------------------------------------------ warp, resize
def warp_ref(df, img):
    """SpatialTransformer (grid_sample, bilinear, border, align_corners=False) on df's device and dtype"""
    return O.warp(df, img)


def warp_coords(df, img_size: Sequence[int]):
    """(3, B, D, H, W) unclamped sample coordinates in image voxels along z, y, x (what grid_sample un-normalises to)"""
    Sg = df.shape[2:]
    loc = O.identity_grid(Sg, df.dtype).to(df.device) + df
    return torch.stack([((2 * (loc[:, i] / (Sg[i] - 1) - 0.5) + 1) * img_size[i] - 1) / 2 for i in range(3)])


def lin1(v, dim: int, out_size: int, step: float):
    """linear resampling along one axis, align_corners=False: source = step * (o + 0.5) - 0.5, clamped at 0 (ATen's
    area_pixel_compute_source_index), taps i0 and min(i0 + 1, n - 1)"""
    n = v.shape[dim]
    o = torch.arange(out_size, device=v.device, dtype=v.dtype)
    s = (step * (o + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    lam = (s - i0.to(v.dtype)).reshape([-1 if d == dim % v.dim() else 1 for d in range(v.dim())])
    return v.index_select(dim, i0) * (1 - lam) + v.index_select(dim, i1) * lam


def resize_ref(x, size: Sequence[int], steps: Optional[Sequence[float]] = None):
    """trilinear F.interpolate(x, size, align_corners=False) as three separable linear passes; steps: the source step per output voxel
    along each axis (default in / out, what size= uses; F.interpolate(scale_factor=f) uses 1 / f)"""
    for k, d in enumerate((2, 3, 4)):
        step = steps[k] if steps is not None else x.shape[d] / size[k]
        x = lin1(x, d, int(size[k]), float(step))
    return x


# ------------------------------------------------------------------------------------------------ VecInt (scaling and squaring)
def self_warp_ref(d, i):
    """O.warp(d, i) for a field d and an image i of the field's own size; a depth-1 grid is the reference's 2-D case (bilinear over y and x
    with channels 1 and 2 of d, no coordinate along z: slice_ref.warp_ref), every channel of i sampled alike"""
    if d.shape[2] == 1:
        return _warp2d_ref(d[:, 1:, 0], i[:, :, 0]).unsqueeze(2)
    return O.warp(d, i)


def vecint_step_ref(w):
    """one squaring step of VecInt (network_blocks.py:173-177): w + warp(w, w), in w's dtype and on its device"""
    return w + self_warp_ref(w, w)


def vecint_chain_ref(v, nsteps: int):
    """the nsteps + 1 fields of O.vecint(v, nsteps): v / 2^nsteps, then every squaring step's result (the last one is the operator's)"""
    out = [v * (1.0 / (2 ** nsteps))]
    for _ in range(nsteps):
        out.append(vecint_step_ref(out[-1]))
    return out


def vecint_step_grads_ref(w, g, disp=None):
    """(gd, gi): the gradient of sum(g * warp(d, i)) with respect to the displacement d and to the image i, two leaves that both hold w -
    the gradient of the step w + warp(w, w) is g + gd + gi.  disp: another displacement to sample the same image with (a nudged w: gd is
    the part that jumps where a sample coordinate crosses a cell boundary; the scatter gi is continuous there)"""
    d = (w if disp is None else disp).detach().clone().requires_grad_(True)
    i = w.detach().clone().requires_grad_(True)
    gd, gi = torch.autograd.grad((self_warp_ref(d, i) * g).sum(), [d, i])
    return gd, gi


def vecint_coords(w):
    """[(axis, S, (B, D, H, W) unclamped sample coordinates of one squaring step along that axis)] for the axes longer than 1"""
    size = w.shape[2:]
    c = warp_coords(w, size)
    return [(a, size[a], c[a]) for a in range(3) if size[a] > 1]


def vecint_near_cell_boundary(w, eps: float = 1e-4):
    """(B, 3, D, H, W) bool: voxels one of whose sample coordinates lies within eps voxel of an integer, of 0 or of S - 1 (a clamp), where
    a rounded coordinate may take the other cell and the displacement gradient jumps (test_warp_vs_float64's rule)"""
    near = torch.zeros(w.shape[0], *w.shape[2:], dtype=torch.bool, device=w.device)
    for _, S, c in vecint_coords(w):
        near |= ((c - c.round()).abs() < eps) | ((c - (S - 1)).abs() < eps) | (c.abs() < eps)
    return near.unsqueeze(1).expand(*w.shape)


def vecint_clamped_at_every_face(w) -> bool:
    """some sample of the squaring step of w lies beyond each face of the volume (border padding clamps it), in every batch element"""
    return all(bool((c < 0).flatten(1).any(1).all()) and bool((c > S - 1).flatten(1).any(1).all()) for _, S, c in vecint_coords(w))


def vecint_corner_contributions(w, g, b: int, c: int, z: int, y: int, x: int):
    """[((iz, iy, ix), value)]: what voxel (z, y, x) of batch element b adds to the image-role gradient of channel c in one squaring step -
    g[b, c, z, y, x] times the trilinear weight of each corner of its sample cell (clamped coordinate, upper corner min(i0 + 1, S - 1)),
    in Python floats.  Their scatter over all voxels is vecint_step_grads_ref's gi"""
    size, pos, axes = w.shape[2:], (z, y, x), []
    for a in range(3):
        S = size[a]
        if S == 1:
            axes.append([(0, 1.0)])
            continue
        cc = ((2 * ((pos[a] + float(w[b, a, z, y, x])) / (S - 1) - 0.5) + 1) * S - 1) / 2
        cc = min(max(cc, 0.0), S - 1.0)
        i0 = int(cc // 1)
        axes.append([(i0, 1.0 - (cc - i0)), (min(i0 + 1, S - 1), cc - i0)])
    gv = float(g[b, c, z, y, x])
    return [((iz, iy, ix), gv * wz * wy * wx) for iz, wz in axes[0] for iy, wy in axes[1] for ix, wx in axes[2]]


def _coarse_to(size, nodes, B, seed):
    c = torch.randn(B, 3, *nodes, generator=torch.Generator().manual_seed(seed))
    return F.interpolate(c, size=tuple(size), mode="trilinear", align_corners=True)


def vecint_field(kind: str, B: int, size: Sequence[int], amp: float = 3.0, seed: int = 1):
    """float32 (B, 3, *size) test fields on the CPU, seeded.  A depth-1 field has a zero z channel (the 2-D form).
    smooth      inverse_ref.smooth_field: 4 control points per axis, largest |value| amp
    smooth_large  control points every 6 voxels: the value changes by about amp within one 4 x 8 x 8 tile
    bands       y and x displacements piecewise linear in y and in x with slopes -1, 0, +1 voxel per voxel in successive 6-voxel bands
                (0.97 cumsum(slope) + 0.13: no coordinate on an integer), z displacement constant: neighbouring voxels sample the same
                cell, adjacent cells and cells two apart
    noise       white noise of standard deviation amp
    zero        the zero field (not the identity for this sampler)"""
    D, H, W = size
    if kind == "smooth":
        v = smooth_field(size, amp, seed, B)
    elif kind == "smooth_large":
        v = _coarse_to(size, [max(2, -(-s // 6) + 1) for s in size], B, seed)
        v = v * (amp / float(v.abs().max()))
    elif kind == "bands":
        def ramp(n):
            slope = torch.tensor([-1.0] * 6 + [0.0] * 6 + [1.0] * 6).repeat(n // 18 + 1)[:n]
            return 0.97 * torch.cumsum(slope, 0) + 0.13
        v = torch.empty(B, 3, D, H, W)
        for b in range(B):
            v[b, 0] = 0.21 + 0.05 * b
            v[b, 1] = (ramp(H) + 0.05 * b).reshape(1, H, 1)
            v[b, 2] = (ramp(W) + 0.05 * b).reshape(1, 1, W)
    elif kind == "noise":
        v = torch.randn(B, 3, D, H, W, generator=torch.Generator().manual_seed(seed)) * amp
    elif kind == "zero":
        v = torch.zeros(B, 3, D, H, W)
    else:
        raise ValueError(kind)
    if D == 1:
        v[:, 0] = 0
        if kind in ("smooth", "smooth_large"):
            v = v * (amp / float(v.abs().max()))
    return v.contiguous()


# ------------------------------------------------------------------------------------------------ 3x3x3 convolution (ConvUnit)
def _taps(x):
    """the 27 shifted windows of the zero-padded volume, channels last: yields (kd, kh, kw, (B, D, H, W, C) view)"""
    B, C, D, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1)).permute(0, 2, 3, 4, 1)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                yield kd, kh, kw, xp[:, kd:kd + D, kh:kh + H, kw:kw + W]


def conv3_ref(x, w, b=None):
    """Conv3d(kernel 3, padding 1) in x's dtype: out[b, o, v] = bias[o] + sum over taps and channels of x[b, c, v + tap - 1] w[o, c, tap], one
    matmul over the channels per tap, accumulated in tap order (no F.conv3d: it runs in double on any device)"""
    B, C, D, H, W = x.shape
    out = None
    for kd, kh, kw, xs in _taps(x):
        t = torch.matmul(xs.reshape(-1, C), w[:, :, kd, kh, kw].t())
        out = t if out is None else out.add_(t)
    if b is not None:
        out = out + b
    return out.reshape(B, D, H, W, w.shape[0]).permute(0, 4, 1, 2, 3)


def conv3_dgrad_ref(dy, w):
    """gradient of conv3_ref with respect to x: the same convolution of dy with the transposed, tap-flipped weights"""
    return conv3_ref(dy, w.transpose(0, 1).flip(2, 3, 4))


def conv3_wgrad_ref(x, dy):
    """gradient of conv3_ref with respect to w: dw[o, c, tap] = sum over batch and voxels of x[b, c, v + tap - 1] dy[b, o, v]"""
    B, C, D, H, W = x.shape
    N = dy.shape[1]
    g = dy.permute(0, 2, 3, 4, 1).reshape(-1, N)
    dw = x.new_empty(N, C, 3, 3, 3)
    for kd, kh, kw, xs in _taps(x):
        dw[:, :, kd, kh, kw] = torch.matmul(g.t(), xs.reshape(-1, C))
    return dw


def conv3_mag(x, w, b=None):
    """A = |bias| + sum |x| |w| per output element: the magnitude sum a rounding-error bound of the convolution is proportional to"""
    return conv3_ref(x.abs(), w.abs(), None if b is None else b.abs())


def conv3_dgrad_mag(dy, w):
    return conv3_dgrad_ref(dy.abs(), w.abs())


def conv3_wgrad_mag(x, dy, random_walk: bool = False):
    """sum |x| |dy| per weight; random_walk: sqrt(sum x^2 dy^2), the size a sum of that many independently rounded terms drifts by"""
    if random_walk:
        return conv3_wgrad_ref(x * x, dy * dy).sqrt()
    return conv3_wgrad_ref(x.abs(), dy.abs())


# ------------------------------------------------------------------------------------------------ BatchNorm3d + LeakyReLU (ConvUnit)
def bn_train_ref(y, gamma, beta, eps: float = 1e-5, momentum: float = 0.1, running_mean=None, running_var=None, slope: float = 0.2):
    """training-mode BatchNorm3d + LeakyReLU of a (B, C, D, H, W) tensor in its dtype.  Returns a dict: mean, var (biased), rstd,
    scale = gamma rstd, shift = beta - mean scale, bn = y scale + shift, z = leaky_relu(bn), and - with running statistics given - their
    update (1 - momentum) old + momentum new, the variance unbiased (n / (n - 1)), as nn.BatchNorm3d does"""
    n = y.numel() // y.shape[1]
    v = lambda t: t.reshape(1, -1, 1, 1, 1)
    mean = y.mean(dim=(0, 2, 3, 4))
    var = ((y - v(mean)) ** 2).mean(dim=(0, 2, 3, 4))
    rstd = (var + eps).rsqrt()
    scale = gamma * rstd
    shift = beta - mean * scale
    bn = y * v(scale) + v(shift)
    r = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, bn=bn, z=torch.where(bn > 0, bn, slope * bn))
    if running_mean is not None:
        r["running_mean"] = (1 - momentum) * running_mean + momentum * mean
        r["running_var"] = (1 - momentum) * running_var + momentum * var * (n / max(n - 1, 1))
    return r


def bn_lrelu_bwd_ref(dz, y, mean, rstd, scale, shift, slope: float = 0.2):
    """backward of bn_train_ref's z with respect to y, gamma and beta.  dbn = dz lrelu'(y scale + shift) (slope at bn <= 0, as
    aten::leaky_relu_backward), sum_dbn and sum_dbn_c = sum dbn (y - mean) per channel, dbeta = sum_dbn, dgamma = rstd sum_dbn_c,
    dy = scale (dbn - sum_dbn / n - (y - mean) rstd^2 sum_dbn_c / n).  Returns a dict with those names"""
    n = y.numel() // y.shape[1]
    v = lambda t: t.reshape(1, -1, 1, 1, 1)
    bn = y * v(scale) + v(shift)
    dbn = torch.where(bn > 0, dz, slope * dz)
    yc = y - v(mean)
    s1 = dbn.sum(dim=(0, 2, 3, 4))
    s2 = (dbn * yc).sum(dim=(0, 2, 3, 4))
    dy = v(scale) * (dbn - v(s1) / n - yc * v(rstd * rstd * s2) / n)
    return dict(dbn=dbn, sum_dbn=s1, sum_dbn_c=s2, dbeta=s1, dgamma=rstd * s2, dy=dy)


# ------------------------------------------------------------------------------------------------ pooling, x2 up-sampling + cat
def avgpool2_ref(x):
    """AvgPool3d(2, 2, ceil_mode=True): windows that hang over the far faces are averaged over the voxels they hold (ATen's divisor without
    padding: 8, 4, 2 or 1 voxels), as zero-padded window sums over the window's voxel count"""
    D, H, W = x.shape[2:]
    xp = F.pad(x, (0, W % 2, 0, H % 2, 0, D % 2))
    B, C, Dp, Hp, Wp = xp.shape
    s = xp.reshape(B, C, Dp // 2, 2, Hp // 2, 2, Wp // 2, 2).sum(dim=(3, 5, 7))

    def cnt(n):
        c = torch.full(((n + 1) // 2,), 2.0, dtype=x.dtype, device=x.device)
        if n % 2:
            c[-1] = 1.0
        return c
    return s / (cnt(D).reshape(-1, 1, 1) * cnt(H).reshape(-1, 1) * cnt(W))


def up2_cat_ref(srcs):
    """cat([F.interpolate(s, scale_factor=2, trilinear, align_corners=False) for s in srcs], dim=1)"""
    return torch.cat([resize_ref(s, [2 * n for n in s.shape[2:]]) for s in srcs], dim=1)


# ------------------------------------------------------------------------------------------------ element-wise comparison
def ratio(got, ref, tol) -> float:
    """largest |got - ref| / tol over the elements (tol: a number or a tensor of got's shape); inf where a value is not finite"""
    err = (got.detach().to(ref.dtype) - ref.detach()).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    r = err / tol if isinstance(tol, torch.Tensor) else err / float(tol)
    return float(r.max())


def perturbed(ref, index: int, rel: float = 1e-3):
    """ref with one element (flat index) moved by rel * max|ref|: what a comparison with power must reject"""
    bad = ref.detach().clone(memory_format=torch.contiguous_format)
    bad.view(-1)[index] += rel * float(ref.detach().abs().max())
    return bad


# ------------------------------------------------------------------------------------------------ bf16-stored results
BF16_MIN_EXP = -133                     # log2 of the bf16 subnormal spacing (the smallest binade's ulp)


def bf16_grid(r):
    """(ulp, q) of a float64 tensor on the bf16 grid: ulp = the spacing of bf16 values in r's binade (8 significant bits; the subnormal
    spacing below 2^-126), q = |r| / ulp: 128 <= q < 256 for normal values.  Both exact: the powers of two are assembled from their exponent
    bits (torch.ldexp multiplies by pow(2, n), which a GPU's pow may round) and q is a product with one"""
    a = r.abs()
    e = ((a.view(torch.int64) >> 52) - 1022 - 8).clamp_min(BF16_MIN_EXP)          # frexp's exponent of |r|, less the 8 significant bits
    ulp = ((e + 1023) << 52).view(torch.float64)
    return ulp, a * ((1023 - e) << 52).view(torch.float64)


def rne_bf16(r):
    """a float64 tensor rounded to the nearest bf16 value, ties to even, in ONE rounding (r.float().bfloat16() rounds twice), as float64"""
    ulp, q = bf16_grid(r)
    fl = torch.floor(q)
    frac = q - fl                                            # (exact: q has at most 53 - 8 fraction bits)
    up = (frac > 0.5) | ((frac == 0.5) & (torch.remainder(fl, 2) == 1))       # half to even, spelled out; 255.5 -> 256: the next binade's first value
    return torch.sign(r) * (fl + up) * ulp


def bf16_midpoint_distance(r):
    """distance from r to the nearest midpoint between two adjacent bf16 values.  Inside a binade the midpoints are (k + 1/2) ulp; just above
    a power of two the midpoint below it belongs to the finer binade underneath, (128 - 1/4) ulp.  0 for r = 0 (its neighbours' midpoints
    are 2^-134 away)"""
    ulp, q = bf16_grid(r)
    fl = torch.floor(q)
    d = (q - (fl + 0.5)).abs()
    d = torch.where(fl == 128, torch.minimum(d, q - 127.75), d)
    return torch.where(r == 0, torch.zeros_like(r), d * ulp)


def judge_bf16(got, ref, T, exempt=None):
    """the two rules a bf16-storing kernel is held to (its fp32 value v obeys |v - ref| <= T and it stores RNE_bf16(v)):
      1. got is finite and |got - ref| <= T + 2^-8 (|ref| + T): half a bf16 ulp at the far end of the interval;
      2. where ref lies farther than T from every midpoint between adjacent bf16 values (or T = 0: the arithmetic is exact, ties included),
         v rounds as ref does: got == RNE_bf16(ref) bit for bit (int16 views; +0 and -0 count as equal).
    exempt: elements taken out of rule 2 on top (bool).  Returns (rule-1 ratio, covered mask, mismatch mask among the covered)"""
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float64 and got.shape == ref.shape
    T = T if isinstance(T, torch.Tensor) else torch.full_like(ref, float(T))
    r1 = ratio(got, ref, T + 2.0 ** -8 * (ref.abs() + T) + 1e-300)
    covered = (bf16_midpoint_distance(ref) > T) | (T == 0)
    if exempt is not None:
        covered &= ~exempt
    want = rne_bf16(ref).to(torch.bfloat16)
    g = got.contiguous()
    same = (g.view(torch.int16) == want.view(torch.int16)) | ((g == 0) & (want == 0))
    return r1, covered, covered & ~same


def held_bf16(name, got, ref, T, cap, power=None, exempt=None):
    """judge_bf16 asserted.  Prints RATIO (rule 1) and NEARMID (the share of elements outside rule 2), asserts that share <= cap, and shows
    power: ref with ONE element moved by one bf16 ulp of that element must be rejected.  power: the channel of the last voxel of the last
    batch element to move (default: the last one that rule 2 covers in the interior of its binade - one must exist)"""
    r1, covered, bad = judge_bf16(got, ref, T, exempt)
    share = 1.0 - float(covered.double().mean())
    print(f"RATIO {name} {r1:.3g}")
    print(f"NEARMID {name} {share:.4g}")
    if bool(bad.any()):
        i = int(bad.reshape(-1).to(torch.int8).argmax())
        idx = []
        for n in reversed(ref.shape):
            idx.append(i % n)
            i //= n
        idx = tuple(reversed(idx))
        print(f"WORST {name} first of {int(bad.sum())} bit mismatches at {idx} of {tuple(ref.shape)}: got {float(got[idx])!r} ref {float(ref[idx])!r}")
    assert r1 <= 1.0, f"{name}: rule 1, max error / (T + 2^-8 (|ref| + T)) = {r1:.3g}"
    assert not bool(bad.any()), f"{name}: rule 2, {int(bad.sum())} of {int(covered.sum())} covered elements are not RNE_bf16(ref)"
    assert share <= cap, f"{name}: {share:.4g} of the elements lie within T of a bf16 midpoint (cap {cap}): the inputs leave rule 2 too little to check"
    last = (ref.shape[0] - 1, slice(None)) + tuple(n - 1 for n in ref.shape[2:])
    _, q = bf16_grid(ref[last])
    if power is None:
        ok = covered[last] & (q >= 130) & (q <= 253)
        assert bool(ok.any()), f"{name}: no channel of the last voxel is covered by rule 2"
        power = int(ok.nonzero()[-1])
    assert bool(covered[last][power]), f"{name}: power channel {power} is not covered by rule 2"
    moved = ref.detach().clone(memory_format=torch.contiguous_format)
    at = (ref.shape[0] - 1, power) + tuple(n - 1 for n in ref.shape[2:])
    moved[at] += bf16_grid(ref[at])[0]
    r1m, _, badm = judge_bf16(got, moved, T, exempt)
    assert r1m > 1.0 or bool(badm.any()), f"{name}: a one-ulp error in channel {power} of the last voxel is not rejected"
