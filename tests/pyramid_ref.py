"""float64 references of the training step's head, loss, field and ConvUnit operators, written with plain torch ops (matmul, einsum,
softplus, cumsum, index_select, grid_sample) so that they also run on the GPU at the pyramid's sizes, and the element-wise comparison the
pyramid tests use.  tests/test_oracle_golden.py pins every helper to oracle/pulpo_oracle.py and torch.nn.functional at small shapes;
tests/test_gpu_pyramid_ops.py and tests/test_gpu_pyramid_convunit.py hold the HIP kernels to them."""
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import pulpo_oracle as O


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
