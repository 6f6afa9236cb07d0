"""The 2-D (slice) mode's operators written in 2-D: plain torch functions on (B, C, H, W) tensors with torch's native 2-D operators, in the
dtype of their arguments (float64 or float32) and on their device.  Nothing here lifts a slice to a depth-1 volume, so that the lifting
of pulpo_amd/ops.py (3x3 taps in the middle slice of a 3x3x3 weight, (y, x) fields as (0, y, x), padded head rows, the identity depth
mapping of the resize) is under test wherever a kernel is compared with these.  tests/test_host_slice_ref.py pins every function to the
reference-derived arrays of tests/golden/ops2d.npz; tests/test_gpu_slices.py holds the HIP kernels to them."""
from typing import Optional, Sequence

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ 3x3 convolution
def conv2_ref(x, w, b=None):
    """Conv2d(kernel 3, padding 1): w (Cout, Cin, 3, 3)"""
    return F.conv2d(x, w, b, padding=1)


def conv2_grads_ref(x, w, dy):
    """(dx, dw) of conv2_ref for the upstream gradient dy, by autograd through F.conv2d"""
    xg, wg = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    return torch.autograd.grad(F.conv2d(xg, wg, None, padding=1), [xg, wg], grad_outputs=dy)


def conv2_mag(x, w, b=None):
    """sum |x| |w| (+ |b|) per output element: what a rounding-error bound of the convolution is proportional to"""
    return conv2_ref(x.abs(), w.abs(), None if b is None else b.abs())


def conv2_grads_mag(x, w, dy):
    return conv2_grads_ref(x.abs(), w.abs(), dy.abs())


# ------------------------------------------------------------------------------------------------ BatchNorm2d + LeakyReLU
def _ch(t):
    return t.reshape(1, -1, 1, 1)


def bn_train_ref(y, gamma, beta, eps: float = 1e-5, momentum: float = 0.1, running_mean=None, running_var=None, slope: float = 0.2):
    """training-mode BatchNorm2d + LeakyReLU (the formulas of pyramid_ref.bn_train_ref over (B, H, W)): mean, biased var, rstd, scale, shift,
    bn, z, and the running statistics' update with the unbiased variance"""
    n = y.numel() // y.shape[1]
    mean = y.mean(dim=(0, 2, 3))
    var = ((y - _ch(mean)) ** 2).mean(dim=(0, 2, 3))
    rstd = (var + eps).rsqrt()
    scale = gamma * rstd
    shift = beta - mean * scale
    bn = y * _ch(scale) + _ch(shift)
    r = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, bn=bn, z=torch.where(bn > 0, bn, slope * bn))
    if running_mean is not None:
        r["running_mean"] = (1 - momentum) * running_mean + momentum * mean
        r["running_var"] = (1 - momentum) * running_var + momentum * var * (n / max(n - 1, 1))
    return r


def bn_lrelu_bwd_ref(dz, y, mean, rstd, scale, shift, slope: float = 0.2):
    """backward of bn_train_ref's z with respect to y, gamma and beta (pyramid_ref.bn_lrelu_bwd_ref over (B, H, W))"""
    n = y.numel() // y.shape[1]
    bn = y * _ch(scale) + _ch(shift)
    dbn = torch.where(bn > 0, dz, slope * dz)
    yc = y - _ch(mean)
    s1 = dbn.sum(dim=(0, 2, 3))
    s2 = (dbn * yc).sum(dim=(0, 2, 3))
    dy = _ch(scale) * (dbn - _ch(s1) / n - yc * _ch(rstd * rstd * s2) / n)
    return dict(dbn=dbn, dbeta=s1, dgamma=rstd * s2, dy=dy)


def bn_eval_ref(y, gamma, beta, running_mean, running_var, eps: float = 1e-5, slope: float = 0.2):
    """eval-mode BatchNorm2d + LeakyReLU"""
    bn = (y - _ch(running_mean)) * _ch(gamma * (running_var + eps).rsqrt()) + _ch(beta)
    return torch.where(bn > 0, bn, slope * bn)


def conv_unit_train_ref(x, w, b, gamma, beta, running_mean, running_var, up, eps: float = 1e-5, momentum: float = 0.1, slope: float = 0.2):
    """ConvUnit (Conv2d 3x3 + BatchNorm2d + LeakyReLU(0.2)) in training mode, forward and backward for the upstream gradient `up`:
    a dict with out, running_mean, running_var, dx, dw, db (the convolution's bias gradient: the sum of dy, zero in exact arithmetic),
    dgamma, dbeta and the intermediate y, bn, dy"""
    y = conv2_ref(x, w, b)
    f = bn_train_ref(y, gamma, beta, eps, momentum, running_mean, running_var, slope)
    bw = bn_lrelu_bwd_ref(up, y, f["mean"], f["rstd"], f["scale"], f["shift"], slope)
    dx, dw = conv2_grads_ref(x, w, bw["dy"])
    return dict(out=f["z"], running_mean=f["running_mean"], running_var=f["running_var"], dx=dx, dw=dw, db=bw["dy"].sum(dim=(0, 2, 3)),
                dgamma=bw["dgamma"], dbeta=bw["dbeta"], y=y, bn=f["bn"], dy=bw["dy"], scale=f["scale"])


def conv_unit_eval_ref(x, w, b, gamma, beta, running_mean, running_var, eps: float = 1e-5, slope: float = 0.2):
    return bn_eval_ref(conv2_ref(x, w, b), gamma, beta, running_mean, running_var, eps, slope)


# ------------------------------------------------------------------------------------------------ pooling, bilinear resize
def avgpool2_ref(x):
    """AvgPool2d(2, 2, ceil_mode=True): windows over the far edges average the pixels they hold"""
    return F.avg_pool2d(x, 2, 2, 0, ceil_mode=True)


def resize_ref(x, size: Optional[Sequence[int]] = None, scale_factor: Optional[float] = None):
    """bilinear F.interpolate(align_corners=False), in the size= form (source step in / out) or the scale_factor= form (source step
    1 / scale_factor, output size floor(in * scale_factor))"""
    if scale_factor is not None:
        return F.interpolate(x, scale_factor=scale_factor, mode="bilinear", align_corners=False)
    return F.interpolate(x, size=tuple(int(s) for s in size), mode="bilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ warp, VecInt
def warp_coords(df, img_size: Sequence[int]):
    """(2, B, H, W): the unclamped sample coordinates along y and x, in pixels of the image, that warp_ref interpolates at"""
    Hg, Wg = df.shape[2:]
    ys, xs = torch.meshgrid(torch.arange(Hg, dtype=df.dtype, device=df.device), torch.arange(Wg, dtype=df.dtype, device=df.device), indexing="ij")
    out = []
    for pos, d, n, S in ((ys, df[:, 0], Hg, img_size[0]), (xs, df[:, 1], Wg, img_size[1])):
        norm = 2 * ((pos + d) / (n - 1) - 0.5)                  # the grid's own extent maps to [-1, 1] ...
        out.append(((norm + 1) * S - 1) / 2)                    # ... which grid_sample(align_corners=False) reads as pixel centres of the image
    return torch.stack(out)


def warp_ref(df, img):
    """the 2-D SpatialTransformer: displacement df (B, 2, Hg, Wg) with channels (y, x) in pixels of its own grid; every grid position p
    samples the image at p + df(p), normalised by the GRID's size - 1 to [-1, 1] per axis and read by grid_sample (bilinear, border padding,
    align_corners=False, which wants the last axis ordered (x, y)).  A zero field is therefore not the identity, and the image may be
    larger than the grid"""
    Hg, Wg = df.shape[2:]
    ys, xs = torch.meshgrid(torch.arange(Hg, dtype=df.dtype, device=df.device), torch.arange(Wg, dtype=df.dtype, device=df.device), indexing="ij")
    ny = 2 * ((ys + df[:, 0]) / (Hg - 1) - 0.5)
    nx = 2 * ((xs + df[:, 1]) / (Wg - 1) - 0.5)
    return F.grid_sample(img, torch.stack([nx, ny], dim=-1), mode="bilinear", padding_mode="border", align_corners=False)


def vecint_ref(v, nsteps: int = 7):
    """scaling and squaring: v / 2^nsteps, then nsteps times v <- v + warp(v, v)"""
    v = v * (1.0 / 2 ** nsteps)
    for _ in range(nsteps):
        v = v + warp_ref(v, v)
    return v


# ------------------------------------------------------------------------------------------------ 1x1 heads (zdim = 2)
def conv1x1_ref(h, w, b):
    """Conv2d(C, n, kernel_size=1): w (n, C, 1, 1) - a channel mix per pixel plus the bias"""
    return torch.einsum("bchw,jc->bjhw", h, w.reshape(w.shape[0], h.shape[1])) + b.reshape(1, -1, 1, 1)


def mu_sigma_ref(h, w_mu, b_mu, w_sigma, b_sigma, eps: Optional[torch.Tensor]):
    """MuSigmaBlock + sampler: mu = W_mu h + b_mu, sigma = softplus(W_sigma h + b_sigma), z = mu + sigma eps (eps None: z = mu)"""
    mu = conv1x1_ref(h, w_mu, b_mu)
    sigma = F.softplus(conv1x1_ref(h, w_sigma, b_sigma))
    return mu, sigma, (mu if eps is None else mu + sigma * eps)
