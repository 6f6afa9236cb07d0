"""float64 references of the training step's head, loss and field operators, written with plain torch ops (einsum, softplus, cumsum,
index_select, grid_sample) so that they also run on the GPU at the pyramid's sizes, and the element-wise comparison the pyramid tests use.
tests/test_oracle_golden.py pins every helper to oracle/pulpo_oracle.py at small shapes; tests/test_gpu_pyramid_ops.py holds the HIP kernels
to them."""
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
