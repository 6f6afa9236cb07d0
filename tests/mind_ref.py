"""MIND-SSC in plain torch, in the dtype and on the device of its arguments (the tests call it in float64): the
definition the HIP kernels of mind.hip are held to.

    offsets e0..e5 = -z, +z, -y, +y, -x, +x, times the dilation d; c(.) clamps every coordinate into its extent (replication padding)
    channel k = offset pair (a, b) of PAIRS:   S_k(p) = (I(c(p + d e_a)) - I(c(p + d e_b)))^2
    D_k(p) = 1/27 sum over q in {-1,0,1}^3 of S_k(c(p + q)),   m_k = D_k - min_j D_j,   V = mean_k m_k + eps,   f_k = exp(-m_k / V)
    cost(p) = 1/12 sum_k (f_k[pred] - f_k[true])^2;  loss = 1/B sum_b sum_p cost;  masked: Vox sum(m cost) / M, exactly 0 when M == 0
"""
from typing import Sequence

import torch

PAIRS = ((0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (3, 5))
OFFSETS = ((2, -1), (2, +1), (3, -1), (3, +1), (4, -1), (4, +1))          # (tensor dim, sign) of e0..e5 on a (B,1,D,H,W) tensor


def _shift(t, dim: int, by: int):
    """t at the clamped coordinate p + by along dim"""
    n = t.shape[dim]
    idx = (torch.arange(n, device=t.device) + by).clamp_(0, n - 1)
    return t.index_select(dim, idx)


def _box3(t):
    """clamped 3x3x3 box mean: three clamped 1-D means"""
    for dim in (2, 3, 4):
        t = (_shift(t, dim, -1) + t + _shift(t, dim, 1)) / 3
    return t


def descriptor(img, dilation: int = 2, eps: float = 1e-5):
    """(B,1,D,H,W) -> (B,12,D,H,W)"""
    assert img.dim() == 5 and img.shape[1] == 1
    nb = [_shift(img, dim, sign * dilation) for dim, sign in OFFSETS]
    D = torch.cat([_box3((nb[a] - nb[b]) ** 2) for a, b in PAIRS], dim=1)
    m = D - D.min(dim=1, keepdim=True).values
    V = m.mean(dim=1, keepdim=True) + eps
    return torch.exp(-m / V)


def cost_map(pred, true, dilation: int = 2, eps: float = 1e-5):
    """(B,1,D,H,W): the per-voxel cost"""
    return ((descriptor(pred, dilation, eps) - descriptor(true, dilation, eps)) ** 2).mean(dim=1, keepdim=True)


def loss(pred, true, dilation: int = 2, eps: float = 1e-5):
    return cost_map(pred, true, dilation, eps).sum() / pred.shape[0]


def loss_masked(pred, true, mask, mask2=None, dilation: int = 2, eps: float = 1e-5):
    m = (mask if mask2 is None else mask * mask2).to(pred.dtype)
    M = m.sum()
    if float(M) == 0.0:
        return pred.sum() * 0.0
    vox = pred.shape[2] * pred.shape[3] * pred.shape[4]
    return vox * (m * cost_map(pred, true, dilation, eps)).sum() / M


def grad(pred, true, dilation: int = 2, eps: float = 1e-5, mask=None, mask2=None, upstream: float = 1.0):
    """upstream * d loss / d pred by autograd (the masked loss when a mask is given)"""
    p = pred.detach().clone().requires_grad_(True)
    val = loss(p, true, dilation, eps) if mask is None else loss_masked(p, true, mask, mask2, dilation, eps)
    (val * upstream).backward()
    return p.grad


def noise(B: int, size: Sequence[int], seed: int, smooth: int = 0, dtype=torch.float64, device="cpu"):
    """(B,1,*size) uniform noise in [0,1), passed `smooth` times through the clamped 3^3 box mean: free of ties in min_j D_j"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand((B, 1) + tuple(size), generator=g, dtype=torch.float64)
    for _ in range(smooth):
        t = _box3(t)
    return t.to(dtype).to(device)


# The loss of a one-voxel shift against an inverted copy is at least this many times the aligned pair's.  In float64 the aligned loss is
# rounding noise (5e-28 against 146 at 16^3); in fp32 it is the squared descriptor error summed over the voxels, 1.1e-10 on a CPU - a
# factor of 1e6 leaves four decades to either.
SHIFT_FACTOR = 1e6


def shifted_pair():
    """(a, 1 - a, a shifted by one voxel along x): twice box-filtered noise at 16^3, float64"""
    a = noise(1, (16, 16, 16), 5, smooth=2)
    return a, 1.0 - a, _shift(a, 4, 1)
