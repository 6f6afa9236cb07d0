"""Cost-function masking in plain torch, in the dtype and on the device of its arguments (the tests call it in
float64): the definitions the masked HIP kernels are held to.  m = mask * mask2 weights the per-voxel cost; the window sums of the
local correlation run over all voxels; every loss is normalised by M = sum(m) and is 0 for an empty mask."""
from typing import Optional, Sequence

import torch

import pyramid_ref as R


def product(mask, mask2=None):
    return mask if mask2 is None else mask * mask2


def ball(B: int, size: Sequence[int], outer: float = 0.9, inner: float = 0.35, device="cpu"):
    """(B,1,*size) fp32 mask: 1 between the radii `inner` and `outer` (cell centres on [-1, 1]: an axis of extent 1 sits at 0) - a ball
    with a hole; the batch rows are the same"""
    axes = [(torch.arange(s, device=device, dtype=torch.float32) + 0.5) * (2.0 / s) - 1.0 for s in size]
    grids = torch.meshgrid(*axes, indexing="ij")
    r2 = sum(g * g for g in grids)
    m = ((r2 <= outer * outer) & (r2 >= inner * inner)).float()
    return m[None, None].expand(B, 1, *size).contiguous()


def cc_map(pred, true, win: int):
    """the reference's local squared correlation per voxel (src/losses.py:113-132: zero-padded win^ndims window, 1e-8)"""
    I, J, n, SI, SJ, SII, SJJ, SIJ = R._ncc_terms(pred, true, win)
    uI, uJ = SI / n, SJ / n
    cross = SIJ - uJ * SI - uI * SJ + uI * uJ * n
    Iv = SII - 2 * uI * SI + uI * uI * n
    Jv = SJJ - 2 * uJ * SJ + uJ * uJ * n
    return cross * cross / (Iv * Jv + 1e-8)


def _voxels(t) -> int:
    v = 1
    for s in t.shape[2:]:
        v *= int(s)
    return v


def ncc_masked_ref(pred, true, mask, mask2, win: int, gamma: float):
    """-gamma V sum(m cc) / M, exactly 0 when M == 0"""
    m = product(mask, mask2).to(pred.dtype)
    M = m.sum()
    if float(M) == 0.0:
        return torch.zeros((), dtype=pred.dtype, device=pred.device)
    return -gamma * _voxels(pred) * torch.sum(m * cc_map(pred, true, win)) / M


def ncc_masked_grad_ref(pred, true, mask, mask2, win: int, gamma: float):
    """d ncc_masked_ref / d pred in closed form: -gamma V / M (box(m a) + 2 J box(m b) + I box(m c)), the a, b, c of R.ncc_grad_ref"""
    m = product(mask, mask2).to(pred.dtype)
    M = m.sum()
    if float(M) == 0.0:
        return torch.zeros_like(pred)
    I, J, n, SI, SJ, SII, SJJ, SIJ = R._ncc_terms(pred, true, win)
    cross = SIJ - SI * SJ / n
    Iv = SII - SI * SI / n
    Jv = SJJ - SJ * SJ / n
    Dn = Iv * Jv + 1e-8
    a = -2 * cross * SI / (n * Dn) + 2 * cross * cross * Iv * SJ / (n * Dn * Dn)
    b = -cross * cross * Iv / (Dn * Dn)
    c = 2 * cross / Dn
    return -(gamma * _voxels(pred) / M) * (R.box_sum(m * a, win) + 2 * J * R.box_sum(m * b, win) + I * R.box_sum(m * c, win))


def l2_masked_ref(a, b, mask, mask2=None):
    """V sum(m (a - b)^2) / (C M), m broadcast over the channels, 0 when M == 0"""
    m = product(mask, mask2).to(a.dtype)
    M = m.sum()
    if float(M) == 0.0:
        return torch.zeros((), dtype=a.dtype, device=a.device)
    return _voxels(a) * torch.sum(m * (a - b) ** 2) / (a.shape[1] * M)


def rmse_masked_ref(a, b, mask, mask2=None):
    """(sqrt(L2_masked / V), MaskFrac = M / (B V))"""
    m = product(mask, mask2).to(a.dtype)
    V = _voxels(a)
    return torch.sqrt(l2_masked_ref(a, b, mask, mask2) / V), m.sum() / (a.shape[0] * V)


def outside_reach(mask, mask2, win: int):
    """bool (B,1,...): voxels whose win^3 window holds no voxel with m > 0, i.e. farther than win // 2 (Chebyshev) from the mask's support:
    they cannot change the masked loss, and its gradient there is exactly 0"""
    m = product(mask, mask2)
    return R.box_sum((m > 0).double(), win) == 0
