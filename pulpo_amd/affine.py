"""Affine pre-alignment: fit the twelve (or six) parameters of an affine transform that brings a moving image onto a fixed one, and the small
algebra around such transforms.

    res = affine.fit(x, y)                                   # x moving, y fixed; res["theta"] (B,3,4), res["history"]
    x_aff = ops.affine_warp(res["theta"], x)                 # what the network sees
    field = ops.affine_compose(res["theta"], final_df)       # "affine, then deformable" as one field: one interpolation for labels / landmarks

Conventions.  theta = [M | t] in voxel units of a stated grid (D,H,W), about the grid's centre c = (size - 1) / 2: voxel v is sent to
p = c + M (v - c) + t, and ops.affine_warp(theta, img) samples img where the SpatialTransformer would with the displacement p - v.  That
sampler normalises by S - 1 but samples with align_corners=False: its index is s(p) = p S / (S - 1) - 0.5, so a zero displacement is not the
identity, and the transform that undoes x = affine_warp(A, y) is S^-1 A^-1 S^-1 (expected_fit), not A^-1.  Slices use (B,2,3).  No
reference counterpart: the reference's pairs arrive affinely aligned by an outside tool."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import ops

LOSSES = ("ncc", "mse", "mind", "mi")
# Step size and iterations per level, coarsest first, of fit().  A float64 sweep of the fitter's definition on the CPU (DESIGN.md section 3m has
# the table): lr in {0.003, 0.01, 0.03} x iterations {15/20/30, 30/40/60, 60/80/120} on one synthetic pair at 32^3 and 24x32x28, NCC and MSE.
# Every setting with 130 iterations or more ends between 0.30 and 0.49 voxels of corner error, a spread one pair cannot resolve; halving the
# iterations costs up to 1.0 voxel at lr 0.003 and 0.64 at 0.01.  Kept: the middle of the grid.  Windows: the NCC window per level.
DEFAULT_LR = 0.01
DEFAULT_ITERS = (30, 40, 60)
DEFAULT_WIN = (9, 7, 5)
# Joint-histogram bins of the "mi" term per level, coarsest first: an 8^3 level has 512 voxels, too few for 32 x 32 joint bins
DEFAULT_MI_BINS = (16, 16, 32)


# ------------------------------------------------------------------------------------------------ helpers (tiny torch algebra, off the hot path)
def identity(B: int, device, ndims: int = 3) -> torch.Tensor:
    """[I | 0]: (B,3,4), or (B,2,3) for ndims = 2"""
    if ndims not in (2, 3):
        raise ValueError("identity: ndims 2 or 3")
    return torch.eye(ndims, ndims + 1, device=device, dtype=torch.float32).unsqueeze(0).repeat(int(B), 1, 1)


def _centre(size, like: torch.Tensor) -> torch.Tensor:
    return torch.tensor([(int(s) - 1) / 2.0 for s in size], device=like.device, dtype=torch.float64)


def _to_abs(theta: torch.Tensor, size) -> torch.Tensor:
    """(B,n+1,n+1) float64 in absolute voxel coordinates: p = M v + (c - M c + t)"""
    n = theta.shape[1]
    if theta.dim() != 3 or theta.shape[2] != n + 1 or n not in (2, 3) or len(size) != n:
        raise ValueError(f"theta (B,3,4) with a size of 3 extents, or (B,2,3) with 2, expected; got {tuple(theta.shape)} and {tuple(size)}")
    th, c = theta.double(), _centre(size, theta)
    A = torch.zeros(theta.shape[0], n + 1, n + 1, device=theta.device, dtype=torch.float64)
    A[:, :n, :n] = th[:, :, :n]
    A[:, :n, n] = c - th[:, :, :n] @ c + th[:, :, n]
    A[:, n, n] = 1.0
    return A


def _from_abs(A: torch.Tensor, size, dtype) -> torch.Tensor:
    n = A.shape[1] - 1
    c, M = _centre(size, A), A[:, :n, :n]
    return torch.cat([M, (A[:, :n, n] - c + M @ c).unsqueeze(2)], dim=2).to(dtype)


def invert(theta: torch.Tensor, size) -> torch.Tensor:
    """the inverse transform on the same grid (4 x 4 algebra in float64)"""
    return _from_abs(torch.linalg.inv(_to_abs(theta, size)), size, theta.dtype)


def rescale(theta: torch.Tensor, from_size, to_size) -> torch.Tensor:
    """the same physical transform on a grid of another resolution: with r = to / from per axis, M_ab r_a / r_b and t_a r_a"""
    n = theta.shape[1]
    if len(from_size) != n or len(to_size) != n:
        raise ValueError("rescale: sizes of theta's dimension expected")
    r = torch.tensor([float(t) / float(f) for f, t in zip(from_size, to_size)], device=theta.device, dtype=torch.float64)
    th = theta.double()
    return torch.cat([th[:, :, :n] * r.view(1, n, 1) / r.view(1, 1, n), (th[:, :, n] * r).unsqueeze(2)], dim=2).to(theta.dtype)


def _sampler_matrix(size, like: torch.Tensor) -> torch.Tensor:
    n = len(size)
    S = torch.eye(n + 1, device=like.device, dtype=torch.float64)
    for a, s in enumerate(size):
        if int(s) > 1:
            S[a, a] = int(s) / (int(s) - 1.0)
            S[a, n] = -0.5
    return S


def expected_fit(theta_gen: torch.Tensor, size) -> torch.Tensor:
    """the transform that maps x = ops.affine_warp(theta_gen, y) back onto y on one grid: S^-1 A_gen^-1 S^-1 as 4 x 4 matrices, S the sampler's
    own map s(p) = p S / (S - 1) - 0.5.  Its own inverse: expected_fit(expected_fit(A)) = A."""
    Sinv = torch.linalg.inv(_sampler_matrix(size, theta_gen))
    return _from_abs(Sinv @ torch.linalg.inv(_to_abs(theta_gen, size)) @ Sinv, size, theta_gen.dtype)


def corner_error(theta_a: torch.Tensor, theta_b: torch.Tensor, size) -> torch.Tensor:
    """largest distance in voxels, over the batch and the corners of the grid, between where the two transforms send a corner (0-d tensor)"""
    n = theta_a.shape[1]
    corners = torch.cartesian_prod(*[torch.tensor([0.0, int(s) - 1.0], dtype=torch.float64) for s in size]).to(theta_a.device)
    pts = torch.cat([corners, torch.ones_like(corners[:, :1])], dim=1).t()                      # (n+1, 2^n)
    d = (_to_abs(theta_a, size) - _to_abs(theta_b, size)) @ pts
    return d[:, :n].norm(dim=1).max()


# ------------------------------------------------------------------------------------------------ the fitter
def _skew(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1), torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def _theta_of(P: torch.Tensor, r: float, dof: int, nd: int) -> torch.Tensor:
    """theta in voxels from the normalised parameters.  3-D: dof 12: M = I + P[:9], t = r P[9:]; dof 6: M = exp(skew(P[:3])), t = r P[3:].
    2-D: dof 12 means the six entries of a (2,3) transform, dof 6 a rotation angle and a translation."""
    if nd == 3:
        M = (torch.eye(3, device=P.device, dtype=P.dtype) + P[:, :9].view(-1, 3, 3)) if dof == 12 else torch.linalg.matrix_exp(_skew(P[:, :3]))
        return torch.cat([M, (r * P[:, -3:]).unsqueeze(2)], dim=2)
    if dof == 12:
        M = torch.eye(2, device=P.device, dtype=P.dtype) + P[:, :4].view(-1, 2, 2)
    else:
        c, s = torch.cos(P[:, 0]), torch.sin(P[:, 0])
        M = torch.stack([torch.stack([c, -s], 1), torch.stack([s, c], 1)], 1)
    return torch.cat([M, (r * P[:, -2:]).unsqueeze(2)], dim=2)


def _params_of(theta: torch.Tensor, r: float, dof: int, nd: int) -> torch.Tensor:
    """the normalised parameters of a start transform (dof 6: the rotation nearest in the sense of its skew part, angle below pi)"""
    th = theta.detach().double()
    t, M = th[:, :, nd] / r, th[:, :, :nd]
    if dof == 12:
        return torch.cat([(M - torch.eye(nd, device=M.device, dtype=M.dtype)).reshape(-1, nd * nd), t], dim=1).float()
    if nd == 2:
        return torch.cat([torch.atan2(M[:, 1, 0] - M[:, 0, 1], M[:, 0, 0] + M[:, 1, 1]).unsqueeze(1), t], dim=1).float()
    w = torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], 1) / 2          # sin(angle) x axis
    s = w.norm(dim=1, keepdim=True)
    ang = torch.atan2(s, (M.diagonal(dim1=1, dim2=2).sum(1, keepdim=True) - 1) / 2)
    return torch.cat([torch.where(s > 1e-12, w * ang / s.clamp_min(1e-300), w), t], dim=1).float()


def _per_level(given, default, levels: int):
    """one entry per level, coarsest first: the given ones, or the default's last `levels` (its first repeated for deeper pyramids)"""
    if given is not None:
        return tuple(given)
    return tuple(default[-levels:]) if levels <= len(default) else (default[0],) * (levels - len(default)) + tuple(default)


def fit(x: torch.Tensor, y: torch.Tensor, *, dof: int = 12, levels: int = 3, iters: Optional[Sequence[int]] = None, lr: float = DEFAULT_LR,
        loss: str = "ncc", win: Optional[Sequence[int]] = None, mask_x: Optional[torch.Tensor] = None, mask_y: Optional[torch.Tensor] = None,
        theta0: Optional[torch.Tensor] = None, mi_bins=None) -> Dict[str, torch.Tensor]:
    """Fit the affine transform that brings the moving image x onto the fixed image y (both (B,1,D,H,W), or (B,1,H,W) slices, on one grid):
    minimise loss(ops.affine_warp(theta, x), y) over theta, coarse to fine.

    dof       12: a full affine, M = I + P[:9]; 6: rigid, M = matrix_exp(skew(omega)); each plus a translation (slices: 6 and 3 parameters).
              Anything else raises ValueError.
    levels    pyramid levels: ops.avg_pool2 pyramids of both images (and masks), the coarsest level first.
    iters     Adam iterations per level, coarsest first (default DEFAULT_ITERS, for another level count its last `levels` entries repeated
              as needed); lr the step size (DEFAULT_LR).  Adam starts from zero moments at every level.
    loss      "ncc" (window win[k] at the k-th level visited, default DEFAULT_WIN), "mse" or "mind" (3-D only, NotImplementedError on slices
              as ops.mind_loss) or "mi" (mutual information, for pairs of different contrast; images in [0,1]): the project's similarity
              terms, with gamma = 1 - sums over the level's voxels, so rows of history from different levels are not on one scale.
    mi_bins   joint-histogram bins of "mi": an int, or one entry per level, coarsest first, like win (default DEFAULT_MI_BINS).
    mask_x / mask_y   weight volumes (B,1,...) of the moving / the fixed image: the masked forms of the terms.  mask_x is re-warped by the
              current transform every iteration, without gradient (ops.warp_mask(ops.affine_field(theta), mask_x)), as the training step
              re-warps it by the current field.
    theta0    the start (default the identity), in voxels of the full grid.
    The parameters live in a normalised frame: coordinates divided by one scalar r = (max(size) - 1) / 2, halved per level, so a step of lr in a
    matrix entry and in a translation entry move the volume's edge by the same amount, and one parameter vector serves every level.  The
    update is ops.anchored_adam_step(mean=None) on the (B, n) parameter tensor; the few-element torch ops from it to theta carry autograd
    down to ops.affine_warp's gradient kernel.  Nothing in the loop synchronises with the host or touches a weight pack; under
    ops.set_deterministic(True) two calls give the same bits.

    Returns {"theta": (B,3,4) (slices: (B,2,3)) in voxels of the full grid, "history": device tensor (sum(iters) + 1, 2) = (loss, level);
    row i is the loss at the iterate before step i, the last row an extra forward pass at the result on the full grid}."""
    if dof not in (6, 12):
        raise ValueError(f"affine.fit: dof {dof} - 12 (affine) or 6 (rigid) expected")
    if loss not in LOSSES:
        raise ValueError(f"affine.fit: loss {loss!r} - one of {LOSSES} expected")
    if x.dim() not in (4, 5) or x.shape != y.shape or x.shape[1] != 1:
        raise ValueError(f"affine.fit: a moving and a fixed image (B,1,D,H,W) or (B,1,H,W) on one grid expected, got {tuple(x.shape)} and {tuple(y.shape)}")
    levels = int(levels)
    if levels < 1:
        raise ValueError("affine.fit: levels >= 1 expected")
    iters, win = _per_level(iters, DEFAULT_ITERS, levels), _per_level(win, DEFAULT_WIN, levels)
    if len(iters) != levels or len(win) != levels or min(iters) < 0:
        raise ValueError(f"affine.fit: iters and win need one entry per level ({levels}), coarsest first")
    bins = _per_level((int(mi_bins),) * levels if isinstance(mi_bins, int) else mi_bins, DEFAULT_MI_BINS, levels)
    if len(bins) != levels or not all(4 <= int(k) <= 64 for k in bins):
        raise ValueError(f"affine.fit: mi_bins needs an int or one entry per level ({levels}), coarsest first, each in [4, 64]")
    nd = x.dim() - 2
    if loss == "mind" and nd == 2:
        ops.mind_loss(x, y)                              # (raises the project's NotImplementedError for slices before any work)
    B, size = x.shape[0], tuple(int(s) for s in x.shape[2:])
    dev = x.device
    r0 = (max(size) - 1) / 2.0
    with torch.no_grad():
        pyr = [(x.detach(), y.detach(), mask_x, mask_y)]
        for _ in range(levels - 1):
            pyr.append(tuple(None if t is None else ops.avg_pool2(t.detach().float()).contiguous() for t in pyr[-1]))
        start = identity(B, dev, nd) if theta0 is None else theta0.to(device=dev)
        P = _params_of(start, r0, dof, nd).to(dev).contiguous()
    P.requires_grad_(True)
    P.grad = torch.zeros_like(P)
    total = int(sum(iters))
    history = torch.zeros((total + 1, 2), device=dev, dtype=torch.float32)

    def evaluate(lvl: int, k: int):
        xl, yl, mxl, myl = pyr[lvl]
        theta = _theta_of(P, r0 / 2 ** lvl, dof, nd)
        wx = ops.warp_mask(ops.affine_field(theta, xl.shape[2:]), mxl) if mxl is not None else None
        return ops.similarity(loss, ops.affine_warp(theta, xl), yl, wx, myl, gamma=1.0, win=int(win[k]), bins=int(bins[k]))

    row = 0
    for k, lvl in enumerate(reversed(range(levels))):
        m, v = torch.zeros_like(P), torch.zeros_like(P)
        history[row:row + iters[k], 1] = float(lvl)
        for i in range(iters[k]):
            with torch.enable_grad():
                val = evaluate(lvl, k)
                val.backward()
            ops.anchored_adam_step(P.detach().view(-1), P.grad.view(-1), m.view(-1), v.view(-1), float(lr), i + 1)
            P.grad.zero_()
            history[row, 0] = val.detach().reshape(())
            row += 1
    with torch.no_grad():
        history[row, 0] = evaluate(0, levels - 1).reshape(())
        theta = _theta_of(P.detach(), r0, dof, nd).clone()
    return {"theta": theta, "history": history}
