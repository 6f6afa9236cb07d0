"""Synthetic volume pairs for benchmarks and tests (no dataset ships with the reference).

uniform_pair : x, y ~ U[0,1)                                  (BASELINE configs 1-3)
oasis_like_pair : a smooth "anatomy" inside an ellipsoidal head mask with zero background, and a moving image that is the
                  fixed one deformed by a smooth random displacement of a few voxels (BASELINE configs 4-5, "OASIS-style")
multimodal_pair : oasis_like_pair with the fixed image in another "contrast" (a non-monotonic intensity map): the pair for the MIND term
affine_pair : oasis_like_pair's fixed image and the same image under an affine transform, with the transform a fit should recover
All are generated on the CPU generator (reproducible across devices) and finished on the GPU with the HIP resampling / warp
operators of the hot path."""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import ops


def uniform_pair(size: Sequence[int], batch: int, seed: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, 1, *size, generator=g).to(device)
    y = torch.rand(batch, 1, *size, generator=g).to(device)
    return x, y


def oasis_like_pair(size: Sequence[int], batch: int, seed: int, device, max_disp: float = 3.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """fixed y = smooth texture (U[0,1) on a size/8 lattice, tri-linearly up-sampled) x ellipsoid mask (semi-axes 0.4 * extent);
    moving x = y resampled through a smooth random displacement (U[-max_disp, max_disp] voxels on a size/16 lattice, up-sampled);
    both clipped to [0, 1]."""
    size = [int(s) for s in size]
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(batch, 1, *[max(s // 8, 2) for s in size], generator=g).to(device)
    base = ops.resize_trilinear(coarse, size)
    axes = [torch.linspace(-0.5, 0.5, s, device=device) for s in size]
    zz, yy, xx = torch.meshgrid(*axes, indexing="ij")
    mask = ((zz / 0.4) ** 2 + (yy / 0.4) ** 2 + (xx / 0.4) ** 2 <= 1.0).float()[None, None]
    y = (base * mask).clamp_(0.0, 1.0).contiguous()
    lattice = (torch.rand(batch, 3, *[max(s // 16, 2) for s in size], generator=g) * 2 - 1).to(device) * max_disp
    field = ops.resize_trilinear(lattice, size)
    # displacement in voxels -> the SpatialTransformer's convention: the field is added to the voxel grid (network_blocks.py:101-121)
    x = ops.warp3d(field.contiguous(), y).clamp_(0.0, 1.0).contiguous()
    return x, y


def multimodal_pair(size: Sequence[int], batch: int, seed: int, device, max_disp: float = 3.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """oasis_like_pair with the fixed image passed through v -> 4 v (1 - v) inside the head (0 outside, where v is 0): dark and bright tissue
    of the moving image are both dark in the fixed one, mid-grey is bright - no linear relation between the two intensities, the case
    NCC and MSE cannot handle and the MIND term is for."""
    x, y = oasis_like_pair(size, batch, seed, device, max_disp)
    return x, (4.0 * y * (1.0 - y)).contiguous()


def default_theta_gen(batch: int, device) -> torch.Tensor:
    """the generating transform of affine_pair: a rotation of 6 degrees about a generic axis, scales of 1.05 / 0.95 / 1.03 and a shift of
    (1.5, -1, 2) voxels - about 5 voxels at the corners of a 32^3 grid"""
    ang = torch.tensor(6.0 * 3.141592653589793 / 180.0, dtype=torch.float64)
    axis = torch.tensor([0.6, -0.5, 0.62449979983984], dtype=torch.float64)
    w = ang * axis / axis.norm()
    K = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=torch.float64)
    M = torch.linalg.matrix_exp(K) @ torch.diag(torch.tensor([1.05, 0.95, 1.03], dtype=torch.float64))
    t = torch.tensor([[1.5], [-1.0], [2.0]], dtype=torch.float64)
    return torch.cat([M, t], dim=1).float().unsqueeze(0).repeat(batch, 1, 1).to(device)


def affine_pair(size: Sequence[int], batch: int, seed: int, device, theta_gen=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(x, y, expected): y = oasis_like_pair's fixed image, x = ops.affine_warp(theta_gen, y) the moving one (theta_gen (B,3,4) in voxels of
    `size` about its centre; default default_theta_gen), expected = affine.expected_fit(theta_gen, size), the transform a fit of x onto y
    should return - not the inverse of theta_gen, because the sampler carries its own map."""
    from . import affine
    _, y = oasis_like_pair(size, batch, seed, device)
    theta_gen = default_theta_gen(batch, device) if theta_gen is None else theta_gen.to(device=device, dtype=torch.float32)
    x = ops.affine_warp(theta_gen, y).contiguous()
    return x, y, affine.expected_fit(theta_gen, [int(s) for s in size])
