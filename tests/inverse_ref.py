"""float64 CPU restatements of the inverse-field operators (pulpo_amd/csrc/inverse.hip) for tests/test_host_inverse.py and
tests/test_gpu_inverse.py.  A helper, not a test.

The GEOMETRIC sampler: a field d is displacements in voxels at voxel centres; its value at a position p (voxel units) is the trilinear
interpolant at clamp(p, 0, S - 1), with upper corner min(i0 + 1, S - 1).  F.grid_sample(align_corners=True, padding_mode="border") on
2 clamp(p) / (S - 1) - 1 is that sampler (a zero field is the identity; the normalised coordinate rounds in float64, 1e-16).  It is not
SpatialTransformer's sampling (O.warp), whose positions are normalised by S - 1 and sampled with align_corners=False.  Fields with one
spatial dimension less, (B, 2, H, W), take the 2-D form; points are (n, ndims) in the order of the field's axes."""
import torch
import torch.nn.functional as F


def geo_sample(field, pos):
    """field (B, C, *S); pos (B, *P, nd) positions in voxel units, last axis in the order of the field's axes -> (B, C, *P), float64"""
    field, pos = field.double(), pos.double()
    size = field.shape[2:]
    nd = len(size)
    comps = []
    for i in range(nd):
        hi = float(size[i] - 1)
        c = pos[..., i].clamp(0.0, hi)
        comps.append(2.0 * c / hi - 1.0 if hi > 0 else torch.zeros_like(c))
    while pos.dim() < nd + 2:                      # a list of points: (B, n, nd) -> (B, 1, ..., n, nd)
        comps = [c.unsqueeze(1) for c in comps]
        pos = pos.unsqueeze(1)
    grid = torch.stack(comps[::-1], dim=-1)       # grid_sample wants (x, y, z)
    return F.grid_sample(field, grid, mode="bilinear", padding_mode="border", align_corners=True)


def identity(size, dtype=torch.float64):
    """(1, *size, nd) voxel coordinates, 'ij' order, channels last"""
    axes = [torch.arange(s, dtype=dtype) for s in size]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).unsqueeze(0)


def consistency_residual(a, b):
    """||b(p) + a(p + b(p))||_2 per voxel: (B, *S) float64 - the distance of a o b from the identity"""
    a, b = a.double(), b.double()
    nd = a.dim() - 2
    perm = (0, *range(2, nd + 2), 1)
    pos = identity(a.shape[2:]) + b.permute(*perm)
    r = b + geo_sample(a, pos)
    return r.pow(2).sum(dim=1).sqrt()


def inverse_consistency(a, b):
    """(mean, max) of consistency_residual over all voxels, as Python floats"""
    r = consistency_residual(a, b)
    return float(r.mean()), float(r.max())


def transport_points(pts, field):
    """pts (n, nd) or (1, n, nd); field (S, nd, ...) -> (S, n, nd) float64: pts + field[s](pts)"""
    p = pts.double().reshape(1, -1, pts.shape[-1])
    ns = field.shape[0]
    val = geo_sample(field, p.expand(ns, -1, -1))                     # (S, nd, 1, .., n)
    val = val.reshape(ns, field.shape[1], -1).transpose(1, 2)           # (S, n, nd)
    return p + val


def smooth_field(size, amplitude=3.0, seed=1, B=1):
    """the smooth test velocity: randn on a coarse grid of 4 per axis (seed `seed`), interpolated tri/bilinearly (align_corners=True) to
    `size` and scaled to a maximum absolute value of `amplitude` voxels.  float32 (B, nd, *size)."""
    nd = len(size)
    c = torch.randn(B, nd, *([4] * nd), generator=torch.Generator().manual_seed(seed))
    v = F.interpolate(c, size=tuple(size), mode="trilinear" if nd == 3 else "bilinear", align_corners=True)
    return (v * (amplitude / float(v.abs().max()))).contiguous()


def points_with_preimages(fwd, n=64, seed=2, margin=4.0):
    """n positions p on the fixed image's grid (at least `margin` voxels inside the volume) and q = p + fwd(p), where the moving image's
    content at q is shown at p: p is the known preimage of q.  fwd (1, nd, *S).  Returns (q, p) as float32 (n, nd); points whose q leaves
    the volume are drawn again."""
    size = fwd.shape[2:]
    nd = len(size)
    gen = torch.Generator().manual_seed(seed)
    hi = torch.tensor([s - 1.0 for s in size], dtype=torch.float64)
    out_p, out_q = [], []
    while len(out_p) < n:
        p = (margin + torch.rand(nd, generator=gen, dtype=torch.float64) * (hi - 2 * margin)).float().double()
        q = transport_points(p[None], fwd)[0, 0]
        qf = q.float().double()
        if bool((qf >= 0).all()) and bool((qf <= hi).all()):
            out_p.append(p)
            out_q.append(qf)
    return torch.stack(out_q).float(), torch.stack(out_p).float()
