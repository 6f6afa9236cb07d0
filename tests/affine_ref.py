"""Affine pre-alignment (pulpo_amd/affine.py, csrc/affine.hip) in plain torch, in the dtype and on the device of its
arguments (the tests call it in float64, and in float32 for the reference's own deviation): the displacement field of an affine, the warp
through the sampler's coordinate (clamp and dscale included), the analytic gradient with respect to theta, the composition with a dense
field, the expected fit of a synthetic pair and the whole fitting loop with Adam.  Everything is written for volumes (B,C,D,H,W) and
theta (B,3,4); a depth-1 volume is the 2-D form (no coordinate along the depth), slices are lifted by lift_theta / unsqueeze(2)."""
import functools
from typing import Sequence

import torch
import torch.nn.functional as F

import refine_ref as RR


# ------------------------------------------------------------------------------------------------ conventions
def identity(B: int, dtype=torch.float64):
    return torch.eye(3, 4, dtype=dtype).unsqueeze(0).repeat(B, 1, 1)


def lift_theta(theta2):
    """(B,2,3) -> (B,3,4) with an identity depth row and column"""
    out = F.pad(theta2, (1, 0, 1, 0))
    out[:, 0, 0] = 1.0
    return out


def centre(size, dtype, device="cpu"):
    return torch.tensor([(s - 1) / 2 for s in size], dtype=dtype, device=device)


def grid(size, dtype, device="cpu"):
    """(3, D, H, W) voxel indices"""
    return torch.stack(torch.meshgrid(*[torch.arange(s, dtype=dtype, device=device) for s in size], indexing="ij"))


def positions(theta, pts, size):
    """p = c + M (v - c) + t for points pts (3, ...) of the grid `size`, shared by the batch: (B, 3, ...)"""
    return positions_each(theta, pts.unsqueeze(0).expand(theta.shape[0], *pts.shape), size)


def positions_each(theta, pts, size):
    """the same for points pts (B, 3, ...) of their own per batch element"""
    c = centre(size, theta.dtype, theta.device).view(1, 3, *([1] * (pts.dim() - 2)))
    p = torch.einsum("bij,bj...->bi...", theta[:, :, :3], pts - c) + theta[:, :, 3].view(-1, 3, *([1] * (pts.dim() - 2)))
    return p + c


def field(theta, size):
    """d = p - v, (B,3,D,H,W); a depth-1 grid has no depth displacement"""
    v = grid(size, theta.dtype, theta.device)
    d = positions(theta, v, size) - v
    if size[0] == 1:
        d = torch.cat([torch.zeros_like(d[:, :1]), d[:, 1:]], dim=1)
    return d


def sample_coords(loc, Sg: Sequence[int], Si: Sequence[int]):
    """the sampler's map per axis for positions loc (B,3,...) on a grid Sg into an image Si: (clamped coordinate, unclamped, dscale) each
    (B,3,...).  s(p) = p Si / (Sg - 1) - 0.5; dscale = Si / (Sg - 1) strictly inside (0, Si - 1), 0 where clamped; an axis of extent 1 on the
    grid has coordinate 0 and dscale 0 (the 2-D form)."""
    cs, raws, ds = [], [], []
    for a in range(3):
        if Sg[a] == 1:
            z = torch.zeros_like(loc[:, a])
            cs.append(z); raws.append(z + 0.25); ds.append(z)
            continue
        t = 2 * (loc[:, a] / (Sg[a] - 1) - 0.5)
        raw = ((t + 1) * Si[a] - 1) / 2
        hi = float(Si[a] - 1)
        inside = (raw > 0) & (raw < hi)
        cs.append(raw.clamp(0.0, hi))
        raws.append(raw)
        ds.append(inside.to(loc.dtype) * (Si[a] / (Sg[a] - 1)))
    return torch.stack(cs, 1), torch.stack(raws, 1), torch.stack(ds, 1)


def _corners(c, Si):
    i0 = c.detach().floor().long()
    i1 = torch.minimum(i0 + 1, torch.tensor([s - 1 for s in Si], device=c.device).view(1, 3, *([1] * (c.dim() - 2))))
    return i0, i1, c - i0.to(c.dtype)


def _gather(img, iz, iy, ix):
    B, C = img.shape[:2]
    Hi, Wi = img.shape[3:]
    flat = ((iz * Hi + iy) * Wi + ix).view(B, 1, -1).expand(B, C, -1)
    return torch.gather(img.flatten(2), 2, flat).view(B, C, *iz.shape[1:])


def interp(img, c):
    """trilinear value of img (B,C,Di,Hi,Wi) at clamped coordinates c (B,3,...): (B,C,...); differentiable with respect to c"""
    i0, i1, f = _corners(c, img.shape[2:])
    out = 0.0
    for kz, wz in ((i0[:, 0], 1 - f[:, 0]), (i1[:, 0], f[:, 0])):
        for ky, wy in ((i0[:, 1], 1 - f[:, 1]), (i1[:, 1], f[:, 1])):
            for kx, wx in ((i0[:, 2], 1 - f[:, 2]), (i1[:, 2], f[:, 2])):
                out = out + (wz * wy * wx).unsqueeze(1) * _gather(img, kz, ky, kx)
    return out


def warp_field(df, img):
    """SpatialTransformer on a given field through sample_coords (= oracle warp; pinned in tests/test_host_affine.py)"""
    Sg = tuple(df.shape[2:])
    c, _, _ = sample_coords(grid(Sg, df.dtype, df.device).unsqueeze(0) + df, Sg, tuple(img.shape[2:]))
    return interp(img, c)


def warp(theta, img, size=None):
    """the image under the affine: warp_field(field(theta, size), img)"""
    size = tuple(img.shape[2:]) if size is None else tuple(size)
    return warp_field(field(theta, size), img)


def gtheta(theta, img, gout, size=None):
    """analytic gradient of sum(gout * warp(theta, img, size)) with respect to theta: gpos_a = dscale_a sum_c gout_c d interp / d coord_a;
    gtheta[a][b] = sum_v gpos_a (v_b - c_b), gtheta[a][3] = sum_v gpos_a"""
    size = tuple(img.shape[2:]) if size is None else tuple(size)
    v = grid(size, theta.dtype, theta.device)
    c, _, dscale = sample_coords(v.unsqueeze(0) + field(theta, size), size, tuple(img.shape[2:]))
    i0, i1, f = _corners(c, img.shape[2:])
    s = {(a, b, k): _gather(img, (i0, i1)[a][:, 0], (i0, i1)[b][:, 1], (i0, i1)[k][:, 2]) for a in (0, 1) for b in (0, 1) for k in (0, 1)}
    w = lambda ax, k: (f[:, ax] if k else 1 - f[:, ax]).unsqueeze(1)
    dz = sum(w(1, b) * w(2, k) * (s[1, b, k] - s[0, b, k]) for b in (0, 1) for k in (0, 1))
    dy = sum(w(0, a) * w(2, k) * (s[a, 1, k] - s[a, 0, k]) for a in (0, 1) for k in (0, 1))
    dx = sum(w(0, a) * w(1, b) * (s[a, b, 1] - s[a, b, 0]) for a in (0, 1) for b in (0, 1))
    gpos = torch.stack([(gout * d).sum(1) for d in (dz, dy, dx)], 1) * dscale                       # (B,3,D,H,W)
    u = v - centre(size, theta.dtype, theta.device).view(3, 1, 1, 1)
    return torch.cat([torch.einsum("badhw,jdhw->baj", gpos, u), gpos.flatten(2).sum(2, keepdim=True)], dim=2)


def compose(theta, df, image_size=None):
    """"affine first, deformable second" as one field on df's grid; theta in the frame of the image grid"""
    Sg = tuple(df.shape[2:])
    Si = Sg if image_size is None else tuple(image_size)
    v = grid(Sg, df.dtype, df.device).unsqueeze(0)
    q, _, _ = sample_coords(v + df, Sg, Si)
    p = positions_each(theta, q, Si)
    out = []
    for a in range(3):
        if Sg[a] == 1:
            out.append(torch.zeros_like(p[:, a]))
            continue
        idx = p[:, a] * Si[a] / (Si[a] - 1) - 0.5
        out.append((idx + 0.5) * (Sg[a] - 1) / Si[a] - v[:, a])
    return torch.stack(out, 1)


# ------------------------------------------------------------------------------------------------ 4 x 4 algebra
def to_abs(theta, size):
    """(B,4,4) in absolute voxel coordinates: p = M v + (c - M c + t)"""
    c = centre(size, theta.dtype, theta.device)
    A = torch.zeros(theta.shape[0], 4, 4, dtype=theta.dtype, device=theta.device)
    A[:, :3, :3] = theta[:, :, :3]
    A[:, :3, 3] = c - theta[:, :, :3] @ c + theta[:, :, 3]
    A[:, 3, 3] = 1.0
    return A


def from_abs(A, size):
    c = centre(size, A.dtype, A.device)
    M = A[:, :3, :3]
    return torch.cat([M, (A[:, :3, 3] - c + M @ c).unsqueeze(2)], dim=2)


def sampler_matrix(size, dtype):
    """s(p) = p S / (S - 1) - 0.5 per axis as a 4 x 4 matrix (an axis of extent 1: the identity)"""
    S = torch.eye(4, dtype=dtype)
    for a, s in enumerate(size):
        if s > 1:
            S[a, a] = s / (s - 1)
            S[a, 3] = -0.5
    return S


def invert(theta, size):
    return from_abs(torch.linalg.inv(to_abs(theta, size)), size)


def expected_fit(theta_gen, size):
    """the transform that maps x = warp(theta_gen, y) back onto y: S^-1 A_gen^-1 S^-1, because the sampler carries its own map s"""
    Sinv = torch.linalg.inv(sampler_matrix(size, theta_gen.dtype)).to(theta_gen.device)
    return from_abs(Sinv @ torch.linalg.inv(to_abs(theta_gen, size)) @ Sinv, size)


def corner_error(theta_a, theta_b, size):
    """largest distance, over the batch and the eight corners of the grid, between the positions the two transforms send a corner to"""
    pts = torch.tensor([[z, y, x] for z in (0, size[0] - 1) for y in (0, size[1] - 1) for x in (0, size[2] - 1)], dtype=theta_a.dtype,
                       device=theta_a.device).t()
    return float((positions(theta_a, pts, size) - positions(theta_b.to(theta_a), pts, size)).norm(dim=1).max())


# ------------------------------------------------------------------------------------------------ the fitter
DEFAULT_ITERS, DEFAULT_WIN, DEFAULT_LR = (30, 40, 60), (9, 7, 5), 0.01


def _skew(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1), torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def theta_of(P, r: float, dof: int):
    """theta (B,3,4) in voxels from the normalised parameters: dof 12: M = I + P[:9], t = r P[9:]; dof 6: M = exp(skew(P[:3])), t = r P[3:]"""
    if dof == 12:
        M = torch.eye(3, dtype=P.dtype, device=P.device) + P[:, :9].view(-1, 3, 3)
    else:
        M = torch.linalg.matrix_exp(_skew(P[:, :3]))
    return torch.cat([M, (r * P[:, dof - 3:]).unsqueeze(2)], dim=2)


def params_of(theta, r: float, dof: int):
    """the inverse of theta_of for a start transform (dof 6: the rotation vector of a rotation matrix, angle below pi)"""
    t = theta[:, :, 3] / r
    M = theta[:, :, :3]
    if dof == 12:
        return torch.cat([(M - torch.eye(3, dtype=M.dtype, device=M.device)).reshape(-1, 9), t], dim=1)
    w = torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], 1) / 2          # sin(angle) axis
    s = w.norm(dim=1, keepdim=True)
    ang = torch.atan2(s, ((M.diagonal(dim1=1, dim2=2).sum(1, keepdim=True) - 1) / 2))
    return torch.cat([torch.where(s > 1e-12, w * ang / s.clamp_min(1e-300), w), t], dim=1)


def level_loss(name: str, pred, true, pair, win: int):
    """the project's similarity term of one level with gamma = 1: a sum over the level's voxels (the masked forms: scaled to one)"""
    return RR.similarity_term(name, pred, true, pair, win, 1.0)


def fit(x, y, dof: int = 12, levels: int = 3, iters: Sequence[int] = DEFAULT_ITERS, lr: float = DEFAULT_LR, loss: str = "ncc",
        win: Sequence[int] = DEFAULT_WIN, mask_x=None, mask_y=None, theta0=None):
    """pulpo_amd.affine.fit in torch: (theta (B,3,4), history (sum(iters) + 1, 2): loss, level).  Coarse to fine over avg-pool pyramids
    (iters / win from the coarsest level to the finest), parameters in the frame normalised by r = (max(size) - 1) / 2, halved per level,
    Adam from zero moments at every level."""
    assert dof in (6, 12) and len(iters) == levels and len(win) == levels
    B, size = x.shape[0], tuple(x.shape[2:])
    r0 = (max(size) - 1) / 2
    pyr = [(x, y, mask_x, mask_y)]
    for _ in range(levels - 1):
        pyr.append(tuple(None if t is None else RR.pool2(t) for t in pyr[-1]))
    P = params_of(identity(B, x.dtype).to(x.device) if theta0 is None else theta0.to(x), r0, dof)
    rows = []

    def evaluate(Pl, lvl, k):
        xl, yl, mxl, myl = pyr[lvl]
        th = theta_of(Pl, r0 / 2 ** lvl, dof)
        pred = warp(th, xl)
        pair = None
        if mxl is not None or myl is not None:
            wx = warp(th.detach(), mxl) if mxl is not None else None
            pair = (wx, myl) if wx is not None else (myl, None)
        return level_loss(loss, pred, yl, pair, win[k])

    for k, lvl in enumerate(reversed(range(levels))):
        m, s = torch.zeros_like(P), torch.zeros_like(P)
        for i in range(iters[k]):
            leaf = P.clone().requires_grad_(True)
            val = evaluate(leaf, lvl, k)
            (g,) = torch.autograd.grad(val, leaf)
            P, m, s, _ = RR.adam_update(P, g, m, s, lr, i + 1)
            rows.append(torch.stack([val.detach(), torch.tensor(float(lvl), dtype=P.dtype, device=P.device)]))
    with torch.no_grad():
        rows.append(torch.stack([evaluate(P, 0, levels - 1), torch.tensor(0.0, dtype=P.dtype, device=P.device)]))
    return theta_of(P, r0, dof), torch.stack(rows)


# ------------------------------------------------------------------------------------------------ inputs
def smooth_image(B: int, C: int, size, seed: int, dtype=torch.float64, lattice_div: int = 4):
    """a coarse lattice of uniform noise trilinearly up-sampled (as synthetic.oasis_like_pair's texture)"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.rand(B, C, *[max(s // lattice_div, 2) for s in size], generator=g, dtype=torch.float64)
    mode = "trilinear"
    return F.interpolate(lat, size=tuple(size), mode=mode, align_corners=False).to(dtype)


def theta_generic(B: int, seed: int, rot: float = 0.08, scale: float = 0.05, shift: float = 1.5, dtype=torch.float64):
    """a generic transform per batch element: I + U[-rot - scale, rot + scale] entries, translations U[-shift, shift] voxels"""
    g = torch.Generator().manual_seed(seed)
    M = torch.eye(3, dtype=torch.float64) + (2 * torch.rand(B, 3, 3, generator=g, dtype=torch.float64) - 1) * (rot + scale)
    t = (2 * torch.rand(B, 3, 1, generator=g, dtype=torch.float64) - 1) * shift
    return torch.cat([M, t], dim=2).to(dtype)


def theta_lattice(B: int, seed: int, grid, isize, shift: float = 1.5, extra=(0, 0, 0), dtype=torch.float64):
    """a generic transform per batch element - a full matrix, every entry its own - whose sample coordinates keep clear of the integers by
    construction: the matrix is I + k / 32 (k a non-zero integer, |k| <= 4), so with half-integer v - c the positions p lie on t + Z / 64;
    a coordinate p Si / (Sg - 1) - 0.5 is an integer where p lies on Z (Sg - 1) / (2 Si) - for Sg = Si (and for the unequal grids of the
    tests, 9 10 11 on 12 8 10, after scaling by Sg - 1) a subset of Z / lcm(64, 2 Si) - and the translation is j / 64 (|j| <= 64 shift,
    plus extra / 64) plus half that lattice's spacing.  Picking seeds cannot do this: at 24 x 20 x 28, B = 2, some 16 of the 80 640
    coordinates of a random transform lie within 1e-4 of an integer.  The tests still assert the distance."""
    import math
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(1, 5, (B, 3, 3), generator=g) * (2 * torch.randint(0, 2, (B, 3, 3), generator=g) - 1)
    M = torch.eye(3, dtype=torch.float64) + k.double() / 32
    j = torch.randint(-int(64 * shift), int(64 * shift) + 1, (B, 3), generator=g).double() + torch.tensor(extra, dtype=torch.float64)
    half = torch.tensor([0.5 / math.lcm(64 * max(sg - 1, 1), 2 * si) * max(sg - 1, 1) for sg, si in zip(grid, isize)], dtype=torch.float64)
    return torch.cat([M, (j / 64 + half).unsqueeze(2)], dim=2).to(dtype)


def theta_gen_case(rigid: bool = False, dtype=torch.float64):
    """the transform of the recovery cases: a rotation about a generic axis by 6 degrees with +-5 % scales, or - rigid - by 9 degrees without
    scales (so that the rigid case, too, starts at least 4.4 voxels off at the corners of 24 x 32 x 28), and a 1-2 voxel shift"""
    ang = torch.tensor((9.0 if rigid else 6.0) * 3.141592653589793 / 180.0, dtype=torch.float64)
    axis = torch.tensor([0.6, -0.5, 0.62449979983984], dtype=torch.float64)
    Rm = torch.linalg.matrix_exp(_skew((ang * axis / axis.norm()).unsqueeze(0)))[0]
    Sc = torch.eye(3, dtype=torch.float64) if rigid else torch.diag(torch.tensor([1.05, 0.95, 1.03], dtype=torch.float64))
    t = torch.tensor([1.5, -1.0, 2.0], dtype=torch.float64)
    return torch.cat([Rm @ Sc, t.unsqueeze(1)], dim=1).unsqueeze(0).to(dtype)


def head_image(size, seed: int, dtype=torch.float64):
    """synthetic.oasis_like_pair's fixed image on the CPU: a size/8 lattice up-sampled, times an ellipsoid of semi-axes 0.4 extent"""
    base = smooth_image(1, 1, size, seed, torch.float64, lattice_div=8)
    axes = [torch.linspace(-0.5, 0.5, s, dtype=torch.float64) for s in size]
    zz, yy, xx = torch.meshgrid(*axes, indexing="ij")
    mask = ((zz / 0.4) ** 2 + (yy / 0.4) ** 2 + (xx / 0.4) ** 2 <= 1.0).to(torch.float64)[None, None]
    return (base * mask).clamp(0.0, 1.0).to(dtype)


def affine_pair(size, seed: int = 3, rigid: bool = False, dtype=torch.float64):
    """(moving x = warp(theta_gen, y), fixed y, expected fit) of a recovery case, built in float64.  rigid: the pair whose EXPECTED FIT is
    the rigid transform theta_gen_case(True) - generated by expected_fit of it, the formula being its own inverse; a rigid generating
    transform has no rigid expected fit, because the sampler's map s scales."""
    y = head_image(size, seed)
    th = expected_fit(theta_gen_case(True), tuple(size)) if rigid else theta_gen_case(False)
    return warp(th, y).to(dtype), y.to(dtype), expected_fit(th, tuple(size)).to(dtype)


@functools.lru_cache(maxsize=None)
def fit_reference(size, loss: str = "ncc", dof: int = 12, masked: bool = False, dtype=torch.float64, levels: int = 3,
                  iters=DEFAULT_ITERS, win=DEFAULT_WIN, lr: float = DEFAULT_LR):
    """fit() on affine_pair(size) (the rigid pair for dof 6; with a ball mask on the moving side and a rand mask on the fixed side when
    masked), computed once per process: (theta, history, expected fit, x, y, mask_x, mask_y) in float64 inputs cast to dtype"""
    import masked_ref as MK
    x, y, want = affine_pair(size, rigid=dof == 6)
    mx = my = None
    if masked:
        mx = MK.ball(1, size, outer=0.95, inner=0.0).double()
        my = 0.5 + 0.5 * torch.rand(1, 1, *size, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    cast = lambda t: None if t is None else t.to(dtype)
    theta, hist = fit(cast(x), cast(y), dof=dof, levels=levels, iters=iters, lr=lr, loss=loss, win=win, mask_x=cast(mx), mask_y=cast(my))
    return theta, hist, want, x, y, mx, my
