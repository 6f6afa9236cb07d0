"""The training augmentation of DESIGN.md section 3p in plain torch, in the dtype of its inputs (float64 when called as the reference, float32 for
"the reference's own fp32 deviation"), and a pure-Python Philox4x32-10.  tests/test_host_augment.py pins the pieces (Random123's known
answers, the B-spline's partition of unity / linear reproduction / C2 continuity, the sampler against grid_sample); tests/test_gpu_augment.py
holds the HIP kernels to them.

Spatial map of an output voxel v: q = v + e(v), p = c + M (q - c) + t.  e: cubic B-spline free-form deformation on a lattice of spacing s,
cell i = floor(z / s), u = z / s - i, e = sum_lmn B_l B_m B_n phi[i + (l, m, n)].  Sampler in voxel units: trilinear with corners outside
the volume contributing `fill`; labels at floor(p + 0.5).  Slices are depth-1 volumes: no depth coordinate, no depth B-spline factor."""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32(counter, key):
    """Philox4x32-10: counter = 4 words, key = 2 words -> 4 words.  Words are Python ints or numpy uint64 arrays holding 32-bit values (the
    same code serves both: every product of two 32-bit words fits 64 bits)"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def noise(seed: int, n: int, dtype=torch.float64):
    """n(i), i = 0..n-1: group g = i >> 2 has counter (g & M32, g >> 32, 0, 0) and key (seed & M32, seed >> 32); lanes 0, 1 take Box-Muller's
    cosine and sine of the word pair (r0, r1), lanes 2, 3 of (r2, r3), with u1 = ((ra >> 8) + 1) 2^-24 and u2 = (rb >> 8) 2^-24"""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(g)
    seed &= (1 << 64) - 1
    r = philox4x32((g & np.uint64(M32), g >> np.uint64(32), zero, zero), (np.uint64(seed & M32), np.uint64(seed >> 32)))
    out = torch.empty(len(g), 4, dtype=dtype)
    for pair in (0, 1):
        ra, rb = (torch.from_numpy((w >> np.uint64(8)).astype(np.int64)) for w in r[2 * pair:2 * pair + 2])
        u1, u2 = ((ra + 1).to(dtype) * 2.0 ** -24), (rb.to(dtype) * 2.0 ** -24)
        R = torch.sqrt(-2.0 * torch.log(u1))
        out[:, 2 * pair] = R * torch.cos(2.0 * math.pi * u2)
        out[:, 2 * pair + 1] = R * torch.sin(2.0 * math.pi * u2)
    return out.reshape(-1)[:n]


# ------------------------------------------------------------------------------------------------ B-spline
def lattice_size(S: int, s: int) -> int:
    return -(-(S - 1) // s) + 3


def bspline_basis(u):
    """the uniform cubic B-spline basis B_0..B_3 at u in [0, 1)"""
    m = 1 - u
    return (m ** 3 / 6, (3 * u ** 3 - 6 * u ** 2 + 4) / 6, (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) / 6, u ** 3 / 6)


def bspline_matrix(S: int, G: int, s: int, dtype, device=None):
    """(S, G): row z holds B_l(u) at column i + l"""
    A = torch.zeros(S, G, dtype=dtype, device=device)
    z = torch.arange(S, device=device)
    i = z // s
    u = z.to(dtype) / s - i.to(dtype)
    for l, w in enumerate(bspline_basis(u)):
        ok = i + l < G                  # when s divides S - 1 the last voxel sits on a knot: its fourth node lies past the lattice, with B_3(0) = 0
        assert bool((w[~ok] == 0).all())
        A[z[ok], (i + l)[ok]] = w[ok]
    return A


def bspline_field(phi, size, s: int):
    """e (B,3,D,H,W) of phi (B,3,Gz,Gy,Gx); a depth-1 grid (Gz = 1) has no depth factor and no depth displacement"""
    D, H, W = size
    assert tuple(phi.shape[2:]) == (1 if D == 1 else lattice_size(D, s), lattice_size(H, s), lattice_size(W, s)), tuple(phi.shape)
    dev = phi.device
    Az = torch.ones(1, 1, dtype=phi.dtype, device=dev) if D == 1 else bspline_matrix(D, phi.shape[2], s, phi.dtype, dev)
    Ay, Ax = bspline_matrix(H, phi.shape[3], s, phi.dtype, dev), bspline_matrix(W, phi.shape[4], s, phi.dtype, dev)
    e = torch.einsum("bcijk,zi,yj,xk->bczyx", phi, Az, Ay, Ax)
    if D == 1:
        e = torch.cat([torch.zeros_like(e[:, :1]), e[:, 1:]], dim=1)
    return e


def grid(size, dtype, device=None):
    return torch.stack(torch.meshgrid(*[torch.arange(s, dtype=dtype, device=device) for s in size], indexing="ij"))


def positions(size, theta=None, phi=None, s=None, dtype=torch.float64):
    """p (B,3,D,H,W); B from theta / phi (1 when both are None)"""
    D, H, W = size
    B = theta.shape[0] if theta is not None else phi.shape[0] if phi is not None else 1
    dev = theta.device if theta is not None else phi.device if phi is not None else None
    q = grid(size, dtype, dev).unsqueeze(0).expand(B, 3, D, H, W)
    if phi is not None:
        q = q + bspline_field(phi.to(dtype), size, s)
    if theta is not None:
        theta = theta.to(dtype)
        c = torch.tensor([(n - 1) / 2 for n in size], dtype=dtype, device=dev).view(1, 3, 1, 1, 1)
        q = c + torch.einsum("bij,bjzyx->bizyx", theta[:, :, :3], q - c) + theta[:, :, 3].view(B, 3, 1, 1, 1)
        if D == 1:
            q = torch.cat([torch.zeros_like(q[:, :1]), q[:, 1:]], dim=1)
    return q


def displacement(size, theta=None, phi=None, s=None, dtype=torch.float64):
    """what ops.bspline_field returns: e, or p - v with an affine"""
    if theta is None:
        return bspline_field(phi.to(dtype), size, s)
    d = positions(size, theta, phi, s, dtype) - grid(size, dtype, theta.device).unsqueeze(0)
    return torch.cat([torch.zeros_like(d[:, :1]), d[:, 1:]], dim=1) if size[0] == 1 else d


# ------------------------------------------------------------------------------------------------ samplers
def _gather(src, iz, iy, ix, fill):
    """src (B,C,D,H,W) at integer (B,D',H',W') indices; `fill` outside"""
    B, C, D, H, W = src.shape
    inside = (iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    flat = ((iz.clamp(0, D - 1) * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)).view(B, 1, -1).expand(B, C, -1)
    got = src.reshape(B, C, -1).gather(2, flat).view(B, C, *iz.shape[1:])
    return torch.where(inside.unsqueeze(1), got, torch.full_like(got, fill))


def sample_linear(src, p, fill=0.0):
    """trilinear at p (B,3,...) in voxel units, in p's dtype; corners outside the volume contribute fill"""
    src = src.to(p.dtype)
    i0 = torch.floor(p)
    f = p - i0
    i0 = i0.long()
    out = 0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[:, 0] if dz else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dx else 1 - f[:, 2])
                out = out + w.unsqueeze(1) * _gather(src, i0[:, 0] + dz, i0[:, 1] + dy, i0[:, 2] + dx, fill)
    return out


def sample_nearest(labels, p, fill_label=0):
    """labels (B,1,D,H,W) at floor(p + 0.5) per axis; fill_label outside"""
    i = torch.floor(p + 0.5).long()
    return _gather(labels, i[:, 0], i[:, 1], i[:, 2], fill_label)


def rounding_margin(p, size):
    """per voxel, the distance of p to the nearest rounding boundary of sample_nearest on any axis - which the edges of the volume at -0.5 and
    S - 0.5 are among (all half-integers)"""
    h = p + 0.5
    return (h - torch.round(h)).abs().amin(dim=1)


# ------------------------------------------------------------------------------------------------ intensity
def bias_field(bias, size):
    """beta (B,1,D,H,W): trilinear interpolation of the lattice (B,Lz,Ly,Lx) whose end nodes sit on the volume's end voxels"""
    out = bias
    for a, S in enumerate(size):
        L = bias.shape[1 + a]
        g = torch.arange(S, dtype=bias.dtype, device=bias.device) * ((L - 1) / (S - 1)) if (S > 1 and L > 1) else torch.zeros(S, dtype=bias.dtype, device=bias.device)
        i0 = g.long().clamp(max=max(L - 2, 0))
        i1 = (i0 + 1).clamp(max=L - 1)
        f = (g - i0.to(bias.dtype)).view([-1 if k == a else 1 for k in range(3)])
        out = out.index_select(1 + a, i0) * (1 - f) + out.index_select(1 + a, i1) * f
    return out.unsqueeze(1)


def _per_sample(v, B, dtype, dev):
    return (v.to(dtype) if torch.is_tensor(v) else torch.full((B,), float(v), dtype=dtype)).view(B, 1, 1, 1, 1).to(dev)


def intensity(r, cfg, seed_noise=None):
    """the intensity transform on a sampled image r (B,C,D,H,W), in r's dtype; cfg: the dict of ops.augment"""
    B, dt = r.shape[0], r.dtype
    if cfg.get("gamma") is not None:
        r = r.clamp(0, 1) ** _per_sample(cfg["gamma"], B, dt, r.device)
    if cfg.get("bias") is not None:
        r = r * torch.exp(bias_field(cfg["bias"].to(r.device, dt), tuple(r.shape[2:])))
    if cfg.get("gain") is not None or cfg.get("offset") is not None:
        r = _per_sample(cfg["gain"] if cfg.get("gain") is not None else 1.0, B, dt, r.device) * r \
            + _per_sample(cfg["offset"] if cfg.get("offset") is not None else 0.0, B, dt, r.device)
    if cfg.get("sigma") is not None:
        r = r + _per_sample(cfg["sigma"], B, dt, r.device) * noise(int(cfg["seed"]), r.numel(), dt).view(r.shape).to(r.device)
    if cfg.get("clip"):
        r = r.clamp(0, 1)
    return r


# ------------------------------------------------------------------------------------------------ the operator
def lift(t):
    return None if t is None else t.unsqueeze(2)


def lift_theta(theta):
    """(B,2,3) -> (B,3,4) with an identity depth row and column"""
    out = torch.nn.functional.pad(theta, (1, 0, 1, 0)).clone()
    out[:, 0, 0] = 1
    return out


def lift_phi(phi):
    """(B,2,Gy,Gx) -> (B,3,1,Gy,Gx) with a zero depth component"""
    return torch.cat([torch.zeros_like(phi[:, :1]), phi], dim=1).unsqueeze(2)


def augment(img=None, mask=None, labels=None, *, theta=None, phi=None, spacing=None, intensity_cfg=None, fill=0.0, fill_label=0,
            dtype=torch.float64):
    """ops.augment on 5-D (lifted) arguments: (img, mask, labels) results, None for absent sources; positions in `dtype`"""
    first = next(t for t in (img, mask, labels) if t is not None)
    size = tuple(first.shape[2:])
    p = positions(size, theta, phi, spacing, dtype)
    if p.shape[0] != first.shape[0]:
        p = p.expand(first.shape[0], *p.shape[1:])
    out_img = out_mask = out_lab = None
    if img is not None:
        out_img = sample_linear(img, p, fill)
        if intensity_cfg:
            out_img = intensity(out_img, intensity_cfg)
    if mask is not None:
        out_mask = sample_linear(mask, p, fill)
    if labels is not None:
        out_lab = sample_nearest(labels, p, fill_label)
    return out_img, out_mask, out_lab
