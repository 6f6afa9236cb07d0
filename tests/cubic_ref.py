"""Cubic B-spline interpolation (pulpo_amd.ops.bspline_prefilter / warp3d_cubic, csrc/cubic.hip) in plain torch, in the
dtype and on the device of its arguments (the tests call it in float64, and in float32 for the reference's own deviation): the prefilter is
Unser's recursion with the whole-sample mirror starts, the value an explicit 64-tap sum at the sampler's clamped coordinate
(affine_ref.sample_coords), the field gradient torch autograd through that sum.  tests/test_host_cubic.py pins both to scipy.ndimage
(spline_filter and map_coordinates, order 3, mode "mirror"); tests/test_gpu_cubic.py holds the kernels to them."""
import math

import torch
import torch.nn.functional as F

import affine_ref as AR

POLE = math.sqrt(3.0) - 2.0
GAIN = 6.0


def mirror(j, N: int):
    """whole-sample mirror of integer tensor j into [0, N - 1]: period 2 (N - 1), m(-1) = 1, m(N) = N - 2; an axis of one sample has one index"""
    if N == 1:
        return torch.zeros_like(j)
    p = 2 * (N - 1)
    j = j.abs() % p
    return torch.where(j < N, j, p - j)


def prefilter_axis(s, dim: int):
    """the recursion along one axis: c+[k] = 6 s[k] + z c+[k-1] from the mirror start, c[k] = z (c[k+1] - c+[k]) from
    c[N-1] = z / (z^2 - 1) (c+[N-1] + z c+[N-2]); an axis of one sample is returned as it is"""
    N = s.shape[dim]
    if N == 1:
        return s
    s = s.movedim(dim, 0) * GAIN
    z = torch.tensor(POLE, dtype=s.dtype, device=s.device)
    k = torch.arange(1, N - 1, dtype=s.dtype, device=s.device)
    w = (z ** k + z ** (2 * N - 2 - k)).view(-1, *([1] * (s.dim() - 1)))
    start = (s[0] + z ** (N - 1) * s[N - 1] + (w * s[1:N - 1]).sum(0)) / (1 - z ** (2 * N - 2))
    cp = [start]
    for i in range(1, N):
        cp.append(s[i] + z * cp[-1])
    c = [None] * N
    c[N - 1] = z / (z * z - 1) * (cp[N - 1] + z * cp[N - 2])
    for i in range(N - 2, -1, -1):
        c[i] = z * (c[i + 1] - cp[i])
    return torch.stack(c, 0).movedim(0, dim)


def prefilter(img):
    """coefficients of a plane stack (B,C,D,H,W), axis by axis (W, H, D: the kernels' order; the passes commute up to rounding)"""
    out = img
    for dim in (4, 3, 2):
        out = prefilter_axis(out, dim)
    return out


def weights(f):
    """B_0..B_3 at fraction f, stacked in front"""
    f2, f3, m = f * f, f * f * f, 1 - f
    return torch.stack([m * m * m / 6, (3 * f3 - 6 * f2 + 4) / 6, (-3 * f3 + 3 * f2 + 3 * f + 1) / 6, f3 / 6])


def dweights(f):
    """B'_0..B'_3 at fraction f"""
    f2, m = f * f, 1 - f
    return torch.stack([-m * m / 2, (3 * f2 - 4 * f) / 2, (-3 * f2 + 2 * f + 1) / 2, f2 / 2])


def interp(coef, c, Sg):
    """the 64-tap tensor-product sum of coef (B,C,Di,Hi,Wi) at clamped coordinates c (B,3,...) of a grid Sg: (B,C,...).  An axis of grid extent
    1 has no coordinate: one tap of weight 1.  Differentiable with respect to c (the cell index is a constant of the derivative)."""
    Si = tuple(coef.shape[2:])
    taps, ws = [], []
    for a in range(3):
        if Sg[a] == 1:
            taps.append([torch.zeros_like(c[:, a], dtype=torch.long)])
            ws.append([torch.ones_like(c[:, a])])
            continue
        i = c[:, a].detach().floor().long()
        w = weights(c[:, a] - i.to(c.dtype))
        taps.append([mirror(i - 1 + l, Si[a]) for l in range(4)])
        ws.append([w[l] for l in range(4)])
    out = 0.0
    for tz, wz in zip(taps[0], ws[0]):
        for ty, wy in zip(taps[1], ws[1]):
            for tx, wx in zip(taps[2], ws[2]):
                out = out + (wz * wy * wx).unsqueeze(1) * AR._gather(coef, tz, ty, tx)
    return out


def coords(df, Si):
    """(clamped coordinate, unclamped, dscale) of the sampler for a field df (B,3,Dg,Hg,Wg) into an image of size Si"""
    Sg = tuple(df.shape[2:])
    return AR.sample_coords(AR.grid(Sg, df.dtype, df.device).unsqueeze(0) + df, Sg, tuple(Si))


def warp_coef(df, coef):
    """warp3d_cubic(df, coef=coef): differentiable with respect to df (the clamp's zero gradient included: clamp() has it)"""
    c, _, _ = coords(df, coef.shape[2:])
    return interp(coef, c, tuple(df.shape[2:]))


def warp(df, img):
    """warp3d_cubic(df, img)"""
    return warp_coef(df, prefilter(img))


def gdf(df, coef, g):
    """gradient of sum(g * warp_coef(df, coef)) with respect to df, by autograd.  Where a coordinate sits exactly on 0 or Si - 1 the definition's
    dscale is 0; clamp()'s gradient is 1 there, so those entries are set to 0 explicitly."""
    leaf = df.detach().clone().requires_grad_(True)
    (warp_coef(leaf, coef) * g).sum().backward()
    _, _, dscale = coords(df.detach(), coef.shape[2:])
    return leaf.grad * (dscale != 0).to(df.dtype)


def gdf_analytic(df, coef, g):
    """the same gradient by the definition's expression: dscale_a sum_c g_c sum_taps B'(f_a) B(f_b) B(f_c) coef_c"""
    Sg, Si = tuple(df.shape[2:]), tuple(coef.shape[2:])
    c, _, dscale = coords(df, Si)
    taps, ws, ds = [], [], []
    for a in range(3):
        if Sg[a] == 1:
            taps.append([torch.zeros_like(c[:, a], dtype=torch.long)])
            ws.append([torch.ones_like(c[:, a])])
            ds.append([torch.zeros_like(c[:, a])])
            continue
        i = c[:, a].floor().long()
        f = c[:, a] - i.to(c.dtype)
        w, d = weights(f), dweights(f)
        taps.append([mirror(i - 1 + l, Si[a]) for l in range(4)])
        ws.append([w[l] for l in range(4)])
        ds.append([d[l] for l in range(4)])
    out = [0.0, 0.0, 0.0]
    for tz, wz, dz in zip(taps[0], ws[0], ds[0]):
        for ty, wy, dy in zip(taps[1], ws[1], ds[1]):
            for tx, wx, dx in zip(taps[2], ws[2], ds[2]):
                s = (AR._gather(coef, tz, ty, tx) * g).sum(1)
                out[0] = out[0] + dz * wy * wx * s
                out[1] = out[1] + wz * dy * wx * s
                out[2] = out[2] + wz * wy * dx * s
    return torch.stack(out, 1) * dscale


# ------------------------------------------------------------------------------------------------ inputs
def smooth_field(B: int, grid, seed: int, amplitude: float, dtype=torch.float64):
    """smooth noise: a 4^3 randn lattice interpolated up to the grid, scaled to `amplitude` voxels of standard deviation; a depth-1 grid
    (the 2-D form) gets a 4^2 lattice and no depth component"""
    g = torch.Generator().manual_seed(seed)
    if grid[0] == 1:
        lat = torch.randn(B, 2, 4, 4, generator=g, dtype=torch.float64)
        f = F.interpolate(lat, size=tuple(grid[1:]), mode="bilinear", align_corners=True)
        f = torch.cat([torch.zeros_like(f[:, :1]), f], dim=1).unsqueeze(2)
    else:
        lat = torch.randn(B, 3, 4, 4, 4, generator=g, dtype=torch.float64)
        f = F.interpolate(lat, size=tuple(grid), mode="trilinear", align_corners=True)
    return (f * amplitude).to(dtype)


def outside_fraction(df, Si) -> float:
    """share of the samples with at least one coordinate outside [0, Si - 1] (clamped: dscale = 0 along that axis)"""
    Sg = tuple(df.shape[2:])
    _, raw, _ = coords(df, Si)
    out = torch.zeros_like(raw[:, 0], dtype=torch.bool)
    for a in range(3):
        if Sg[a] > 1:
            out |= (raw[:, a] < 0) | (raw[:, a] > Si[a] - 1)
    return float(out.double().mean())


def shift_pair(size, shift: float = 0.5, dtype=torch.float64):
    """(there, back): a constant shift of `shift` voxels of the SAMPLE INDEX along every axis and its exact inverse, both in the sampler's own
    coordinates on a grid = image of `size` (index = (v + d) S / (S - 1) - 0.5, so d = (v + 0.5 +- shift)(S - 1) / S - v)"""
    v = AR.grid(size, torch.float64).unsqueeze(0)
    out = []
    for sign in (1.0, -1.0):
        d = [((v[:, a] + 0.5 + sign * shift) * (size[a] - 1) / size[a] - v[:, a]) if size[a] > 1 else torch.zeros_like(v[:, a]) for a in range(3)]
        out.append(torch.stack(d, 1).to(dtype))
    return out[0], out[1]


def interior_rmse(a, b, margin: int = 4) -> float:
    sl = (slice(None), slice(None)) + tuple(slice(margin, s - margin) if s > 2 * margin else slice(None) for s in a.shape[2:])
    return float(((a[sl] - b[sl]) ** 2).mean().sqrt())
