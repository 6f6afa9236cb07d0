"""Plain numpy / torch references of the boundary metrics, written from the definitions; they run on any device.

    surface(mask, nd)             the voxels of a bool mask (..., D, H, W) / (..., H, W) with a face neighbour outside it (6 / 4 neighbours;
                                  the outside of the volume counts as outside the mask)
    edt_sq(feat)                  min over the set voxels q of |p - q|^2 by brute force over the feature points, int64 arithmetic -> int32
    surface_distances(a, b, C, q) per (batch item, class): hd, hd_pct (np.percentile, float64), assd, n_a, n_b and the squared-distance
                                  histograms (B, C, 2, bins)
    voronoi_labels(shape, C, seed) a label map of C nearest-centre regions (every class present)"""
import numpy as np
import torch

EDT_INF = 1 << 29


def surface(mask: torch.Tensor, nd: int) -> torch.Tensor:
    """mask: bool, the last nd dims are spatial"""
    m = mask.bool()
    inner = m.clone()
    for k in range(nd):
        dim = m.dim() - nd + k
        n = m.shape[dim]
        lo = torch.zeros_like(m)                      # lo[i] = m[i - 1], outside = False
        hi = torch.zeros_like(m)                      # hi[i] = m[i + 1]
        if n > 1:
            lo.narrow(dim, 1, n - 1).copy_(m.narrow(dim, 0, n - 1))
            hi.narrow(dim, 0, n - 1).copy_(m.narrow(dim, 1, n - 1))
        inner &= lo & hi
    return m & ~inner


def edt_sq(feat: torch.Tensor, chunk: int = 1 << 22) -> torch.Tensor:
    """feat (B, 1, spatial...) bool / uint8 -> int32 of the same shape"""
    f = feat != 0
    B = f.shape[0]
    size = tuple(f.shape[2:])
    dev = f.device
    axes = [torch.arange(s, device=dev, dtype=torch.int64) for s in size]
    pts = torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing="ij")], dim=1)          # (V, nd)
    out = torch.full((B, pts.shape[0]), EDT_INF, device=dev, dtype=torch.int64)
    for b in range(B):
        q = pts[f[b, 0].reshape(-1)]
        if q.shape[0] == 0:
            continue
        step = max(1, chunk // q.shape[0])
        for s in range(0, pts.shape[0], step):
            d = ((pts[s:s + step, None, :] - q[None, :, :]) ** 2).sum(dim=2)
            out[b, s:s + step] = d.min(dim=1).values
    return out.reshape((B, 1) + size).to(torch.int32)


def surface_distances(lab_a: torch.Tensor, lab_b: torch.Tensor, C: int, q: float = 95.0):
    """label maps (B, 1, spatial...) -> dict of numpy arrays: hd, hd_pct, assd (B, C) float64 (NaN where a class is absent from either
    map), n_a, n_b (B, C) int64, hist (B, C, 2, bins) int64"""
    nd = lab_a.dim() - 2
    B = lab_a.shape[0]
    size = tuple(lab_a.shape[2:])
    bins = sum((s - 1) ** 2 for s in size) + 1
    res = {k: np.full((B, C), np.nan) for k in ("hd", "hd_pct", "assd")}
    res["n_a"], res["n_b"] = np.zeros((B, C), dtype=np.int64), np.zeros((B, C), dtype=np.int64)
    res["hist"] = np.zeros((B, C, 2, bins), dtype=np.int64)
    for c in range(C):
        sa, sb = surface(lab_a == c, nd), surface(lab_b == c, nd)
        ea, eb = edt_sq(sa), edt_sq(sb)
        for b in range(B):
            d2_ab = eb[b][sa[b]].cpu().numpy().astype(np.int64)          # squared distances of S_c(A) to S_c(B)
            d2_ba = ea[b][sb[b]].cpu().numpy().astype(np.int64)
            res["n_a"][b, c], res["n_b"][b, c] = d2_ab.size, d2_ba.size
            if d2_ab.size == 0 or d2_ba.size == 0:
                continue
            res["hist"][b, c, 0] = np.bincount(d2_ab, minlength=bins)
            res["hist"][b, c, 1] = np.bincount(d2_ba, minlength=bins)
            d_ab, d_ba = np.sqrt(d2_ab.astype(np.float64)), np.sqrt(d2_ba.astype(np.float64))
            res["hd"][b, c] = max(d_ab.max(), d_ba.max())
            res["hd_pct"][b, c] = max(np.percentile(d_ab, q), np.percentile(d_ba, q))
            res["assd"][b, c] = (d_ab.sum() + d_ba.sum()) / (d_ab.size + d_ba.size)
    return res


def voronoi_labels(shape, C: int, seed: int = 1) -> torch.Tensor:
    """(1, 1) + shape int64 label map: every voxel carries the index of the nearest of C random centres (ties -> the lowest index)"""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(0, s - 1, size=C) for s in shape], axis=1)                       # (C, nd)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    d = ((grid[..., None, :] - centres) ** 2).sum(axis=-1)
    return torch.from_numpy(d.argmin(axis=-1)).reshape((1, 1) + tuple(shape))


def rolled(lab: torch.Tensor) -> torch.Tensor:
    """the copy rolled by (1, -2, 1) (3-D) / (-2, 1) (2-D) along the spatial axes"""
    nd = lab.dim() - 2
    shifts = (1, -2, 1)[3 - nd:]
    return torch.roll(lab, shifts=shifts, dims=tuple(range(2, 2 + nd)))
