"""The mutual-information similarity term in torch: the definition the HIP kernels of mi.hip are held to.  Everything
follows the dtype of its inputs, so the same code is the float64 reference and its own float32 evaluation.

    u(v)    = clamp(v, 0, 1) (K - 3) + 1
    w_k(v)  = beta3(u(v) - k), k = 0..K-1          (four bins per voxel, summing to 1)
    P[a,c]  = sum_v m_v w_a(pred_v) w_c(true_v),  m = mask * mask2 (1 unmasked),  M = sum_v m_v,  p = P / M
    MI_b    = sum_ac p (log(p + e) - log(pa pb + e)),  e = 1e-12;  0 for M = 0
    loss    = -gamma V mean_b MI_b                  (V the voxels of one batch element; gradient to pred only)

The dense V x K weight matrices are materialised: a reference for small shapes."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-12

# the distance of this file's own float32 evaluation from its float64 one, the worst over CASES (test_host_mi re-measures them): the joint
# histogram p (max abs), the loss (relative), the gradient (relative L2).  The GPU tests allow 8 x these.  The worst cases set them: p by the
# 90 %-zeros images (one bin holds 0.9, summed in fp32; the smooth cases stay below 2e-7), loss and gradient by K = 4, whose MI is below 1e-3
# (one knot span: the loss is a difference of nearly equal logarithms; the cases with K >= 16 stay below 7e-6 and 2.2e-6).
P_OWN = 1.18e-6
LOSS_OWN = 8.34e-4
GRAD_OWN = 2.35e-5


def beta3(t):
    """the cubic B-spline"""
    a = t.abs()
    inner = 2.0 / 3.0 - a * a + a * a * a / 2
    outer = (2.0 - a) ** 3 / 6
    return torch.where(a < 1, inner, torch.where(a < 2, outer, torch.zeros_like(a)))


def weights(v, bins: int):
    """(...,) -> (..., K): the Parzen weights of every value"""
    u = v.clamp(0.0, 1.0) * (bins - 3) + 1.0
    k = torch.arange(bins, dtype=v.dtype, device=v.device)
    return beta3(u.unsqueeze(-1) - k)


def _flat(t):
    return t.reshape(t.shape[0], -1)


def joint(pred, true, bins: int = 32, mask=None, mask2=None):
    """(P (B,K,K) un-normalised, M (B,)): pred's bins on the rows, true's on the columns"""
    wp, wt = weights(_flat(pred), bins), weights(_flat(true), bins)
    if mask is not None:
        m = _flat(mask).to(pred.dtype)
        if mask2 is not None:
            m = m * _flat(mask2).to(pred.dtype)
        wp = wp * m.unsqueeze(-1)
        M = m.sum(1)
    else:
        M = torch.full((pred.shape[0],), float(pred[0].numel()), dtype=pred.dtype, device=pred.device)
    return torch.einsum("bva,bvc->bac", wp, wt), M


def mi_of(P, M):
    """(p (B,K,K), MI (B,)) of a joint histogram and its weight"""
    ok = M > 0
    p = P / torch.where(ok, M, torch.ones_like(M)).view(-1, 1, 1)
    pa, pb = p.sum(2, keepdim=True), p.sum(1, keepdim=True)
    val = (p * (torch.log(p + EPS) - torch.log(pa * pb + EPS))).sum((1, 2))
    return p, torch.where(ok, val, torch.zeros_like(val))


def mi(pred, true, bins: int = 32, mask=None, mask2=None):
    """MI_b, (B,)"""
    return mi_of(*joint(pred, true, bins, mask, mask2))[1]


def histogram(pred, true, bins: int = 32, mask=None, mask2=None):
    """the normalised joint histogram p (B,K,K) (zeros for an empty mask)"""
    return mi_of(*joint(pred, true, bins, mask, mask2))[0]


def loss_masked(pred, true, mask, mask2=None, bins: int = 32, gamma: float = 0.05):
    return -gamma * float(pred[0].numel()) * mi(pred, true, bins, mask, mask2).mean()


def loss(pred, true, bins: int = 32, gamma: float = 0.05):
    return loss_masked(pred, true, None, None, bins, gamma)


def grad(pred, true, bins: int = 32, gamma: float = 0.05, mask=None, mask2=None, upstream: float = 1.0):
    """(loss, d (upstream loss) / d pred) by autograd"""
    p = pred.detach().clone().requires_grad_(True)
    val = loss_masked(p, true, mask, mask2, bins, gamma)
    (g,) = torch.autograd.grad(val * upstream, p)
    return val.detach(), g


# ------------------------------------------------------------------------------------------------ inputs
def remap(v):
    """another 'contrast': a non-monotonic intensity map of [0,1] onto itself"""
    return 4.0 * v * (1.0 - v)


def smooth(B: int, size, seed: int, dtype=torch.float64):
    """a coarse lattice of uniform noise, linearly up-sampled: (B,1,*size) in [0,1], volumes or slices"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.rand(B, 1, *[max(s // 4, 2) for s in size], generator=g, dtype=torch.float64)
    return F.interpolate(lat, size=tuple(size), mode="trilinear" if len(size) == 3 else "bilinear", align_corners=False).to(dtype)


def ball(B: int, size, radius: float = 0.4):
    """1 inside an ellipsoid of semi-axes radius x extent, 0 outside: (B,1,*size) float64"""
    axes = [torch.linspace(-0.5, 0.5, s, dtype=torch.float64) for s in size]
    r2 = sum((g / radius) ** 2 for g in torch.meshgrid(*axes, indexing="ij"))
    return (r2 <= 1.0).double()[None, None].repeat(B, 1, *([1] * len(size)))


def make_pair(B: int, size, kind: str, seed: int = 11):
    """(pred, true) float64 holding fp32-representable values (the float64 reference and the fp32 runs see the same numbers).
    smooth: a lattice image and a shifted neighbour of it remapped; edges: the same stretched past [0,1], with values exactly 0 and 1;
    sparse: 90 % of the voxels exactly 0 in both images (a skull-stripped scan's background)"""
    a, b = smooth(B, size, seed), smooth(B, size, seed + 1)
    pred, true = 0.7 * a + 0.3 * b, remap(a)
    if kind == "edges":
        pred, true = 3.0 * (pred - 0.5) + 0.5, 1.4 * true - 0.2
        flat = pred.view(-1)
        flat[0::7], flat[3::7] = 0.0, 1.0
        true.view(-1)[1::5] = 1.0
        true.view(-1)[2::5] = 0.0
    elif kind == "sparse":
        keep = (torch.rand(pred.shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64) < 0.1).double()
        pred, true = pred * keep, true * keep
    elif kind != "smooth":
        raise ValueError(kind)
    return pred.float().double(), true.float().double()


def make_masks(B: int, size, kind):
    """None / 'ball' / 'ball_x_rand' -> (mask, mask2) float64 (fp32-representable)"""
    if kind is None:
        return None, None
    m = ball(B, size)
    if kind == "ball":
        return m, None
    r = torch.rand(B, 1, *size, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    return m, r.float().double()


# (B, size, bins, input kind, masks) of the GPU tests.  Shapes: less than one 64-voxel chunk x 4 with an odd tail; odd with two batch elements;
# several workgroups with a ragged last one; a slice.  Bins: the smallest, one tile, the one-tile edge, the first two-tile size, the largest.
SHAPES = [(1, (5, 6, 7)), (2, (7, 9, 11)), (2, (20, 24, 20)), (2, (33, 47))]
BINS = [4, 16, 32, 33, 64]
CASES = ([(B, size, K, "smooth", None) for B, size in SHAPES for K in BINS]
         + [(2, (7, 9, 11), K, "edges", None) for K in (32, 64)]
         + [(2, (20, 24, 20), K, "sparse", None) for K in (32, 33)]
         + [(B, size, K, "smooth", mk) for B, size, K in ((2, (20, 24, 20), 32), (2, (7, 9, 11), 64), (2, (33, 47), 16)) for mk in ("ball", "ball_x_rand")])
UPSTREAM = 1.7


@functools.lru_cache(maxsize=None)
def case(B, size, bins, kind, masks, dtype=torch.float64):
    """(pred, true, mask, mask2, p, MI, loss, gradient) of one case, evaluated once in dtype and left unchanged"""
    cast = lambda t: None if t is None else t.to(dtype)
    pred, true = (cast(t) for t in make_pair(B, size, kind))
    m1, m2 = (cast(t) for t in make_masks(B, size, masks))
    p, val = mi_of(*joint(pred, true, bins, m1, m2))
    lv, g = grad(pred, true, bins, 0.05, m1, m2, UPSTREAM)
    return pred, true, m1, m2, p, val, lv, g


def rel_l2(got, ref) -> float:
    ref = ref.double()
    return float((got.double().to(ref.device) - ref).norm() / ref.norm())


def own_figures(cases=None):
    """(p max abs, loss relative, gradient relative L2) of the float32 evaluation against float64: the worst over the cases"""
    worst = [0.0, 0.0, 0.0]
    for c in (CASES if cases is None else cases):
        *_, p64, _, l64, g64 = case(*c)
        *_, p32, _, l32, g32 = case(*c, torch.float32)
        worst[0] = max(worst[0], float((p32.double() - p64).abs().max()))
        worst[1] = max(worst[1], abs(float(l32) - float(l64)) / abs(float(l64)))
        worst[2] = max(worst[2], rel_l2(g32, g64))
    return tuple(worst)
