"""The bending-energy regulariser's definition in float64, plain torch: the value written with slices, the gradient
from autograd.  Central differences at interior voxels only - no padding, no one-sided stencil -, which is what makes an affine field
cost exactly nothing.

    u_xx = u[x+1] - 2u + u[x-1]                                               (u_yy, u_zz alike)
    u_xy = (u[x+1,y+1] - u[x+1,y-1] - u[x-1,y+1] + u[x-1,y-1]) / 4            (u_xz, u_yz alike)
    e    = u_xx^2 + u_yy^2 + u_zz^2 + 2 u_xy^2 + 2 u_xz^2 + 2 u_yz^2
    Bending_reg(u, lamb) = lamb * D*H*W * mean over (B, C, interior voxels) of e

A depth of 1 (or a 4-D (B,C,H,W) field) is the 2-D form: no z term, interior 1..H-2, 1..W-2, factor H*W."""
import torch


def _sl(o):
    """the interior shifted by o in {-1, 0, 1}"""
    return slice(1 + o, None if o == 1 else o - 1)


def density(u: torch.Tensor) -> torch.Tensor:
    """e at the interior voxels: (B,C,D-2,H-2,W-2) of a 5-D field with D >= 3, (B,C,H-2,W-2) of a 4-D field or, with a depth axis kept,
    of a 5-D field with D == 1"""
    if u.dim() == 5 and u.shape[2] == 1:
        return density(u[:, :, 0]).unsqueeze(2)
    nd = u.dim() - 2
    if nd not in (2, 3) or min(u.shape[2:]) < 3:
        raise ValueError(f"bending_ref: every extent of {tuple(u.shape)} other than a depth of 1 must be at least 3")

    def at(*offs):
        return u[(slice(None), slice(None)) + tuple(_sl(o) for o in offs)]

    zero = (0,) * nd
    e = 0.0
    for a in range(nd):
        p, m = list(zero), list(zero)
        p[a], m[a] = 1, -1
        e = e + (at(*p) - 2.0 * at(*zero) + at(*m)) ** 2
        for b in range(a + 1, nd):
            pp, pm, mp, mm = list(zero), list(zero), list(zero), list(zero)
            pp[a], pp[b] = 1, 1
            pm[a], pm[b] = 1, -1
            mp[a], mp[b] = -1, 1
            mm[a], mm[b] = -1, -1
            e = e + 2.0 * ((at(*pp) - at(*pm) - at(*mp) + at(*mm)) / 4.0) ** 2
    return e


def bending_ref(u: torch.Tensor, lamb: float) -> torch.Tensor:
    """Bending_reg(u, lamb) in u's dtype (use float64); differentiable"""
    size = 1
    for s in u.shape[2:]:
        size *= int(s)
    return lamb * size * density(u).mean()


def bending_grad_ref(u: torch.Tensor, lamb: float, upstream: float = 1.0) -> torch.Tensor:
    x = u.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad(bending_ref(x, lamb), [x], grad_outputs=torch.tensor(upstream, dtype=x.dtype, device=x.device))
    return g


def affine_field(theta: torch.Tensor, size) -> torch.Tensor:
    """the displacement field u(p) = A p + t - p of theta = [A | t] ((B, n, n+1), voxels, coordinates in the order of `size`): (B, n, *size)"""
    n = len(size)
    axes = [torch.arange(s, dtype=theta.dtype, device=theta.device) for s in size]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"))                       # (n, *size)
    lin = torch.einsum("bij,j...->bi...", theta[:, :, :n], grid)
    t = theta[:, :, n].reshape(theta.shape[0], n, *([1] * n))
    return lin + t - grid.unsqueeze(0)
