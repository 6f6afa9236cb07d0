"""Affine pre-alignment without a GPU: the float64 definition of tests/affine_ref.py checked against itself (autograd,
brute force, the oracle's warp), the recovery of a known transform by its fitting loop, and the public surface - header, library argument
checks, the refusals of pulpo_amd.ops / affine / evaluation.  tests/test_gpu_affine.py holds the kernels and pulpo_amd.affine.fit to this
definition."""
import ctypes
import inspect

import pytest
import torch

import affine_ref as AR
from oracle import pulpo_oracle as O

FB = list(O.FEEDBACK_DEFAULT)
# the recovery condition: from a start of at least START_MIN voxels of corner displacement the fit ends within END_MAX of the expected fit
START_MIN, END_MAX = 4.4, 1.0
RECOVERY_SIZE = (24, 32, 28)


# ================================================================================================ the definition against itself
def test_reference_warp_is_the_oracles():
    """warp_field (explicit corners through sample_coords) = the oracle's grid_sample warp, on unequal grids and with clamped samples"""
    img = AR.smooth_image(2, 3, (6, 5, 8), 1)
    df = AR.field(AR.theta_generic(2, 4, shift=3.0), (5, 6, 7))
    assert float((AR.warp_field(df, img) - O.warp(df, img)).abs().max()) < 1e-13


@pytest.mark.parametrize("size,isize,shift", [((5, 6, 7), (5, 6, 7), 1.5), ((9, 10, 11), (12, 8, 10), 1.5), ((5, 6, 7), (5, 6, 7), 4.0),
                                              ((1, 12, 10), (1, 12, 10), 1.0)])
def test_analytic_gtheta_is_autograd_of_the_warp(size, isize, shift):
    """gtheta (the expression the kernel evaluates) against torch autograd through the reference's own warp, float64; the third case clamps
    a good part of the samples (dscale = 0 there), the last is the 2-D form: the depth row and column of the gradient are exactly 0"""
    B, C = 2, 3
    img = AR.smooth_image(B, C, isize, 2)
    theta = AR.theta_generic(B, 5, shift=shift)
    if size[0] == 1:
        theta = AR.lift_theta(theta[:, 1:, 1:].contiguous())
    gout = torch.randn(B, C, *size, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    leaf = theta.clone().requires_grad_(True)
    (AR.warp(leaf, img, size) * gout).sum().backward()
    got = AR.gtheta(theta, img, gout, size)
    if size[0] == 1:
        assert bool((got[:, 0] == 0).all()) and bool((got[:, :, 0] == 0).all())
        keep = torch.ones(3, 4, dtype=torch.bool)
        keep[0], keep[:, 0] = False, False
        got, want = got[:, keep], leaf.grad[:, keep]
    else:
        want = leaf.grad
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if shift > 3:
        _, raw, dscale = AR.sample_coords(AR.grid(size, torch.float64).unsqueeze(0) + AR.field(theta, size), size, isize)
        assert float((dscale == 0).double().mean()) > 0.05, "the clamp case clamps nothing"


def test_compose_is_the_two_step_route_where_nothing_is_interpolated_twice():
    """df built so that the first sampling lands on integer indices: warp(compose(theta, df), img) = warp(df, warp(theta, img)) to rounding"""
    Sg, Si = (6, 5, 7), (12, 10, 14)
    img = AR.smooth_image(1, 2, Si, 6)
    theta = AR.theta_generic(1, 7)
    v = AR.grid(Sg, torch.float64).unsqueeze(0)
    df = integer_landing_field(Sg, Si, (1, -1, 2))
    q, _, _ = AR.sample_coords(v + df, Sg, Si)
    assert float((q - q.round()).abs().max()) < 1e-12
    one = AR.warp_field(AR.compose(theta, df, Si), img)
    two = AR.warp_field(df, AR.warp(theta, img))
    assert float((one - two).abs().max()) < 1e-12


def integer_landing_field(Sg, Si, shift):
    """df on grid Sg with v + df(v) = (w + 0.5)(Sg - 1)/Si, w = 2 v + shift clamped into the image: the sampler's index is the integer w"""
    v = AR.grid(Sg, torch.float64).unsqueeze(0)
    out = []
    for a in range(3):
        w = (2 * v[:, a] + shift[a]).clamp(0, Si[a] - 1)
        out.append((w + 0.5) * (Sg[a] - 1) / Si[a] - v[:, a])
    return torch.stack(out, 1)


def test_expected_fit_against_brute_force():
    """y -> x = warp(A_gen, y) -> warp(expected_fit, x) comes back to y: RMSE well below the unaligned pair's, and below what the plain
    inverse of A_gen gives; the formula is its own inverse; invert() is the matrix inverse"""
    size = (24, 32, 28)
    x, y, want = AR.affine_pair(size)
    rm = lambda a, b: float(((a - b) ** 2).mean().sqrt())
    unaligned, back, naive = rm(x, y), rm(AR.warp(want, x), y), rm(AR.warp(AR.invert(AR.theta_gen_case(), size), x), y)
    print(f"FIGURE rmse unaligned {unaligned:.4f} expected_fit {back:.4f} plain inverse {naive:.4f}")
    assert back < 0.4 * unaligned and back < naive
    th = AR.theta_gen_case()
    assert float((AR.expected_fit(AR.expected_fit(th, size), size) - th).abs().max()) < 1e-12
    assert float((AR.to_abs(AR.invert(th, size), size) @ AR.to_abs(th, size) - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-12


def test_package_helpers_are_the_references():
    """pulpo_amd.affine's identity / invert / rescale / expected_fit / corner_error on CPU tensors against affine_ref"""
    from pulpo_amd import affine
    size = (24, 32, 28)
    th = AR.theta_generic(2, 9)
    assert torch.equal(affine.identity(2, "cpu"), AR.identity(2, torch.float32)) and tuple(affine.identity(1, "cpu", ndims=2).shape) == (1, 2, 3)
    assert float((affine.invert(th, size) - AR.invert(th, size)).abs().max()) < 1e-12
    assert float((affine.expected_fit(th, size) - AR.expected_fit(th, size)).abs().max()) < 1e-12
    assert abs(float(affine.corner_error(th, AR.identity(2), size)) - AR.corner_error(th, AR.identity(2), size)) < 1e-12
    # rescale: the same physical transform - a point's image on the fine grid, scaled, is the scaled point's image on the coarse grid
    to = (12, 16, 14)
    r = torch.tensor([t / f for f, t in zip(size, to)], dtype=torch.float64)
    small = affine.rescale(th, size, to)
    pts = torch.rand(3, 50, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 20
    c, cs = AR.centre(size, torch.float64).view(3, 1), AR.centre(to, torch.float64).view(3, 1)
    fine = AR.positions(th, pts + c, size) - c
    coarse = AR.positions(small, pts * r.view(3, 1) + cs, to) - cs
    assert float((fine * r.view(1, 3, 1) - coarse).abs().max()) < 1e-10
    th2 = AR.theta_generic(1, 3)[:, 1:, 1:].contiguous()
    assert tuple(affine.invert(th2, (20, 24)).shape) == (1, 2, 3)


# ================================================================================================ the fitting loop recovers a known transform
@pytest.mark.parametrize("dof", [12, 6])
def test_reference_fit_recovers_the_transform(dof):
    """the float64 fit on the synthetic pair at 24 x 32 x 28 (dof 6: the pair whose expected fit is rigid): the largest corner displacement
    from the expected fit ends at most 1.0 voxel from a start of at least 4.4; the loss history does not rise at its last row against its
    first, nor within any level.  Measured: affine 4.90 -> 0.45, rigid 4.45 -> see the FIGURE line."""
    theta, hist, want, *_ = AR.fit_reference(RECOVERY_SIZE, "ncc", dof)
    start, end = AR.corner_error(AR.identity(1), want, RECOVERY_SIZE), AR.corner_error(theta, want, RECOVERY_SIZE)
    print(f"FIGURE reference fit dof {dof}: corner error {start:.3f} -> {end:.3f}; loss {float(hist[0, 0]):.2f} -> {float(hist[-1, 0]):.2f}")
    assert start >= START_MIN and end <= END_MAX
    assert tuple(hist.shape) == (sum(AR.DEFAULT_ITERS) + 1, 2)
    assert float(hist[-1, 0]) <= float(hist[0, 0])
    for lvl in (2, 1, 0):
        rows = hist[:-1][hist[:-1, 1] == lvl, 0]
        assert float(rows[-1]) <= float(rows[0]), lvl


# ================================================================================================ the public surface
def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert protos["pulpo_affine_field"] == (I, [P, P, I, I, I, I, P])
    assert protos["pulpo_affine_warp_fwd"] == (I, [P, P, P] + [I] * 8 + [P])
    assert protos["pulpo_affine_warp_bwd_ws_bytes"] == (ctypes.c_size_t, [I, I, I, I])
    assert protos["pulpo_affine_warp_bwd"] == (I, [P, P, P, P, P] + [I] * 8 + [P])
    assert protos["pulpo_affine_compose"] == (I, [P, P, P] + [I] * 7 + [P])
    assert header_abi_version() == 8


def test_library_refuses_bad_arguments():
    """null pointers, zero extents, C = 0, B = 0, a null workspace, a 3-D grid on a depth-1 image: the library's error code before any launch"""
    from pulpo_amd._lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = lambda: lib.raw("pulpo_last_error")()
    f = lib.raw("pulpo_affine_field")
    assert f(None, p, 1, 2, 2, 2, None) != 0 and f(p, None, 1, 2, 2, 2, None) != 0 and b"null" in err()
    assert f(p, p, 0, 2, 2, 2, None) != 0 and f(p, p, 1, 0, 2, 2, None) != 0 and f(p, p, 1, 2, 0, 2, None) != 0 and f(p, p, 1, 2, 2, 0, None) != 0
    f = lib.raw("pulpo_affine_warp_fwd")
    ok = (1, 1, 2, 2, 2, 2, 2, 2)
    for bad in range(3):
        args = [p, p, p]
        args[bad] = None
        assert f(*args, *ok, None) != 0 and b"null" in err()
    for bad in range(8):
        dims = list(ok)
        dims[bad] = 0
        assert f(p, p, p, *dims, None) != 0, bad
    assert f(p, p, p, 1, 1, 1, 2, 2, 2, 2, 2, None) != 0 and b"2-D" in err()           # a depth-1 grid on a 3-D image
    f = lib.raw("pulpo_affine_warp_bwd")
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        assert f(*args, p, *ok, None) != 0 and b"null" in err()
    assert f(p, p, p, p, None, *ok, None) != 0 and b"workspace" in err()
    for bad in range(8):
        dims = list(ok)
        dims[bad] = 0
        assert f(p, p, p, p, p, *dims, None) != 0, bad
    q = lib.raw("pulpo_affine_warp_bwd_ws_bytes")
    assert q(0, 2, 2, 2) == 0 and q(1, 0, 2, 2) == 0 and q(2, 5, 6, 7) == 2 * 12 * 8 and q(1, 64, 64, 64) == 1024 * 12 * 8
    f = lib.raw("pulpo_affine_compose")
    ok = (1, 2, 2, 2, 2, 2, 2)
    for bad in range(3):
        args = [p, p, p]
        args[bad] = None
        assert f(*args, *ok, None) != 0 and b"null" in err()
    for bad in range(7):
        dims = list(ok)
        dims[bad] = 0
        assert f(p, p, p, *dims, None) != 0, bad
    assert f(p, p, p, 1, 1, 4, 4, 2, 4, 4, None) != 0                                     # depth 1 on one grid only


def test_cpu_tensors_and_wrong_arguments_are_refused():
    from pulpo_amd import affine, ops, synthetic
    from pulpo_amd._lib import PulpoHipError
    theta, img = AR.identity(1, torch.float32), torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(PulpoHipError):
        ops.affine_field(theta, (4, 4, 4))
    with pytest.raises(PulpoHipError):
        ops.affine_warp(theta, img)
    with pytest.raises(PulpoHipError):
        ops.affine_compose(theta, torch.zeros(1, 3, 4, 4, 4))
    with pytest.raises(PulpoHipError):
        affine.fit(img, img, levels=1, iters=[1])
    with pytest.raises(ValueError, match="data"):
        ops.affine_warp(theta, img.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ops.affine_field(torch.zeros(1, 4, 4), (4, 4, 4))
    with pytest.raises(ValueError):
        ops.affine_field(theta, (4, 4))
    with pytest.raises(ValueError):
        ops.affine_warp(theta, torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match="dof"):
        affine.fit(img, img, dof=7)
    with pytest.raises(ValueError):
        affine.fit(img, img, loss="dice")
    with pytest.raises(ValueError):
        affine.fit(img, img, levels=2, iters=[1])
    assert list(inspect.signature(synthetic.affine_pair).parameters) == ["size", "batch", "seed", "device", "theta_gen"]
    sig = inspect.signature(affine.fit).parameters
    assert [k for k in sig][:2] == ["x", "y"] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    assert sig["dof"].default == 12 and sig["levels"].default == 3 and sig["loss"].default == "ncc" and sig["lr"].default == affine.DEFAULT_LR
    assert (affine.DEFAULT_LR, affine.DEFAULT_ITERS, affine.DEFAULT_WIN) == (AR.DEFAULT_LR, AR.DEFAULT_ITERS, AR.DEFAULT_WIN)


def test_performance_accepts_affine_and_refuses_it_with_inverse():
    """a CPU model and CPU tensors: affine= with inverse=True raises NotImplementedError before anything else; without it the call reaches the
    operators, which refuse the CPU tensors"""
    import src.models as models
    from pulpo_amd import evaluation
    from pulpo_amd._lib import PulpoHipError
    assert inspect.signature(evaluation.performance).parameters["affine"].default is None
    assert inspect.signature(evaluation.affine_scores).parameters["theta"].default is None
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2).eval()
    x = torch.zeros(1, 1, 16, 16, 16)
    theta = AR.identity(1, torch.float32)
    with pytest.raises(NotImplementedError):
        evaluation.performance(m, x, x, affine=theta, inverse=True)
    with pytest.raises(NotImplementedError):
        evaluation.performance(m, x, x, affine={}, inverse=True)
    with pytest.raises(PulpoHipError):
        evaluation.performance(m, x, x, affine=theta)
