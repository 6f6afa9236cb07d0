"""CPU-side tests of the inverse-field feature: the property it rests on, shown on the CPU oracle with the float64 helpers of
tests/inverse_ref.py (the integral of -v inverts the integral of v far better than the negated field does), and the argument checks of
the three entry points of pulpo_amd/csrc/inverse.hip."""
import ctypes

import pytest
import torch

import inverse_ref as R
from oracle import pulpo_oracle as O

SIZES = [(16, 16, 16), (24, 20, 28)]


@pytest.fixture(scope="module")
def integrated():
    """{size: (fwd, inv)} = (O.vecint(v), O.vecint(-v)) in float64 for the smooth field of the recipe, amplitude 3: computed once"""
    out = {}
    for size in SIZES:
        v = R.smooth_field(size, 3.0).double()
        out[size] = (O.vecint(v), O.vecint(-v))
    return out


@pytest.mark.parametrize("size", SIZES)
def test_integral_of_negated_velocity_is_the_better_inverse(integrated, size):
    """mean ||inv(p) + fwd(p + inv(p))|| with inv = VecInt(-v) at most half of that with inv = -fwd.  Measured: 0.0525 against 0.2460
    (ratio 0.21) at 16^3, 0.0225 against 0.1545 (0.15) at 24 x 20 x 28."""
    fwd, inv = integrated[size]
    exact, _ = R.inverse_consistency(fwd, inv)
    first_order, _ = R.inverse_consistency(fwd, -fwd)
    print(f"{size}: residual {exact:.4f} with VecInt(-v), {first_order:.4f} with -fwd, ratio {exact / first_order:.2f}")
    assert 0.0 < exact <= 0.5 * first_order


@pytest.mark.parametrize("size", SIZES)
def test_transport_by_the_inverse_field_beats_the_first_order_rule(integrated, size):
    """64 points q with known preimages p (q = p + fwd(p)): q + inv(q) lands at most half as far from p in the mean as the interpolated
    first-order rule q - fwd(q).  Measured: 0.028 against 0.147 voxels (ratio 0.19) at 16^3, 0.016 against 0.094 (0.17) at 24 x 20 x 28."""
    fwd, inv = integrated[size]
    q, p = R.points_with_preimages(fwd, 64)
    exact = (R.transport_points(q, inv)[0] - p.double()).norm(dim=1)
    first_order = (q.double() - R.geo_sample(fwd, q.double()[None])[0].reshape(3, -1).t() - p.double()).norm(dim=1)
    print(f"{size}: transport error mean / max {float(exact.mean()):.3f} / {float(exact.max()):.3f} with q + inv(q), "
          f"{float(first_order.mean()):.3f} / {float(first_order.max()):.3f} with q - fwd(q)")
    assert 0.0 < float(exact.mean()) <= 0.5 * float(first_order.mean())


def test_helper_sampler_is_the_geometric_one():
    """a zero field is the identity, values at voxel centres are the field's own, positions clamp to the border, 2-D form"""
    gen = torch.Generator().manual_seed(0)
    f = torch.randn(2, 3, 5, 6, 7, generator=gen)
    pos = R.identity((5, 6, 7)).expand(2, -1, -1, -1, -1)
    tight = dict(rtol=0.0, atol=1e-13)           # (the normalised coordinate of grid_sample rounds in float64: 1e-16 of a neighbour's value)
    torch.testing.assert_close(R.geo_sample(f, pos), f.double(), **tight)
    assert R.inverse_consistency(torch.zeros(1, 3, 4, 5, 6), torch.zeros(1, 3, 4, 5, 6)) == (0.0, 0.0)
    out = R.transport_points(torch.tensor([[1.5, 2.0, 3.0], [-4.0, 2.0, 99.0]]), f)
    assert tuple(out.shape) == (2, 2, 3)
    torch.testing.assert_close(out[1, 0], torch.tensor([1.5, 2.0, 3.0]).double() + 0.5 * (f[1, :, 1, 2, 3] + f[1, :, 2, 2, 3]).double())
    torch.testing.assert_close(out[0, 1], torch.tensor([-4.0, 2.0, 99.0]).double() + f[0, :, 0, 2, 6].double())
    f2 = torch.randn(1, 2, 6, 7, generator=gen)
    torch.testing.assert_close(R.geo_sample(f2, R.identity((6, 7))), f2.double(), **tight)
    shifted = R.consistency_residual(torch.zeros(1, 2, 6, 7), torch.ones(1, 2, 6, 7))
    torch.testing.assert_close(shifted, torch.full((1, 6, 7), 2.0 ** 0.5, dtype=torch.float64))


def test_entry_points_reject_null_pointers_and_bad_sizes():
    from pulpo_amd._lib import header_abi_version, lib, parse_header
    protos = parse_header()
    names = ("pulpo_vecint_pair_fwd", "pulpo_vecint_pair_scratch_floats", "pulpo_inverse_consistency", "pulpo_inverse_consistency_ws_bytes",
             "pulpo_transport_points")
    for name in names:
        assert name in protos, name
    assert header_abi_version() >= 6
    pair, cons, pts = (lib.raw(n) for n in ("pulpo_vecint_pair_fwd", "pulpo_inverse_consistency", "pulpo_transport_points"))
    p = ctypes.c_void_p(256)                        # never dereferenced: every call below fails its argument check first
    flag = ctypes.cast(256, ctypes.POINTER(ctypes.c_int))
    assert pair(None, p, p, p, 1, 8, 8, 8, 7, None) != 0 and pair(p, None, p, p, 1, 8, 8, 8, 7, None) != 0
    assert pair(p, p, None, p, 1, 8, 8, 8, 7, None) != 0
    assert pair(p, p, p, None, 1, 16, 16, 16, 7, None) != 0          # the step form needs its scratch
    for bad in ((0, 8, 8, 8, 7), (1, 0, 8, 8, 7), (1, 8, 1, 8, 7), (1, 8, 8, -3, 7), (1, 8, 8, 8, -1)):
        assert pair(p, p, p, p, *bad, None) != 0, bad
    assert b"vecint_pair_fwd" in lib.raw("pulpo_last_error")()
    assert cons(None, p, p, p, 1, 8, 8, 8, None) != 0 and cons(p, None, p, p, 1, 8, 8, 8, None) != 0
    assert cons(p, p, None, p, 1, 8, 8, 8, None) != 0 and cons(p, p, p, None, 1, 8, 8, 8, None) != 0
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0)):
        assert cons(p, p, p, p, *bad, None) != 0, bad
    assert pts(None, p, p, 4, 1, 3, 8, 8, 8, flag, None) != 0 and pts(p, None, p, 4, 1, 3, 8, 8, 8, flag, None) != 0
    assert pts(p, p, None, 4, 1, 3, 8, 8, 8, flag, None) != 0 and pts(p, p, p, 4, 1, 3, 8, 8, 8, None, None) != 0
    for bad in ((0, 1, 3, 8, 8, 8), (4, 0, 3, 8, 8, 8), (4, 1, 4, 8, 8, 8), (4, 1, 2, 8, 8, 8), (4, 1, 3, 0, 8, 8), (4, 1, 3, 8, 8, -2)):
        assert pts(p, p, p, *bad, flag, None) != 0, bad
    # the size queries: two scratch fields for the step form, none for the one-launch form (up to 2048 voxels) and for nsteps == 0
    q = lambda *a: lib.query("pulpo_vecint_pair_scratch_floats", *a)
    assert q(1, 10, 10, 10, 7) == 0 and q(2, 8, 16, 16, 7) == 0 and q(1, 13, 13, 13, 7) == 2 * 3 * 13 ** 3
    assert q(2, 24, 20, 28, 4) == 2 * 2 * 3 * 24 * 20 * 28 and q(1, 24, 20, 28, 0) == 0 and q(0, 8, 8, 8, 7) == 0
    w = lambda *a: lib.query("pulpo_inverse_consistency_ws_bytes", *a)
    assert w(1, 16, 16, 16) == 16 * 16 and w(1, 160, 160, 160) == 1024 * 16 and w(1, 1, 24, 20) == 2 * 16 and w(1, 0, 4, 4) == 0
