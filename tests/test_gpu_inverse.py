"""GPU tests of the inverse-field feature (pulpo_amd/csrc/inverse.hip): ops.vecint_pair against the float64 oracle, its memory and its
differentiable fallback; ops.inverse_consistency and ops.transport_points against the float64 helpers of tests/inverse_ref.py; the
property the feature rests on, on the device; PULPo.predict_bidirectional / combine_dfs_bidirectional against the existing operators;
the inverse rows of evaluation.performance."""
import functools
import os

import pytest
import torch

import inverse_ref as R
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
FB = list(O.FEEDBACK_DEFAULT)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ================================================================================================ vecint_pair
@functools.lru_cache(maxsize=None)
def _velocity(B, size, amp, nsteps):
    """a randn * amp velocity and the float64 oracle's integrals of +v and -v: computed once per case, never written to"""
    gen = torch.Generator().manual_seed(B * 1000 + size[0] * 10 + nsteps)
    v = torch.randn(B, 3, *size, generator=gen) * amp
    return v, O.vecint(v.double(), nsteps), O.vecint(-v.double(), nsteps)


# the one-launch form (<= 2048 voxels per batch element) | just above the switch | the step form, the last case clamping at the border
PAIR_CASES = [(1, (10, 10, 10), 1.5, 7), (2, (6, 7, 5), 1.0, 7), (1, (13, 13, 13), 2.0, 7), (2, (24, 20, 28), 1.0, 7), (1, (16, 32, 18), 12.0, 7),
              # the parity of the ping-pong, and nsteps == 0, on one small and one large case
              (2, (6, 7, 5), 1.0, 0), (2, (6, 7, 5), 1.0, 4), (2, (24, 20, 28), 1.0, 0), (2, (24, 20, 28), 1.0, 4)]


@pytest.mark.parametrize("B,size,amp,nsteps", PAIR_CASES)
def test_vecint_pair_against_fp64_oracle(ops, B, size, amp, nsteps):
    """fwd and inv within rel_l2 1e-5 of O.vecint(+-v.double()), the bound test_vecint_backward_lds_tiled_scatter_vs_oracle holds ops.vecint
    to; fwd equal to ops.vecint(v) at the same bound (the test prints whether the bits agree: pytest -s); the input is not written to."""
    v, ref_f, ref_i = _velocity(B, size, amp, nsteps)
    vg = v.cuda()
    with torch.no_grad():
        fwd, inv = ops.vecint_pair(vg, nsteps)
        single = ops.vecint(vg, nsteps)
    assert fwd.shape == vg.shape == inv.shape and not fwd.requires_grad and not inv.requires_grad
    assert torch.equal(vg.cpu(), v)
    ef, ei, es = rel_l2(fwd, ref_f), rel_l2(inv, ref_i), rel_l2(fwd, single)
    print(f"vecint_pair B={B} {size} amp={amp} nsteps={nsteps}: fwd {ef:.2e}, inv {ei:.2e}, fwd against ops.vecint {es:.2e} "
          f"(bits equal: {torch.equal(fwd, single)})")
    assert ef < 1e-5 and ei < 1e-5
    assert es < 1e-5
    if nsteps == 0:
        assert torch.equal(fwd, vg) and torch.equal(inv, -vg)
    # a tensor that requires grad takes the kernel too when autograd is off
    with torch.no_grad():
        f2, i2 = ops.vecint_pair(vg.clone().requires_grad_(True), nsteps)
    assert torch.equal(f2, fwd) and torch.equal(i2, inv)


def test_vecint_pair_2d(ops):
    gen = torch.Generator().manual_seed(11)
    v = (torch.randn(1, 2, 24, 20, generator=gen) * 1.5).cuda()
    fwd, inv = ops.vecint_pair(v)
    assert tuple(fwd.shape) == (1, 2, 24, 20) == tuple(inv.shape)
    assert rel_l2(fwd, ops.vecint(v)) < 1e-5 and rel_l2(inv, ops.vecint(-v)) < 1e-5


def test_vecint_pair_keeps_no_intermediate_fields(ops):
    """40^3, B = 1: above the input, two results and two scratch fields (4 n, n = 3 D H W 4 bytes; bound 4.5 n); two ops.vecint calls hold
    the nsteps + 1 fields of each direction (16 n; printed)."""
    S = 40
    n = 3 * S ** 3 * 4
    v = torch.randn(1, 3, S, S, S, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        ops.vecint_pair(v)                                   # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fwd, inv = ops.vecint_pair(v)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        del fwd, inv
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        a, b = ops.vecint(v), ops.vecint(-v)
        torch.cuda.synchronize()
        two_calls = torch.cuda.max_memory_allocated() - before
    print(f"peak above the input at 40^3: vecint_pair {grown / n:.2f} n, two vecint calls {two_calls / n:.2f} n")
    assert 2 * n <= grown <= 4.5 * n, grown / n


def test_vecint_pair_differentiable_fallback(ops):
    """with v.requires_grad (and autograd on) the results carry a graph through the existing backward kernels: the gradient of
    (inv * up).sum() is that of ops.vecint(-v).  Exactly so with the ordered sums of ops.set_deterministic: the default backward adds
    with float atomics in arrival order, so even two runs of ops.vecint(-v) itself differ in the last bits - there the two are held to
    rel_l2 1e-6."""
    gen = torch.Generator().manual_seed(21)
    v = (torch.randn(2, 3, 12, 10, 14, generator=gen) * 1.5).cuda()
    up = torch.randn(2, 3, 12, 10, 14, generator=gen).cuda()
    env_det = os.environ.get("PULPO_DETERMINISTIC", "0") == "1"
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            v1 = v.clone().requires_grad_(True)
            fwd, inv = ops.vecint_pair(v1)
            assert fwd.requires_grad and inv.requires_grad
            g1, = torch.autograd.grad((inv * up).sum(), [v1])
            v2 = v.clone().requires_grad_(True)
            g2, = torch.autograd.grad((ops.vecint(-v2) * up).sum(), [v2])
            assert float(g1.abs().max()) > 0
            if det:
                assert torch.equal(g1, g2)
            else:
                assert rel_l2(g1, g2) < 1e-6
            gf, = torch.autograd.grad((fwd * up).sum(), [v1])
            assert rel_l2(gf, torch.autograd.grad((ops.vecint(v2) * up).sum(), [v2])[0]) < 1e-6
    finally:
        ops.set_deterministic(env_det)


# ================================================================================================ inverse_consistency
CONS_CASES = [("smooth", 1, (16, 16, 16)), ("smooth", 2, (17, 23, 12)), ("clamp", 1, (16, 16, 16)), ("smooth", 1, (24, 20))]


@pytest.mark.parametrize("kind,B,size", CONS_CASES)
def test_inverse_consistency_against_fp64(ops, kind, B, size):
    """mean and maximum within 1e-5 relative of the float64 helper on the same fp32 fields; two calls give the same bits.  The smooth pairs
    are the device's integrals of +v and -v of the recipe's field, amplitude 3: displacements of a few voxels whose residual is a few
    hundredths of a voxel (0.0525 in the mean at 16^3 on the CPU oracle); "clamp" is randn * 6, whose positions leave the volume."""
    nd = len(size)
    if kind == "clamp":
        gen = torch.Generator().manual_seed(9)
        a, b = (torch.randn(B, nd, *size, generator=gen) * 6).cuda(), (torch.randn(B, nd, *size, generator=gen) * 6).cuda()
    else:
        a, b = ops.vecint_pair(R.smooth_field(size, 3.0, B=B).cuda())
    mean, mx = ops.inverse_consistency(a, b)
    assert mean.dim() == 0 and mx.dim() == 0 and mean.is_cuda and mean.dtype == torch.float32
    ref_mean, ref_max = R.inverse_consistency(a.cpu(), b.cpu())
    print(f"inverse_consistency {kind} B={B} {size}: mean {float(mean):.6f} (fp64 {ref_mean:.6f}, dev {abs(float(mean) - ref_mean) / ref_mean:.2e}), "
          f"max {float(mx):.6f} (fp64 {ref_max:.6f}, dev {abs(float(mx) - ref_max) / ref_max:.2e})")
    assert ref_mean > 1e-3 and ref_max >= ref_mean
    assert abs(float(mean) - ref_mean) <= 1e-5 * ref_mean
    assert abs(float(mx) - ref_max) <= 1e-5 * ref_max
    again = ops.inverse_consistency(a, b)
    assert torch.equal(mean, again[0]) and torch.equal(mx, again[1])


def test_inverse_consistency_of_the_identity_and_argument_errors(ops):
    from pulpo_amd._lib import PulpoHipError
    z = torch.zeros(2, 3, 5, 6, 7, device="cuda")
    mean, mx = ops.inverse_consistency(z, z)
    assert float(mean) == 0.0 and float(mx) == 0.0              # a zero field is the identity
    with pytest.raises(PulpoHipError):
        ops.inverse_consistency(z, z[:1])
    with pytest.raises(PulpoHipError):
        ops.inverse_consistency(z.cpu(), z.cpu())


@pytest.mark.parametrize("size", [(16, 16, 16), (24, 20, 28)])
def test_integral_of_negated_velocity_is_the_better_inverse_on_the_device(ops, size):
    """the property of tests/test_host_inverse.py with the device's integrals and the device's residual"""
    fwd, inv = ops.vecint_pair(R.smooth_field(size, 3.0).cuda())
    exact, first_order = float(ops.inverse_consistency(fwd, inv)[0]), float(ops.inverse_consistency(fwd, -fwd)[0])
    print(f"{size}: residual {exact:.4f} with VecInt(-v), {first_order:.4f} with -fwd, ratio {exact / first_order:.2f}")
    assert 0.0 < exact <= 0.5 * first_order


# ================================================================================================ transport_points
@pytest.mark.parametrize("size", [(12, 17, 9), (24, 20)])
def test_transport_points_against_fp64(ops, size):
    from pulpo_amd import eval_metrics
    nd = len(size)
    gen = torch.Generator().manual_seed(13)
    field = torch.randn(3, nd, *size, generator=gen) * 2.0                    # three sample fields at once
    hi = torch.tensor([s - 1.0 for s in size])
    pts = (0.01 + torch.rand(1, 64, nd, generator=gen) * 0.98) * hi          # strictly inside the volume, fractional
    out = ops.transport_points(pts.cuda(), field.cuda())
    assert tuple(out.shape) == (3, 64, nd) and out.dtype == torch.float32
    ref = R.transport_points(pts, field)
    err = float((out.cpu().double() - ref).abs().max())
    print(f"transport_points {size}: max error {err:.2e} voxels")
    assert err <= 1e-5
    assert torch.equal(out, eval_metrics.transport_landmarks(pts.cuda(), field.cuda()))
    # points on the border are inside; a point beyond it raises
    edge = torch.stack([torch.zeros(nd), hi])[None]
    got = ops.transport_points(edge.cuda(), field.cuda())
    assert float((got.cpu().double() - R.transport_points(edge, field)).abs().max()) <= 1e-5
    for bad in (hi + 0.5, -0.25 * torch.ones(nd)):
        with pytest.raises(IndexError):
            ops.transport_points(torch.stack([pts[0, 0], bad])[None].cuda(), field.cuda())


# ================================================================================================ model surface
def _model(df_resolution="level_res"):
    import src.models as models
    import src.network_blocks as nb
    torch.manual_seed(7)
    model = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=8, df_resolution=df_resolution).cuda().eval()
    gen = torch.Generator().manual_seed(8)
    for l in range(2):
        s = 16 >> (l + 1)
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=gen).cuda())
    x, y = torch.rand(1, 1, 16, 16, 16, generator=gen).cuda(), torch.rand(1, 1, 16, 16, 16, generator=gen).cuda()
    return model, nb, x, y


@pytest.mark.parametrize("df_resolution", ["level_res", "full_res"])
@pytest.mark.parametrize("deterministic", [True, False])
def test_predict_bidirectional_against_existing_operators(ops, df_resolution, deterministic):
    model, nb, x, y = _model(df_resolution)
    res = model.predict_bidirectional(x, y, N=1, deterministic=deterministic)
    assert set(res) == {"outputs", "individual_dfs", "final_dfs", "final_dfs_inv", "outputs_inv"}
    with torch.no_grad():
        outputs, ind = model.predict_deterministic(x, y) if deterministic else model.predict(x, y, 1)
        combined, final = model.combine_dfs(ind)
        for l in range(2):
            assert torch.equal(res["individual_dfs"][l], ind[l])
            assert res["final_dfs"][l].shape == final[l].shape and rel_l2(res["final_dfs"][l], final[l]) < 1e-5
            if deterministic:
                assert torch.equal(res["outputs"][l], outputs[l])
            else:
                assert rel_l2(res["outputs"][l], outputs[l]) < 1e-5
            integrated = ops.vecint(-combined[l], 7)
            target = 16 if (l == 0 or df_resolution == "full_res") else integrated.shape[2]
            inv = nb.ResizeTransform(vel_resize=1 / (target / integrated.shape[2]), ndims=3)(integrated)
            assert res["final_dfs_inv"][l].shape == final[l].shape
            assert float(inv.abs().max()) > 0 and rel_l2(res["final_dfs_inv"][l], inv) < 1e-5
            assert torch.equal(res["outputs_inv"][l], model.autoencoder.decoders[l].spatial_transform(res["final_dfs_inv"][l], y))
            assert res["outputs_inv"][l].shape == res["outputs"][l].shape
        c2, f2, i2 = model.combine_dfs_bidirectional(ind)
        assert all(torch.equal(c2[l], combined[l]) and torch.equal(f2[l], res["final_dfs"][l]) and torch.equal(i2[l], res["final_dfs_inv"][l])
                   for l in range(2))


# ================================================================================================ evaluation
def test_performance_inverse_rows(ops):
    from pulpo_amd import eval_metrics
    from pulpo_amd.evaluation import INVERSE_METRICS, METRICS, performance
    model, nb, x, y = _model()
    gen = torch.Generator().manual_seed(17)
    lm_x = (2.0 + 11.0 * torch.rand(1, 6, 3, generator=gen)).cuda()             # fractional positions inside the volume
    lm_y = (lm_x + 0.5 * torch.randn(1, 6, 3, generator=gen).cuda()).clamp(0, 15)
    seg_x = torch.randint(0, 4, (1, 1, 16, 16, 16), generator=gen).to(torch.uint8).cuda()
    seg_y = torch.randint(0, 4, (1, 1, 16, 16, 16), generator=gen).to(torch.uint8).cuda()
    kw = dict(seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=4)
    plain = performance(model, x, y, **kw)
    both = performance(model, x, y, inverse=True, **kw)
    assert set(plain) == set(METRICS) and set(both) == set(METRICS) | set(INVERSE_METRICS)
    assert set(INVERSE_METRICS) == {"InvCons", "InvConsMax", "LM_MAE_inv", "LM_Euclid_inv"}
    for m in METRICS:
        for l in range(2):
            assert torch.equal(plain[m][l], both[m][l]), (m, l)
    for m in INVERSE_METRICS:
        assert all(both[m][l].is_cuda and both[m][l].dim() == 0 for l in range(2))
    res = model.predict_bidirectional(x, y, deterministic=True)
    for l in range(2):
        mean, mx = ops.inverse_consistency(res["final_dfs"][l], res["final_dfs_inv"][l])
        assert torch.equal(both["InvCons"][l], mean) and torch.equal(both["InvConsMax"][l], mx)
        assert 0.0 < float(mean) <= float(mx)
    moved = eval_metrics.transport_landmarks(lm_x, res["final_dfs_inv"][0])
    assert torch.equal(both["LM_Euclid_inv"][0], eval_metrics.lm_euclid(moved, lm_y))
    assert torch.equal(both["LM_MAE_inv"][0], eval_metrics.lm_mae(moved, lm_y))
    assert float(both["LM_Euclid_inv"][0]) > 0 and float(both["LM_MAE_inv"][1]) == 0.0 and float(both["LM_Euclid_inv"][1]) == 0.0
    # without landmarks only the consistency rows are added
    assert set(performance(model, x, y, inverse=True)) == {"RMSE", "JDetStd", "JDetLeq0", "InvCons", "InvConsMax"}
