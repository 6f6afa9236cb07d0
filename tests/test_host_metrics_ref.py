"""tests/metrics_ref.py against what the reference project computed: the goldens tests/golden/metrics.npz and evalmetrics.npz, evaluated in
float64 at the tolerances the golden tests of the HIP kernels use (test_gpu_ops.py), against oracle/pulpo_oracle.py where the reference
restates an oracle expression on the argument's device, and - Adam - against torch.optim.Adam.  CPU only."""
import numpy as np
import pytest
import torch

import metrics_ref as M
from oracle import pulpo_oracle as O

T = lambda a: torch.from_numpy(np.asarray(a).copy()).double()


def close(got, want, rtol=0.0, atol=0.0):
    np.testing.assert_allclose(got.detach().numpy() if isinstance(got, torch.Tensor) else got, want, rtol=rtol, atol=atol)


def test_l2_and_dice_reproduce_the_goldens(golden):
    g = golden("metrics")
    a = T(g["l2_in"]).requires_grad_(True)
    l = M.l2_loss(a, T(g["l2_tgt"]))
    close(l, g["l2_loss"], rtol=1e-5)
    close(torch.autograd.grad(l * 0.7, [a])[0], 0.7 * g["l2_gin"], atol=1e-7, rtol=1e-5)
    a = T(g["dice_in"]).requires_grad_(True)
    for f in (1, 4):
        l = M.soft_dice(a, T(g["dice_tgt"]), f)
        close(l, g[f"dice{f}_loss"], rtol=1e-5)
        close(torch.autograd.grad(l, [a])[0], g[f"dice{f}_gin"], atol=1e-6, rtol=1e-4)


def test_jacobian_det_and_std_reproduce_the_goldens(golden):
    g = golden("metrics")
    d = T(g["jdet_df"]).requires_grad_(True)
    for norm in (1, 0):
        close(M.jacobian_det(d, bool(norm)), g[f"jdet_norm{norm}"], atol=1e-5, rtol=1e-5)
        s = M.jdet_std(d, 0.3, bool(norm))
        close(s, g[f"jstd_norm{norm}"], rtol=1e-4)
        close(torch.autograd.grad(s, [d])[0], g[f"jstd_gd_norm{norm}"], atol=1e-6, rtol=1e-3)


def test_kl_nondiagonal_reproduces_the_golden(golden):
    g = golden("metrics")
    mu, sg = T(g["kln_mu"]).requires_grad_(True), T(g["kln_sigma"]).requires_grad_(True)
    close(M.degree((5, 6, 7), torch.float64, "cpu")[None, None], g["kln_D"])
    l = M.kl_nondiagonal(mu, sg, 20.0)
    close(l, g["kln_loss"], rtol=1e-5)
    gm, gs = torch.autograd.grad(l, [mu, sg])
    close(gm, g["kln_gmu"], atol=1e-5, rtol=1e-4)
    close(gs, g["kln_gsigma"], atol=1e-4, rtol=1e-4)


def test_evaluation_scalars_reproduce_the_golden(golden):
    g = golden("evalmetrics")
    close(M.rmse(T(g["rmse_a"]), T(g["rmse_b"])), g["rmse"], rtol=1e-6)
    close(M.dsc(T(g["dsc_in"]), T(g["dsc_tgt"])), g["dsc"], rtol=1e-6)
    jd = M.jacobian_det(T(g["leq_df"]))
    close(jd, g["leq_jdet"], atol=1e-5, rtol=1e-5)
    # a determinant within rounding of 0 may fall on either side of it in float64 (test_eval_metrics_golden's allowance)
    near = float((np.abs(g["leq_jdet"]) < 1e-4).sum()) * 100.0 / g["leq_jdet"].size
    assert abs(M.percent_leq0(jd) - float(g["leq_pct"])) <= near + 1e-4
    close(np.float32(M.percent_leq0(T(g["leq_jdet"]))), g["leq_pct"], rtol=1e-6)
    close(M.warp_landmarks(T(g["lm"]), T(g["lm_df"])), g["lm_out"], atol=1e-6)          # (the fixture is the fp32 subtraction)


def test_landmark_reference_wraps_raises_and_takes_slices():
    gen = torch.Generator().manual_seed(1)
    df = torch.randn(2, 3, 4, 5, 6, generator=gen, dtype=torch.float64)
    lm = torch.tensor([[[-1.0, -5.0, 5.0], [3.9, 0.0, -6.0]]], dtype=torch.float64)
    out = M.warp_landmarks(lm, df)
    assert torch.equal(out, O.warp_landmarks(lm, df))
    assert torch.equal(out[1, 0], torch.tensor([-1.0, -5.0, 5.0], dtype=torch.float64) - df[1, :, 3, 0, 5])
    assert torch.equal(out[0, 1], torch.tensor([3.0, 0.0, -6.0], dtype=torch.float64) - df[0, :, 3, 0, 0])
    with pytest.raises(IndexError):
        M.warp_landmarks(torch.tensor([[[0.0, 5.0, 0.0]]]), df)
    d2 = torch.randn(3, 2, 7, 9, generator=gen, dtype=torch.float64)
    l2 = torch.tensor([[[6.0, -9.0], [0.0, 8.0]]])
    assert torch.equal(M.warp_landmarks(l2, d2)[2, 0], torch.tensor([6.0, -9.0], dtype=torch.float64) - d2[2, :, 6, 0])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_device_generic_forms_are_the_oracle_expressions(dtype):
    """the determinant and KL_nondiagonal of metrics_ref build their index tensors on the argument's device: on the CPU they are the oracle's
    values bit for bit, in either dtype; the 2-D forms against the oracle's separate statements"""
    gen = torch.Generator().manual_seed(3)
    df = torch.randn(2, 3, 5, 7, 6, generator=gen).to(dtype) * 2
    for norm in (True, False):
        assert torch.equal(M.jacobian_det(df, norm), O.jacobian_det(df, norm))
        assert torch.equal(M.jdet_std(df, 0.3, norm), O.jdet_std(df, 0.3, norm))
    mu, sg = torch.randn(2, 3, 4, 5, 6, generator=gen).to(dtype), (torch.rand(2, 3, 4, 5, 6, generator=gen) + 0.1).to(dtype)
    torch.testing.assert_close(M.kl_nondiagonal(mu, sg, 20.0), O.kl_nondiagonal(mu, sg, 20.0), rtol=4 * torch.finfo(dtype).eps, atol=0.0)
    mu2, sg2 = mu[:, :2, 0], sg[:, :2, 0]
    torch.testing.assert_close(M.kl_nondiagonal(mu2, sg2, 20.0), O.kl_nondiagonal(mu2, sg2, 20.0), rtol=4 * torch.finfo(dtype).eps, atol=0.0)
    # 2-D determinant from first principles: the 2 x 2 Jacobian of the scaled, flipped field by central differences at an interior pixel
    d2 = torch.randn(1, 2, 6, 8, generator=gen).to(dtype)
    j = M.jacobian_det_2d(d2, True)
    assert j.shape == (1, 6, 8)
    u = torch.stack([d2[0, 1] * (2 / 8) * (6 - 2) / 2, d2[0, 0] * (2 / 6) * (8 - 2) / 2])       # flipped channel c, scaled by (S_c - 2) / 2
    y, x = 3, 4
    J = [[0.5 * (u[c, y + 1, x] - u[c, y - 1, x]) + (c == 0) for c in range(2)], [0.5 * (u[c, y, x + 1] - u[c, y, x - 1]) + (c == 1) for c in range(2)]]
    torch.testing.assert_close(j[0, y, x], J[0][0] * J[1][1] - J[1][0] * J[0][1], rtol=1e-5, atol=1e-6)


def test_mc_std_map_and_percent():
    gen = torch.Generator().manual_seed(5)
    stack = torch.randn(6, 3, 4, 5, 6, generator=gen, dtype=torch.float64)
    want = stack.std(dim=0, unbiased=True).mean(dim=0)
    assert torch.equal(M.mc_std_map(stack), want)
    x = torch.tensor([0.0, -0.0, 1.0, -2.0, 3.0])
    assert M.percent_leq0(x) == 60.0


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_adam_reference_is_torch_adam(gscale):
    """three steps from zero moments against torch.optim.Adam in float64 on gradients already multiplied by gscale"""
    gen = torch.Generator().manual_seed(2)
    p = torch.randn(37, generator=gen, dtype=torch.float64)
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=1e-3)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        g = torch.randn(37, generator=gen, dtype=torch.float64)
        g[::5] = 0.0
        tp.grad = g * gscale
        opt.step()
        p, m, v = M.adam_ref(p, g, m, v, 1e-3, step, gscale=gscale)
        st = opt.state[tp]
        torch.testing.assert_close(p, tp.detach(), rtol=1e-14, atol=1e-15)
        torch.testing.assert_close(m, st["exp_avg"], rtol=1e-14, atol=0.0)
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-14, atol=0.0)
