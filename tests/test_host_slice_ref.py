"""tests/slice_ref.py (the 2-D mode's operators written with torch's native 2-D operators) against the arrays that the REAL reference
produced for tests/golden/ops2d.npz (make_golden.py 2d), in float64 on the CPU and at the tolerances tests/test_gpu_2d.py holds the HIP
kernels to on the same arrays.  This pins the definitions tests/test_gpu_slices.py compares the kernels with."""
import numpy as np
import torch

import slice_ref as S


def T64(a):
    return torch.from_numpy(np.asarray(a)).double()


def close(a, b, atol=1e-5, rtol=1e-5):
    np.testing.assert_allclose(a.detach().numpy(), np.asarray(b, dtype=np.float64), atol=atol, rtol=rtol)


def rel_l2(a, b):
    b = T64(b)
    return float((a.detach() - b).norm() / (b.norm() + 1e-30))


def test_warp_and_vecint_reproduce_the_reference(golden):
    g = golden("ops2d")
    df, img, up = T64(g["w_df"]).requires_grad_(True), T64(g["w_img"]).requires_grad_(True), T64(g["w_up"])
    out = S.warp_ref(df, img)
    close(out, g["w_out"], atol=2e-6)
    gd, gi = torch.autograd.grad((out * up).sum(), [df, img])
    close(gd, g["w_gdf"], atol=1e-5)
    close(gi, g["w_gimg"], atol=1e-5)
    H, W = df.shape[2:]
    close(S.warp_ref(torch.zeros(1, 2, H, W, dtype=torch.float64), img[:1].detach()), g["w_zero"], atol=2e-6)      # a zero field is not the identity
    close(S.warp_ref(df[:1].detach(), T64(g["w_big"])), g["w_big_out"], atol=2e-6)                                  # image larger than the grid
    v = T64(g["vi_in"]).requires_grad_(True)
    vo = S.vecint_ref(v, 7)
    close(vo, g["vi_out"], atol=1e-5)
    gv, = torch.autograd.grad((vo * up[:1, :2]).sum(), [v])
    assert rel_l2(gv, g["vi_g"]) < 1e-4


def test_warp_coords_are_the_positions_grid_sample_reads(golden):
    """warp_coords (the cell-boundary test of the GPU comparison rests on it): bilinear interpolation written out at those coordinates, clamped
    to the image, gives warp_ref's output"""
    g = golden("ops2d")
    for df, img in ((T64(g["w_df"]), T64(g["w_img"])), (T64(g["w_df"])[:1], T64(g["w_big"]))):
        Hi, Wi = img.shape[2:]
        c = S.warp_coords(df, (Hi, Wi))
        cy, cx = c[0].clamp(0, Hi - 1), c[1].clamp(0, Wi - 1)
        y0, x0 = cy.floor().long().clamp(max=Hi - 2), cx.floor().long().clamp(max=Wi - 2)
        fy, fx = (cy - y0).unsqueeze(1), (cx - x0).unsqueeze(1)
        b = torch.arange(img.shape[0]).reshape(-1, 1, 1)
        pick = lambda yy, xx: img[b, :, yy, xx].permute(0, 3, 1, 2)
        want = ((1 - fy) * ((1 - fx) * pick(y0, x0) + fx * pick(y0, x0 + 1)) + fy * ((1 - fx) * pick(y0 + 1, x0) + fx * pick(y0 + 1, x0 + 1)))
        close(want, S.warp_ref(df, img).numpy(), atol=1e-12)


def test_pool_and_resize_reproduce_the_reference(golden):
    g = golden("ops2d")
    x = T64(g["r_x"])
    close(S.avgpool2_ref(x), g["r_pool"], atol=1e-6)
    close(S.resize_ref(x, size=[18, 24]), g["r_up"], atol=1e-6)
    close(S.resize_ref(x, size=[5, 7]), g["r_down"], atol=1e-6)
    f = T64(g["r_f"])
    close(S.resize_ref(2.0 * f, scale_factor=2.0), g["r_rt_up"], atol=1e-5)            # ResizeTransform(0.5): multiply, then resize
    close(0.5 * S.resize_ref(f, scale_factor=0.5), g["r_rt_down"], atol=1e-5)          # ResizeTransform(2): resize, then multiply


def test_conv_unit_and_heads_reproduce_the_reference(golden):
    g = golden("ops2d")
    sd = {k[7:]: T64(v) for k, v in g.items() if k.startswith("cu_sd0.")}
    x, up = T64(g["cu_x"]), T64(g["cu_up"])
    r = S.conv_unit_train_ref(x, sd["_op.0.weight"], sd["_op.0.bias"], sd["_op.1.weight"], sd["_op.1.bias"], sd["_op.1.running_mean"],
                              sd["_op.1.running_var"], up)
    close(r["out"], g["cu_out"], atol=2e-5)
    assert rel_l2(r["dx"], g["cu_gx"]) < 1e-4
    assert rel_l2(r["dw"], g["cu_g._op.0.weight"]) < 1e-4
    assert rel_l2(r["dgamma"], g["cu_g._op.1.weight"]) < 1e-4 and rel_l2(r["dbeta"], g["cu_g._op.1.bias"]) < 1e-4
    assert float(r["db"].abs().max()) <= 1e-3 * max(1e-3, float(np.abs(g["cu_g._op.0.weight"]).max()))            # true gradient 0 (BatchNorm follows)
    close(r["running_mean"], g["cu_sd1._op.1.running_mean"], atol=1e-6)
    close(r["running_var"], g["cu_sd1._op.1.running_var"], atol=1e-6)
    close(S.conv_unit_eval_ref(x, sd["_op.0.weight"], sd["_op.0.bias"], sd["_op.1.weight"], sd["_op.1.bias"], T64(g["cu_sd1._op.1.running_mean"]),
                               T64(g["cu_sd1._op.1.running_var"])), g["cu_out_eval"], atol=2e-5)
    # the unit's backward formulas against autograd through the same forward
    xg = x.clone().requires_grad_(True)
    ps = [sd[k].clone().requires_grad_(True) for k in ("_op.0.weight", "_op.0.bias", "_op.1.weight", "_op.1.bias")]
    z = S.bn_train_ref(S.conv2_ref(xg, ps[0], ps[1]), ps[2], ps[3])["z"]
    ag = torch.autograd.grad((z * up).sum(), [xg] + ps)
    for a, b in zip(ag, (r["dx"], r["dw"], r["db"], r["dgamma"], r["dbeta"])):
        close(a, b.numpy(), atol=1e-10)
    ms = {k[6:]: T64(v) for k, v in g.items() if k.startswith("ms_sd.")}
    mu, sigma, z = S.mu_sigma_ref(x, ms["_conv_mu.weight"], ms["_conv_mu.bias"], ms["_conv_sigma.0.weight"], ms["_conv_sigma.0.bias"], None)
    close(mu, g["ms_mu"], atol=1e-5)
    close(sigma, g["ms_sigma"], atol=1e-5)
    assert torch.equal(z, mu) and tuple(mu.shape) == (2, 2, 12, 10)


def test_float32_evaluation_runs_and_stays_near_float64(golden):
    """every function also runs in float32 (the evaluation the GPU comparison's bounds are measured from)"""
    g = golden("ops2d")
    x, w = torch.from_numpy(g["cu_x"]), torch.from_numpy(g["cu_sd0._op.0.weight"])
    assert S.conv2_ref(x, w).dtype == torch.float32
    close(S.conv2_ref(x, w).double(), S.conv2_ref(x.double(), w.double()).numpy(), atol=1e-5)
    dy = torch.from_numpy(g["cu_up"])
    for a, b in zip(S.conv2_grads_ref(x, w, dy), S.conv2_grads_ref(x.double(), w.double(), dy.double())):
        assert a.dtype == torch.float32
        close(a.double(), b.numpy(), atol=1e-4)
    assert float(S.conv2_mag(x.double(), w.double()).min()) > 0
