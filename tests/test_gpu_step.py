"""GPU parity of the whole training step (DownPath -> Autoencoder -> losses -> backward) through the drop-in API
(`src.models.PULPo`), against
  (1) the full-step golden vectors generated from the real reference (state dict, inputs, noise -> all 8 output
      dictionaries, the loss terms and every parameter gradient), and
  (2) the CPU oracle at a BASELINE-like channel width (n0 = 32), plus size-independent properties at larger sizes.
Stated fp32 tolerances: fields / warped atol 1e-4 (scaled by the tensor's magnitude), loss terms rtol 1e-4,
parameter gradients relative-L2 <= 1e-3 on the golden cases (<= 5e-3 where LeakyReLU slope flips against fp64 occur, see
test_step_vs_oracle_at_baseline_width); biases that feed a BatchNorm have a true gradient of 0 and are compared on the
scale of their layer's weight gradient (SURVEY.md §7 'hard parts')."""
import numpy as np
import pytest
import torch

from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FB = list(O.FEEDBACK_DEFAULT)
OUT = O.OUT_NAMES



def _free_port() -> str:
    """a TCP port that is free right now (the rendezvous of the multi-process tests)"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])

@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb


def rel_l2(a, b):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _record_unit(store, name, out):
    """forward hook of a ConvUnit: its output - or nothing where the un-pooled activation is never written (round 5: the last unit of a DownPath
    level above the first latent level hands on only AvgPool(z): ConvUnit.forward then returns (None, pooled))"""
    if isinstance(out, tuple):
        out = out[0]
    if out is not None:
        if out.dim() == 6:                           # (round 5: the activation between two units of a ConvSequence may travel channel-blocked)
            from pulpo_amd import ops
            out = ops.blocked_to_cl(out)
        store[name] = out.detach()


def build_from_golden(models, nb, g, key="sd0.", case=""):
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0, df_resolution="full_res" if "fullres" in case else "level_res",
                         cp_depth=0 if "_cp0_" in case else 3)
    sd = model.state_dict()
    loaded = 0
    for k, v in g.items():
        if k.startswith(key):
            assert k[len(key):] in sd, k
            sd[k[len(key):]] = T(v.copy())
            loaded += 1
    missing, unexpected = model.load_state_dict(sd, strict=True), None
    assert loaded > 50
    model = model.cuda()
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(T(g[f"eps.{l}"]).cuda())
    return model, (Tl, L, n0, B, size)


def check_outputs(outs, g, prefix, atol=1e-4):
    for name, d in zip(OUT, outs):
        for l, v in d.items():
            ref = g[f"{prefix}.{name}.{l}"]
            assert tuple(v.shape) == ref.shape, (name, l, v.shape, ref.shape)
            err = np.abs(v.detach().cpu().numpy() - ref).max()
            assert err <= atol * max(1.0, np.abs(ref).max()), (name, l, err)


# (step_cp0_*: cp_depth = 0 - the latent sample IS the velocity field, network_blocks.py:76-77 - through the whole step)
STEP_CASES = ["step_T3L2_n4_16", "step_T4L3_n2_16x24x16", "step_fullres_T3L2_n2_16", "step_T3L2_n8_32", "step_cp0_T3L2_n2_16"]


# (case, forward / data-gradient kernel): None = the library's per-shape default (the Winograd kernels - F(2x2x2,3x3x3) on whole 4x8x8 tiles,
# F(2x2,3x3) elsewhere - where eligible, which on these fixtures is the 32^3 case only); that case is also pinned with the direct kernels forced
STEP_ALGO_CASES = [(c, None) for c in STEP_CASES] + [("step_T3L2_n8_32", "direct"), ("step_T3L2_n8_32", "deterministic"), ("step_fullres_T3L2_n2_16", "deterministic")]

# the 32^3 golden step in DETERMINISTIC mode: the GPU's gradients are then one fixed set of numbers (bit-identical run to run), so the bound
# against the reference's fp32 gradients is set on what that evaluation measures (4.24e-3; the atomic mode sits within 1e-5 of it, so the default
# kernel selection is held to the same bound).  It cannot reach SURVEY 8(c)'s 1e-3: the reference's own fp32 gradients sit up to 2e-3 from an fp64
# evaluation on this case (windowed-variance cancellation at 9^3 NCC windows), and a LeakyReLU slope that differs moves a gradient by more.
GRAD_BOUND_32_DETERMINISTIC = 5e-3          # measured 4.24e-3 (0 slope flips), a fixed number in this mode


@pytest.mark.parametrize("case,algo", STEP_ALGO_CASES)
def test_training_step_matches_reference_golden(api, golden, case, algo):
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    if case == "step_T3L2_n8_32":           # the shipped default really is the (y, x) Winograd kernel on this case's full-resolution layers
        assert lib.query("pulpo_conv3d_k3_algo", 1, 32, 32, 32, 8, 8) == 2
    det = algo == "deterministic"
    ops.CONV_ALGO = None if det else algo
    ops.set_deterministic(det or ops.DETERMINISTIC)
    try:
        _training_step_vs_golden(api, golden, case, det)
    finally:
        ops.CONV_ALGO = None
        ops.set_deterministic(__import__("os").environ.get("PULPO_DETERMINISTIC", "0") == "1")


def _training_step_vs_golden(api, golden, case, det=False):
    models, nb = api
    g = golden(case)
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, g, case=case)
    model.train()
    x, y = T(g["x"]).cuda(), T(g["y"]).cuda()
    gpu_units = {}
    for name, mod in model.named_modules():
        if isinstance(mod, nb.ConvUnit):
            mod.register_forward_hook(lambda m, i, o, name=name: _record_unit(gpu_units, name, o))
    outs, priors, (total, kl, rec, reg), levels = model._forward_and_losses(x, y)
    check_outputs(outs, g, "train")
    # LeakyReLU slope flips against the reference's own fp32 evaluation (the oracle reproduces the reference to 1e-5, so its
    # activations stand in for the reference's): one flip moves every upstream gradient by ~1e-3 (see the n0 = 32 test below), so the
    # gradient bound is 1e-3 without flips and 2e-2 with (measured up to 8.5e-3 on the 32^3 case, for the direct and both Winograd
    # kernels alike - scripts/golden32_check.py)
    ref_units = {}
    orig_unit = O.conv_unit

    def recording_unit(h, sd_, prefix, training):
        out = orig_unit(h, sd_, prefix, training)
        ref_units[prefix] = out.detach()
        return out

    O.conv_unit = recording_unit
    try:
        sd0 = {k[4:]: T(v.copy()) for k, v in g.items() if k.startswith("sd0.")}
        cfg = O.Cfg(Tl, L, size, n0=n0, df_resolution="full_res" if "fullres" in case else "level_res", cp_depth=0 if "_cp0_" in case else 3)
        O.forward(sd0, cfg, T(g["x"]), T(g["y"]), {l: T(g[f"eps.{l}"]) for l in range(L)}, training=True)
    finally:
        O.conv_unit = orig_unit
    # (every unit but the ones whose un-pooled output is never written: one per DownPath level above the first latent level)
    assert set(gpu_units) <= set(ref_units) and len(ref_units) - len(gpu_units) <= Tl - L, (sorted(set(ref_units) - set(gpu_units)))
    flips = sum(int(((gpu_units[k].cpu() > 0) != (ref_units[k] > 0)).sum()) for k in gpu_units)
    assert flips <= 1e-5 * sum(v.numel() for v in ref_units.values()), flips
    grad_bound = 1e-3 if flips == 0 else 2e-2
    g64 = None
    if case == "step_T3L2_n8_32":
        # On this case (smooth images, 9^3 NCC windows at 32^3) the reference's own fp32 gradients sit 5e-4 (median) to 2e-3 from an fp64
        # evaluation of the same arithmetic - the cancellation noise of the windowed variances - and so do these, in a different direction
        # (scripts/golden32_check.py), varying from run to run with the order of the atomic accumulations.  The criterion is therefore
        # statistical: median distance from fp64 <= 4x the reference's (+2e-4), maximum <= 6x the reference's maximum (+1e-3), and every
        # parameter within 1e-2 of the reference.
        sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        _, g64, _ = O.train_step(O.clone_sd(sd64, requires_grad=True), cfg, T(g["x"]).double(), T(g["y"]).double(),
                                 {l: T(g[f"eps.{l}"]).double() for l in range(L)})
        # (default kernel selection: 4.24e-3 measured, the same to 1e-5 with and without the float atomics; the direct kernels' single 216-term
        #  fmaf chain per output sits further from the reference's blocked sums: 8.5e-3)
        from pulpo_amd import ops as _ops
        grad_bound = GRAD_BOUND_32_DETERMINISTIC if (det or _ops.CONV_ALGO is None) else 1e-2
    for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
        np.testing.assert_allclose(float(val), float(g["train." + key]), rtol=1e-4)
    for nm, d in zip(("kl_l", "rec_l", "reg_l"), levels):
        for l, v in d.items():
            np.testing.assert_allclose(float(v), float(g[f"train.{nm}.{l}"]), rtol=1e-4, atol=1e-6)
    total.backward()
    named = dict(model.named_parameters())
    n_checked = 0
    worst = 0.0
    vs64 = []
    for k, p in named.items():
        if "grad." + k in g:
            ref = g["grad." + k]
            assert p.grad is not None, k
            if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
                # conv bias in front of a BatchNorm: the true gradient is zero, the reference holds rounding noise
                wref = np.abs(g["grad." + k[:-4] + "weight"]).max()
                assert np.abs(p.grad.cpu().numpy()).max() <= 1e-3 * max(wref, 1e-3), k
                continue
            e = rel_l2(p.grad, ref)
            worst = max(worst, e)
            assert e < grad_bound, (k, e, flips)
            if g64 is not None:
                vs64.append((rel_l2(p.grad, g64[k]), rel_l2(T(ref), g64[k])))
            n_checked += 1
        else:
            assert "nograd." + k in g, k
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k     # encoders[L-1].sample_merge_block is never used
    assert n_checked > 40
    print(f"{case} (deterministic {det}): {flips} slope flips, largest gradient distance from the reference {worst:.3e} (bound {grad_bound:g})")
    if vs64:        # noise-dominated quantities (they move run to run with the atomic order): compare the distributions, not parameter by parameter
        e_gpu, e_ref = np.array(vs64).T
        # (measured medians: reference 5.6e-4, Winograd kernels 5.4e-4, direct kernels - one sequential 216-term fmaf chain per output
        #  where ATen and the Winograd form sum in blocks - 1.7e-3)
        assert np.median(e_gpu) <= 4.0 * np.median(e_ref) + 2e-4, (np.median(e_gpu), np.median(e_ref))
        assert e_gpu.max() <= 6.0 * e_ref.max() + 1e-3, (e_gpu.max(), e_ref.max())
    # BatchNorm running statistics after exactly one training forward
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("sd1."):
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), v, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("res", ["full_res", "level_res"])
def test_dice_recon_with_segmentations_matches_reference_golden(api, golden, res):
    """--recon_loss ncc dice with --segs: the segmentation maps are warped per level as reference models.py:370-388 does - with
    df_resolution == "full_res" EVERY level warps the full-resolution map (models.py:375-376), otherwise the avg-pool chain - and enter
    HierarchicalReconstructionLoss (losses.py:319-321).  Golden = the reference's own modules (tests/golden/make_golden.py dice)."""
    models, nb = api
    g = golden(f"step_dice_{res}_T3L2_n2_16")
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0, df_resolution=res, recon_loss=["ncc", "dice"], segs=True)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("sd0."):
            assert k[4:] in sd, k
            sd[k[4:]] = T(v.copy())
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(T(g[f"eps.{l}"]).cuda())
    x, y, seg_x, seg_y = (T(g[k]).cuda() for k in ("x", "y", "seg_x", "seg_y"))
    outs, _, (total, kl, rec, reg), (_, rec_l, _) = model._forward_and_losses(x, y, seg_x, seg_y)
    segs = model.transform_segmentation(outs[6], seg_x)
    for l, v in segs.items():
        ref = g[f"train.y_hat_seg.{l}"]
        assert tuple(v.shape) == ref.shape, (l, v.shape, ref.shape)
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref, atol=1e-4)
    for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
        np.testing.assert_allclose(float(val), float(g["train." + key]), rtol=1e-4)
    for l, v in rec_l.items():
        np.testing.assert_allclose(float(v), float(g[f"train.rec_l.{l}"]), rtol=1e-4, atol=1e-6)
    total.backward()
    n = 0
    for k, p in model.named_parameters():
        if "grad." + k not in g:
            continue
        ref = g["grad." + k]
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            wref = np.abs(g["grad." + k[:-4] + "weight"]).max()
            assert np.abs(p.grad.cpu().numpy()).max() <= 1e-3 * max(wref, 1e-3), k
            continue
        assert rel_l2(p.grad, ref) < 2e-2, (k, rel_l2(p.grad, ref))      # (flip-aware bound of the golden step test)
        n += 1
    assert n > 40


@pytest.mark.parametrize("res", ["level_res", "full_res"])
def test_pulpo_class_api_matches_the_reference_class(api, golden, res):
    """The drop-in class against what the reference's OWN `src.models.PULPo` returns (tests/golden/models_api_*.npz: generated by
    `make_golden.py models` from /root/reference/src/models.py itself): PULPo.__init__ tables, training_step incl. what it logs,
    predict_output_samples(N=2), predict(N=2), predict_deterministic, forward, combine_dfs, transform_segmentation
    (models.py:104-123, 134-196, 312-388), every parameter gradient of the step, configure_optimizers."""
    models, nb = api
    g = golden(f"models_api_{res}_T3L2_n2_16")
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0, df_resolution=res, recon_loss=["ncc", "dice"], segs=True)
    for l in range(L):
        assert model.hierarchical_recon_loss.window_size[l] == int(g["hparams.window_size"][l])
        assert model.hierarchical_kl_loss.weight_dict[l] == float(g["hparams.kl_w"][l])
        assert model.hierarchical_recon_loss.weight_dict[l] == float(g["hparams.rec_w"][l])
        assert model.hierarchical_regularization.weight_dict[l] == float(g["hparams.reg_w"][l])
    opt = model.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == float(g["optimizer.lr"]) and tuple(opt.param_groups[0]["betas"]) == tuple(g["optimizer.betas"])
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("sd0."):
            assert k[4:] in sd, k
            sd[k[4:]] = T(v.copy())
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    eps = {l: T(g[f"eps.{l}"]).cuda() for l in range(L)}

    def set_eps(nb_):
        for l in range(L):
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l][:nb_].contiguous())

    x, y, seg_x, seg_y = (T(g[k]).cuda() for k in ("x", "y", "seg_x", "seg_y"))
    x1, y1 = x[:1].contiguous(), y[:1].contiguous()
    dev = lambda t: t.detach().cpu().numpy()
    model.eval()
    with torch.no_grad():
        set_eps(2)
        o_s, d_s = model.predict_output_samples(x1, y1, N=2)
        avg_out, avg_dfs = model.predict(x1, y1, N=2)
        comb, fin = model.combine_dfs(avg_dfs)
        tseg = model.transform_segmentation(fin, seg_x[:1].contiguous())
        for l in range(L):
            for got, key in ((o_s[l], "samples.outputs"), (d_s[l], "samples.individual_dfs"), (avg_out[l], "predict.outputs"),
                             (avg_dfs[l], "predict.avg_dfs"), (comb[l], "combine.combined"), (fin[l], "combine.final"),
                             (tseg[l], "transform_segmentation")):
                ref = g[f"{key}.{l}"]
                assert tuple(got.shape) == ref.shape, (key, l, got.shape, ref.shape)
                assert np.abs(dev(got) - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (key, l)
        set_eps(1)
        det_out, det_dfs = model.predict_deterministic(x1, y1)
        for l in range(L):
            np.testing.assert_allclose(dev(det_out[l]), g[f"deterministic.outputs.{l}"], atol=1e-4)
            np.testing.assert_allclose(dev(det_dfs[l]), g[f"deterministic.individual_dfs.{l}"], atol=1e-4)
        set_eps(2)
        np.testing.assert_allclose(dev(model(x, y)), g["forward"], atol=1e-4)
    model.train()
    model.logger = object()                    # somebody reads the per-level log entries: _log_levels computes them
    total = model.training_step((x, y, seg_x, seg_y, None, None, None, None), 0)
    np.testing.assert_allclose(float(total), float(g["train.total"]), rtol=1e-4)
    for k in ("kl_loss", "reconstruction_loss", "regularization_loss", "total_loss"):
        np.testing.assert_allclose(float(model.logged["train/" + k]), float(g["train.logged." + k]), rtol=1e-4)
    for l in range(L):
        for k in ("kl loss level", "recon loss level", "regularization loss level"):
            np.testing.assert_allclose(float(model.logged[f"train_levels/{k} {l}"]), float(g[f"train.logged.{k.replace(' ', '_')}.{l}"]), rtol=1e-4, atol=1e-6)
    total.backward()
    n = 0
    for k, p in model.named_parameters():
        if "grad." + k not in g:
            continue
        ref = g["grad." + k]
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            wref = np.abs(g["grad." + k[:-4] + "weight"]).max()
            assert np.abs(p.grad.cpu().numpy()).max() <= 1e-3 * max(wref, 1e-3), k
            continue
        assert rel_l2(p.grad, ref) < 2e-2, (k, rel_l2(p.grad, ref))      # (flip-aware bound of the golden step test)
        n += 1
    assert n > 40


@pytest.mark.parametrize("case", STEP_CASES)
def test_eval_deterministic_and_inference_api(api, golden, case):
    models, nb = api
    g = golden(case)
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, g, case=case)
    sd = model.state_dict()
    for k, v in g.items():                     # eval goldens were taken after one training forward
        if k.startswith("sd1."):
            sd[k[4:]] = T(v.copy())
    model.load_state_dict(sd)
    model.eval()
    x, y = T(g["x"]).cuda(), T(g["y"]).cuda()
    with torch.no_grad():
        outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y)
        check_outputs(outs, g, "eval")
        for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
            np.testing.assert_allclose(float(val), float(g["eval." + key]), rtol=1e-4)
        det_out, det_ind = model.predict_deterministic(x, y)
        for l in det_out:
            np.testing.assert_allclose(det_out[l].cpu().numpy(), g[f"det.transformed.{l}"], atol=1e-4)
            np.testing.assert_allclose(det_ind[l].cpu().numpy(), g[f"det.individual_dfs.{l}"], atol=1e-4)
        comb, fin = model.combine_dfs(outs[4])
        for l in comb:
            np.testing.assert_allclose(comb[l].cpu().numpy(), g[f"eval.combined_dfs.{l}"], atol=1e-4)
            np.testing.assert_allclose(fin[l].cpu().numpy(), g[f"eval.final_dfs.{l}"], atol=1e-4)
        np.testing.assert_allclose(model(x, y).cpu().numpy(), g["eval.transformed.0"], atol=1e-4)
        # predict(): N copies on the batch axis with the SAME injected noise -> the averaged fields equal the single
        # ones; every level warps the full-resolution image (grid smaller than the image for l >= 1)
        for l in range(L):
            e = model.autoencoder.encoders[l].sampler.fixed_eps
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(e.repeat(2, 1, 1, 1, 1))
        o_s, d_s = model.predict_output_samples(x, y, N=2)
        for l in o_s:
            assert tuple(o_s[l].shape[:3]) == (B, 2, 1) and tuple(d_s[l].shape[:3]) == (B, 2, 3)
            np.testing.assert_allclose(o_s[l][:, 0].cpu().numpy(), g[f"eval.transformed.{l}"], atol=1e-4)
            np.testing.assert_allclose(d_s[l][:, 1].cpu().numpy(), g[f"eval.individual_dfs.{l}"], atol=1e-4)
        avg_out, avg_dfs = model.predict(x, y, N=2)
        _, fin_o = O.combine_dfs({l: T(g[f"eval.individual_dfs.{l}"]) for l in range(L)},
                                 O.Cfg(Tl, L, size, n0=n0, df_resolution="full_res" if "fullres" in case else "level_res"))
        for l in avg_out:
            ref = O.warp(fin_o[l], T(g["x"]))
            np.testing.assert_allclose(avg_out[l].cpu().numpy(), ref.numpy(), atol=1e-4)


def _copy_oracle_sd_into(model, sd):
    msd = model.state_dict()
    assert set(msd) == set(sd), set(msd) ^ set(sd)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})


def test_step_vs_oracle_at_baseline_width(api):
    """n0 = 32 (the BASELINE channel plan: 32/64/128 + 96-channel feedback path), 32^3, T=3/L=2, B=1: config 1 of BASELINE.json.

    Gradients are judged against an fp64 run of the oracle.  LeakyReLU's derivative jumps (1 <-> 0.2) where a BatchNorm
    output is ~0: any fp32 evaluation (this one, or the reference's own CPU path) flips the slope of a few of the ~5e6
    activations relative to fp64, and ONE flip moves the gradient of every upstream parameter by ~1e-3 relative
    (scripts/step_accuracy.py shows the three flips of this seed and that every kernel on its own is at 1e-7).  The
    test therefore counts the flips and applies the tight bound when there are none, the SURVEY.md §8(c) envelope
    (5e-3) otherwise."""
    models, nb = api
    cfg = O.Cfg(3, 2, [32, 32, 32], n0=32)
    sd = O.init_state_dict(cfg, seed=1)
    gen = torch.Generator().manual_seed(9)
    x, y = torch.rand(1, 1, 32, 32, 32, generator=gen), torch.rand(1, 1, 32, 32, 32, generator=gen)
    eps = {0: torch.randn(1, 3, 16, 16, 16, generator=gen), 1: torch.randn(1, 3, 8, 8, 8, generator=gen)}
    model = models.PULPo(3, 2, 0.1, [32, 32, 32], feedback=FB, n0=32)
    model._needed_levels = None       # (every ConvUnit's output is materialised here: the slope-flip count below looks at all of them)
    _copy_oracle_sd_into(model, sd)
    model = model.cuda().train()
    for l in range(2):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l].cuda())
    gpu_units = {}
    for name, mod in model.named_modules():
        if isinstance(mod, nb.ConvUnit):
            mod.register_forward_hook(lambda m, i, o, name=name: _record_unit(gpu_units, name, o))

    # oracle in fp32 (values) and fp64 (gradient ground truth), recording every ConvUnit output
    ref_units = {}
    orig_unit = O.conv_unit

    def recording_unit(h, sd_, prefix, training):
        out = orig_unit(h, sd_, prefix, training)
        ref_units[prefix] = out.detach()
        return out

    osd = O.clone_sd(sd, requires_grad=True)
    ls, grads, outs_o = O.train_step(osd, cfg, x, y, eps)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    O.conv_unit = recording_unit
    try:
        _, grads64, _ = O.train_step(O.clone_sd(sd64, requires_grad=True), cfg, x.double(), y.double(), {l: e.double() for l, e in eps.items()})
    finally:
        O.conv_unit = orig_unit

    outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x.cuda(), y.cuda())
    for name, d, do in zip(OUT, outs, outs_o):
        for l in d:
            err = float((d[l].cpu() - do[l]).abs().max())
            assert err <= 1e-4 * max(1.0, float(do[l].abs().max())), (name, l, err)
    for a, b in zip((total, kl, rec, reg), ls[:4]):
        np.testing.assert_allclose(float(a), float(b), rtol=1e-4)
    total.backward()
    flips = sum(int(((gpu_units[k].cpu() > 0) != (ref_units[k] > 0)).sum()) for k in ref_units)
    n_act = sum(v.numel() for v in ref_units.values())
    assert set(gpu_units) == set(ref_units) and flips <= 1e-5 * n_act, (flips, n_act)
    bound = 2e-4 if flips == 0 else 5e-3
    checked = 0
    worst_gpu = worst_cpu = 0.0
    for k, p in model.named_parameters():
        gr = grads64.get(k)
        if gr is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            continue                              # zero-mean gradient (BatchNorm follows): noise on both sides
        e_gpu, e_cpu = rel_l2(p.grad, gr), rel_l2(grads[k], gr)
        worst_gpu, worst_cpu = max(worst_gpu, e_gpu), max(worst_cpu, e_cpu)
        assert e_gpu < bound, (k, e_gpu, e_cpu, flips)
        checked += 1
    print(f"LeakyReLU slope flips vs fp64: {flips} of {n_act}; worst grad rel-L2 vs fp64: gpu {worst_gpu:.2e}, cpu-fp32 oracle {worst_cpu:.2e}")
    assert checked > 60


@pytest.mark.parametrize("activations", ["fp32", "bf16"])
def test_bf16_operand_mode_step_vs_oracle_definition(api, activations):
    """BASELINE configs 4-5 name bf16; the reference has no such mode, so the mode is DEFINED in oracle/pulpo_oracle.py
    (3x3x3 conv operands rounded to bf16, fp32 accumulation, all else fp32 - "parity unpinned" against the reference).
    Same case as the fp32 test above (n0 = 32, 32^3, T3/L2).

    A whole step cannot be compared tightly with its definition: rounding to bf16 is discontinuous, so two evaluations whose
    activations differ by fp32 rounding put a fraction e / 2^-8 of the operands on different sides of a bf16 boundary and the
    difference grows layer by layer towards the bf16 rounding level (e -> sqrt(e * 2^-8)); scripts/bf16_step_accuracy.py
    shows the oracle's own fp32 and fp64 evaluations of the definition 4-10 % apart in the parameter gradients.  The tight
    check of the kernels is the per-operator test (2e-6 against the definition, tests/test_gpu_ops.py).  Here:
      * the GPU step is no further from the fp64 evaluation of the definition than the oracle's fp32 evaluation is
        (x1.5 + 1e-2 for gradients, x2 + 1e-3 for outputs), loss terms rtol 1e-2;
      * stated cost of the mode against the fp32 arithmetic of the reference (oracle, fp64): loss terms rtol 5e-2, final
        displacement field 5e-2 of its maximum, parameter gradients relative-L2 <= 0.5 (measured 0.03 - 0.25 on this
        batch-1 32^3 case: the gradient noise bf16 operands cost, the same in the oracle's evaluation)."""
    models, nb = api
    from pulpo_amd import ops
    cfg = O.Cfg(3, 2, [32, 32, 32], n0=32)
    sd = O.init_state_dict(cfg, seed=1)
    gen = torch.Generator().manual_seed(9)
    x, y = torch.rand(1, 1, 32, 32, 32, generator=gen), torch.rand(1, 1, 32, 32, 32, generator=gen)
    eps = {0: torch.randn(1, 3, 16, 16, 16, generator=gen), 1: torch.randn(1, 3, 8, 8, 8, generator=gen)}
    eps64 = {l: e.double() for l, e in eps.items()}
    model = models.PULPo(3, 2, 0.1, [32, 32, 32], feedback=FB, n0=32)
    _copy_oracle_sd_into(model, sd)
    model = model.cuda().train()
    for l in range(2):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l].cuda())
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ls_true, g_true, outs_true = O.train_step(O.clone_sd(sd64, requires_grad=True), cfg, x.double(), y.double(), eps64)
    # activations == "bf16": the mode of BASELINE configs 4-5 as benched - the multi-channel activation tensors and their gradients are
    # additionally STORED as bf16 (ops.ACT_BF16; the oracle rounds value and gradient at the same tensors, O.ACT_PRECISION) - same criteria
    O.CONV_PRECISION, O.ACT_PRECISION = "bf16", activations
    ops.set_conv_precision("bf16", activations=activations)
    try:
        ls, g_def64, outs_o = O.train_step(O.clone_sd(sd64, requires_grad=True), cfg, x.double(), y.double(), eps64)
        _, g_def32, outs_o32 = O.train_step(O.clone_sd(sd, requires_grad=True), cfg, x, y, eps)
        outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x.cuda(), y.cuda())
        total.backward()
        if activations == "bf16":       # the storage really is bf16 where the definition says so
            acts = model.downpath(x.cuda(), y.cuda())
            assert all(a.dtype == torch.bfloat16 for a in acts.values())
    finally:
        O.CONV_PRECISION, O.ACT_PRECISION = "fp32", "fp32"
        ops.set_conv_precision("fp32")

    def maxerr(a, b):
        return float((a.detach().cpu().double() - b.detach().double()).abs().max()) / max(1.0, float(b.detach().abs().max()))

    worst_out = 0.0
    for name, d, do, do32 in zip(OUT, outs, outs_o, outs_o32):
        for l in d:
            e_gpu, e_cpu = maxerr(d[l], do[l]), maxerr(do32[l], do[l])
            worst_out = max(worst_out, e_gpu)
            assert e_gpu <= 2 * e_cpu + 1e-3, (name, l, e_gpu, e_cpu)
    for a, b in zip((total, kl, rec, reg), ls[:4]):
        np.testing.assert_allclose(float(a), float(b), rtol=1e-2)
    worst = worst_true = 0.0
    checked = 0
    for k, p in model.named_parameters():
        if g_def64.get(k) is None or (k.endswith("_op.0.bias") and "velocity_field._op.2" not in k):
            continue
        e_gpu, e_cpu, e_true = rel_l2(p.grad, g_def64[k]), rel_l2(g_def32[k], g_def64[k]), rel_l2(p.grad, g_true[k])
        worst, worst_true = max(worst, e_gpu), max(worst_true, e_true)
        # (bf16 storage: every stored tensor is one more discontinuous rounding - two fp32 evaluations of the definition drift further apart, and
        #  the product path sums the bf16 gradients of a tensor with several consumers in bf16, which the definition's single rounding of the
        #  fp32 sum does not model; the kernels themselves are held to the definition per operator, tests/test_gpu_ops.py::test_bf16_storage_*)
        assert e_gpu <= (1.5 if activations == "fp32" else 2.5) * e_cpu + (1e-2 if activations == "fp32" else 2e-2), (k, e_gpu, e_cpu)
        assert e_true <= 0.5, (k, e_true)
        checked += 1
    assert checked > 60
    for a, b in zip((total, kl, rec, reg), ls_true[:4]):
        np.testing.assert_allclose(float(a), float(b), rtol=5e-2)
    fin = OUT.index("final_dfs")
    dfe = maxerr(outs[fin][0], outs_true[fin][0]) * max(1.0, float(outs_true[fin][0].abs().max())) / float(outs_true[fin][0].abs().max())
    assert dfe < 5e-2, dfe
    print(f"bf16-operand mode, {activations} activations: worst output err vs definition {worst_out:.2e}, worst grad rel-L2 vs definition {worst:.2e}, vs fp32 arithmetic "
          f"{worst_true:.2e}; final field vs fp32 {dfe:.2e}; total loss {float(total):.6f} vs fp32 {float(ls_true[0]):.6f}")


@pytest.mark.parametrize("side_stream", ["auto", "1"])
def test_fused_adam_arena_step_matches_torch_adam(api, side_stream, monkeypatch):
    """DataParallelStepper (flat arenas + fused Adam, world size 1) vs torch.optim.Adam on the same model; with the weight gradients in line
    (the fp32 default) and forced onto the side stream (PULPO_WGRAD_SIDE_STREAM=1: the bf16 configurations' path, here in fp32)"""
    models, nb = api
    from pulpo_amd.dp import DataParallelStepper
    monkeypatch.setenv("PULPO_WGRAD_SIDE_STREAM", side_stream)
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(4)
    x, y = torch.rand(1, 1, 16, 16, 16, generator=gen).cuda(), torch.rand(1, 1, 16, 16, 16, generator=gen).cuda()
    eps = [torch.randn(1, 3, 8, 8, 8, generator=gen).cuda(), torch.randn(1, 3, 4, 4, 4, generator=gen).cuda()]
    empty = torch.empty((0,))
    batch = (x, y, empty, empty, empty, empty, empty, empty)

    def make():
        torch.manual_seed(0)
        m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=8, lr=1e-3).cuda().train()
        for l in range(2):
            m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        return m

    a, b = make(), make()
    stepper = DataParallelStepper(a)
    assert stepper.wgrad_on_side_stream() == (side_stream == "1")
    opt = b.configure_optimizers()
    for _ in range(2):
        stepper.step(batch)
        opt.zero_grad()
        b.training_step(batch, 0).backward()
        opt.step()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            continue      # Adam normalises pure rounding noise on these (documented): not comparable element-wise
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), atol=2e-4, rtol=0)


def test_full_resolution_properties_96(api):
    """BASELINE config 2 shape (96^3, T=4/L=3, B=2, n0=32): no oracle at this size in the test budget; check
    size-independent properties instead: finite outputs, shapes, KL >= 0, NCC in [-gamma*w*V, 0], gradient present on
    every used parameter, and determinism of the forward given fixed noise."""
    models, nb = api
    torch.manual_seed(0)
    size = [96, 96, 96]
    model = models.PULPo(4, 3, 0.1, size, feedback=FB, n0=32).cuda().train()
    gen = torch.Generator().manual_seed(1)
    x, y = torch.rand(2, 1, *size, generator=gen).cuda(), torch.rand(2, 1, *size, generator=gen).cuda()
    for l in range(3):
        s = 96 // (2 ** (l + 1))
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(2, 3, s, s, s, generator=gen).cuda())
    outs, _, (total, kl, rec, reg), levels = model._forward_and_losses(x, y)
    assert outs[7][0].shape == (2, 1, 96, 96, 96) and outs[6][0].shape == (2, 3, 96, 96, 96)
    assert outs[7][1].shape == (2, 1, 24, 24, 24) and outs[5][0].shape == (2, 3, 48, 48, 48)
    for d in outs:
        for v in d.values():
            assert bool(torch.isfinite(v).all())
    assert float(kl) >= 0 and float(reg) >= 0 and float(rec) <= 0
    total.backward()
    for k, p in model.named_parameters():
        if "encoders.2.sample_merge_block" in k:
            assert p.grad is None
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    with torch.no_grad():
        model.eval()
        a = model(x, y)
        b = model(x, y)
        assert bool((a == b).all())        # the forward path has no atomics: bitwise reproducible


def test_config5_shape_bf16_train_step_and_mc_uncertainty(api):
    """BASELINE config 5: 192 x 224 x 160 pair, 5-level pyramid (T6/L5, n0 = 32), bf16 conv operands, OASIS-style synthetic data, one
    training step through the data-parallel stepper plus the 8-sample Monte-Carlo uncertainty maps.  No oracle at this size in the test
    budget (a CPU step takes minutes): size-independent properties - shapes of every level (deepest 6 x 7 x 5), finite values, loss
    decrease over three Adam steps on one pair, std maps finite, non-negative and zero outside the head mask for the warped image."""
    models, nb = api
    from pulpo_amd import dp, ops, synthetic
    from pulpo_amd.uncertainty import mc_uncertainty
    size = [192, 224, 160]
    torch.manual_seed(0)
    model = models.PULPo(6, 5, 0.1, size, feedback=FB, n0=32).cuda().train()
    x, y = synthetic.oasis_like_pair(size, 1, 7, "cuda")
    assert 0.2 < float((y > 0).float().mean()) < 0.35            # ellipsoid with semi-axes 0.4: 4/3 pi 0.4^3 = 0.27 of the box
    empty = torch.empty((0,), device="cuda")
    ops.set_conv_precision("bf16", activations="bf16")
    try:
        stepper = dp.DataParallelStepper(model)
        losses = [float(stepper.step((x, y, empty, empty, empty, empty, empty, empty))) for _ in range(3)]
        assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
        model.eval()
        with torch.no_grad():
            outs = model.autoencoder(x, model.downpath(x, y))
        for l in range(5):
            k = l + 1
            lvl = tuple(s // 2 ** k for s in size)
            assert tuple(outs[0][l].shape) == (1, 3) + lvl                                       # mus
            assert tuple(outs[7][l].shape) == (1, 1) + (tuple(size) if l == 0 else lvl)            # transformed
        assert tuple(outs[0][4].shape[2:]) == (6, 7, 5)
        res = mc_uncertainty(model, x, y, 8)
        for l in range(5):
            for key in ("output_std", "individual_df_std", "final_df_std"):
                v = res[key][l]
                assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0, (key, l)
            assert float(res["individual_df_std"][l].max()) > 0.0
        corner = res["output_std"][0][:8, :8, :8]
        assert float(corner.abs().max()) < 1e-6          # background stays background under small deformations
    finally:
        ops.set_conv_precision("fp32")


def test_config4_160_bf16_oasis_step(api):
    """BASELINE config 4: 160^3 OASIS-style T1 pair, 4-level pyramid (T5/L4, n0 = 32), bf16 conv operands, batch 1, through the
    data-parallel stepper (the per-GPU body of the 8-GPU job).  The bf16 mode is a definition of this repository ("parity unpinned"
    against the reference; its kernels are held to the definition per operator in test_gpu_ops.py), so at full size the
    checks are properties: shapes of every level, finite values, background stays background in the warped image, the loss falls over
    three Adam steps on one pair, and the bf16 forward stays within the mode's stated distance of the exact-fp32 forward of the same
    weights (loss terms rtol 5e-2, full-resolution field 5e-2 of its maximum)."""
    models, nb = api
    from pulpo_amd import dp, ops, synthetic
    size = [160, 160, 160]
    torch.manual_seed(0)
    model = models.PULPo(5, 4, 0.1, size, feedback=FB, n0=32).cuda().train()
    x, y = synthetic.oasis_like_pair(size, 1, 7, "cuda")
    assert 0.2 < float((y > 0).float().mean()) < 0.35
    gen = torch.Generator().manual_seed(3)
    for l in range(4):
        s_ = 160 // 2 ** (l + 1)
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s_, s_, s_, generator=gen).cuda())
    state = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        outs32, _, losses32, _ = model._forward_and_losses(x, y)
    outs32 = [{l: v.clone() for l, v in d.items()} for d in outs32]
    model.load_state_dict(state)
    empty = torch.empty((0,), device="cuda")
    ops.set_conv_precision("bf16", activations="bf16")
    try:
        with torch.no_grad():
            outs, _, losses, _ = model._forward_and_losses(x, y)
        for l in range(4):
            lvl = tuple(s // 2 ** (l + 1) for s in size)
            assert tuple(outs[0][l].shape) == (1, 3) + lvl
            assert tuple(outs[6][l].shape) == (1, 3) + (tuple(size) if l == 0 else lvl)            # final_dfs
            assert tuple(outs[7][l].shape) == (1, 1) + (tuple(size) if l == 0 else lvl)            # transformed
            for d in outs:
                assert bool(torch.isfinite(d[l]).all())
        assert float(outs[7][0][0, 0, :6, :6, :6].abs().max()) < 1e-6          # background stays background
        np.testing.assert_allclose([float(v) for v in losses], [float(v) for v in losses32], rtol=5e-2)
        f32, f16 = outs32[6][0], outs[6][0]
        assert float((f32 - f16).abs().max()) <= 5e-2 * float(f32.abs().max())
        model.load_state_dict(state)
        stepper = dp.DataParallelStepper(model)
        hist = [float(stepper.step((x, y, empty, empty, empty, empty, empty, empty))) for _ in range(3)]
        assert all(np.isfinite(hist)) and hist[2] < hist[0], hist
    finally:
        ops.set_conv_precision("fp32")


# per-parameter bound (relative L2) of the 160^3 step's gradients against the fp32 CPU oracle: SURVEY 8(c)'s 5e-3 for >= 64^3.
# profiles/r5_parity_160.md holds the measured distribution: maximum 3.89e-3 over 129 parameters (the fp32 oracle itself sits 3.88e-3 from
# fp64, the GPU 2.08e-3).  Round 5 measured what the float atomics contribute to that distance: the atomic and the deterministic mode differ
# by < 1e-5 relative L2 per parameter (test_deterministic_mode_gives_bit_identical_gradients) - the distance from the oracle is fp32 rounding
# of two different summation orders, not run-to-run spread, so the 6e-3 of rounds 3 - 4 ("room for the atomic order") was not needed.
GRAD_BOUND_160 = 5e-3
# ... and in DETERMINISTIC mode (ops.set_deterministic: ordered sums instead of float atomics) the gradients are one fixed set of numbers: the
# bound is SURVEY 8(c)'s 5e-3 itself (measured maximum: profiles/r5_parity_160.md)
GRAD_BOUND_160_DETERMINISTIC = 5e-3


def _write_parity_report(vs32, e_gpu, e_ref, mode="atomic", bound=None):
    """the measured gradient distances of the 160^3 step, kept as a file (gpurun_out/parity_160.md; a builder run's copy is committed as
    profiles/r3_parity_160.md): the evidence the bound above is set from"""
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        d = np.array([v for v, _ in vs32])
        worst = sorted(vs32, reverse=True)[:8]
        with open(os.path.join(out, "parity_160.md"), "w" if mode == "atomic" else "a") as f:
            f.write(f"# 160^3 / T5 / L4 / n0 32 training step: parameter gradients, GPU ({mode} mode) vs CPU oracle (test_headline_160_step_vs_cpu_oracle)\n\n")
            f.write(f"{len(d)} parameters compared (conv biases in front of a BatchNorm excluded: true gradient zero).\n\n")
            f.write("| relative L2 distance | median | p90 | p99 | max |\n|---|---|---|---|---|\n")
            f.write(f"| GPU vs fp32 CPU oracle | {np.median(d):.2e} | {np.percentile(d, 90):.2e} | {np.percentile(d, 99):.2e} | {d.max():.2e} |\n")
            f.write(f"| GPU vs fp64 oracle | {np.median(e_gpu):.2e} | {np.percentile(e_gpu, 90):.2e} | {np.percentile(e_gpu, 99):.2e} | {e_gpu.max():.2e} |\n")
            f.write(f"| fp32 CPU oracle vs fp64 oracle | {np.median(e_ref):.2e} | {np.percentile(e_ref, 90):.2e} | {np.percentile(e_ref, 99):.2e} | {e_ref.max():.2e} |\n\n")
            f.write("Largest GPU-vs-fp32 distances:\n\n" + "".join(f"* `{k}` {v:.2e}\n" for v, k in worst))
            f.write(f"\nBound applied by the test: every parameter < {bound if bound else GRAD_BOUND_160:g} of the fp32 oracle; distance from fp64 distributed like the fp32 oracle's own.\n\n")
    except OSError:
        pass


def test_headline_160_step_vs_cpu_oracle(api):
    """The metric's workload at FULL size (160^3, T5/L4, n0 = 32, B = 1), default kernel selection (F(2x2x2,3x3x3) Winograd forward / data
    gradient / weight gradient on the 160^3 - 40^3 levels, the (y, x) form F(2x2,3x3) on the 20^3 / 10^3 levels), against ONE step of the CPU oracle in fp32 (the reference's arithmetic; ~11 s) and in fp64
    (the ground truth for gradients; ~30 s): every output dictionary atol 1e-4 (scaled by the tensor's magnitude), loss terms rtol 1e-4.
    Gradients: at this size every fp32 evaluation flips LeakyReLU slopes against any other (~6e8 activations) and carries the
    summation noise of 4e6-voxel reductions (the reference's own fp32-vs-fp64 envelope grows with the volume), so the
    criterion is the flip-aware one of the 32^3 golden test: every parameter within GRAD_BOUND_160 (relative L2) of the fp32 oracle, and the
    distance from fp64 distributed like the fp32 oracle's own (median <= 4x + 2e-4, maximum <= 6x + 1e-3)."""
    models, nb = api
    size = [160, 160, 160]
    cfg = O.Cfg(5, 4, size, n0=32)
    sd = O.init_state_dict(cfg, seed=0)
    gen = torch.Generator().manual_seed(21)
    x, y = torch.rand(1, 1, *size, generator=gen), torch.rand(1, 1, *size, generator=gen)
    eps = {l: torch.randn(1, 3, *[160 // 2 ** (l + 1)] * 3, generator=gen) for l in range(4)}
    from pulpo_amd import ops
    env_det = __import__("os").environ.get("PULPO_DETERMINISTIC", "0") == "1"

    def gpu_step(det):
        # (round 5: the step is evaluated twice - with the float atomics of the default mode and in deterministic mode - against ONE oracle pair)
        ops.set_deterministic(det)
        try:
            model = models.PULPo(5, 4, 0.1, size, feedback=FB, n0=32)
            _copy_oracle_sd_into(model, sd)
            model = model.cuda().train()
            for l in range(4):
                model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l].cuda())
            outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x.cuda(), y.cuda())
            total.backward()
            torch.cuda.synchronize()
            res = ([{l: v.detach().cpu() for l, v in d.items()} for d in outs], [float(v) for v in (total, kl, rec, reg)],
                   {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in model.named_parameters()})
            del outs, total, kl, rec, reg, model
            torch.cuda.empty_cache()
            return res
        finally:
            ops.set_deterministic(env_det)

    gpu_out, gpu_loss, gpu_grad = gpu_step(False)
    det_out, det_loss, det_grad = gpu_step(True)
    assert det_loss == gpu_loss                       # (the forward pass is the same kernels in both modes)
    del det_out

    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    ls, grads, outs_o = O.train_step(O.clone_sd(sd, requires_grad=True), cfg, x, y, eps)
    for name, d, do in zip(OUT, gpu_out, outs_o):
        for l in d:
            err = float((d[l] - do[l]).abs().max())
            assert err <= 1e-4 * max(1.0, float(do[l].abs().max())), (name, l, err)
    np.testing.assert_allclose(gpu_loss, [float(v) for v in ls[:4]], rtol=1e-4)
    del outs_o, gpu_out
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    _, grads64, _ = O.train_step(O.clone_sd(sd64, requires_grad=True), cfg, x.double(), y.double(), {l: e.double() for l, e in eps.items()})
    for mode, grad_set, bound in (("atomic", gpu_grad, GRAD_BOUND_160), ("deterministic", det_grad, GRAD_BOUND_160_DETERMINISTIC)):
        vs64, vs32 = [], []
        for k, g in grad_set.items():
            gr = grads.get(k)
            if gr is None:
                assert g is None or float(g.abs().max()) == 0.0, k
                continue
            if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
                wref = float(grads[k[:-4] + "weight"].abs().max())          # true gradient zero (a BatchNorm follows): noise on both sides
                assert float(g.abs().max()) <= 1e-2 * max(wref, 1e-3), k
                continue
            d32 = rel_l2(g, gr)
            assert d32 < bound, (mode, k, d32)
            vs32.append((d32, k))
            vs64.append((rel_l2(g, grads64[k]), rel_l2(gr, grads64[k])))
        assert len(vs64) > 100
        e_gpu, e_ref = np.array(vs64).T
        print(f"160^3 gradients vs fp64 ({mode} mode): gpu median {np.median(e_gpu):.2e} max {e_gpu.max():.2e}; cpu fp32 oracle median {np.median(e_ref):.2e} "
              f"max {e_ref.max():.2e}; largest distance from the fp32 oracle {max(vs32)[0]:.2e} (bound {bound:g})")
        _write_parity_report(vs32, e_gpu, e_ref, mode, bound)
        assert np.median(e_gpu) <= 4.0 * np.median(e_ref) + 2e-4, (np.median(e_gpu), np.median(e_ref))
        assert e_gpu.max() <= 6.0 * e_ref.max() + 1e-3, (e_gpu.max(), e_ref.max())


def test_config2_96_step_vs_cpu_oracle(api):
    """BASELINE config 2 (96^3 synthetic pair, 3-level pyramid = T4/L3, n0 = 32, fp32, batch 2 on one GPU) against ONE fp32 step of the CPU
    oracle on the same weights, inputs and noise (a few seconds on the box's cores): every output dictionary atol 1e-4 (scaled by the
    tensor's magnitude), loss terms rtol 1e-4, every parameter gradient within 5e-3 relative L2 (SURVEY 8(c)'s bound for >= 64^3; conv
    biases in front of a BatchNorm - true gradient zero - on the scale of their layer's weight gradient)."""
    models, nb = api
    size, B, Tl, L = [96, 96, 96], 2, 4, 3
    cfg = O.Cfg(Tl, L, size, n0=32)
    sd = O.init_state_dict(cfg, seed=2)
    gen = torch.Generator().manual_seed(96)
    x, y = torch.rand(B, 1, *size, generator=gen), torch.rand(B, 1, *size, generator=gen)
    eps = {l: torch.randn(B, 3, *[96 // 2 ** (l + 1)] * 3, generator=gen) for l in range(L)}
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=32)
    _copy_oracle_sd_into(model, sd)
    model = model.cuda().train()
    for l in range(L):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l].cuda())
    outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x.cuda(), y.cuda())
    total.backward()
    torch.cuda.synchronize()
    gpu_out = [{l: v.detach().cpu() for l, v in d.items()} for d in outs]
    gpu_loss = [float(v) for v in (total, kl, rec, reg)]
    gpu_grad = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in model.named_parameters()}
    del outs, total, kl, rec, reg, model
    torch.cuda.empty_cache()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    ls, grads, outs_o = O.train_step(O.clone_sd(sd, requires_grad=True), cfg, x, y, eps)
    for name, d, do in zip(OUT, gpu_out, outs_o):
        for l in d:
            err = float((d[l] - do[l]).abs().max())
            assert err <= 1e-4 * max(1.0, float(do[l].abs().max())), (name, l, err)
    np.testing.assert_allclose(gpu_loss, [float(v) for v in ls[:4]], rtol=1e-4)
    dist = []
    for k, g in gpu_grad.items():
        gr = grads.get(k)
        if gr is None:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            wref = float(grads[k[:-4] + "weight"].abs().max())
            assert float(g.abs().max()) <= 1e-2 * max(wref, 1e-3), k
            continue
        d32 = rel_l2(g, gr)
        dist.append((d32, k))
        assert d32 < 5e-3, (k, d32)
    assert len(dist) > 80
    print(f"96^3 B=2 gradients vs fp32 CPU oracle: median {np.median([d for d, _ in dist]):.2e}, max {max(dist)[0]:.2e} ({max(dist)[1]})")


def _assert_bn_buffers_follow_the_parameter_noise(model_named_buffers, bn_ref, param_delta, momentum=0.1):
    """BatchNorm running statistics of two runs whose ConvUnit parameters differ by `param_delta` (name -> |p_a - p_b|).  The batch mean of
    a unit's convolution output carries its bias one to one and a weight difference dW[c] times the input's mean (|mean| <= 1 for the
    unit-scale activations of this network), so after one more forward pass channel c's running mean may differ by
    momentum * (|db[c]| + ||dW[c]||_1) - plus rounding - and by nothing else; returns the largest observed / allowed ratio."""
    worst = 0.0
    for k, v in model_named_buffers:
        if k.endswith("running_var"):
            np.testing.assert_allclose(v.detach().cpu().numpy(), bn_ref[k].cpu().numpy(), rtol=2e-4, atol=1e-7)
        elif k.endswith("running_mean"):
            d = (v.detach() - bn_ref[k]).abs().cpu().numpy()
            db = param_delta[k.replace("_op.1.running_mean", "_op.0.bias")].cpu().numpy()
            dw = param_delta[k.replace("_op.1.running_mean", "_op.0.weight")].flatten(1).sum(1).cpu().numpy()
            bound = momentum * (db + dw) + 1e-4 * np.abs(bn_ref[k].cpu().numpy()) + 1e-5        # (rounding of a 4e6-voxel mean, upstream layers' own noise)
            assert (d <= bound).all(), (k, float(d.max()), float(db.max()), float(dw.max()))
            worst = max(worst, float((d / bound).max()))
    return worst


def test_headline_160_stepper_and_lightning_hooks_equal_autograd(api):
    """The path bench.py TIMES, at the metric's size (160^3, T5/L4, n0 = 32, B = 1), three ways on the same weights, inputs and noise:

      A  plain autograd: loss.backward() + torch.optim.Adam (the path test_headline_160_step_vs_cpu_oracle holds to the oracle);
      B  `DataParallelStepper.step` with its default switches - parameter gradients straight into the arena, weight gradients on the side
         stream, BatchNorm sums from the data-gradient epilogue, one grad_finish_multi launch, fused Adam, in-place re-pack;
      C  the LightningModule hooks of PULPo driven in pytorch_lightning 1.8's call order (HookOrderTrainer: training_step ->
         optimizer_zero_grad -> on_before_backward / backward / on_after_backward -> optimizer.step(closure) on what configure_optimizers
         returned) - what an unchanged train.py runs (train.py:106-116, models.py:134-196, 398-400).

    The step's loss is bit-equal on all three (same forward kernels); every parameter gradient of B and C agrees with A to 1e-5 relative L2
    (float-atomic order is the only difference); the loss of a SECOND step agrees to 1e-5 (covers fused Adam and the in-place pack refresh
    at the size where stream hazards would show).  BatchNorm running statistics: after ONE step they are equal to rounding (rtol 1e-6: the
    forward pass is the same kernels on the same weights); after two steps the means may differ by what the unit's own parameters
    differ - Adam turns rounding-noise gradients (every conv bias in front of a BatchNorm, a few near-zero weight elements) into +-lr moves -
    times the momentum, per channel, which is asserted as such with the measured parameter differences."""
    models, nb = api
    from pulpo_amd import dp, ops
    from pulpo_amd._lightning import HookOrderTrainer
    size = [160, 160, 160]
    gen = torch.Generator().manual_seed(33)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    eps = [torch.randn(1, 3, *[160 // 2 ** (l + 1)] * 3, generator=gen).cuda() for l in range(4)]
    batch = (x, y, None, None, None, None, None, None)

    def make():
        torch.manual_seed(5)
        m = models.PULPo(5, 4, 0.1, size, feedback=FB, n0=32).cuda().train()
        for l in range(4):
            m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        return m

    def snapshot(model):
        """after the first step: gradients, BatchNorm buffers, the ConvUnit convolutions' parameters (moved once by Adam)"""
        return ({k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: v.detach().clone() for k, v in model.named_buffers() if "running" in k},
                {k: p.detach().clone() for k, p in model.named_parameters() if "_op.0." in k})

    # ---- A: plain autograd + torch.optim.Adam
    model = make()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    loss_a = model.training_step(batch, 0)
    loss_a.backward()
    grads_a, bn_a1, _ = snapshot(model)
    opt.step()
    par_a = {k: p.detach().clone() for k, p in model.named_parameters() if "_op.0." in k}
    opt.zero_grad(set_to_none=True)
    loss_a2 = model.training_step(batch, 0).detach()
    bn_a = {k: v.detach().clone() for k, v in model.named_buffers() if "running" in k}
    torch.cuda.synchronize()
    l_a, l_a2 = float(loss_a), float(loss_a2)
    del model, opt, loss_a, loss_a2
    torch.cuda.empty_cache()

    def compare(tag, model, l_1, first, l_2):
        grads, bn_1, par_1 = first
        assert l_1 == l_a, (tag, l_1, l_a)
        worst = 0.0
        for k, ga in grads_a.items():
            if float(ga.abs().max()) == 0.0:
                assert k not in grads or float(grads[k].abs().max()) == 0.0, (tag, k)
                continue
            if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
                # conv bias in front of a BatchNorm: true gradient zero, both sides hold rounding noise of differently ordered sums
                wmax = float(grads_a[k[:-4] + "weight"].abs().max())
                assert float((grads[k] - ga).abs().max()) <= 1e-4 * max(wmax, 1e-6), (tag, k)
                continue
            d = rel_l2(grads[k], ga)
            worst = max(worst, d)
            assert d < 1e-5, (tag, k, d)
        np.testing.assert_allclose(l_2, l_a2, rtol=1e-5)
        for k, v in bn_1.items():                    # after ONE step: nothing but the forward pass has touched them
            np.testing.assert_allclose(v.cpu().numpy(), bn_a1[k].cpu().numpy(), rtol=1e-6, atol=1e-9, err_msg=f"{tag} {k}")
        delta = {k: (p - par_a[k]).abs() for k, p in par_1.items()}       # the parameters the SECOND forward pass ran on
        assert max(float(v.max()) for v in delta.values()) <= 2.0e-4 * 1.0001      # one Adam move of at most lr on either side
        ratio = _assert_bn_buffers_follow_the_parameter_noise(model.named_buffers(), bn_a, delta)
        print(f"{tag}: running means after two steps at most {ratio:.2f} of what the parameter noise allows")
        return worst

    # ---- B: the stepper
    model = make()
    stepper = dp.DataParallelStepper(model, lr=1e-4)
    assert stepper.async_wgrad and ops.BN_REDUCE_IN_DGRAD, "default switches"
    assert stepper.wgrad_on_side_stream() is False, "fp32: the weight gradient holds its CUs whole and runs in line (dp.DataParallelStepper.wgrad_on_side_stream)"
    l_b = float(stepper.step(batch))
    first_b = snapshot(model)
    l_b2 = float(stepper.step(batch))
    torch.cuda.synchronize()
    worst_b = compare("stepper", model, l_b, first_b, l_b2)
    grads_b = first_b[0]
    del model, stepper
    torch.cuda.empty_cache()

    # ---- C: Lightning's hook order over the module's own hooks
    model = make()
    trainer = HookOrderTrainer()
    opt = trainer.attach(model)
    assert isinstance(opt, torch.optim.Adam) and isinstance(opt, dp.ArenaAdam) and opt.engine.async_wgrad
    l_c = float(trainer.run_batch(batch, 0))
    assert trainer.calls == ["on_train_batch_start", "optimizer_step", "training_step", "on_before_zero_grad", "optimizer_zero_grad",
                             "on_before_backward", "backward", "on_after_backward", "on_before_optimizer_step", "on_train_batch_end"]
    first_c = snapshot(model)
    l_c2 = float(trainer.run_batch(batch, 1))
    torch.cuda.synchronize()
    worst_c = compare("lightning-hooks", model, l_c, first_c, l_c2)
    grads_c = first_c[0]
    assert l_c == l_b
    for k, gb in grads_b.items():                   # B and C are the same kernels in the same order: atomic order is all that differs
        if float(gb.abs().max()) > 0.0 and not (k.endswith("_op.0.bias") and "velocity_field._op.2" not in k):
            assert rel_l2(grads_c[k], gb) < 1e-5, k
    print(f"160^3: worst gradient distance from plain autograd - stepper {worst_b:.2e}, lightning hooks {worst_c:.2e}; "
          f"losses {l_b} / {l_b2}, {l_c} / {l_c2} vs {l_a} / {l_a2}")


def test_headline_config_160_direct_and_winograd_kernels_agree(api):
    """BASELINE config 3 / the metric's workload at FULL size (160^3, T5/L4, n0 = 32, B = 1): no oracle run fits the test budget
    (11 s per CPU step), so the size-independent property is the agreement of independent kernels - the direct implicit-GEMM
    convolution (pinned against the reference goldens at small sizes) and the Winograd kernels - on every output dictionary and the
    loss terms of one training-mode forward, plus finite gradients and a bitwise reproducible forward."""
    models, nb = api
    from pulpo_amd import ops
    size = [160, 160, 160]
    torch.manual_seed(0)
    model = models.PULPo(5, 4, 0.1, size, feedback=FB, n0=32).cuda().train()
    gen = torch.Generator().manual_seed(11)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    for l in range(4):
        s_ = 160 // 2 ** (l + 1)
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s_, s_, s_, generator=gen).cuda())
    bn_state = {k: v.clone() for k, v in model.state_dict().items()}
    res = {}
    try:
        for algo in ("direct", "wino2"):
            ops.CONV_ALGO = algo
            model.load_state_dict(bn_state)                 # same BatchNorm running statistics going in
            with torch.no_grad():
                outs, _, losses, _ = model._forward_and_losses(x, y)
            res[algo] = ([{l: v.clone() for l, v in d.items()} for d in outs], [float(v) for v in losses])
        ops.CONV_ALGO = None
        for algo in ("wino2",):
            for name, d0, d1 in zip(OUT, res["direct"][0], res[algo][0]):
                for l in d0:
                    err = float((d0[l] - d1[l]).abs().max()) / max(1.0, float(d0[l].abs().max()))
                    assert err <= 1e-4, (algo, name, l, err)
            np.testing.assert_allclose(res[algo][1], res["direct"][1], rtol=1e-4)
        model.load_state_dict(bn_state)
        outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y)
        total.backward()
        for k, p in model.named_parameters():
            if "encoders.3.sample_merge_block" in k:
                assert p.grad is None
            else:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        model.eval()
        with torch.no_grad():
            assert bool((model(x, y) == model(x, y)).all())
    finally:
        ops.CONV_ALGO = None


def test_mc_uncertainty_matches_stacked_statistics(api, golden):
    """pulpo_amd.uncertainty.mc_uncertainty (streaming moments) against the reference's procedure (evaluate.py:222-251) carried out
    with stacked samples on the same latent noise: the sampler is replaced by one that replays a recorded noise sequence."""
    models, nb = api
    from pulpo_amd.uncertainty import mc_uncertainty
    g = golden("step_T3L2_n4_16")
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, g)
    model.eval()
    x, y = T(g["x"])[:1].cuda(), T(g["y"])[:1].cuda()
    N = 4
    gen = torch.Generator().manual_seed(5)
    noise = {l: [torch.randn(1, 3, *[s // 2 ** (l + Tl - L) for s in size], generator=gen).cuda() for _ in range(N)] for l in range(L)}

    class Replay:
        def __init__(self, seq):
            self.seq, self.i = seq, 0

        def __call__(self, mu, sigma):
            e = self.seq[self.i % len(self.seq)]
            self.i += 1
            return mu + sigma * e

    def set_samplers():
        for l in range(L):
            model.autoencoder.encoders[l].sampler = Replay(noise[l])

    set_samplers()
    res = mc_uncertainty(model, x, y, N)
    set_samplers()
    outs, inds, fins = {l: [] for l in range(L)}, {l: [] for l in range(L)}, {l: [] for l in range(L)}
    with torch.no_grad():
        for _ in range(N):
            o, ind = model.predict(x, y, N=1)
            _, fin = model.combine_dfs(ind)
            for l in range(L):
                outs[l].append(o[l][0].cpu()); inds[l].append(ind[l][0].cpu()); fins[l].append(fin[l][0].cpu())
    for l in range(L):
        for key, lst in (("output_std", outs), ("individual_df_std", inds), ("final_df_std", fins)):
            ref = O.mc_std_map(torch.stack(lst[l]))
            err = float((res[key][l].cpu() - ref).abs().max())
            assert err <= 1e-5 * max(1.0, float(ref.abs().max())), (key, l, err)
        # reference quirk (evaluate.py:239): the "average" individual field is the last sample's
        assert float((res["individual_dfs"][l].cpu() - inds[l][-1][None]).abs().max()) <= 1e-6
    set_samplers()
    res2 = mc_uncertainty(model, x, y, N, mean_of_samples=True)
    for l in range(L):
        ref = torch.stack(inds[l]).mean(dim=0)
        assert float((res2["individual_dfs"][l][0].cpu() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


DP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from pulpo_amd import dp
import src.models as models, src.network_blocks as nb
dp.init_from_env("gloo")                     # two ranks share the one GPU of the test box: gloo moves CUDA tensors, RCCL would refuse
rank = dist.get_rank()
dev = torch.device("cuda", 0)
FB = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
size = [32, 32, 32]

def build():
    torch.manual_seed(0)
    m = models.PULPo(4, 3, 0.1, size, feedback=FB, n0=8).to(dev).train()
    g = torch.Generator().manual_seed(3)
    for l in range(3):
        s = 32 // 2 ** (l + 1)
        m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s, s, s, generator=g).to(dev))
    return m

g = torch.Generator().manual_seed(50 + rank)           # a different pair on every rank
x, y = torch.rand(1, 1, *size, generator=g).to(dev), torch.rand(1, 1, *size, generator=g).to(dev)
e = torch.empty((0,), device=dev)
batch = (x, y, e, e, e, e, e, e)
ref = build()
ref.training_step(batch, 0).backward()
exp = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
for t in exp.values():
    dist.all_reduce(t)
net = build()
stepper = dp.DataParallelStepper(net, overlap=True)
assert len(stepper.buckets) == 3 and stepper.overlap
stepper.opt.step = lambda scale: None
launches = []
orig = stepper._launch_upto
def spy(i):
    launches.append(i)
    return orig(i)
stepper._launch_upto = spy
stepper.step(batch)
torch.cuda.synchronize()
assert launches == [0, 1, 2], launches
worst = 0.0
for n, p in net.named_parameters():
    if n in exp:
        err = float((p.grad - exp[n]).norm() / (exp[n].norm() + 1e-12))
        if not (n.endswith("_op.0.bias") and "velocity_field._op.2" not in n):      # zero-mean gradients in front of a BatchNorm: noise
            worst = max(worst, err)
            assert err < 1e-3, (n, err)
    else:
        assert float(p.grad.abs().max()) == 0.0, n
print(f"rank {rank} dp ok worst {worst:.2e}")
dist.destroy_process_group()
'''


def test_bucketed_allreduce_with_the_real_model_two_ranks_one_gpu(tmp_path):
    """the overlapped, bucketed gradient exchange of DataParallelStepper with the real PULPo model: two ranks (gloo over CUDA tensors,
    both on the single GPU of the test box) with different pairs; every parameter's gradient after the step equals the sum of the two
    ranks' plain local gradients, i.e. no bucket was reduced before its last contribution had been enqueued."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "dp_worker.py"
    script.write_text(DP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), root], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=420)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o[-3000:]
        assert f"rank {r} dp ok" in o


def test_device_prefetcher_delivers_batches_in_order(api):
    """pulpo_amd.prefetch.DevicePrefetcher (the device half of the input pipeline): every batch arrives on the GPU, bit-identical and in
    order, empty optional entries (segmentations / landmarks / masks of the reference's 8-tuples) included; a training step consumes it"""
    models, nb = api
    from pulpo_amd import dp
    from pulpo_amd.prefetch import DevicePrefetcher
    gen = torch.Generator().manual_seed(2)
    empty = torch.empty((0,))
    batches = [(torch.rand(1, 1, 16, 16, 16, generator=gen), torch.rand(1, 1, 16, 16, 16, generator=gen), empty, empty, empty, empty, empty, empty)
               for _ in range(5)]
    got = list(DevicePrefetcher(batches, "cuda"))
    assert len(got) == 5
    for b_cpu, b_gpu in zip(batches, got):
        assert all(t.is_cuda for t in b_gpu)
        assert torch.equal(b_gpu[0].cpu(), b_cpu[0]) and torch.equal(b_gpu[1].cpu(), b_cpu[1]) and b_gpu[2].numel() == 0
    torch.manual_seed(0)
    model = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=4).cuda().train()
    stepper = dp.DataParallelStepper(model)
    losses = [float(stepper.step(b)) for b in DevicePrefetcher(batches, "cuda")]
    assert len(losses) == 5 and all(np.isfinite(losses))
    with pytest.raises(ValueError):
        DevicePrefetcher(batches, "cpu")


@pytest.mark.parametrize("loop", ["stepper", "lightning"])
def test_bench_two_rank_rehearsal(tmp_path, loop):
    """bench.py's multi-rank path (rendezvous from the torchrun environment, weight broadcast, bucketed exchange, barrier + max-over-ranks
    timing, one JSON line from rank 0) rehearsed with two ranks on the one GPU of the test box: gloo instead of RCCL, which refuses two
    ranks per device.  The driver's real N > 1 runs use the identical code with backend nccl."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PULPO_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", _free_port(),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "32", "32", "32", "--levels", "3", "2",
           "--full", "--no-cpu-baseline", "--loop", loop]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]                     # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["config"]["global_batch"] == 2
    assert d["value"] > 0 and abs(d["value"] - 2 * 1 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]       # pairs of ALL ranks / time
    assert d["roofline"] is not None and d["cpu_baseline"] is None
    # the audit fields of a multi-rank record: the loop that drove the step, the stepper's switches as they were in the timed
    # region, whether a fallback happened, what the process group saw, and the exposed part of the gradient exchange
    assert d["loop"] == {"stepper": "stepper", "lightning": "lightning-hooks"}[loop]
    st = d["stepper"]
    assert st["overlap"] is True and st["async_wgrad"] is True and st["buckets"] == 3 and st["fallback"] == "none"
    assert st["exposed_exchange_ms_per_step"] is not None and st["exposed_exchange_ms_per_step"] >= 0.0
    assert d["dist"]["backend"] == "gloo" and d["dist"]["world"] == 2 and len(d["dist"]["devices"]) == 2
    assert all("cuda:" in n for n in d["dist"]["devices"])


def test_bench_self_launch_two_ranks_without_torchrun():
    """`python bench.py --gpus 2` with NO torchrun environment: the script starts its two ranks itself (before touching a GPU), runs the real
    training step on each (gloo instead of RCCL - two ranks share the one GPU of the test box), and relays exactly one JSON line; also the
    first-step agreement: with an injected first-step failure on every rank all ranks fall back to the plain stepper together, and with one
    on a single rank the job is restarted by the launcher with the overlapped exchange switched off."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    base.update(PULPO_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "32", "32", "32", "--levels", "3", "2",
           "--no-cpu-baseline"]
    for inject, expect, fallback in (("", None, "none"), ("all", "falling back", "in-place"), ("1", "starting all ranks again", "relaunched")):
        # (one rank failing: its peer sits in the gloo collective of the step until the failed rank's vote times out - with RCCL the
        #  collective is enqueued and the host goes on to the vote; the rehearsal shortens the 300 s default of that time-out)
        r = subprocess.run(cmd, env=dict(base, PULPO_BENCH_INJECT_FAILURE=inject, PULPO_BENCH_AGREE_TIMEOUT_S="20"), capture_output=True, text=True,
                           timeout=900, cwd=root)
        assert r.returncode == 0, (inject, r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, (inject, r.stdout[-1500:])
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2 and d["value"] > 0
        if expect is not None:
            assert expect in r.stderr, (inject, r.stderr[-3000:])
        # a record produced on the fallback path says so (it would otherwise look like a healthy overlapped run)
        assert d["stepper"]["fallback"] == fallback, (inject, d["stepper"])
        assert d["stepper"]["overlap"] is (fallback == "none") and d["stepper"]["async_wgrad"] is (fallback == "none"), (inject, d["stepper"])
        assert d["dist"]["world"] == 2 and d["dist"]["backend"] == "gloo"


def test_bench_json_contract_single_gpu():
    """the one JSON line bench.py --full prints (driver contract): every required key, the roofline and cpu_baseline objects, and the
    arithmetic value = pairs / time - on a small workload so that the CPU-baseline leg takes seconds"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "32", "32", "32",
                        "--levels", "3", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "loop", "loops_ms_per_step", "stepper", "dist", "hbm_rooflines"):
        assert k in d, k
    assert d["loop"] == "stepper" and set(d["loops_ms_per_step"]) == {"stepper", "lightning-hooks", "plain-autograd"}
    assert d["stepper"]["fallback"] == "none" and d["dist"]["world"] == 1 and d["dist"]["backend"] is None
    for cls in ("bn_lrelu_apply", "warp3d_fwd", "warp3d_bwd", "vecint_fwd", "vecint_bwd", "ncc_fwd", "ncc_bwd", "heads_fwd", "adam_step", "kl_fwd", "l2reg_fwd"):
        assert cls in d["hbm_rooflines"], cls          # per-class HBM fractions of the memory-bound kernels
        assert d["hbm_rooflines"][cls]["bound"] == "hbm" and d["hbm_rooflines"][cls]["achieved"] > 0
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["unit"] == "volume-pairs/s" and d["dtype"] == "f32" and "workload" in d["config"]
    assert abs(d["value"] - 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and rf["achieved"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1
    assert d["value"] > cb["value"]
    assert d["full"] is True


def test_bench_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """a plain bench.py run (no --full) is the timed steps alone: no brackets, no extra steps, no CPU baseline in the line.  --dump-outputs
    writes the last timed step's loss, updated parameters and gradients in float32.  That step starts from the seeded weights and a fresh
    optimizer, so two runs with the same arguments write the same numbers: the loss bit for bit (the forward pass has no atomics), the
    gradients to the rounding of the backward pass's float atomics, the parameters to Adam's first update of it - lr * g / (|g| + eps) turns
    the rounding noise of a gradient that is zero in exact arithmetic (conv biases in front of a BatchNorm) into up to +-lr.  In deterministic
    mode the files are identical.  --mode infer writes what predict_deterministic returned."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(out, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "32", "32", "32",
                            "--levels", "3", "2", "--dump-outputs", str(tmp_path / out)] + list(extra), capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    def load(out):
        names = sorted(os.listdir(tmp_path / out))
        assert names == ["grads.npy", "loss.npy", "params.npy"], names
        d = {n[:-4]: np.load(tmp_path / out / n) for n in names}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
        assert sum(a.nbytes for a in d.values()) <= 64 << 20
        return d

    d = run("a")
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert d["unit"] == "volume-pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    for k in ("roofline", "cpu_baseline", "loops_ms_per_step", "hbm_rooflines", "time_split"):
        assert d[k] is None, k
    assert d["conv_kernels"] == {} and d["deterministic"]["ms_per_step_deterministic_mode"] is None
    run("b")
    a, b = load("a"), load("b")
    assert np.array_equal(a["loss"], b["loss"])
    g = np.abs(a["grads"]).max()
    assert g > 0 and np.abs(a["grads"] - b["grads"]).max() <= 1e-5 * g
    assert np.linalg.norm(a["grads"] - b["grads"]) <= 1e-5 * np.linalg.norm(a["grads"])
    assert np.abs(a["params"] - b["params"]).max() <= 2.5e-4                     # 2 lr (lr = 1e-4) and float32 rounding
    assert np.linalg.norm(a["params"] - b["params"]) <= 1e-3 * np.linalg.norm(a["params"])
    run("d1", "--deterministic")
    run("d2", "--deterministic")
    d1, d2 = load("d1"), load("d2")
    for k in d1:
        assert np.array_equal(d1[k], d2[k]), k
    run("c", "--mode", "infer")
    inf = sorted(os.listdir(tmp_path / "c"))
    assert inf and all(n.startswith("out_infer_") for n in inf), inf
    assert all(np.load(tmp_path / "c" / n).dtype == np.float32 for n in inf)


def test_training_resumes_bit_identically_from_a_checkpoint(api, tmp_path):
    """checkpoint / resume: model.state_dict() + FusedAdam.state_dict() saved after two steps and loaded into a fresh model + stepper
    reproduce the third step's weights (forward is deterministic; the weight-gradient atomics reorder and Adam normalises, so compare at 2e-5)"""
    models, nb = api
    from pulpo_amd import dp

    def make():
        torch.manual_seed(0)
        m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=4).cuda().train()
        g = torch.Generator().manual_seed(4)
        for l in range(2):
            s_ = 16 // 2 ** (l + 1)
            m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, s_, s_, s_, generator=g).cuda())
        return m

    gen = torch.Generator().manual_seed(8)
    e = torch.empty((0,), device="cuda")
    batch = (torch.rand(1, 1, 16, 16, 16, generator=gen).cuda(), torch.rand(1, 1, 16, 16, 16, generator=gen).cuda(), e, e, e, e, e, e)
    a = make()
    sa = dp.DataParallelStepper(a, lr=1e-3)
    sa.step(batch); sa.step(batch)
    torch.save({"model": a.state_dict(), "opt": sa.opt.state_dict()}, tmp_path / "ckpt.pt")
    sa.step(batch)
    b = make()
    ck = torch.load(tmp_path / "ckpt.pt", weights_only=False)
    b.load_state_dict(ck["model"])
    sb = dp.DataParallelStepper(b, lr=1e-3)
    sb.opt.load_state_dict(ck["opt"])
    assert sb.opt.t == 2
    sb.step(batch)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            continue        # conv bias in front of a BatchNorm: its gradient is rounding noise, which Adam turns into +-lr steps (in the reference too)
        assert float((pa - pb).abs().max()) <= 2e-5 * max(1.0, float(pa.abs().max())), k
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        if ba.is_floating_point():
            assert float((ba - bb).abs().max()) <= 1e-4 * max(1.0, float(ba.abs().max())), k
        else:
            assert torch.equal(ba, bb), k
    # the optimizer state is in torch.optim.Adam's layout: it loads into the reference's optimizer (configure_optimizers, models.py:398-400)
    # and comes back from it unchanged, whatever the arena's internal bucket order
    c = make()
    topt = c.configure_optimizers()
    topt.load_state_dict({k: v for k, v in ck["opt"].items() if k != "param_names"})
    back = topt.state_dict()
    names = [n for n, _ in c.named_parameters()]
    assert ck["opt"]["param_names"] == names
    sc = dp.DataParallelStepper(make(), lr=1e-3)
    assert [id(p) for p in sc.arena.params] != [id(p) for p in sc.arena.module_order]          # the arena really is permuted
    sc.opt.load_state_dict(back)                                # torch layout, no names: matched by index
    assert sc.opt.t == 2
    again = sc.opt.state_dict()
    for i, n in enumerate(names):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(again["state"][i][key].cpu(), ck["opt"]["state"][i][key].cpu()), (n, key)
            assert tuple(again["state"][i][key].shape) == tuple(dict(c.named_parameters())[n].shape)
    bad = {"state": dict(back["state"]), "param_groups": [dict(back["param_groups"][0], params=back["param_groups"][0]["params"][:-1])]}
    with pytest.raises(ValueError):
        sc.opt.load_state_dict(bad)


def _grads_of_one_step(model, x, y):
    for p in model.parameters():
        p.grad = None
    outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y)
    total.backward()
    torch.cuda.synchronize()
    return float(total), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("size,T_L,n0", [([32, 32, 32], (3, 2), 8), ([160, 160, 160], (5, 4), 32)])
def test_deterministic_mode_gives_bit_identical_gradients(api, size, T_L, n0):
    """PULPO_DETERMINISTIC / ops.set_deterministic(True): the weight-gradient flushes (ordered per-split slabs), the VecInt / warp backward
    scatter (64-bit fixed point) and the generic resize backward (gather) replace the float atomics - two evaluations of the same training step
    on the same weights, inputs and noise give BIT-identical losses and parameter gradients, as the reference's CPU backward does,
    at 32^3 and at the metric's 160^3.  The plain mode is held to the deterministic one at 1e-5 relative L2 (atomic order only)."""
    models, nb = api
    from pulpo_amd import ops
    import os
    torch.manual_seed(0)
    model = models.PULPo(T_L[0], T_L[1], 0.1, size, feedback=FB, n0=n0).cuda().train()
    gen = torch.Generator().manual_seed(5)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    for l in range(T_L[1]):
        shape = [s_ // 2 ** (l + (T_L[0] - T_L[1])) for s_ in size]
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(torch.randn(1, 3, *shape, generator=gen).cuda())
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    env_det = os.environ.get("PULPO_DETERMINISTIC", "0") == "1"
    try:
        ops.set_deterministic(True)
        runs = []
        for _ in range(3):
            model.load_state_dict(state)                # (BatchNorm running statistics move with every training forward)
            runs.append(_grads_of_one_step(model, x, y))
        for loss_b, grads_b in runs[1:]:
            assert loss_b == runs[0][0]
            assert grads_b.keys() == runs[0][1].keys()
            for k, g in grads_b.items():
                assert torch.equal(g, runs[0][1][k]), (k, float((g - runs[0][1][k]).abs().max()))
        ops.set_deterministic(False)
        model.load_state_dict(state)
        loss_p, grads_p = _grads_of_one_step(model, x, y)
        assert loss_p == runs[0][0]                      # (the forward pass has no atomics in either mode)
        moved = 0
        for k, g in grads_p.items():
            ref = runs[0][1][k]
            if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
                continue                                 # (true gradient zero in front of a BatchNorm: pure rounding noise on both sides)
            assert rel_l2(g, ref) < 1e-5, (k, rel_l2(g, ref))
            moved += int(not torch.equal(g, ref))
        print(f"{size[0]}^3: {moved} of {len(grads_p)} parameter gradients differ in their last bits between the atomic and the deterministic mode")
    finally:
        ops.set_deterministic(env_det)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_step_equals_the_eager_step(api, precision):
    """dp.DataParallelStepper(graph=True): zero_grad + forward + backward + gradient finishing captured into one HIP graph (third step) and replayed;
    Adam and the weight re-pack stay eager.  With fixed noise the losses of the first six steps equal the eager stepper's on the same weights and
    batch (bit for bit in fp32 up to the float atomics of the gradients that feed the updates: 1e-5), the batch is read from the static copies
    (a NEW batch tensor changes the result), and the parameters end up where the eager loop puts them."""
    models, nb = api
    from pulpo_amd import dp, ops
    size, Tl, L, n0 = [32, 32, 32], 3, 2, 8
    gen = torch.Generator().manual_seed(3)
    batches = [tuple([torch.rand(1, 1, *size, generator=gen).cuda() for _ in range(2)] + [torch.empty((0,), device="cuda")] * 6) for _ in range(2)]
    eps = [torch.randn(1, 3, *[s_ // 2 ** (l + 1) for s_ in size], generator=gen).cuda() for l in range(L)]

    def run(graph):
        torch.manual_seed(0)
        model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0).cuda().train()
        for l in range(L):
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        st = dp.DataParallelStepper(model, graph=graph)
        losses = [float(st.step(batches[i % 2])) for i in range(6)]
        assert (st._graph is not None) == graph
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    if precision == "bf16":
        ops.set_conv_precision("bf16", activations="bf16")
    try:
        eager, sd_e = run(False)
        graphed, sd_g = run(True)
    finally:
        ops.set_conv_precision("fp32")
    np.testing.assert_allclose(graphed, eager, rtol=1e-4 if precision == "fp32" else 5e-3)       # (float-atomic noise of five updates)
    assert abs(eager[0] - eager[1]) > 1e-6 * abs(eager[0])          # (the two batches do differ: the replay really reads the step's batch)
    for k, v in sd_e.items():
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            # a conv bias in front of a BatchNorm: its true gradient is zero, what Adam normalises to +-lr per step is rounding noise (float atomics)
            assert float((sd_g[k] - v).abs().max()) <= 6 * 2e-4, k
        elif k.endswith("running_mean"):
            # ... and the batch mean of that unit's convolution carries the bias one to one (momentum 0.1 per step)
            assert float((sd_g[k] - v).abs().max()) <= 2e-3 * max(1.0, float(v.abs().max())), k
        elif v.is_floating_point():
            tol = (1e-4 if precision == "fp32" else 5e-3)
            assert float((sd_g[k] - v).abs().max()) <= tol * max(1.0, float(v.abs().max())), k
        else:
            assert torch.equal(sd_g[k], v), k


@pytest.mark.parametrize("switch", ["prewritten_cat", "skip_unused_activations", "pooled_bn_backward", "fuse_input_wgrad", "blocked_dy", "blocked_z"])
def test_round5_fusions_equal_the_separate_passes(api, switch):
    """Each round-5 shortcut of the step switched OFF gives the same training step as the shipped default: concatenation buffers written in place
    (ops.cat_channels), activations nobody reads not written (DownPath `_needed`), the gradient of a pooled ConvUnit output formed inside the
    BatchNorm-backward passes (ops.POOLED_BN_BACKWARD), the input layer's BatchNorm backward inside its weight gradient (ops.FUSE_INPUT_WGRAD), the
    gradient of the pre-norm tensors in the channel-blocked layout where the F(2x2x2,3x3x3) kernels read it (ops.BLOCKED_DY), the activations between
    the units of a ConvSequence and their gradients in that layout (ops.BLOCKED_Z).
    n0 = 16 at 64^3 / T3 / L2 so that the channel counts take the in-place buffers (multiples of 8) and the kernels of the large levels run.
    Loss bit-equal (the forward pass computes the same values), every parameter gradient within 1e-5 (summation order of fp32 partial sums)."""
    models, nb = api
    from pulpo_amd import ops
    size, Tl, L, n0 = [64, 64, 64], 3, 2, 16
    gen = torch.Generator().manual_seed(11)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    eps = [torch.randn(1, 3, *[s_ // 2 ** (l + 1) for s_ in size], generator=gen).cuda() for l in range(L)]

    def run(off):
        torch.manual_seed(0)
        model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0).cuda().train()
        for l in range(L):
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        if off == "prewritten_cat":
            model.downpath._pulpo_skip_room = {}
        if off == "skip_unused_activations":
            model._needed_levels = None
        saved = (ops.POOLED_BN_BACKWARD, ops.FUSE_INPUT_WGRAD, ops.BLOCKED_DY, ops.BLOCKED_Z)
        try:
            if off == "blocked_z":                  # (an opt-in: this one is switched ON against the default)
                ops.BLOCKED_Z = True
            if off == "blocked_dy":
                ops.BLOCKED_DY = False
            if off == "pooled_bn_backward":
                ops.POOLED_BN_BACKWARD = False
            if off == "fuse_input_wgrad":
                ops.FUSE_INPUT_WGRAD = False
            outs, _, (total, kl, rec, reg), _ = model._forward_and_losses(x, y)
            total.backward()
            torch.cuda.synchronize()
        finally:
            ops.POOLED_BN_BACKWARD, ops.FUSE_INPUT_WGRAD, ops.BLOCKED_DY, ops.BLOCKED_Z = saved
        used = hasattr(outs[0][0], "shape")
        assert used
        return float(total), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}, model

    hits0, blk0, blz0 = ops.CAT_PREWRITTEN_HITS, ops.BLOCKED_DY_HITS, ops.BLOCKED_Z_HITS
    loss_on, g_on, m_on = run(None)
    blk1, blz1 = ops.BLOCKED_DY_HITS, ops.BLOCKED_Z_HITS
    assert blk1 > blk0, "no ConvUnit of the 64^3 level took the channel-blocked gradient"
    assert blz1 == blz0, "blocked activations are an opt-in"
    assert getattr(m_on.downpath, "_pulpo_skip_room", None), "the in-place concatenation buffers are not armed"
    assert ops.CAT_PREWRITTEN_HITS == hits0 + (L - 1), "the encoders' concatenations did not take the in-place buffers"
    hits1 = ops.CAT_PREWRITTEN_HITS
    loss_off, g_off, _ = run(switch)
    assert (ops.CAT_PREWRITTEN_HITS == hits1) == (switch == "prewritten_cat")
    assert (ops.BLOCKED_DY_HITS == blk1) == (switch == "blocked_dy")
    assert (ops.BLOCKED_Z_HITS > blz1) == (switch == "blocked_z"), "no ConvUnit of the 64^3 level handed a channel-blocked activation to the next one"
    assert loss_on == loss_off
    assert g_on.keys() == g_off.keys()
    for k, g in g_on.items():
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            wscale = float(g_off[k[:-4] + "weight"].abs().max())
            assert float((g - g_off[k]).abs().max()) <= 1e-3 * max(wscale, 1e-3), k          # (true gradient zero: rounding noise on both sides)
            continue
        assert rel_l2(g, g_off[k]) < 1e-5, (k, rel_l2(g, g_off[k]))


def test_two_differentiable_passes_over_one_downpath_call(api):
    """several samples from ONE DownPath call with gradients enabled (user code may do that): the second Autoencoder pass must not write its feedback
    path into the concatenation buffer the first pass's backward still reads - it falls back to plain tensors.  Gradients of loss_1 + loss_2 equal
    the sum of two independent evaluations."""
    models, nb = api
    from pulpo_amd import ops
    size, Tl, L, n0 = [32, 32, 32], 3, 2, 16
    gen = torch.Generator().manual_seed(2)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    eps = [[torch.randn(1, 3, *[s_ // 2 ** (l + 1) for s_ in size], generator=gen).cuda() for l in range(L)] for _ in range(2)]
    torch.manual_seed(0)
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0).cuda().train()
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def set_eps(i):
        for l in range(L):
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[i][l])

    def zero():
        for p in model.parameters():
            p.grad = None

    # reference: two independent forward / backward evaluations, gradients added
    ref = None
    for i in range(2):
        model.load_state_dict(state); zero(); set_eps(i)
        out = model.autoencoder(x, model.downpath(x, y))
        (out[7][0].sum() + out[6][1].sum()).backward()
        g = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        ref = g if ref is None else {k: ref[k] + g[k] for k in g}
    # one DownPath call, two Autoencoder passes, one backward
    model.load_state_dict(state); zero()
    hits0 = ops.CAT_PREWRITTEN_HITS
    down = model.downpath(x, y)
    total = 0.0
    for i in range(2):
        set_eps(i)
        out = model.autoencoder(x, down)
        total = total + out[7][0].sum() + out[6][1].sum()
    assert ops.CAT_PREWRITTEN_HITS == hits0 + (L - 1)          # (the first pass took the in-place buffers, the second did not)
    total.backward()
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        if k.startswith("downpath.") or (k.endswith("_op.0.bias") and "velocity_field._op.2" not in k):
            continue          # (DownPath ran once here and twice in the reference: its BatchNorm statistics moved differently; pre-norm biases are noise)
        assert rel_l2(p.grad, ref[k]) < 2e-4, (k, rel_l2(p.grad, ref[k]))
