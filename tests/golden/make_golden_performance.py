#!/usr/bin/env python3
"""Generate tests/golden/performance_T3L2_n4_16.npz: the per-level scores of Evaluate.performance from the REAL reference.

evaluate.py itself cannot be imported where the fixtures are made (seaborn, torchvision and h5py are absent), so the sequence of
evaluate.py:1423-1474 is run here on the reference's own classes - PULPo (src/models.py, behind make_golden's plumbing-only stand-ins),
HierarchicalReconstructionLoss, HierarchicalRegularization, JDetStd, jacobian_det (src/losses.py) and SpatialTransformer
(src/network_blocks.py) - with the three one-line methods of evaluate.py restated inline, as gen_evalmetrics does for rmse / dsc:
    lm_mae         evaluate.py:355-366   torch.median(torch.abs(lm1 - lm2).sum(dim=2))
    lm_euclid      evaluate.py:368-379   torch.mean(torch.sqrt(((lm1 - lm2) ** 2).sum(dim=2)))
    warp_landmarks evaluate.py:410-423   = src/components/utils.py:15-25, imported from there

Case A (keys a.*): the reference PULPo (T3 / L2, n0 = 4, 16^3) with the sd0.* state of step_T3L2_n4_16.npz, eval mode, on x[:1], y[:1] of
    that fixture, the latent noise that fixture's eps.* (it reaches level 0 through the `samples` feedback even in the deterministic
    prediction), 5-class uint8 label maps and 6 landmarks.
Case B (keys b.*): synthetic outputs / final fields at 16^3 (level 0) and 8^3 (level 1); the fields are coarse random fields of amplitude 3
    (level 1: 4) interpolated up, so that folding occurs (the recipe of tests/test_gpu_performance.py).  The reference's determinant maps are stored
    for the near-zero allowance of the JDetLeq0 comparison.

usage:  python tests/golden/make_golden_performance.py   (writes next to itself; only data goes into the .npz)
"""
import contextlib
import io

import make_golden as mg           # noqa: F401  (sets sys.path to the reference and checks that `src` resolves there)
from make_golden import F, HERE, ls, nb, np, npy, os, save, torch

METRICS = ["RMSE", "JDetStd", "JDetLeq0", "Dice", "LM_MAE", "LM_Euclid"]
C = 5


def lm_mae(lm1, lm2):
    return torch.median(torch.abs(lm1 - lm2).sum(dim=2))


def lm_euclid(lm1, lm2):
    return torch.mean(torch.sqrt(((lm1 - lm2) ** 2).sum(dim=2)))


def one_hot(lab):
    return F.one_hot(lab[:, 0].long(), C).permute(0, 4, 1, 2, 3).float().contiguous()


def level_losses(outputs, final_dfs, transformers, y, seg_x, seg_y, lm_x, lm_y, L):
    """evaluate.py:1426-1474 with all six metrics, segmentations and landmarks present; returns ({metric: {l: tensor}}, {l: jdet map})"""
    import src.components.utils as cu
    ones = lambda: {l: 1.0 for l in range(L)}
    hierarchical_mse = ls.HierarchicalReconstructionLoss(["mse"], ones(), similarity_pyramid=False, ndims=3, window_size=ones())
    hierarchical_jdet_std = ls.HierarchicalRegularization(ls.JDetStd, ones(), similarity_pyramid=False)
    hierarchical_dice = ls.HierarchicalReconstructionLoss(["dice"], ones(), similarity_pyramid=False, ndims=3, window_size=ones())
    pred_segs = {key: transformers[key](final_dfs[key], seg_x) for key in range(L)}
    num_pixels = {l: torch.prod(torch.tensor(outputs[l].size()[2:])) for l in range(L)}
    res, jdets = {}, {}
    _, level_mse = hierarchical_mse(y_hat=outputs, y=y, y_hat_seg=pred_segs, seg_y=seg_y, gamma=1, dice_factor=1)
    res["RMSE"] = {key: torch.sqrt(level_mse[key] / num_pixels[key]) for key in level_mse.keys()}
    _, res["JDetStd"] = hierarchical_jdet_std(final_dfs, lamb=1)
    res["JDetLeq0"] = {}
    for key in range(L):
        jdet = ls.jacobian_det(final_dfs[key])
        jdets[key] = jdet
        res["JDetLeq0"][key] = (torch.sum(jdet <= 0) / torch.prod(torch.tensor(jdet.squeeze().size()))) * 100
    _, level_dice = hierarchical_dice(y_hat=outputs, y=y, y_hat_seg=pred_segs, seg_y=seg_y, gamma=1, dice_factor=1)
    res["Dice"] = {key: 1 - (level_dice[key] / num_pixels[key]) for key in level_dice.keys()}
    res["LM_MAE"] = {key: torch.tensor(0.0) for key in range(L)}
    res["LM_Euclid"] = {key: torch.tensor(0.0) for key in range(L)}
    res["LM_MAE"][0] = lm_mae(cu.warp_landmarks(lm_x, final_dfs[0]).detach(), lm_y)
    res["LM_Euclid"][0] = lm_euclid(cu.warp_landmarks(lm_x, final_dfs[0]).detach(), lm_y)
    return res, jdets


def folded_field(B, grid, gen, amplitude=3.0):
    c = (torch.rand(B, len(grid), *[max(2, s // 3) for s in grid], generator=gen) * 2 - 1) * amplitude
    return F.interpolate(c, size=grid, mode="trilinear", align_corners=False)


def main():
    with np.load(os.path.join(HERE, "step_T3L2_n4_16.npz")) as z:
        step = {k: z[k] for k in z.files}
    Tl, L, n0, _, *size = [int(v) for v in step["cfg"]]
    gen = torch.Generator().manual_seed(230)
    seg_x = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8)
    seg_y = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8)
    lm_x = torch.stack([torch.randint(0, s, (6,), generator=gen) for s in size], dim=-1)[None].float()
    lm_y = (lm_x + 1.5 * torch.randn(lm_x.shape, generator=gen)).clamp(0, min(size) - 1)
    out = {"cfg": np.array([Tl, L, n0, C] + size, dtype=np.int64), "metrics": np.array(METRICS), "seg_x": npy(seg_x), "seg_y": npy(seg_y),
           "lm_x": npy(lm_x), "lm_y": npy(lm_y)}
    ohx, ohy = one_hot(seg_x), one_hot(seg_y)

    # ---- case A: the reference's PULPo, evaluate.py:1423-1424
    rm = mg._import_reference_models()
    with contextlib.redirect_stdout(io.StringIO()):
        model = rm.PULPo(Tl, L, 0.1, list(size), feedback=list(mg.FEEDBACK), n0=n0)
    sd = model.state_dict()
    loaded = set()
    for k, v in step.items():
        if k.startswith("sd0."):
            assert k[4:] in sd, k
            sd[k[4:]] = torch.from_numpy(v.copy())
            loaded.add(k[4:])
    assert all(k.endswith(".grid") for k in set(sd) - loaded), sorted(set(sd) - loaded)
    model.load_state_dict(sd, strict=True)
    model.eval()
    # predict_deterministic decodes mu, but the feedback to the level above carries `samples` (pulpo.py:202), a draw of the level's
    # sampler: the noise is pinned to the fixture's eps.* (first batch row), the seam make_golden's set_eps uses
    for l in range(L):
        model.autoencoder.encoders[l].sampler = (lambda mu, sigma, e=torch.from_numpy(step[f"eps.{l}"])[:1]: mu + sigma * e)
    x, y = torch.from_numpy(step["x"])[:1], torch.from_numpy(step["y"])[:1]
    with torch.no_grad():
        outputs, individual_dfs = model.predict_deterministic(x, y)
        _, final_dfs = model.combine_dfs(individual_dfs)
        transformers = {key: model.autoencoder.decoders[key].spatial_transform for key in range(L)}
        res, jdets = level_losses(outputs, final_dfs, transformers, y, ohx, ohy, lm_x, lm_y, L)
    for m in METRICS:
        out["a." + m] = np.array([float(res[m][l]) for l in range(L)], dtype=np.float64)
    for l in range(L):
        out[f"a.jdet.{l}"] = npy(jdets[l])

    # ---- case B: synthetic outputs and folded fields
    gb = torch.Generator().manual_seed(231)
    grids = {0: tuple(size), 1: tuple(s // 2 for s in size)}
    yb = torch.rand(1, 1, *size, generator=gb)
    outs_b = {l: torch.rand(1, 1, *grids[l], generator=gb) for l in grids}
    amplitude = {0: 3.0, 1: 4.0}        # 8^3 comes from a 2^3 coarse field: amplitude 3 folds no voxel there, 4 folds 2.3 %
    dfs_b = {l: folded_field(1, grids[l], gb, amplitude[l]) for l in grids}
    with torch.no_grad():
        res, jdets = level_losses(outs_b, dfs_b, {l: nb.SpatialTransformer(grids[l]) for l in grids}, yb, ohx, ohy, lm_x, lm_y, len(grids))
    for l in grids:
        assert 1.0 < float(res["JDetLeq0"][l]) < 99.0, (l, float(res["JDetLeq0"][l]))
        out[f"b.outputs.{l}"], out[f"b.final_dfs.{l}"], out[f"b.jdet.{l}"] = npy(outs_b[l]), npy(dfs_b[l]), npy(jdets[l])
    out["b.y"] = npy(yb)
    for m in METRICS:
        out["b." + m] = np.array([float(res[m][l]) for l in grids], dtype=np.float64)
    save("performance_T3L2_n4_16", **out)
    for case in "ab":
        for m in METRICS:
            print("  %s.%-10s" % (case, m), out[f"{case}.{m}"])


if __name__ == "__main__":
    main()
