"""The deterministic half of the reference's evaluation harness on the device: `Evaluate.performance` (evaluate.py:1379-1498), the per
latent level RMSE, JDetStd, JDetLeq0, Dice, LM_MAE and LM_Euclid of `predict_deterministic`, and the naive baseline of
`Evaluate.performance_affine` (evaluate.py:1190-1204).  `uncertainty.mc_uncertainty` + `uncertainty_scores` are the Monte-Carlo half.

    scores = performance(model, x, y, seg_x=..., seg_y=..., lm_x=..., lm_y=..., num_classes=...)     # evaluate.py:1423-1474 for one pair
    table.add(k, j, scores)                                                                            # evaluate.py:1476-1478, no host sync
    data, (sets, mets) = table.mean()                                                                  # evaluate.py:1480-1488

The two field-quality rows come from one pass over each level's field (ops.field_quality: no determinant map), the Dice row from one
fused pass per level over the field and the two full-resolution label maps (ops.warp_labels_soft_dice: no one-hot tensor, neither the
warped one nor the resized target).  Pandas, LaTeX and plots stay with the caller.  Evaluation only: no autograd, GPU tensors only."""
from __future__ import annotations

import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import affine as affine_mod
from . import eval_metrics, ops
from .uncertainty import _as_labels

METRICS = ("RMSE", "JDetStd", "JDetLeq0", "Dice", "LM_MAE", "LM_Euclid")
# the rows level_scores adds when it is given the inverse fields (no counterpart in the reference, which has no inverse transform)
INVERSE_METRICS = ("InvCons", "InvConsMax", "LM_MAE_inv", "LM_Euclid_inv")
# the rows level_scores adds when it is given the fixed image under the inverse fields: the scores of the inverse direction
INVERSE_IMAGE_METRICS = ("RMSE_inv", "Dice_inv")
# the rows level_scores adds when it is given cost-function masks
MASK_METRICS = ("RMSE_masked", "MaskFrac")
# the row level_scores adds with mind=True: the cross-contrast counterpart of RMSE, which means nothing between contrasts
MIND_METRICS = ("MIND",)
# the rows level_scores adds with surface=True: the boundary metrics beside Dice, in voxels
SURFACE_METRICS = ("HD95", "ASSD")
# the row level_scores adds with bending=True: the second-order smoothness of the field beside JDetStd
BENDING_METRICS = ("BendingE",)
# the row level_scores adds with mi=True: mutual information between the warped and the fixed image, higher is better
MI_METRICS = ("MI",)


def _zero(ref: torch.Tensor) -> torch.Tensor:
    return torch.zeros((), device=ref.device, dtype=torch.float32)


@torch.no_grad()
def level_scores(outputs: Dict[int, torch.Tensor], final_dfs: Dict[int, torch.Tensor], y: torch.Tensor, *, seg_x: Optional[torch.Tensor] = None,
                 seg_y: Optional[torch.Tensor] = None, lm_x: Optional[torch.Tensor] = None, lm_y: Optional[torch.Tensor] = None,
                 num_classes: Optional[int] = None, final_dfs_inv: Optional[Dict[int, torch.Tensor]] = None,
                 mask_x: Optional[torch.Tensor] = None, mask_y: Optional[torch.Tensor] = None, mind: bool = False, mind_dilation: int = 2,
                 mind_eps: float = 1e-5, surface: bool = False, include_background: bool = False,
                 bending: bool = False, mi: bool = False, mi_bins: int = 32, outputs_inv: Optional[Dict[int, torch.Tensor]] = None,
                 inverse_fields: Optional[Dict[int, torch.Tensor]] = None, x: Optional[torch.Tensor] = None) -> Dict[str, Dict[int, torch.Tensor]]:
    """The level losses of evaluate.py:1433-1474 for one pair: {metric: {level: 0-d device tensor}}.

    outputs[l], final_dfs[l]: the warped image and the final field of level l (predict_deterministic + combine_dfs); y: the fixed image.
      RMSE[l]      sqrt(L2_loss(outputs[l], y resized to the level) / num_pixels_l)                       (evaluate.py:1437-1438)
      JDetStd[l]   unbiased std of jacobian_det(final_dfs[l])      = HierarchicalRegularization(JDetStd)(final_dfs, lamb=1)   (:1441)
      JDetLeq0[l]  100 * count(jacobian_det(final_dfs[l]) <= 0) / numel                                   (:1444-1448)
    seg_x and seg_y (label maps (B, 1, ...) uint8 / int32 / int64 with num_classes, or the reference's float one-hot maps), both at full
    resolution, add
      Dice[l]      1 - Soft_dice_loss(spatial_transform(final_dfs[l], seg_x), seg_y resized to the level) / num_pixels_l   (:1427, 1454-1455)
    lm_x and lm_y (1, n, ndims) add
      LM_MAE / LM_Euclid: lm_mae / lm_euclid(warp_landmarks(lm_x, final_dfs[0]), lm_y) at level 0, the reference's 0 at the levels above
      and, for empty landmark tensors, at level 0 too (:1457-1474).
    Without segmentations or landmarks their rows are absent (the reference stores 0: PerformanceTable fills rows that were not added with 0).
    final_dfs_inv[l] (the inverse fields of model.combine_dfs_bidirectional) adds, beside the rows above, which do not change,
      InvCons[l] / InvConsMax[l]   mean / maximum over the voxels of ||inv(p) + fwd(p + inv(p))||_2 in voxels (ops.inverse_consistency)
      LM_MAE_inv / LM_Euclid_inv   with landmarks: lm_mae / lm_euclid(transport_landmarks(lm_x, final_dfs_inv[0]), lm_y) at level 0, the
                                   landmarks carried by the inverse field sampled at their own positions; 0 where LM_MAE / LM_Euclid are.
    mask_x and / or mask_y (weight volumes (B,1,...) in [0,1] at full resolution, 1 = counted; no counterpart in the reference) add,
    beside the rows above, which do not change, with m_l = warp_mask(final_dfs[l], mask_x) * (mask_y resized to the level), the level masks
    of the training step (PULPo.level_masks),
      RMSE_masked[l]   sqrt(sum(m_l (outputs[l] - target)^2) / (C sum(m_l))), 0 for an empty m_l      (ops.rmse_masked)
      MaskFrac[l]      mean of m_l
    mind=True (3-D only; no counterpart in the reference) adds, beside the rows above, which do not change,
      MIND[l]          mean over batch, voxels and the 12 channels of the squared difference of the MIND-SSC descriptors of outputs[l] and
                       the target = mind_loss(outputs[l], target, mind_dilation, mind_eps) / num_pixels_l
    surface=True (needs the segmentations; no counterpart in the reference) adds, beside the rows above, which do not change, at every level
    whose field lies on seg_y's own grid (level 0, and every level under df_resolution="full_res"), from
    ops.surface_distances(ops.warp_labels(final_dfs[l], seg_x, argmax=True), seg_y), in voxels,
      HD95[l]          mean over the batch and the classes present in both maps of the 95th-percentile Hausdorff distance
      ASSD[l]          the same mean of the average symmetric surface distance
    class 0 is left out unless include_background; 0 when no class qualifies and at the other levels (PerformanceTable reads 0 as missing).
    bending=True (no counterpart in the reference) adds, beside the rows above, which do not change,
      BendingE[l]      mean over batch, components and interior voxels of the bending-energy density of final_dfs[l], in voxels^2
                       = losses.Bending_reg(final_dfs[l], 1) / num_pixels_l; 0 for an affine field (every extent of a level at least 3).
    mi=True (no counterpart in the reference) adds, beside the rows above, which do not change,
      MI[l]            mean over the batch of the mutual information of outputs[l] and the target over mi_bins x mi_bins Parzen bins
                       (ops.joint_histogram; images in [0,1]); higher is better.
    outputs_inv[l], inverse_fields[l] and x (the fixed image under the inverse field of level l, that field, and the moving image: what
    bidirectional training compares; no counterpart in the reference) add, beside the rows above, which do not change,
      RMSE_inv[l]      ops.rmse(outputs_inv[l], x resized to the level): RMSE's quantity for the inverse direction
      Dice_inv[l]      with segmentations: the Dice row with the maps exchanged, ops.warp_labels_soft_dice(inverse_fields[l], seg_y, C, seg_x)."""
    levels = sorted(outputs.keys())
    if sorted(final_dfs.keys()) != levels:
        raise ValueError(f"level_scores: outputs has levels {levels}, final_dfs {sorted(final_dfs.keys())}")
    if (seg_x is None) != (seg_y is None):
        raise ValueError("level_scores: seg_x and seg_y go together")
    if (lm_x is None) != (lm_y is None):
        raise ValueError("level_scores: lm_x and lm_y go together")
    if surface and seg_x is None:
        raise ValueError("level_scores: surface=True needs seg_x and seg_y")
    if final_dfs_inv is not None and sorted(final_dfs_inv.keys()) != levels:
        raise ValueError(f"level_scores: outputs has levels {levels}, final_dfs_inv {sorted(final_dfs_inv.keys())}")
    res: Dict[str, Dict[int, torch.Tensor]] = {"RMSE": {}, "JDetStd": {}, "JDetLeq0": {}}
    for l in levels:
        out = outputs[l]
        size = tuple(out.shape[2:])
        target = y if size == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)          # F.interpolate(y, size), skipped at equal size
        num_pixels = float(np.prod(size))
        res["RMSE"][l] = torch.sqrt(ops.l2_loss(out, target) / num_pixels)
        _, res["JDetStd"][l], res["JDetLeq0"][l] = ops.field_quality(final_dfs[l], True)
    if mask_x is not None or mask_y is not None:
        res["RMSE_masked"], res["MaskFrac"] = {}, {}
        for l in levels:
            size = tuple(outputs[l].shape[2:])
            target = y if size == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)
            wx = ops.warp_mask(final_dfs[l], mask_x) if mask_x is not None else None
            wy = None if mask_y is None else (mask_y.float() if size == tuple(mask_y.shape[2:]) else ops.resize_trilinear(mask_y.float(), size))
            pair = (wx, wy) if wx is not None else (wy, None)
            res["RMSE_masked"][l], res["MaskFrac"][l] = ops.rmse_masked(outputs[l], target, pair[0], pair[1])
    if mind:
        res["MIND"] = {}
        for l in levels:
            size = tuple(outputs[l].shape[2:])
            target = y if size == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)
            res["MIND"][l] = ops.mind_loss(outputs[l], target, mind_dilation, mind_eps) / float(np.prod(size))
    if mi:
        res["MI"] = {}
        for l in levels:
            size = tuple(outputs[l].shape[2:])
            target = y if size == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)
            res["MI"][l] = ops.joint_histogram(outputs[l], target, mi_bins)[1].mean().float()
    if bending:
        res["BendingE"] = {l: ops.bending_reg(final_dfs[l], 1.0) / float(np.prod(final_dfs[l].shape[2:])) for l in levels}
    if seg_x is not None:
        lab_x, C = _as_labels(seg_x, num_classes, "level_scores")
        lab_y, _ = _as_labels(seg_y, C, "level_scores")
        res["Dice"] = {l: ops.warp_labels_soft_dice(final_dfs[l], lab_x, C, lab_y)[1] for l in levels}
        if surface:
            res["HD95"] = {l: _zero(y) for l in levels}
            res["ASSD"] = {l: _zero(y) for l in levels}
            first = 0 if include_background else 1
            for l in levels:
                if tuple(final_dfs[l].shape[2:]) != tuple(lab_y.shape[2:]):
                    continue
                # both maps passed the Dice row's range check and the arg-max writes classes only: no further host read
                warped = ops._warp_labels(final_dfs[l], lab_x, C, None, False, True, False)
                sd = ops._surface_distances(warped, lab_y, C, 95.0, False, False)
                for name, key in (("HD95", "hd_pct"), ("ASSD", "assd")):
                    v = sd[key][:, first:]
                    ok = ~torch.isnan(v)
                    res[name][l] = torch.where(ok, v, torch.zeros_like(v)).sum() / ok.sum().clamp(min=1)
    if lm_x is not None:
        res["LM_MAE"] = {l: _zero(y) for l in levels}
        res["LM_Euclid"] = {l: _zero(y) for l in levels}
        if lm_x.numel() and lm_y.numel():
            moved = ops.warp_landmarks(lm_x, final_dfs[0])
            ref = lm_y.to(device=moved.device, dtype=moved.dtype)
            res["LM_MAE"][0] = eval_metrics.lm_mae(moved, ref)
            res["LM_Euclid"][0] = eval_metrics.lm_euclid(moved, ref)
    if outputs_inv is not None:
        if inverse_fields is None or x is None or sorted(outputs_inv.keys()) != levels or sorted(inverse_fields.keys()) != levels:
            raise ValueError(f"level_scores: outputs_inv goes with inverse_fields and x, on the levels {levels}")
        res["RMSE_inv"] = {}
        for l in levels:
            size = tuple(outputs_inv[l].shape[2:])
            res["RMSE_inv"][l] = ops.rmse(outputs_inv[l], x if size == tuple(x.shape[2:]) else ops.resize_trilinear(x, size))
        if seg_x is not None:
            res["Dice_inv"] = {l: ops.warp_labels_soft_dice(inverse_fields[l], lab_y, C, lab_x)[1] for l in levels}
    if final_dfs_inv is not None:
        res["InvCons"], res["InvConsMax"] = {}, {}
        for l in levels:
            res["InvCons"][l], res["InvConsMax"][l] = ops.inverse_consistency(final_dfs[l], final_dfs_inv[l])
        if lm_x is not None:
            res["LM_MAE_inv"] = {l: _zero(y) for l in levels}
            res["LM_Euclid_inv"] = {l: _zero(y) for l in levels}
            if lm_x.numel() and lm_y.numel():
                moved = eval_metrics.transport_landmarks(lm_x, final_dfs_inv[0])
                ref = lm_y.to(device=moved.device, dtype=moved.dtype)
                res["LM_MAE_inv"][0] = eval_metrics.lm_mae(moved, ref)
                res["LM_Euclid_inv"][0] = eval_metrics.lm_euclid(moved, ref)
    return res


@torch.no_grad()
def performance(model, x: torch.Tensor, y: torch.Tensor, *, seg_x: Optional[torch.Tensor] = None, seg_y: Optional[torch.Tensor] = None,
                lm_x: Optional[torch.Tensor] = None, lm_y: Optional[torch.Tensor] = None,
                num_classes: Optional[int] = None, inverse: bool = False, mask_x: Optional[torch.Tensor] = None,
                mask_y: Optional[torch.Tensor] = None, mind: bool = False, mind_dilation: int = 2,
                mind_eps: float = 1e-5, refine: Optional[Dict[str, object]] = None, surface: bool = False,
                include_background: bool = False, affine=None, bending: bool = False, mi: bool = False,
                mi_bins: int = 32, interpolation: str = "linear", inverse_image: bool = False) -> Dict[str, Dict[int, torch.Tensor]]:
    """evaluate.py:1423-1474 for one pair (x, y): model.predict_deterministic, model.combine_dfs, level_scores.  The model's mode is the
    caller's (evaluate.py:100 puts it in eval mode).  As in the reference, the deterministic prediction decodes mu at every level, but the
    feedback to the level above still carries `samples` (pulpo.py:202), a draw of the level's sampler: two calls differ in the last digits
    unless the samplers are pinned (network_blocks.FixedNoiseSampler).  inverse=True also integrates the inverse fields
    (model.combine_dfs_bidirectional: one integration call per level for both directions) and adds the INVERSE_METRICS rows; mask_x / mask_y
    add the MASK_METRICS rows, mind=True the MIND_METRICS row, surface=True (with segmentations) the SURFACE_METRICS rows, bending=True the
    BENDING_METRICS row (of the refined and of the affine-composed fields where those are scored, like JDetStd), mi=True the MI_METRICS row
    over mi_bins bins.  refine (a dict of pulpo_amd.refine.refine's keyword arguments, {} for its
    defaults; no counterpart in the reference): the same rows for the fields of model.refine(x, y, **refine) instead of the prediction's
    (DESIGN.md section 3k); the masks given here score, they reach the refinement only through the dict.
    affine (no counterpart in the reference): None - the pair is taken as affinely aligned, today's path; a (B,3,4)
    ((B,2,3) for slices) tensor theta in voxels of x's grid, or a dict of pulpo_amd.affine.fit's keyword arguments ({} for its defaults) that
    fits one.  The model (and a refinement) then sees ops.affine_warp(theta, x), and every row that reads a field reads
    ops.affine_compose(theta, final_dfs[l], x's size) - "affine first, deformable second" as one field - together with the ORIGINAL seg_x /
    lm_x / mask_x: one interpolation carries them through both transforms.  With inverse=True it raises NotImplementedError (the inverse of
    the composition is not built).
    interpolation: "linear" - the trilinear outputs, today's path; "cubic" - the image rows (RMSE, RMSE_masked, MIND, MI)
    are scored on cubic B-spline outputs (model.predict_deterministic / model.refine with interpolation="cubic"; a refinement then descends on
    the cubic image model too, unless its dict names an interpolation of its own).  With affine= the ORIGINAL x goes once through
    ops.warp3d_cubic under the composed field: one interpolation, as for the segmentations.  Segmentation, landmark and field rows do not
    depend on it; masks and label maps stay on their own samplers.  Cubic outputs may leave x's range by overshoot (the MI row clamps).
    inverse_image=True adds the INVERSE_IMAGE_METRICS rows: y warped by the inverse fields
    (model.combine_dfs_bidirectional) against x, and seg_y carried by them against seg_x - what a model trained with bidirectional=True is
    trained on.  It does not add the INVERSE_METRICS rows (inverse=True does); with affine= it raises NotImplementedError like inverse=True."""
    ops.check_interpolation(interpolation, "performance")
    final_dfs_inv = None
    if surface and seg_x is None:
        raise ValueError("performance: surface=True needs seg_x and seg_y")
    theta = None
    if affine is not None:
        if inverse_image:
            raise NotImplementedError("performance: inverse_image=True together with affine= (the inverse of the composed transform) is not implemented")
        if inverse:
            raise NotImplementedError("performance: inverse=True together with affine= (the inverse of the composed transform) is not implemented")
        theta = affine_mod.fit(x, y, **affine)["theta"] if isinstance(affine, dict) else affine
        x_original, x = x, ops.affine_warp(theta, x)
    if refine is not None:
        res = model.refine(x, y, **(refine if interpolation == "linear" else {"interpolation": interpolation, **refine}))
        outputs, individual_dfs, final_dfs = res["outputs"], res["individual_dfs"], res["final_dfs"]
        if inverse or inverse_image:
            _, final_dfs, final_dfs_inv = model.combine_dfs_bidirectional(individual_dfs)
    else:
        outputs, individual_dfs = model.predict_deterministic(x, y) if interpolation == "linear" else \
            model.predict_deterministic(x, y, interpolation=interpolation)
        if inverse or inverse_image:
            _, final_dfs, final_dfs_inv = model.combine_dfs_bidirectional(individual_dfs)
        else:
            _, final_dfs = model.combine_dfs(individual_dfs)
    if theta is not None:
        final_dfs = {l: ops.affine_compose(theta, df, x.shape[2:]) for l, df in final_dfs.items()}
        if interpolation == "cubic":                    # affine and deformable in one cubic resample of the original image
            coef = ops.bspline_prefilter(x_original)
            outputs = {l: ops.warp3d_cubic(df, coef=coef) for l, df in final_dfs.items()}
    inv_image = {}
    if inverse_image:
        inv_image = dict(outputs_inv=model._resample(interpolation, final_dfs_inv, y), inverse_fields=final_dfs_inv, x=x)
    return level_scores(outputs, final_dfs, y, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, lm_y=lm_y, num_classes=num_classes,
                        final_dfs_inv=final_dfs_inv if inverse else None,
                        mask_x=mask_x, mask_y=mask_y, mind=mind, mind_dilation=mind_dilation, mind_eps=mind_eps,
                        surface=surface, include_background=include_background, bending=bending, mi=mi, mi_bins=mi_bins, **inv_image)


@torch.no_grad()
def affine_scores(x: torch.Tensor, y: torch.Tensor, seg_x: Optional[torch.Tensor] = None, seg_y: Optional[torch.Tensor] = None,
                  lm_x: Optional[torch.Tensor] = None, lm_y: Optional[torch.Tensor] = None, theta: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The naive baseline of Evaluate.performance_affine (evaluate.py:1190-1204), the scores of the unregistered pair: RMSE = rmse(x, y);
    with (one-hot or soft) segmentation maps Dice = dsc(seg_x, seg_y); with landmarks LM_MAE / LM_Euclid of the unwarped landmarks.
    theta ((B,3,4) in voxels of x's grid, (B,2,3) for slices): the scores of the affinely aligned pair instead - x and
    the channels of seg_x under ops.affine_warp(theta, .), the landmarks under warp_landmarks by ops.affine_field(theta)."""
    if theta is not None:
        x = ops.affine_warp(theta, x)
        if seg_x is not None and seg_y is not None:
            seg_x = ops.affine_warp(theta, seg_x.float())
        if lm_x is not None and lm_y is not None and lm_x.numel():
            lm_x = ops.warp_landmarks(lm_x, ops.affine_field(theta, x.shape[2:])[:1])
    res = {"RMSE": eval_metrics.rmse(x, y)}
    if seg_x is not None and seg_y is not None:
        res["Dice"] = eval_metrics.dsc(seg_x, seg_y)
    if lm_x is not None and lm_y is not None:
        ref = lm_y.to(device=lm_x.device, dtype=lm_x.dtype)
        res["LM_MAE"] = eval_metrics.lm_mae(lm_x, ref)
        res["LM_Euclid"] = eval_metrics.lm_euclid(lm_x, ref)
    return res


class PerformanceTable:
    """The all_metrics array of Evaluate.performance (evaluate.py:1388, 1476-1488) kept on the device: add() stores one pair's scalars
    without a host synchronisation, mean() makes one device -> host transfer and applies the reference's aggregation - entries that are
    exactly 0 (a metric the pair does not have, a level without landmarks, an input slot a shorter loader never filled) are missing."""

    def __init__(self, metric_names: Sequence[str], latent_levels: int, loader_names: Sequence[str], num_inputs: int) -> None:
        self.metric_names, self.loader_names = list(metric_names), list(loader_names)
        self.latent_levels, self.num_inputs = int(latent_levels), int(num_inputs)
        if not self.metric_names or not self.loader_names or self.latent_levels < 1 or self.num_inputs < 1:
            raise ValueError("PerformanceTable: at least one metric, level, loader and input")
        self._values = None               # [metrics, levels, datasets, inputs] on the device of the first score

    def add(self, k: int, j: int, scores: Dict[str, Dict[int, torch.Tensor]]) -> None:
        """loader k, input j: scores as level_scores / performance return them; a metric of the table that is absent from scores stays 0"""
        if not (0 <= k < len(self.loader_names) and 0 <= j < self.num_inputs):
            raise IndexError(f"PerformanceTable.add: loader {k}, input {j} outside ({len(self.loader_names)}, {self.num_inputs})")
        unknown = set(scores) - set(self.metric_names)
        if unknown:
            raise KeyError(f"PerformanceTable.add: metrics {sorted(unknown)} are not in the table ({self.metric_names})")
        for h, name in enumerate(self.metric_names):
            for l, v in scores.get(name, {}).items():
                if not 0 <= l < self.latent_levels:
                    raise IndexError(f"PerformanceTable.add: level {l} of {name} outside {self.latent_levels} levels")
                v = torch.as_tensor(v).detach().reshape(())
                if self._values is None:
                    self._values = torch.zeros((len(self.metric_names), self.latent_levels, len(self.loader_names), self.num_inputs),
                                               device=v.device, dtype=torch.float64)
                self._values[h, l, k, j] = v                       # a device-side copy of one scalar: nothing waits for it

    def mean(self) -> Tuple[np.ndarray, Tuple[np.ndarray, np.ndarray]]:
        """([levels, datasets x metrics] array, (sets, mets) column labels): zeros -> NaN, nanmean over the inputs, columns ordered as
        evaluate.py:1483-1488 (np.repeat(loader_names, num_metrics), np.tile(metric_names, num_datasets))"""
        shape = (len(self.metric_names), self.latent_levels, len(self.loader_names), self.num_inputs)
        all_metrics = np.zeros(shape, dtype=float) if self._values is None else self._values.cpu().numpy()        # the one transfer
        all_metrics = all_metrics.copy()
        all_metrics[all_metrics == 0] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)                      # "Mean of empty slice": an all-missing cell is NaN
            mean_metrics = np.nanmean(all_metrics, axis=-1)
        data = np.concatenate(mean_metrics.T, axis=1)
        sets = np.repeat(self.loader_names, len(self.metric_names))
        mets = np.tile(self.metric_names, len(self.loader_names))
        return data, (sets, mets)
