"""Monte-Carlo uncertainty of a registration (BASELINE config 5: "8-sample MC"), as `Evaluate` computes it in the reference
(evaluate.py:222-251, 3-D branch): `num_samples` stochastic `model.predict(x, y, N=1)` passes, the mean individual fields ->
combined / final fields -> warped image, and per-voxel sample standard deviations of the warped image, the individual and the
final fields (mean over the channel axis).  The reference stores every sample ((N, C, D, H, W) per level and quantity); here each
sample is folded into running moments by one streaming kernel, so memory does not grow with N.
The reference has no dropout: the randomness is the latent sampling.

With segmentations and landmarks (keyword extras of mc_uncertainty) the dictionary also carries what Evaluate.uncertainty
(evaluate.py:1500-1576) and the 2-D branch's segmentation warp (:252-274) need - the per-voxel squared error over the samples, every
sample's warped landmarks, the per-class Dice of every sample and the std map of the warped one-hot segmentation - still without storing
a sample: segmentations are warped as label maps by one fused kernel per sample and level (ops.LabelMoments);
uncertainty_scores() turns the dictionary into the reference's scalars."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops


def _as_labels(seg: torch.Tensor, num_classes: Optional[int], who: str = "mc_uncertainty") -> Tuple[torch.Tensor, int]:
    """a label map (B, 1, ...) plus its class count, from either a label map (uint8 / int32 / int64, num_classes required) or the
    reference's float one-hot map (B, C, ...), converted once by arg-max"""
    if seg.is_floating_point() and seg.shape[1] > 1:
        if num_classes is not None and num_classes != seg.shape[1]:
            raise ValueError(f"{who}: num_classes {num_classes} differs from the one-hot map's {seg.shape[1]} channels")
        return ops.labels_from_onehot(seg), int(seg.shape[1])
    if num_classes is None:
        raise ValueError(f"{who}: a label-map segmentation needs num_classes")
    if seg.dtype not in (torch.uint8, torch.int32):
        seg = seg.to(torch.int32)
    return seg, int(num_classes)


@torch.no_grad()
def mc_uncertainty(model, x: torch.Tensor, y: torch.Tensor, num_samples: int, mask_x: Optional[torch.Tensor] = None,
                   mean_of_samples: bool = False, *, seg_x: Optional[torch.Tensor] = None, seg_y: Optional[torch.Tensor] = None,
                   lm_x: Optional[torch.Tensor] = None, num_classes: Optional[int] = None) -> Dict[str, Dict[int, torch.Tensor]]:
    """x, y: (1, 1, D, H, W) moving / fixed volumes (evaluate.py runs batch size 1).  Returns the dictionaries of evaluate.py:
    outputs, individual_dfs, combined_dfs, final_dfs (from the sample-mean individual fields) and output_std, individual_df_std,
    final_df_std ((D, H, W) per level; final_df_std is masked by the warped `mask_x` when one is given, evaluate.py:246-249).

    Reference quirk kept by default: evaluate.py:239 averages `individual_dfs` - the dictionary returned by the LAST predict() call,
    over its batch axis of size 1 - not `all_individual_dfs`, so the "average" fields, and everything derived from them, are the
    last sample's.  mean_of_samples=True uses the mean over the N samples (what the comment in the reference says).

    Keyword extras (none given: the keys and values above, nothing else):
      seg_x / seg_y  moving / fixed segmentation, each a label map (1, 1, D, H, W) with num_classes, or the reference's one-hot map
                     (1, C, D, H, W).  Adds warped_seg[l] (1, C, D_l, H_l, W_l: the mean-field warp of seg_x, evaluate.py:270),
                     warped_labels[l] (its arg-max) and seg_std[l] (D_l, H_l, W_l: mean over classes of the per-voxel std over samples of
                     the warped one-hot map, the output_std convention); with seg_y also dice_samples (N, C: per-sample per-class Dice at
                     level 0) and dice (C,: warped_seg[0] against seg_y).
      lm_x           moving landmarks (1, n, 3): adds lm_samples (N, n, 3: every sample's warp_landmarks(lm_x, final[0])) and lm_hat
                     (1, n, 3: warp_landmarks(lm_x, final_dfs[0]), so the same "average" as final_dfs).
    output_mse (D, H, W) = mean over the samples of (output_s - y)^2 at level 0 is added whenever an extra is given (evaluate.py:1535);
    it comes from the output moments, M2 / N + (mean - y)^2."""
    if num_samples < 1:
        raise ValueError("mc_uncertainty: num_samples must be >= 1")
    L = model.latent_levels
    lab_x, C = _as_labels(seg_x, num_classes) if seg_x is not None else (None, None)
    lab_y = _as_labels(seg_y, C if C is not None else num_classes)[0] if seg_y is not None else None
    if lab_y is not None and lab_x is None:
        raise ValueError("mc_uncertainty: seg_y needs seg_x")
    m_seg = {l: ops.LabelMoments(C) for l in range(L)} if lab_x is not None else None
    dice_samples, lm_samples = [], []
    m_out = {l: ops.StreamingMoments() for l in range(L)}
    m_ind = {l: ops.StreamingMoments() for l in range(L)}
    m_fin = {l: ops.StreamingMoments() for l in range(L)}
    individual = None
    # In eval mode the encoder pyramid is a deterministic function of (x, y): BatchNorm uses its running statistics and the latent
    # noise only enters the autoencoder.  evaluate.py recomputes it for every sample; here it is computed once and each sample runs
    # only the stochastic half (identical results, ~40 % less work per sample).  In training mode fall back to model.predict().
    down = model.downpath(x, y) if not model.training else None
    for _ in range(num_samples):
        if down is not None:
            outs = model.autoencoder(x, down)
            individual = outs[4]                               # predict(N=1): the mean over one sample is the sample
            _, final = model.combine_dfs(individual)
            outputs = {l: model.autoencoder.decoders[l].spatial_transform(final[l], x) for l in final}
        else:
            outputs, individual = model.predict(x, y, N=1)
            _, final = model.combine_dfs(individual)
        for l in range(L):
            m_out[l].update(outputs[l])
            m_ind[l].update(individual[l])
            m_fin[l].update(final[l])
            if m_seg is not None:             # one fused pass: the warped one-hot sample folded in, and at level 0 its Dice against seg_y
                d = m_seg[l].update(final[l], lab_x, target=lab_y if l == 0 else None)
                if d is not None:
                    dice_samples.append(d)
        if lm_x is not None:
            lm_samples.append(ops.warp_landmarks(lm_x, final[0]))
    individual_dfs = {l: (m_ind[l].mean() if mean_of_samples else individual[l].mean(dim=0).unsqueeze(0)) for l in range(L)}
    combined_dfs, final_dfs = model.combine_dfs(individual_dfs)
    warp = lambda l, img: model.autoencoder.decoders[l].spatial_transform(final_dfs[l], img)
    outputs = {l: warp(l, x) for l in range(L)}
    res = {"outputs": outputs, "individual_dfs": individual_dfs, "combined_dfs": combined_dfs, "final_dfs": final_dfs,
           "output_std": {l: m_out[l].std_map()[0] for l in range(L)},
           "individual_df_std": {l: m_ind[l].std_map()[0] for l in range(L)}}
    if mask_x is not None:
        res["final_df_std"] = {l: m_fin[l].std_map(scale=warp(l, mask_x))[0] for l in range(L)}
    else:
        res["final_df_std"] = {l: m_fin[l].std_map()[0] for l in range(L)}
    if lab_x is None and lm_x is None:
        return res
    res["output_mse"] = (m_out[0].m2() / m_out[0].count + (m_out[0].mean() - y) ** 2)[0, 0]
    if lab_x is not None:
        res["warped_seg"], res["warped_labels"] = {}, {}
        for l in range(L):
            if l == 0 and lab_y is not None:
                res["warped_seg"][0], res["warped_labels"][0], dice = ops.warp_labels(final_dfs[0], lab_x, C, target=lab_y, onehot=True, argmax=True)
                res["dice"] = dice[0]
            else:
                res["warped_seg"][l], res["warped_labels"][l] = ops.warp_labels(final_dfs[l], lab_x, C, onehot=True, argmax=True)
        res["seg_std"] = {l: m_seg[l].std_map()[0] for l in range(L)}
        if lab_y is not None:
            res["dice_samples"] = torch.cat(dice_samples, dim=0)
    if lm_x is not None:
        res["lm_samples"] = torch.cat(lm_samples, dim=0)
        res["lm_hat"] = ops.warp_landmarks(lm_x, final_dfs[0])
    return res


def _lms_var(lms: torch.Tensor) -> torch.Tensor:
    """Evaluate.lms_var (evaluate.py:381-390): (N, n, 3) -> (n,)"""
    return torch.mean(torch.var(lms, dim=0), dim=-1)


@torch.no_grad()
def uncertainty_scores(res: Dict, lm_y: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """The scalars of Evaluate.uncertainty (evaluate.py:1537-1556) from an mc_uncertainty dictionary with extras:
    Var = mean(output_std[0]^2); NCC = Evaluate.ncc(var map, output_mse) (ops.map_ncc, on the device); with landmarks LM_VAR =
    lms_var(lm_samples).mean() and, given the fixed landmarks lm_y (1, n, 3), LM_NCC = lms_corr(lm_hat, lm_samples, lm_y); with
    segmentations Dice = mean over classes of dice and Dice_std = mean over classes of the std over samples of dice_samples."""
    var = res["output_std"][0] ** 2
    out = {"Var": float(var.mean()), "NCC": float(ops.map_ncc(var, res["output_mse"]))}
    if "lm_samples" in res:
        lms = res["lm_samples"]
        lv = _lms_var(lms)
        out["LM_VAR"] = float(lv.mean())
        if lm_y is not None:
            err = torch.mean((res["lm_hat"] - lm_y.to(device=lms.device, dtype=lms.dtype)) ** 2, dim=-1).flatten()
            v = lv.flatten()
            en = (err - err.mean()) / (err.std() * len(err))
            vn = (v - v.mean()) / v.std()
            out["LM_NCC"] = float((en * vn).sum())          # np.correlate of two equal-length vectors: their dot product
    if "dice" in res:
        out["Dice"] = float(res["dice"].mean())
        if "dice_samples" in res:
            out["Dice_std"] = float(res["dice_samples"].std(dim=0).mean())
    return out
