"""Loss stack of PULPo on HIP kernels, with the reference's public names (src/losses.py).

On the hot path (BASELINE configs: recon_loss=['ncc'], regularizer='L2', diagonal KL):
    KL_two_gauss_with_diag_cov (:47-76), NCC_loss (:85-135), L2_reg (:208-222) and the three Hierarchical*
    wrappers (:225-355).
Alternative hyper-parameters / evaluation metrics, also on HIP kernels (metrics.hip):
    L2_loss (:79-83, `--recon_loss mse`), Soft_dice_loss (:137-145, `--recon_loss dice`), jacobian_det (:172-199),
    JDetStd (:202-204, `--regularizer jdet`) - the 3-D forms.
KL_nondiagonal (:8-44, `--nondiagonal`) likewise.  2-D inputs (train.py --ndims 2) run the reference's 2-D forms through the same
kernels as depth-1 volumes.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import ops


def _off_path(name: str):
    raise NotImplementedError(
        f"{name} is outside the MI355X hot path built so far (SURVEY.md §8(f)); the BASELINE configurations "
        "use recon_loss=['ncc'], regularizer='L2' and the diagonal KL.")


class KL_nondiagonal:
    """KL against a prior with a non-diagonal (graph-Laplacian) precision, reference losses.py:8-44: the degree matrix is
    computed inside the kernel instead of being materialised."""

    def __init__(self, inshape, prior_lambda=20) -> None:
        self.prior_lambda = prior_lambda
        self.inshape = [int(s) for s in inshape]
        self.ndims = len(self.inshape)
        if self.ndims not in (2, 3):
            _off_path("KL_nondiagonal (ndims %d)" % self.ndims)

    def loss(self, prior_mean, prior_sigma, flow_mean, flow_sigma):
        return ops.kl_nondiagonal(flow_mean, flow_sigma, self.prior_lambda)


def L2_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """spatial sum of squared differences, mean over batch and channels (reference losses.py:79-83)"""
    return ops.l2_loss(input, target)


def L2_loss_masked(input: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, mask2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """L2_loss with the per-voxel cost weighted by m = mask * mask2 ((B,1,...) weights in [0,1], 1 = counted) and normalised by the
    mask's volume: V * sum(m d^2) / (C * sum(m)), 0 for an empty mask"""
    return ops.l2_loss_masked(input, target, mask, mask2)


def Soft_dice_loss(input: torch.Tensor, target: torch.Tensor, dice_factor=1) -> torch.Tensor:
    """mean over (batch, channel) of (1 - soft dice), times voxels / dice_factor (reference losses.py:137-145)"""
    return ops.soft_dice_loss(input, target, dice_factor)


def jacobian_det(deformation_field: torch.Tensor, lamb=None, normalize=True) -> torch.Tensor:
    """(B,3,D,H,W) -> (B,D,H,W) Jacobian determinant (reference losses.py:172-199); the 2-D form has no HIP path"""
    if deformation_field.dim() not in (4, 5):
        _off_path("jacobian_det")
    return ops.jacobian_det(deformation_field, normalize)


def JDetStd(deformation_field: torch.Tensor, lamb=0, normalize=True) -> torch.Tensor:
    """lamb * std of the Jacobian determinant (reference losses.py:202-204), differentiable"""
    if deformation_field.dim() not in (4, 5):
        _off_path("JDetStd")
    return ops.jdet_std(deformation_field, lamb, normalize)


def _is_std_normal(mu1, sigma1) -> bool:
    return getattr(mu1, "_pulpo_std_normal", False) and getattr(sigma1, "_pulpo_std_normal", False)


def KL_two_gauss_with_diag_cov(mu0: torch.Tensor, sigma0: torch.Tensor, mu1: torch.Tensor, sigma1: torch.Tensor, eps: float = 1e-10) -> torch.Tensor:
    """KL[p0 || p1] for diagonal Gaussians: sum over features, mean over the batch.  eps is fixed at the reference's 1e-10."""
    if eps != 1e-10:
        raise NotImplementedError("KL_two_gauss_with_diag_cov: the HIP kernel uses the reference's eps = 1e-10")
    if _is_std_normal(mu1, sigma1):
        return ops.kl_diag(mu0, sigma0, None, None)
    return ops.kl_diag(mu0, sigma0, mu1, sigma1)


def NCC_loss(y_pred: torch.Tensor, y_true: torch.Tensor, win_size: int = 9, gamma: float = 0.05) -> torch.Tensor:
    """-gamma * sum_voxels mean_batch(local squared NCC) with a win_size^3 zero-padded window"""
    if y_pred.dim() not in (4, 5):
        raise NotImplementedError("NCC_loss: volumes (B,1,D,H,W) or slices (B,1,H,W) expected")
    return ops.ncc_loss(y_pred, y_true, win_size, gamma)


def NCC_loss_masked(y_pred: torch.Tensor, y_true: torch.Tensor, mask: torch.Tensor, mask2: Optional[torch.Tensor] = None, win_size: int = 9,
                    gamma: float = 0.05) -> torch.Tensor:
    """NCC_loss with cost-function masking: -gamma * V * sum(m cc) / sum(m), m = mask * mask2, 0 for an empty mask.  The window sums run
    over all voxels; the mask weights the per-voxel cost"""
    if y_pred.dim() not in (4, 5):
        raise NotImplementedError("NCC_loss_masked: volumes (B,1,D,H,W) or slices (B,1,H,W) expected")
    return ops.ncc_loss_masked(y_pred, y_true, mask, mask2, win_size, gamma)


def MIND_loss(y_pred: torch.Tensor, y_true: torch.Tensor, dilation: int = 2, eps: float = 1e-5) -> torch.Tensor:
    """MIND-SSC similarity between two contrasts: sum over voxels, mean over the batch of the squared difference of the 12-channel
    self-similarity descriptors (mean over the channels) - on L2_loss's scale.  3-D volumes only"""
    return ops.mind_loss(y_pred, y_true, dilation, eps)


def MIND_loss_masked(y_pred: torch.Tensor, y_true: torch.Tensor, mask: torch.Tensor, mask2: Optional[torch.Tensor] = None, dilation: int = 2,
                     eps: float = 1e-5) -> torch.Tensor:
    """MIND_loss with cost-function masking: V * sum(m cost) / sum(m), m = mask * mask2, 0 for an empty mask.  The descriptors are formed
    from all voxels; the mask weights the per-voxel cost (DESIGN.md sections 3i, 3j)"""
    return ops.mind_loss_masked(y_pred, y_true, mask, mask2, dilation, eps)


def MI_loss(y_pred: torch.Tensor, y_true: torch.Tensor, bins: int = 32, gamma: float = 0.05) -> torch.Tensor:
    """-gamma * V * mean_batch(MI): Mattes mutual information over a bins x bins cubic-B-spline Parzen joint histogram of images in [0,1]
    (values outside are clamped), on NCC_loss's scale.  Volumes (B,1,D,H,W) or slices (B,1,H,W)"""
    return ops.mi_loss(y_pred, y_true, bins, gamma)


def MI_loss_masked(y_pred: torch.Tensor, y_true: torch.Tensor, mask: torch.Tensor, mask2: Optional[torch.Tensor] = None, bins: int = 32,
                   gamma: float = 0.05) -> torch.Tensor:
    """MI_loss with cost-function masking: every voxel enters the joint histogram with the weight m = mask * mask2, and the histogram is
    normalised by sum(m); 0 for an empty mask (DESIGN.md sections 3i, 3r)"""
    return ops.mi_loss_masked(y_pred, y_true, mask, mask2, bins, gamma)


def L2_reg(deformation_field: torch.Tensor, lamb=0) -> torch.Tensor:
    """lamb * H*W*D * mean of squared forward differences over the [1:,1:,1:] block"""
    if deformation_field.dim() not in (4, 5):
        raise NotImplementedError("L2_reg: fields (B,3,D,H,W) or (B,2,H,W) expected")
    return ops.l2_reg(deformation_field, lamb)


def Bending_reg(deformation_field: torch.Tensor, lamb=0) -> torch.Tensor:
    """lamb * H*W*D * mean over the interior voxels of the bending-energy density u_xx^2 + u_yy^2 + u_zz^2 + 2 u_xy^2 + 2 u_xz^2 + 2 u_yz^2
    (central differences; no counterpart in the reference): L2_reg's scale, nothing charged for an affine field"""
    if deformation_field.dim() not in (4, 5):
        raise NotImplementedError("Bending_reg: fields (B,3,D,H,W) or (B,2,H,W) expected")
    return ops.bending_reg(deformation_field, lamb)


def _apply_pyramid(weight_dict: Dict[int, float], similarity_pyramid: bool) -> Dict[int, float]:
    if similarity_pyramid:                      # in place, like the reference (losses.py:238-240)
        for l in weight_dict.keys():
            weight_dict[l] = weight_dict[l] / 2 ** l
    return weight_dict


def _weighted(weight_dict: Dict[int, float], terms: Dict[int, torch.Tensor], scale=None):
    """(sum_l w_l * term_l, {l: w_l * term_l}) - losses.py:262-276 / 305-325 / 343-355.  Device scalars: one kernel for the whole sum
    (ops.weighted_sum, bit-identical to the reference's per-level mul / add chain); anything else: that chain itself."""
    levels = list(weight_dict.keys())
    vals = [terms[l] for l in levels]
    if all(isinstance(v, torch.Tensor) and v.is_cuda and v.numel() == 1 and v.dtype == torch.float32 for v in vals):
        total, per_level = ops.weighted_sum(vals, [weight_dict[l] for l in levels], scale)
        return total, dict(zip(levels, per_level))
    total, all_levels = 0.0, {}
    for l in levels:
        all_levels[l] = weight_dict[l] * terms[l]
        total = total + all_levels[l]
    if scale is not None:
        total = total * scale
        all_levels = {l: scale * v for l, v in all_levels.items()}
    return total, all_levels


def _weighted_pair(weight_dict: Dict[int, float], terms: Dict[int, torch.Tensor], terms_inv: Dict[int, torch.Tensor]):
    """(1/2 sum_l w_l (term_l + term_inv_l), {l: w_l / 2 * (term_l + term_inv_l)}): the two directions of a bidirectional loss (DESIGN.md
    section 3u).  Device scalars: all 2 L products and their sum in one ops.weighted_sum launch, a level's entry the sum of its two."""
    levels = list(weight_dict.keys())
    vals = [t[l] for l in levels for t in (terms, terms_inv)]
    if all(isinstance(v, torch.Tensor) and v.is_cuda and v.numel() == 1 and v.dtype == torch.float32 for v in vals):
        total, per = ops.weighted_sum(vals, [weight_dict[l] / 2 for l in levels for _ in range(2)])
        return total, {l: per[2 * i] + per[2 * i + 1] for i, l in enumerate(levels)}
    total, all_levels = 0.0, {}
    for l in levels:
        all_levels[l] = weight_dict[l] / 2 * terms[l] + weight_dict[l] / 2 * terms_inv[l]
        total = total + all_levels[l]
    return total, all_levels


class HierarchicalKLLoss(nn.Module):
    """sum_l w_l * KL_l; also returns the per-level terms (losses.py:225-276)"""

    def __init__(self, KL_divergence, weight_dict: Dict[int, float], similarity_pyramid: bool, level_sizes: Dict[int, torch.Tensor] = None) -> None:
        super().__init__()
        self.weight_dict = _apply_pyramid(weight_dict, similarity_pyramid)
        self.KL_divergence = KL_divergence
        if KL_divergence == KL_nondiagonal:          # one instance per level (reference losses.py:242-243)
            self.KL_divergence = {key: KL_nondiagonal(inshape=level_sizes[key]).loss for key in level_sizes.keys()}

    def forward(self, prior_mus, prior_sigmas, posterior_mus, posterior_sigmas, scale=None):
        """scale (not in the reference's signature; models.py applies `* beta` to the results, :161-162): folded into the same launch"""
        assert self.weight_dict.keys() == prior_mus.keys()
        assert prior_mus.keys() == prior_sigmas.keys() == posterior_mus.keys() == posterior_sigmas.keys()
        terms = {}
        for l in self.weight_dict:
            if isinstance(self.KL_divergence, dict):   # argument order of the reference for the non-diagonal class (losses.py:267-269)
                terms[l] = self.KL_divergence[l](prior_mus[l], prior_sigmas[l], posterior_mus[l], posterior_sigmas[l])
            else:
                terms[l] = self.KL_divergence(posterior_mus[l], posterior_sigmas[l], prior_mus[l], prior_sigmas[l])
        return _weighted(self.weight_dict, terms, scale)


class HierarchicalReconstructionLoss(nn.Module):
    """sum_l w_l * recon(y_hat_l, y resized to level l) / len(recon_loss)   (losses.py:279-325)"""

    mi_bins = 32        # joint-histogram bins of the "mi" term; set on the instance to change them (model.hierarchical_recon_loss.mi_bins = 16)

    def __init__(self, recon_loss: List[str], weight_dict: Dict[int, float], similarity_pyramid: bool, ndims: int, window_size: Dict[int, float],
                 mind_dilation: int = 2, mind_eps: float = 1e-5) -> None:
        super().__init__()
        self.recon_loss = recon_loss
        self.mind_dilation, self.mind_eps = mind_dilation, mind_eps
        self.weight_dict = _apply_pyramid(weight_dict, similarity_pyramid)
        self.window_size = window_size
        self.ndims = ndims
        self.mode = "trilinear" if ndims == 3 else "bilinear"

    def _level_term(self, l, w, fast, y_hat, y, y_hat_seg, seg_y, gamma, dice_factor, masks, dice_terms):
        """one direction's term of level l: the bare similarity on the single-term fast path, else the w-weighted sum of the listed terms"""
        size = y_hat[l].shape[2:]
        # F.interpolate(y, size) of the reference; the identity resize at full resolution is skipped
        y_target = y if tuple(size) == tuple(y.shape[2:]) else ops.resize_trilinear(y, size)
        ma, mb = (masks.get(l) if masks is not None else None) or (None, None)
        how = dict(win=self.window_size[l], gamma=gamma, dilation=self.mind_dilation, eps=self.mind_eps, bins=self.mi_bins)
        if fast:
            return ops.similarity(self.recon_loss[0], y_hat[l], y_target, ma, mb, **how)
        term = 0.0
        for kind in ("mse", "ncc", "mind", "mi"):
            if kind in self.recon_loss:
                term = term + w * ops.similarity(kind, y_hat[l], y_target, ma, mb, **how)
        if "dice" in self.recon_loss and dice_terms is not None:
            term = term + w * dice_terms[l]
        elif "dice" in self.recon_loss:
            seg_size = y_hat_seg[l].shape[2:]
            seg_target = seg_y if tuple(seg_size) == tuple(seg_y.shape[2:]) else ops.resize_trilinear(seg_y, seg_size)
            term = term + w * Soft_dice_loss(y_hat_seg[l], seg_target, dice_factor=dice_factor)
        return term

    def forward(self, y_hat, y, y_hat_seg=None, seg_y=None, gamma: float = 0.05, dice_factor: int = 1,
                masks: Optional[Dict[int, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]]] = None,
                dice_terms: Optional[Dict[int, torch.Tensor]] = None, inverse: Optional[dict] = None):
        """masks (not in the reference): {level: (mask_a, mask_b)}, weight volumes at the level's size, either of a pair may be None; a level
        with a pair uses the masked NCC / MSE / MIND / MI term (cost weighted by mask_a * mask_b), the Dice term is unchanged.
        dice_terms (not in the reference): {level: the level's Dice term}, computed by the caller (PULPo.label_dice_terms, from label maps);
        dice_terms[l] stands in for Soft_dice_loss(y_hat_seg[l], ...), and y_hat_seg / seg_y are not read.
        inverse (not in the reference; bidirectional training): the same arguments for the inverse direction, a dict
        with "y_hat" and "y" (the fixed image under the inverse fields, and the moving image it is compared with) and optionally
        "y_hat_seg", "seg_y", "masks", "dice_terms".  The result is then half the sum of the two directions, level by level."""
        single = len(self.recon_loss) == 1 and self.recon_loss[0] in ("mse", "ncc", "dice", "mind", "mi")
        fast = single and self.recon_loss[0] != "dice"      # one term per level (the default, ["ncc"]): weighting and summation of all levels in one launch; x / 1 is x
        loss = 0.0
        all_levels, terms, terms_inv = {}, {}, {}
        for l, w in self.weight_dict.items():
            term = self._level_term(l, w, fast, y_hat, y, y_hat_seg, seg_y, gamma, dice_factor, masks, dice_terms)
            if inverse is not None:
                term_inv = self._level_term(l, w, fast, inverse["y_hat"], inverse["y"], inverse.get("y_hat_seg"), inverse.get("seg_y"), gamma,
                                            dice_factor, inverse.get("masks"), inverse.get("dice_terms"))
            if fast:
                terms[l] = term
                if inverse is not None:
                    terms_inv[l] = term_inv
                continue
            all_levels[l] = term / len(self.recon_loss) if inverse is None else (term + term_inv) / (2 * len(self.recon_loss))
            loss = loss + all_levels[l]
        if terms_inv:
            return _weighted_pair(self.weight_dict, terms, terms_inv)
        if terms:
            return _weighted(self.weight_dict, terms)
        return loss, all_levels


class HierarchicalRegularization(nn.Module):
    """sum_l w_l * regularizer(df_l, lamb)   (losses.py:327-355)"""

    def __init__(self, regularizer, weight_dict: Dict[int, float], similarity_pyramid: bool) -> None:
        super().__init__()
        self.regularizer = regularizer
        self.weight_dict = _apply_pyramid(weight_dict, similarity_pyramid)

    def forward(self, dfs: Dict[int, torch.Tensor], lamb: float = 0, dfs_inv: Optional[Dict[int, torch.Tensor]] = None):
        """dfs_inv (not in the reference; bidirectional training): the inverse fields; given, the result is half the sum over both"""
        assert self.weight_dict.keys() == dfs.keys()
        if dfs_inv is not None:
            assert dfs_inv.keys() == dfs.keys()
            return _weighted_pair(self.weight_dict, {l: self.regularizer(dfs[l], lamb) for l in self.weight_dict},
                                  {l: self.regularizer(dfs_inv[l], lamb) for l in self.weight_dict})
        return _weighted(self.weight_dict, {l: self.regularizer(dfs[l], lamb) for l in self.weight_dict})
