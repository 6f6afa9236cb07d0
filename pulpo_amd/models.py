"""PULPo LightningModule on the MI355X hot path (drop-in for the reference's src/models.py:24-400).

Same constructor signature, hyper-parameter names, sub-module names (downpath / autoencoder / prior -> identical
state-dict keys), step / predict API and logged metric names as the reference.  Conscious deviations, all outside the
arithmetic:
  * torch.autograd.set_detect_anomaly(True) (reference models.py:50) is NOT switched on: it is a global debug mode.
  * the NaN guard (reference models.py:188-194) looks at the previous step's regularisation terms instead of
    synchronising the stream once per level inside the current step; it trips one step later.
  * image logging (reference models.py:258-308) needs torchvision + a TensorBoard logger and is skipped without them.
"""
from __future__ import annotations

import math
import os
from abc import ABC
from typing import Dict, List, Optional

import torch

from ._lightning import LightningModule
from .components.pulpo import Autoencoder, DownPath, PULPoEncoder, PULPoPrior, SVFDecoder  # noqa: F401  (re-exported like the reference)
from .losses import (Bending_reg, HierarchicalKLLoss, HierarchicalReconstructionLoss, HierarchicalRegularization, JDetStd, KL_nondiagonal,
                     KL_two_gauss_with_diag_cov, L2_reg)
from .network_blocks import DFAdder, ResizeTransform, SpatialTransformer, VecInt, gauss_sampler  # noqa: F401
from . import ops


class _DoneEvent:
    def query(self) -> bool:
        return True


class PULPo(ABC, LightningModule):

    def __init__(
        self,
        total_levels: int,
        latent_levels: int,
        beta: float,
        input_size: List[int],
        lr: float = 1e-4,
        recon_loss: list = ["ncc"],
        dice_factor: int = 1,
        similarity_pyramid: bool = False,
        lamb: float = 0.025,
        gamma: float = 0.05,
        regularizer: str = "L2",
        image_logging_frequency: int = 1000,
        feedback: list = ["samples", "velocity_field", "individual_dfs", "combined_dfs", "final_dfs", "transformed"],
        df_resolution: str = "level_res",
        n0: int = 32,
        segs: bool = False,
        lms: bool = False,
        mask: bool = False,
        nondiagonal: bool = False,
        cp_depth: int = 3,
        num_classes: Optional[int] = None,
        bidirectional: bool = False,
        mind_dilation: int = 2,
        mind_eps: float = 1e-5,
    ) -> None:
        super().__init__()
        self.validation_counter = 0
        self.save_hyperparameters()
        self.segs, self.lms, self.mask = segs, lms, mask
        # train the velocity fields from both sides: x under the flow against y AND y under the inverse flow against x,
        # both fields regularised.  No parameter depends on it: a checkpoint trained one way loads the other way.
        self.bidirectional = bool(bidirectional)
        self.latent_levels = latent_levels
        self.total_levels = total_levels
        self.lk_offset = total_levels - latent_levels
        self.beta = beta
        self.df_resolution = df_resolution
        self.recon_loss = recon_loss
        self.input_size = input_size
        self.ndims = len(input_size)
        self.cp_depth = cp_depth
        self.num_classes = None if num_classes is None else int(num_classes)      # classes of integer segmentation maps (label_dice_terms)
        # floor division here, ceil in Autoencoder.level_sizes: reference quirk (models.py:69 vs pulpo.py:95)
        self.level_sizes = {l: torch.tensor(self.input_size) // (2 ** (l + self.lk_offset)) for l in range(latent_levels)}

        self.df_combiner = DFAdder()
        self.prior = PULPoPrior()
        self.downpath = DownPath(total_levels=total_levels, latent_levels=latent_levels, input_size=input_size, input_channels=2, n0=n0)
        # NB: the shipped default feedback list holds 'velocity_field', which Autoencoder rejects exactly like the
        # reference does; pass 'velocity_fields'.
        self.autoencoder = Autoencoder(sampler=gauss_sampler, decoder="SVF", total_levels=total_levels, latent_levels=latent_levels,
                                       zdim=self.ndims, input_size=input_size, feedback=self.hparams.feedback,
                                       df_resolution=self.hparams.df_resolution, n0=n0, cp_depth=cp_depth)

        # the encoders concatenate the feedback path's output IN FRONT of the DownPath activation of their level (components/pulpo.py): DownPath
        # produces those activations as the tail of the concatenation's buffer, the feedback path writes the head (ops.cat_channels).
        # PULPO_PREWRITTEN_CAT=0: plain torch.cat (A/B switch).
        if os.environ.get("PULPO_PREWRITTEN_CAT", "1") != "0" and self.ndims == 3:
            self.downpath._pulpo_skip_room = {int(k): int(blk._op[-1]._op[0].out_channels) for k, blk in self.autoencoder.up_blocks.items()}

        # the Autoencoder reads down_activations[k] for k >= lk_offset only (components/pulpo.py): the levels above are not materialised
        self._needed_levels = frozenset(range(self.lk_offset, total_levels)) if os.environ.get("PULPO_SKIP_UNUSED_ACTIVATIONS", "1") != "0" else None

        if self.hparams.regularizer == "jdet":
            regularization_loss = JDetStd
        elif self.hparams.regularizer == "L2":
            regularization_loss = L2_reg
        elif self.hparams.regularizer == "bending":             # second order, free for affine fields
            regularization_loss = Bending_reg
            sizes = {l: [int(v) for v in (input_size if df_resolution == "full_res" or l == 0 else self.autoencoder.level_sizes[self.lk_offset + l])]
                     for l in range(latent_levels)}                 # the decoders' output sizes: what final_dfs[l] has
            small = {l: s for l, s in sizes.items() if min(s) < 3}
            if small:
                raise ValueError(f"regularizer 'bending' takes central differences at interior voxels: every extent of a level's field must be at "
                                 f"least 3, but the level sizes are {sizes}")
        else:
            raise ValueError(f"Hyperparameter regularizer is {self.hparams.regularizer}. Not a known option (known: 'L2', 'jdet', 'bending').")

        # NCC window per level and the loss-magnitude equalisation weights (reference models.py:104-123)
        window_size = {l: 1 + 2 * (latent_levels - l) for l in range(latent_levels)}
        if latent_levels == 1:
            window_size = {0: 9}
        scale = {l: (2.0 ** self.ndims) ** l for l in range(latent_levels)}
        kl_w = dict(scale)
        if df_resolution == "full_res":
            rec_w = {l: 1.0 for l in range(latent_levels)}
            reg_w = {l: 1.0 for l in range(latent_levels)}
        else:
            rec_w, reg_w = dict(scale), dict(scale)
            full_to_level0 = 2 ** (self.ndims * self.lk_offset)      # level 0 is evaluated at full resolution
            rec_w[0] = scale[0] / full_to_level0
            reg_w[0] = scale[0] / full_to_level0
        rec_w[0] *= 4
        self.window_size = window_size

        kl_fn = KL_nondiagonal if nondiagonal else KL_two_gauss_with_diag_cov
        self.hierarchical_kl_loss = HierarchicalKLLoss(KL_divergence=kl_fn, weight_dict=kl_w, similarity_pyramid=similarity_pyramid,
                                                       level_sizes=self.level_sizes)
        self.hierarchical_recon_loss = HierarchicalReconstructionLoss(recon_loss=recon_loss, weight_dict=rec_w,
                                                                      similarity_pyramid=similarity_pyramid, window_size=window_size,
                                                                      ndims=self.ndims, mind_dilation=mind_dilation, mind_eps=mind_eps)
        self.hierarchical_regularization = HierarchicalRegularization(regularizer=regularization_loss, weight_dict=reg_w,
                                                                      similarity_pyramid=similarity_pyramid)
        self._pending_nan_probe = None          # (pinned flag, event) of an earlier step's NaN test

    # ------------------------------------------------------------------------------------------------ steps
    @torch.no_grad()
    def level_masks(self, final_dfs, mask_x=None, mask_y=None, force: bool = False):
        """{level: (mask_x warped by the level's field - the warp y_hat[l] gets, in the constant-preserving form of ops.warp_mask -, mask_y
        resized to the level as y is)} for cost-function masking; None unless the model was built with mask=True (the flag governs training
        batches; `force` overrides it: pulpo_amd.refine masks whenever it is given masks) and at least one mask is non-empty"""
        has = lambda m: m is not None and m.numel() > 0
        if not (self.mask or force) or not (has(mask_x) or has(mask_y)):
            return None
        mx = mask_x.float() if has(mask_x) else None
        my = mask_y.float() if has(mask_y) else None
        pairs = {}
        for l, df in final_dfs.items():
            size = tuple(df.shape[2:])
            wx = ops.warp_mask(df, mx) if mx is not None else None
            wy = None if my is None else (my if size == tuple(my.shape[2:]) else ops.resize_trilinear(my, size))
            pairs[l] = (wx, wy)
        return pairs

    def _inverse_terms(self, x, final_dfs_inv, x_hat, seg_x, seg_y, mask_x, mask_y) -> dict:
        """the `inverse` argument of HierarchicalReconstructionLoss: what _forward_and_losses prepares for y_hat against y, with the roles of
        the two images, segmentations and masks exchanged and the inverse fields in place of the forward ones"""
        inverse = {"y_hat": x_hat, "y": x}
        if "dice" in self.hparams.recon_loss and self._label_maps(seg_x, seg_y):
            inverse["dice_terms"] = self.label_dice_terms(final_dfs_inv, seg_y, seg_x)
        elif "dice" in self.hparams.recon_loss:
            inverse["y_hat_seg"], inverse["seg_y"] = self.transform_segmentation(final_dfs_inv, seg_y), seg_x
        masks = self.level_masks(final_dfs_inv, mask_y, mask_x)
        if masks is not None:
            inverse["masks"] = masks
        return inverse

    def _forward_and_losses(self, x, y, seg_x=None, seg_y=None, mask_x=None, mask_y=None):
        acts = self.downpath(x, y, _needed=self._needed_levels)
        if self.bidirectional:
            outs = self.autoencoder(x, acts, y=y)
            final_dfs_inv, x_hat = outs[8:]
        else:
            outs = self.autoencoder(x, acts)
        mus, sigmas, samples, velocity_fields, individual_dfs, combined_dfs, final_dfs, y_hat = outs[:8]
        prior_mus, prior_sigmas = self.prior(mus, sigmas)
        dice_terms = None
        if "dice" in self.hparams.recon_loss and self._label_maps(seg_x, seg_y):
            dice_terms = self.label_dice_terms(final_dfs, seg_x, seg_y)        # integer label maps: no one-hot volume
            y_hat_seg = {k: None for k in final_dfs}
        elif "dice" in self.hparams.recon_loss:
            y_hat_seg = self.transform_segmentation(final_dfs, seg_x)
        else:
            y_hat_seg = {k: None for k in final_dfs}
        kl, kl_levels = self.hierarchical_kl_loss(prior_mus, prior_sigmas, mus, sigmas, scale=self.beta)       # (kl * beta, beta * levels: models.py:161-162)
        masks = self.level_masks(final_dfs, mask_x, mask_y)
        rec, rec_levels = self.hierarchical_recon_loss(y_hat, y, y_hat_seg, seg_y, gamma=self.hparams.gamma, dice_factor=self.hparams.dice_factor,
                                                       **({} if masks is None else {"masks": masks}),
                                                       **({} if dice_terms is None else {"dice_terms": dice_terms}),
                                                       **({"inverse": self._inverse_terms(x, final_dfs_inv, x_hat, seg_x, seg_y, mask_x, mask_y)}
                                                          if self.bidirectional else {}))
        reg, reg_levels = self.hierarchical_regularization(final_dfs, lamb=self.hparams.lamb, **({"dfs_inv": final_dfs_inv} if self.bidirectional else {}))
        total = kl + rec + reg
        return outs, (prior_mus, prior_sigmas), (total, kl, rec, reg), (kl_levels, rec_levels, reg_levels)

    def _logging_active(self) -> bool:
        """is anybody going to read what log_dict receives?  (a Lightning trainer, or a logger attached to the stand-alone base)"""
        if getattr(self, "logger", None) is not None:
            return True
        tr = getattr(self, "_trainer", None)                       # pl.LightningModule keeps the attached trainer here
        return tr is not None

    def _log_levels(self, stage: str, mus, sigmas, priors, levels, **kw):
        if not self._logging_active():
            return                    # the 16 per-level mean reductions are only computed when they have a consumer
        kl_l, rec_l, reg_l = levels
        for level in kl_l.keys():
            with torch.no_grad():
                stats = {
                    f"{stage}_distribution_levels/mean_prior_mu_{level}": torch.mean(priors[0][level]),
                    f"{stage}_distribution_levels/mean_prior_sigma_{level}": torch.mean(priors[1][level]),
                    f"{stage}_distribution_levels/mean_posterior_mu_{level}": torch.mean(mus[level]),
                    f"{stage}_distribution_levels/mean_posterior_sigma_{level}": torch.mean(sigmas[level]),
                }
            self.log_dict({
                f"{stage}_levels/kl loss level {level}": kl_l[level],
                f"{stage}_levels/recon loss level {level}": rec_l[level],
                f"{stage}_levels/regularization loss level {level}": reg_l[level],
                **stats}, **kw)

    def _check_previous_step_for_nan(self):
        """the reference tests the regularisation terms for NaN inside the step with a host synchronisation (models.py:188-192); here the
        flag of step n travels to pinned host memory asynchronously and is looked at when its copy has completed (normally at step n+1),
        so the host never waits for the GPU"""
        pending = self._pending_nan_probe
        if pending is None:
            return
        flag, event = pending
        if not event.query():
            return                    # not there yet: look again next step
        self._pending_nan_probe = None
        if bool(flag.item()):
            print("NAN IN REGULARIZATION LOSS")
            torch.save(self.state_dict(), "nan_state_dict.pt")
            self.trainer.should_stop = True

    def _arm_nan_probe(self, reg_levels) -> None:
        if self._pending_nan_probe is not None:
            return                    # the previous flag has not been consumed yet
        bad = torch.isnan(torch.stack([v.detach() for v in reg_levels.values()])).any()
        if bad.is_cuda:
            flag = torch.empty((), dtype=torch.bool, pin_memory=True)
            flag.copy_(bad, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        else:
            flag, event = bad, _DoneEvent()
        self._pending_nan_probe = (flag, event)

    def training_step(self, batch, batch_idx):
        x, y, seg_x, seg_y, lm1, lm2, mask1, mask2 = batch
        in_graph = getattr(self, "_pulpo_in_graph", False)      # dp.DataParallelStepper(graph=True) is capturing this call into a HIP graph:
        if not in_graph:                                        # the host-side NaN probe (pinned memory, events) stays outside, driven by the stepper
            self._check_previous_step_for_nan()
        eng = self._engine()
        if eng is not None and torch.is_grad_enabled():
            eng.arm(not self._ddp_wrapped())          # multi-rank: this forward pass registers the triggers of the bucketed gradient exchange
        outs, priors, (total, kl, rec, reg), levels = self._forward_and_losses(x, y, seg_x, seg_y, mask1, mask2)
        self.log_dict({"train/kl_loss": kl, "train/reconstruction_loss": rec, "train/regularization_loss": reg, "train/total_loss": total},
                      on_step=True, on_epoch=True, prog_bar=True)
        self._log_levels("train", outs[0], outs[1], priors, levels, on_step=False, on_epoch=True)
        if in_graph:
            self._pulpo_last_reg_levels = {k: v.detach() for k, v in levels[2].items()}
        else:
            self._arm_nan_probe(levels[2])
        return total

    def validation_step(self, batch, batch_idx):
        if batch_idx == self.trainer.num_val_batches[0] - 1:
            self.validation_counter += 1
        x, y, seg_x, seg_y, lm1, lm2, mask1, mask2 = batch
        outs, priors, (total, kl, rec, reg), levels = self._forward_and_losses(x, y, seg_x, seg_y, mask1, mask2)
        self.log_dict({"val/kl_loss": kl, "val/reconstruction_loss": rec, "val/regularization_loss": reg, "val/total_loss": total}, on_epoch=True)
        self._log_levels("val", outs[0], outs[1], priors, levels, on_epoch=True)
        return total

    # ------------------------------------------------------------------------------------------------ inference
    def predict_output_samples(self, x: torch.Tensor, y: torch.Tensor, N: int = 1):
        """N stochastic forward passes stacked on the batch axis -> ({l: (B,N,1,...)}, {l: (B,N,3,...)})"""
        bs = x.shape[0]
        xb, yb = torch.cat([x] * N, dim=0), torch.cat([y] * N, dim=0)          # rank-agnostic (3-D volumes and 2-D slices), models.py:314-315
        outs = self.autoencoder(xb, self.downpath(xb, yb))
        individual_dfs, outputs = outs[4], outs[7]
        fold = lambda t: t.view([N, bs] + list(t.shape[1:])).transpose(0, 1)
        return {k: fold(v) for k, v in outputs.items()}, {k: fold(v) for k, v in individual_dfs.items()}

    def _resample(self, interpolation: str, fields: Dict[int, torch.Tensor], images) -> Dict[int, torch.Tensor]:
        """the images handed back: images (one tensor for every level, or {level: tensor}) under the final fields, trilinear
        (SpatialTransformer: today's route) or through the cubic B-spline interpolant (ops.warp3d_cubic).  The fields are
        the same either way; cubic values may leave the image's range by overshoot at edges."""
        img = (lambda k: images[k]) if isinstance(images, dict) else (lambda k: images)
        if interpolation == "cubic":
            coef = {}                                                          # one prefilter per distinct image
            for k in fields:
                if id(img(k)) not in coef:
                    coef[id(img(k))] = ops.bspline_prefilter(img(k).detach())
            return {k: ops.warp3d_cubic(fields[k], coef=coef[id(img(k))]) for k in fields}
        return {k: self.autoencoder.decoders[k].spatial_transform(fields[k], img(k)) for k in fields}

    def predict(self, x: torch.Tensor, y: torch.Tensor, N: int = 1, interpolation: str = "linear"):
        """interpolation: "linear" (trilinear) or "cubic" (cubic B-spline, ops.warp3d_cubic) for the outputs; the fields do not depend on it"""
        ops.check_interpolation(interpolation, "predict")
        _, individual_dfs = self.predict_output_samples(x, y, N)
        avg_dfs = {k: v.mean(dim=1) for k, v in individual_dfs.items()}
        _, avg_final = self.combine_dfs(avg_dfs)
        # every level warps the FULL-resolution moving image (grid smaller than the image for l >= 1, models.py:330)
        avg_outputs = self._resample(interpolation, avg_final, x)
        return avg_outputs, avg_dfs

    def predict_deterministic(self, x: torch.Tensor, y: torch.Tensor, interpolation: str = "linear"):
        """interpolation="cubic": outputs[l] = ops.warp3d_cubic(final_dfs[l], the level's moving image) instead of the trilinear warp"""
        ops.check_interpolation(interpolation, "predict_deterministic")
        outs = self.autoencoder(x, self.downpath(x, y, _needed=self._needed_levels), deterministic=True)
        if interpolation == "cubic":
            return self._resample(interpolation, outs[6], self.autoencoder.level_images(x)), outs[4]
        return outs[7], outs[4]

    @torch.no_grad()
    def predict_bidirectional(self, x: torch.Tensor, y: torch.Tensor, N: int = 1, deterministic: bool = False, interpolation: str = "linear"):
        """predict (or, with deterministic, predict_deterministic) + combine_dfs with the inverse transform beside it: a dict of
          outputs, individual_dfs   what predict / predict_deterministic return
          final_dfs                 combine_dfs(individual_dfs)[1]
          final_dfs_inv             the inverse fields of combine_dfs_bidirectional
          outputs_inv               {l: spatial_transform(final_dfs_inv[l], y)}: the fixed image on the moving image's grid, warped the
                                    way predict warps x
        interpolation: "linear" or "cubic" for outputs and outputs_inv (the same images under the same fields, through ops.warp3d_cubic).
        Inference only: no autograd."""
        ops.check_interpolation(interpolation, "predict_bidirectional")
        if deterministic:
            outputs, individual_dfs = self.predict_deterministic(x, y, interpolation=interpolation)
            _, final, final_inv = self.combine_dfs_bidirectional(individual_dfs)
        else:
            _, samples = self.predict_output_samples(x, y, N)
            individual_dfs = {k: v.mean(dim=1) for k, v in samples.items()}
            _, final, final_inv = self.combine_dfs_bidirectional(individual_dfs)
            outputs = self._resample(interpolation, final, x)                                                  # as predict
        outputs_inv = self._resample(interpolation, final_inv, y)
        return {"outputs": outputs, "individual_dfs": individual_dfs, "final_dfs": final, "final_dfs_inv": final_inv, "outputs_inv": outputs_inv}

    def refine(self, x: torch.Tensor, y: torch.Tensor, interpolation: str = "linear", bidirectional: Optional[bool] = None, **kw):
        """instance-specific optimisation of this pair's level fields from the model's prediction: pulpo_amd.refine.refine(self, x, y, **kw);
        interpolation="cubic" descends on, and hands back, the cubic B-spline image model (pulpo_amd.refine.refine_interpolated);
        bidirectional (None: this model's flag) descends on the two-sided objective of bidirectional training"""
        from .refine import refine_interpolated
        return refine_interpolated(self, x, y, interpolation, bidirectional, **kw)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        return self.autoencoder(x, self.downpath(x, y, _needed=self._needed_levels))[7][0]

    # ------------------------------------------------------------------------------------------------ helpers
    def combine_dfs(self, individual_dfs: Dict[int, torch.Tensor]):
        """individual level fields -> (combined, integrated + resized) fields (reference models.py:349-368)"""
        combined, final = self._combine_levels(individual_dfs), {}
        for l in reversed(range(self.latent_levels)):
            final[l] = self._resize_integrated(l, ops.vecint(combined[l], 7))
        return combined, final

    def _combine_levels(self, individual_dfs: Dict[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
        """the combined velocity field of every level: the level's own plus the resized one of the level below (reference models.py:349-360)"""
        combined = {}
        for l in reversed(range(self.latent_levels)):
            if l + 1 in combined:
                ratio = individual_dfs[l].shape[2] / individual_dfs[l + 1].shape[2]
                combined[l] = ResizeTransform(vel_resize=1 / ratio, ndims=self.ndims)(combined[l + 1], add=individual_dfs[l])
            else:
                combined[l] = individual_dfs[l]
        return combined

    def _resize_integrated(self, l: int, integrated: torch.Tensor) -> torch.Tensor:
        """an integrated level field at its final size: the input size at level 0 and with df_resolution "full_res", its own otherwise"""
        target = self.input_size if (l == 0 or self.hparams.df_resolution == "full_res") else integrated.shape[2:]
        return ResizeTransform(vel_resize=1 / (target[0] / integrated.shape[2]), ndims=self.ndims)(integrated)

    def combine_dfs_bidirectional(self, individual_dfs: Dict[int, torch.Tensor]):
        """combine_dfs with the inverse transform: (combined, final, final_inv).  The level fields are stationary velocity fields, so the
        inverse of the flow is the integral of -combined[l]: final_inv[l] is that integral, resized like final[l].  Both integrals come from
        one ops.vecint_pair call per level (under no_grad: no intermediate fields kept; with gradients: the paired autograd node)."""
        combined = self._combine_levels(individual_dfs)
        final, final_inv = {}, {}
        for l in reversed(range(self.latent_levels)):
            fwd, inv = ops.vecint_pair(combined[l], 7)
            final[l], final_inv[l] = self._resize_integrated(l, fwd), self._resize_integrated(l, inv)
        return combined, final, final_inv

    def transform_segmentation(self, dfs: Dict[int, torch.Tensor], seg: torch.Tensor):
        """warp the (pooled) segmentation maps with each level's field (reference models.py:370-388)"""
        if self.df_resolution == "full_res":        # every level's field is full resolution: every level warps the full map (models.py:375-376)
            level_seg = {l: seg for l in range(self.latent_levels)}
        else:
            level_seg = {0: seg}
            for _ in range(self.lk_offset):
                level_seg[0] = ops.avg_pool2(level_seg[0])
            for l in range(1, self.latent_levels):
                level_seg[l] = ops.avg_pool2(level_seg[l - 1])
            level_seg[0] = seg
        return {k: self.autoencoder.decoders[k].spatial_transform(dfs[k], level_seg[k]) for k in dfs}

    @staticmethod
    def _label_maps(seg_x, seg_y) -> bool:
        """do the batch's segmentations arrive as integer label maps (B, 1, ...)?  Float (B, C, ...) one-hot maps take transform_segmentation"""
        integer = [torch.is_tensor(s) and s.numel() > 0 and not s.is_floating_point() and s.dtype != torch.bool for s in (seg_x, seg_y)]
        if integer[0] != integer[1]:
            raise ValueError("segmentations: seg_x and seg_y must both be integer label maps (B, 1, ...) or both float one-hot maps (B, C, ...)")
        return integer[0]

    def label_dice_terms(self, final_dfs: Dict[int, torch.Tensor], seg_x: torch.Tensor, seg_y: torch.Tensor) -> Dict[int, torch.Tensor]:
        """{level: Soft_dice_loss(transform_segmentation(final_dfs, one_hot(seg_x))[level], one_hot(seg_y) resized to the level)} from integer
        label maps (B, 1, ...), without a full-resolution one-hot volume and without a host read.  A level whose moving map is the
        full-resolution segmentation - level 0, and every level of df_resolution "full_res" - is one ops.label_dice_loss; the coarse levels
        of "level_res" warp transform_segmentation's pooled chain, started from the label map by ops.labels_soft_map(pool2=True), against
        ops.labels_soft_map(size=level).  Labels outside [0, num_classes) count for no class: range-check the maps once where they are loaded."""
        if self.num_classes is None:
            raise ValueError("integer segmentation maps need the number of classes: build the model with PULPo(num_classes=...)")
        C = self.num_classes
        maps = []
        for name, s in (("seg_x", seg_x), ("seg_y", seg_y)):
            if s.dim() != self.ndims + 2 or s.shape[1] != 1:
                raise ValueError(f"{name}: an integer label map (B, 1, ...) expected, got {tuple(s.shape)}")
            maps.append(s if s.dtype in (torch.uint8, torch.int32) else s.to(torch.int32))
        seg_x, seg_y = maps
        dice_factor = self.hparams.dice_factor
        full = [l for l in final_dfs if l == 0 or self.df_resolution == "full_res"]
        terms = {l: ops.label_dice_loss(final_dfs[l], seg_x, C, seg_y, dice_factor, check=False) for l in full}
        coarse = sorted(l for l in final_dfs if l not in terms)
        if coarse:
            # transform_segmentation's chain: level l >= 1 is the map pooled lk_offset + l times (level 0 itself uses the unpooled map)
            soft, pooled = ops.labels_soft_map(seg_x, C, pool2=True), 1
            for l in range(1, max(coarse) + 1):
                while pooled < self.lk_offset + l:
                    soft, pooled = ops.avg_pool2(soft), pooled + 1
                if l in final_dfs:
                    warped = self.autoencoder.decoders[l].spatial_transform(final_dfs[l], soft)
                    target = ops.labels_soft_map(seg_y, C, size=tuple(final_dfs[l].shape[2:]))
                    terms[l] = ops.soft_dice_loss(warped, target, dice_factor)
        return terms

    # ------------------------------------------------------------------------------------------------ optimizer + Lightning's backward hooks
    # The reference leaves the step to Lightning: `return total_loss` (models.py:196) -> Lightning's closure runs optimizer_zero_grad,
    # on_before_backward, backward, on_after_backward and hands the closure to `optimizer.step` of what configure_optimizers returned
    # (models.py:398-400; pytorch_lightning 1.8 loops/optimization/optimizer_loop.py).  The overrides below make that loop run the step
    # bench.py times: parameter gradients straight into the flat arena, weight gradients on the side stream, one finishing launch, fused
    # Adam, in-place re-pack of the weights - the same pieces `dp.DataParallelStepper.step` strings together.  PULPO_LIGHTNING_FAST=0
    # switches all of it off (plain autograd + torch.optim.Adam).
    def configure_optimizers(self):
        first = next(self.parameters())
        if not first.is_cuda or os.environ.get("PULPO_LIGHTNING_FAST", "1") == "0":
            self._pulpo_optimizer = None
            if not first.is_cuda:
                # a strategy that builds its optimizers BEFORE it moves the model to the device would end up here for good: say so instead of
                # silently handing it the slow loop (plain autograd + torch.optim.Adam, every operator still a HIP kernel)
                import warnings
                warnings.warn("pulpo_amd: configure_optimizers() was called while the parameters are not on a GPU - returning plain torch.optim.Adam "
                              "(no flat arena, no fused update, no direct-to-arena gradients).  Move the model to the device first and call "
                              "configure_optimizers() again for the fast step.", RuntimeWarning, stacklevel=2)
            return torch.optim.Adam(self.parameters(), lr=self.hparams.lr)
        from .dp import ArenaAdam
        opt = ArenaAdam(self, lr=float(self.hparams.lr))
        self._pulpo_optimizer = opt                # (a plain attribute: neither a sub-module nor part of the state dict)
        return opt

    def _engine(self):
        opt = getattr(self, "_pulpo_optimizer", None)
        return None if opt is None else opt.engine

    def _ddp_wrapped(self) -> bool:
        """is a DistributedDataParallel wrapper (Lightning's ddp strategies) reducing the gradients?  It needs them from autograd's
        AccumulateGrad nodes, so the direct-to-arena path is off and the optimizer neither exchanges nor rescales them."""
        tr = getattr(self, "_trainer", None)           # (pytorch_lightning >= 1.8: `trainer` is a property that RAISES while no Trainer is attached)
        if tr is None:
            try:
                tr = getattr(self, "trainer", None)
            except RuntimeError:
                tr = None                              # no Trainer: nothing wraps the module
        wrapped = getattr(getattr(tr, "strategy", None), "model", None)
        return isinstance(wrapped, torch.nn.parallel.DistributedDataParallel)

    def optimizer_zero_grad(self, epoch, batch_idx, optimizer, *args, **kwargs):
        optimizer.zero_grad()                      # (ArenaAdam: one fill, the gradient views stay attached)

    def backward(self, loss, *args, **kwargs):
        eng = self._engine()
        if eng is None:
            return loss.backward(*[a for a in args if torch.is_tensor(a)], **kwargs)      # (PL 1.x passes (optimizer, optimizer_idx) first)
        ddp = self._ddp_wrapped()
        self._pulpo_optimizer.reduced_elsewhere = ddp
        eng.backward(loss, direct=not ddp)

