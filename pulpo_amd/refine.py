"""Instance-specific optimisation: refine a predicted registration for one pair at test time.

    res = refine(model, x, y, iters=50)                      # start: model.predict_deterministic
    res = refine(model, x, y, N=8, anchor=0.1)               # start: mean of 8 posterior samples, anchored where the model is certain
    res["final_dfs"], res["outputs"], res["history"]

The variables are the level velocity fields (`individual_dfs`) themselves, held in one flat fp32 arena; the objective is the training
step's similarity + regulariser on `model.combine_dfs` of them, plus an optional Gaussian anchor to the model's posterior; the optimiser is
Adam, one ops.anchored_adam_step launch per iteration over the whole arena (anchor gradient and value inside it).  The network runs once,
for the start; it is not in the loop.  No reference counterpart: the reference stops at what one forward pass predicts."""
from __future__ import annotations

import inspect
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .losses import HierarchicalReconstructionLoss

RECON_TERMS = ("ncc", "mse", "mind", "mi")
# The step size of refine(): the best objective after 50 iterations among lr in {0.01, 0.03, 0.1, 0.3} whose history has no rise larger than
# 1 % of the total drop, from the prediction and from zero fields, on synthetic.oasis_like_pair at 160^3 / T5 / L4 with an untrained model
# (scripts/refine_bench.py, profiles/refine_bench.txt: 0.1 ends lower but rises by 39 % of the drop on the way from zero fields)
DEFAULT_LR = 0.03


def arena_layout(shapes: Sequence[Sequence[int]]) -> Tuple[List[int], int]:
    """(offsets, total) in floats of tensors of `shapes` laid out one after the other in a flat arena, every offset - and the total -
    padded to a multiple of 4 floats: the float4 passes of the arena kernels want every level 16-byte aligned (5 * 6 * 7 * 3 = 630 is not)"""
    offsets, at = [], 0
    for shape in shapes:
        n = 1
        for s in shape:
            n *= int(s)
        offsets.append(at)
        at += (n + 3) // 4 * 4
    return offsets, at


def _views(arena: torch.Tensor, offsets: List[int], shapes: List[Tuple[int, ...]]) -> Dict[int, torch.Tensor]:
    out = {}
    for l, (off, shape) in enumerate(zip(offsets, shapes)):
        n = 1
        for s in shape:
            n *= s
        out[l] = arena[off:off + n].view(shape)
    return out


def _recon_list(model, recon_loss) -> List[str]:
    recon = list(model.hparams.recon_loss if recon_loss is None else recon_loss)
    if "dice" in recon:
        raise ValueError("refine: the 'dice' term needs segmentations of the pair, which a refinement at test time does not have; "
                         f"pass recon_loss with terms of {RECON_TERMS}")
    unknown = [r for r in recon if r not in RECON_TERMS]
    if unknown or not recon:
        raise ValueError(f"refine: recon_loss {recon} - terms of {RECON_TERMS} expected")
    return recon


class Objective:
    """similarity + regulariser of one pair as a function of its level velocity fields - what refine() descends on (its docstring has the
    terms).  obj(fields) -> (similarity, regulariser, combined_dfs, final_dfs); differentiable with respect to the fields only.
    bidirectional (None: the model's flag): the step's two-sided objective - half the sum of both directions'
    similarity and regulariser, the inverse direction being y's level images under the inverse fields against x, with the masks exchanged.
    obj.terms(fields) returns everything by name: rec, reg, combined, final, y_hat and, bidirectional, final_inv and x_hat."""

    def __init__(self, model, x: torch.Tensor, y: torch.Tensor, recon_loss: Optional[Sequence[str]] = None, lamb: Optional[float] = None,
                 gamma: Optional[float] = None, mask_x: Optional[torch.Tensor] = None, mask_y: Optional[torch.Tensor] = None,
                 interpolation: str = "linear", bidirectional: Optional[bool] = None) -> None:
        recon = _recon_list(model, recon_loss)                      # (before anything touches the device)
        self.interpolation = ops.check_interpolation(interpolation, "refine")
        self.model, self.x, self.y = model, x, y
        self.bidirectional = bool(getattr(model, "bidirectional", False) if bidirectional is None else bidirectional)
        self.gamma = float(model.hparams.gamma if gamma is None else gamma)
        self.lamb = float(model.hparams.lamb if lamb is None else lamb)
        ref = model.hierarchical_recon_loss
        self.recon = ref if recon_loss is None else HierarchicalReconstructionLoss(
            recon_loss=recon, weight_dict=dict(ref.weight_dict), similarity_pyramid=False, ndims=ref.ndims, window_size=ref.window_size,
            mind_dilation=ref.mind_dilation, mind_eps=ref.mind_eps)
        if self.recon is not ref:
            self.recon.mi_bins = ref.mi_bins          # (an attribute, not a constructor argument: the bins of the model's "mi" term)
        self.decoders = model.autoencoder.decoders
        with torch.no_grad():
            self.level_x, self.level_coef = self._level_images(x)
            self.level_y, self.level_coef_y = self._level_images(y) if self.bidirectional else (None, None)
        self.mask_x, self.mask_y = mask_x, mask_y

    def _level_images(self, img):
        """(the image on every level, its B-spline coefficients there or None)"""
        level = self.model.autoencoder.level_images(img)
        # cubic: the level images' B-spline coefficients, once; every iteration gathers from them
        if self.interpolation != "cubic":
            return level, None
        coef = {}
        for l, t in level.items():
            if id(t) not in coef:
                coef[id(t)] = ops.bspline_prefilter(t)
        return level, {l: coef[id(t)] for l, t in level.items()}

    def _warp(self, final, level_img, level_coef):
        if level_coef is not None:
            return {l: ops.warp3d_cubic(final[l], coef=level_coef[l]) for l in final}
        return {l: self.decoders[l].spatial_transform(final[l], level_img[l]) for l in final}

    def terms(self, fields: Dict[int, torch.Tensor]) -> Dict[str, object]:
        if not self.bidirectional:
            combined, final = self.model.combine_dfs(fields)
        else:
            combined, final, final_inv = self.model.combine_dfs_bidirectional(fields)
        y_hat = self._warp(final, self.level_x, self.level_coef)
        masks = self.model.level_masks(final, self.mask_x, self.mask_y, force=True)     # (under no_grad: mask_x re-warped by the current fields)
        extra, out = {}, {"combined": combined, "final": final, "y_hat": y_hat}
        if self.bidirectional:
            x_hat = self._warp(final_inv, self.level_y, self.level_coef_y)
            inverse = {"y_hat": x_hat, "y": self.x}
            masks_inv = self.model.level_masks(final_inv, self.mask_y, self.mask_x, force=True)
            if masks_inv is not None:
                inverse["masks"] = masks_inv
            extra = {"inverse": inverse}
            out.update(final_inv=final_inv, x_hat=x_hat)
        out["rec"], _ = self.recon(y_hat, self.y, gamma=self.gamma, **({} if masks is None else {"masks": masks}), **extra)
        out["reg"], _ = self.model.hierarchical_regularization(final, lamb=self.lamb, **({"dfs_inv": final_inv} if self.bidirectional else {}))
        return out

    def __call__(self, fields: Dict[int, torch.Tensor]):
        t = self.terms(fields)
        return t["rec"], t["reg"], t["combined"], t["final"]


@torch.no_grad()
def _start(model, x, y, individual_dfs, N: int):
    """({l: start field}, {l: unbiased per-voxel variance over the N samples} or None)"""
    L = model.latent_levels
    if individual_dfs is not None:
        if sorted(individual_dfs.keys()) != list(range(L)):
            raise ValueError(f"refine: individual_dfs has levels {sorted(individual_dfs.keys())}, the model {list(range(L))}")
        return {l: individual_dfs[l].detach().float() for l in range(L)}, None
    if N == 1:
        return dict(model.predict_deterministic(x, y)[1]), None
    # sample by sample into running moments: memory does not grow with N (predict_output_samples draws an N-fold batch).  In eval mode the
    # encoder pyramid is a deterministic function of the pair and is computed once (uncertainty.mc_uncertainty does the same)
    moments = {l: ops.StreamingMoments() for l in range(L)}
    down = model.downpath(x, y, _needed=model._needed_levels) if not model.training else None
    for _ in range(N):
        acts = down if down is not None else model.downpath(x, y, _needed=model._needed_levels)
        ind = model.autoencoder(x, acts)[4]
        for l in range(L):
            moments[l].update(ind[l])
    return {l: moments[l].mean() for l in range(L)}, {l: moments[l].m2() / float(N - 1) for l in range(L)}


def refine(model, x: torch.Tensor, y: torch.Tensor, *, individual_dfs: Optional[Dict[int, torch.Tensor]] = None, N: int = 1, iters: int = 50,
           lr: float = DEFAULT_LR, anchor: float = 0.0, anchor_floor: float = 1e-4, recon_loss: Optional[Sequence[str]] = None,
           lamb: Optional[float] = None, gamma: Optional[float] = None, mask_x: Optional[torch.Tensor] = None,
           mask_y: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """`iters` Adam steps of size `lr` on the level velocity fields of one pair (x moving, y fixed; a batch is a batch of independent
    pairs under one summed objective) against
        similarity(y_hat, y) + regulariser(final_dfs) + anchor * sum_l kl_w[l] * 1/2 sum (v_l - mean_l)^2 / (var_l + anchor_floor) / B
    with  combined, final = model.combine_dfs(v),  y_hat[l] = the level's moving image (Autoencoder.level_images) warped by final[l].

    Start (and the anchor's mean): `individual_dfs` if given; else, N == 1, model.predict_deterministic(x, y); else the mean over N
    posterior samples, drawn one at a time, whose unbiased per-voxel variance is the anchor's var (1 in the other two cases).  The network
    runs once, without gradients, in the caller's mode (call model.eval() first, as for any prediction: in training mode a forward pass
    moves the BatchNorm statistics).
    similarity    HierarchicalReconstructionLoss with the model's weight table, windows, MIND hyper-parameters and mi_bins over `recon_loss`
                  (None: the model's list; e.g. ["mind"] refines a model trained with NCC across contrasts; "dice" raises ValueError),
                  gamma (None: the model's).  mask_x / mask_y (weight volumes (B,1,...) at full resolution) switch the masked terms on,
                  whatever the model's `mask` hyper-parameter; mask_x is re-warped by the current field every iteration, without gradient.
    regulariser   model.hierarchical_regularization(final, lamb) (None: the model's lamb): the model's own regulariser - a model built with
                  regularizer="bending" is refined against the bending energy, which leaves a residual affine
                  stretch of the field free where L2 pulls it back to the identity.
                  A model built with bidirectional=True is refined against the two-sided objective of its training step (Objective;
                  DESIGN.md section 3u) through model.combine_dfs_bidirectional, and the result gains final_dfs_inv and outputs_inv (y
                  warped by final_dfs_inv[l]); refine_interpolated (model.refine(..., bidirectional=)) overrides the model's flag.
    anchor        the KL divergence between two Gaussians of equal covariance, N(v, var) against the posterior N(mean, var), weighted by
                  level like the training step's KL term (kl_w, divided by B: kl_diag's normalisation): the fields move freely where the
                  model is uncertain and stay close elsewhere.  Folded once into a per-element precision
                  anchor * kl_w[l] / (B (var + anchor_floor)) and applied inside the Adam kernel, not by autograd.  anchor = 0: no term.
    anchor_floor  voxels^2, keeps the precision finite where the samples agree.  Its default, 1e-4 (a standard deviation of 0.01 voxel), is
                  a guess: nobody has measured it.
    The image model is trilinear; refine_interpolated (model.refine(..., interpolation="cubic")) descends on the cubic B-spline one.
    Nothing in the loop synchronises with the host, touches a model parameter's gradient, a BatchNorm statistic or a weight pack; it works
    under an outer torch.no_grad().  2-D models run through the same code, except that the "mind" term is 3-D only (ops.mind_loss
    raises NotImplementedError on slices).

    Returns a dict: individual_dfs, combined_dfs, final_dfs ({level: tensor}, the refined fields), outputs ({l: x warped by final_dfs[l]},
    the way predict warps), history (device tensor (iters + 1, 4): total, similarity, regulariser, anchor; row i is the objective at the
    iterate before step i, the last row an extra forward pass at the result), anchor_mean / anchor_prec ({level: tensor}, None without an
    anchor)."""
    return _run(model, x, y, "linear", individual_dfs, N, iters, lr, anchor, anchor_floor, recon_loss, lamb, gamma, mask_x, mask_y)


def refine_interpolated(model, x: torch.Tensor, y: torch.Tensor, interpolation: str = "linear", bidirectional: Optional[bool] = None,
                        **kw) -> Dict[str, object]:
    """refine(model, x, y, **kw) with the image model named by `interpolation` (what model.refine calls).
    "linear": refine itself, bit for bit.  "cubic": the level images are prefiltered once (ops.bspline_prefilter) and every iteration warps
    their coefficients with ops.warp3d_cubic, whose gradient with respect to the field is continuous across voxel boundaries (the trilinear
    one jumps there); the returned outputs are cubic too and may leave x's range by overshoot (the "mi" term clamps its inputs already).
    Masks stay trilinear (warp_mask).  Anything else raises ValueError.
    bidirectional: None - the model's flag, as refine; True / False - the two-sided objective (refine's docstring) whatever the model's."""
    ops.check_interpolation(interpolation, "refine")
    if interpolation == "linear" and bidirectional is None:
        return refine(model, x, y, **kw)
    bound = inspect.signature(refine).bind(model, x, y, **kw)
    bound.apply_defaults()
    return _run(model, x, y, interpolation, *list(bound.arguments.values())[3:], bidirectional=bidirectional)


def _run(model, x, y, interpolation, individual_dfs, N, iters, lr, anchor, anchor_floor, recon_loss, lamb, gamma, mask_x, mask_y, bidirectional=None):
    objective = Objective(model, x, y, recon_loss, lamb, gamma, mask_x, mask_y, interpolation, bidirectional)
    if iters < 0 or N < 1:
        raise ValueError("refine: iters >= 0 and N >= 1 expected")
    if anchor < 0 or anchor_floor <= 0:
        raise ValueError("refine: anchor >= 0 and anchor_floor > 0 expected")
    L = model.latent_levels
    start, var = _start(model, x, y, individual_dfs, int(N))
    shapes = [tuple(int(s) for s in start[l].shape) for l in range(L)]
    offsets, total = arena_layout(shapes)
    dev = x.device
    new = lambda: torch.zeros(total, device=dev, dtype=torch.float32)
    arena, m, v = new(), new(), new()
    with torch.no_grad():
        for l, t in _views(arena, offsets, shapes).items():
            t.copy_(start[l])
    mean = prec = None
    if anchor > 0:
        mean, prec = arena.clone(), new()
        kl_w, B = model.hierarchical_kl_loss.weight_dict, shapes[0][0]
        with torch.no_grad():
            for l, t in _views(prec, offsets, shapes).items():
                scale = float(anchor) * float(kl_w[l]) / B
                if var is None:
                    t.fill_(scale / (1.0 + float(anchor_floor)))
                else:
                    t.copy_(scale / (var[l] + float(anchor_floor)))
    arena.requires_grad_(True)
    arena.grad = torch.zeros_like(arena)                            # the one buffer every level's gradient is accumulated into

    history = torch.zeros((iters + 1, 4), device=dev, dtype=torch.float32)
    anchor_val = torch.zeros(1, device=dev, dtype=torch.float32)
    for i in range(iters):
        with torch.enable_grad():
            rec, reg, _, _ = objective(_views(arena, offsets, shapes))
            (rec + reg).backward()
        ops.anchored_adam_step(arena, arena.grad, m, v, float(lr), i + 1, mean=mean, prec=prec, loss_out=anchor_val if mean is not None else None)
        arena.grad.zero_()
        history[i, 1:] = torch.stack((rec.detach().reshape(()), reg.detach().reshape(()), anchor_val[0]))
    with torch.no_grad():
        fields = _views(arena, offsets, shapes)
        last = objective.terms(fields)
        rec, reg, combined, final = last["rec"], last["reg"], last["combined"], last["final"]
        if mean is not None:
            d = arena.detach() - mean
            anchor_val[0] = 0.5 * torch.sum(prec * d * d)               # (once, at the result; in the loop the kernel reduces it)
        history[iters, 1:] = torch.stack((rec.reshape(()), reg.reshape(()), anchor_val[0]))
        history[:, 0] = history[:, 1] + history[:, 2] + history[:, 3]
        # own storage for what is handed out: the level fields, and the coarsest combined field, are views of the arena
        fields = {l: t.detach().clone() for l, t in fields.items()}
        combined = {l: (t.detach().clone() if l == L - 1 else t) for l, t in combined.items()}
        outputs = model._resample(interpolation, final, x)
    as_levels = lambda a: None if a is None else {l: t.clone() for l, t in _views(a, offsets, shapes).items()}
    res = {"individual_dfs": fields, "combined_dfs": combined, "final_dfs": final, "outputs": outputs, "history": history,
           "anchor_mean": as_levels(mean), "anchor_prec": as_levels(prec)}
    if objective.bidirectional:
        with torch.no_grad():
            res["final_dfs_inv"], res["outputs_inv"] = last["final_inv"], model._resample(interpolation, last["final_inv"], y)
    return res
