"""float64 CPU reference of bidirectional training, on the oracle and the helpers of tests/pyramid_ref.py: the paired
integration chain, the level fields of both directions with the images they warp, and the two-sided objective

    rec = 1/2 sum_l w_l [ sim(y_hat_l, y -> size_l) + sim(x_hat_l, x -> size_l) ] / len(recon)
    reg = 1/2 sum_l w_l [ R(final_l) + R(final_inv_l) ]

for given combined level velocity fields, with  final_l / final_inv_l = resize(VecInt(+-combined_l)),  y_hat_l = warp(final_l, x's level
image),  x_hat_l = warp(final_inv_l, y's level image).  Works in the dtype of what it is given (float64 in the tests that call it)."""
from typing import Callable, Dict, Optional, Sequence

import torch

import pyramid_ref as R
from oracle import pulpo_oracle as O


def pair_chain(v, nsteps: int):
    """[(field after k squarings of v / 2^nsteps, the same for -v / 2^nsteps)] for k = 0 .. nsteps"""
    return list(zip(R.vecint_chain_ref(v, nsteps), R.vecint_chain_ref(-v, nsteps)))


def level_images(cfg: O.Cfg, img) -> Dict[int, torch.Tensor]:
    """Autoencoder.level_images (pulpo.py:171-179): level 0 keeps the full-resolution image, level l >= 1 the image pooled offset + l times"""
    L, o = cfg.latent_levels, cfg.offset
    if cfg.df_resolution == "full_res":
        return {l: img for l in range(L)}
    out = {0: img}
    for _ in range(o):
        out[0] = O.pool2(out[0])
    for l in range(1, L):
        out[l] = O.pool2(out[l - 1])
    out[0] = img
    return out


def final_pair(cfg: O.Cfg, combined: Dict[int, torch.Tensor]):
    """({l: final_l}, {l: final_inv_l}): the integrals of +combined_l and -combined_l, resized as PULPo.combine_dfs resizes (models.py:361-367)"""
    fin, inv = {}, {}
    for l, c in combined.items():
        tgt = cfg.input_size if (l == 0 or cfg.df_resolution == "full_res") else c.shape[2:]
        ratio = tgt[0] / c.shape[2]
        fin[l], inv[l] = O.resize_field(O.vecint(c, 7), 1.0 / ratio), O.resize_field(O.vecint(-c, 7), 1.0 / ratio)
    return fin, inv


def warped(cfg: O.Cfg, fields: Dict[int, torch.Tensor], img) -> Dict[int, torch.Tensor]:
    """{l: img's level image under fields[l]}: y_hat for (final, x), x_hat for (final_inv, y)"""
    lv = level_images(cfg, img)
    return {l: O.warp(f, lv[l]) for l, f in fields.items()}


def _sim(kind: str) -> Callable:
    if kind == "ncc":
        return lambda pred, true, win, gamma: O.ncc(pred, true, win, gamma)
    if kind == "mse":
        return lambda pred, true, win, gamma: O.l2_loss(pred, true)
    raise ValueError(kind)


def rec_from_images(cfg: O.Cfg, y_hat, y, x_hat=None, x=None, recon: Sequence = ("ncc",), sims: Optional[Dict[str, Callable]] = None,
                    extra: Optional[Dict[int, torch.Tensor]] = None, extra_inv: Optional[Dict[int, torch.Tensor]] = None):
    """(rec, {l: level term}) from warped images.  x_hat None: the unidirectional sum_l w_l sim(y_hat_l, y_l) / len(recon); else half the sum of
    both directions.  recon: names of _sim ("ncc", "mse") or of `sims` (name -> f(pred, true, level) for terms this module does not hold);
    extra / extra_inv: {l: a term the caller computed (Dice)} added to the level's sum of each direction, counted in len(recon) by `recon`
    naming it "dice"."""
    window, _, rec_w, _ = O.weight_tables(cfg)
    levels = {}
    for l, w in rec_w.items():
        def side(img_hat, img, more):
            tgt = img if tuple(img_hat[l].shape[2:]) == tuple(img.shape[2:]) else O.resize_to(img, img_hat[l].shape[2:])
            t = 0.0
            for kind in recon:
                if kind == "dice":
                    t = t + more[l]
                elif sims is not None and kind in sims:
                    t = t + sims[kind](img_hat[l], tgt, l)
                else:
                    t = t + _sim(kind)(img_hat[l], tgt, window[l], cfg.gamma)
            return w * t / len(recon)
        fwd = side(y_hat, y, extra)
        levels[l] = fwd if x_hat is None else 0.5 * (fwd + side(x_hat, x, extra_inv))
    return sum(levels.values()), levels


def reg_from_fields(cfg: O.Cfg, final, final_inv=None, regularizer: Callable = None):
    """(reg, {l: level term}); regularizer(field) defaults to O.l2_reg(field, cfg.lamb)"""
    reg_fn = regularizer if regularizer is not None else (lambda f: O.l2_reg(f, cfg.lamb))
    _, _, _, reg_w = O.weight_tables(cfg)
    levels = {l: w * (reg_fn(final[l]) if final_inv is None else 0.5 * (reg_fn(final[l]) + reg_fn(final_inv[l]))) for l, w in reg_w.items()}
    return sum(levels.values()), levels


def objective(cfg: O.Cfg, x, y, combined: Dict[int, torch.Tensor], recon: Sequence[str] = ("ncc",), bidirectional: bool = True):
    """the objective of given combined level velocity fields as a dict: rec, reg, total, final, final_inv, y_hat, x_hat (the last three None /
    absent terms with bidirectional=False, which is the unidirectional reference: O.losses' rec and reg on the same fields)"""
    final, final_inv = final_pair(cfg, combined)
    y_hat = warped(cfg, final, x)
    x_hat = warped(cfg, final_inv, y) if bidirectional else None
    rec, rec_l = rec_from_images(cfg, y_hat, y, x_hat, x if bidirectional else None, recon)
    reg, reg_l = reg_from_fields(cfg, final, final_inv if bidirectional else None)
    return {"rec": rec, "reg": reg, "total": rec + reg, "rec_levels": rec_l, "reg_levels": reg_l, "final": final,
            "final_inv": final_inv if bidirectional else None, "y_hat": y_hat, "x_hat": x_hat}
