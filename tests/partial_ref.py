"""float64 references and bookkeeping for tests/test_gpu_partial_grads.py: the ConvUnit and its heads as plain differentiable torch ops (run on
the GPU in double, like tests/pyramid_ref.py), the requires_grad subsets, the gradient pre-fill of a direct backward pass, and the oracle runs
of the training step with frozen parts (CPU, float64, once per module).

A float64 gradient is always taken with EVERY leaf trainable: the gradient of a leaf does not depend on which other leaves ask for one, so one
reference serves every subset of a case."""
import itertools
from typing import Dict, Iterable, Sequence, Tuple

import torch
import torch.nn.functional as F

import pyramid_ref as R
from oracle import pulpo_oracle as O

SLOPE = 0.2
FROZEN_FILL = 7.0                                # what a frozen leaf's attached .grad holds before a pass, and bit for bit after it


def rel_l2(got, ref) -> float:
    """|got - ref|_2 / |ref|_2 in double on the tensors' device; inf where got is not finite"""
    a, b = got.detach().double(), ref.detach().double().to(got.device)
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    return float((a - b).norm() / (b.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------ subsets of the leaves that ask for a gradient
def all_subsets(names: Sequence[str]):
    """every non-empty subset, as frozensets, smallest first"""
    return [frozenset(c) for n in range(1, len(names) + 1) for c in itertools.combinations(names, n)]


def edge_subsets(names: Sequence[str], extra: Iterable[Iterable[str]] = ()):
    """everything, "one frozen" and "one only" for every leaf, plus the given ones - without repeats, in that order"""
    out = [frozenset(names)] + [frozenset(names) - {n} for n in names] + [frozenset({n}) for n in names] + [frozenset(e) for e in extra]
    seen, uniq = set(), []
    for s in out:
        if s and s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def sid(names: Sequence[str], req) -> str:
    return "+".join(n for n in names if n in req) or "none"


# ------------------------------------------------------------------------------------------------ ConvUnit, heads (differentiable, any dtype)
def conv_unit_ref(x, w, b, gamma, beta, rm, rv, training: bool, eps: float = 1e-5):
    """LeakyReLU(BatchNorm3d(Conv3d(x))): batch statistics (biased variance) in training mode, the running ones otherwise"""
    y = R.conv3_ref(x, w, b)
    v = lambda t: t.reshape(1, -1, 1, 1, 1)
    if training:
        mean = y.mean(dim=(0, 2, 3, 4))
        var = ((y - v(mean)) ** 2).mean(dim=(0, 2, 3, 4))
    else:
        mean, var = rm, rv
    bn = (y - v(mean)) * v(gamma * (var + eps).rsqrt()) + v(beta)
    return torch.where(bn > 0, bn, SLOPE * bn)


def grads_of(loss, leaves: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    gs = torch.autograd.grad(loss, list(leaves.values()))
    return {k: g.detach() for k, g in zip(leaves, gs)}


def double_leaves(t: Dict[str, torch.Tensor], names: Sequence[str]) -> Dict[str, torch.Tensor]:
    return {n: t[n].detach().double().requires_grad_(True) for n in names}


def prefill_like(ref: Dict[str, torch.Tensor], like: Dict[str, torch.Tensor], scale: Dict[str, float], gen) -> Dict[str, torch.Tensor]:
    """g0 per leaf: fp32 normal variates in the leaf's own layout, scaled to the rms of its float64 gradient (scale[n] overrides: a gradient
    whose true value is zero is pre-filled on the scale it is judged on)"""
    out = {}
    for n, r in ref.items():
        s = scale.get(n, float(r.pow(2).mean().sqrt()))
        g = torch.empty_like(like[n], dtype=torch.float32)
        g.normal_(generator=gen)
        out[n] = g * s
    return out


# ------------------------------------------------------------------------------------------------ the training step's oracle runs
def oracle_step(sd, cfg, x, y, eps, down_training: bool = True, record=None):
    """O.train_step with the DownPath optionally in eval mode (a frozen encoder under .eval()) -> (loss tuple, gradients by name, outputs).
    record: a dict that receives every ConvUnit's output by prefix.  sd's BatchNorm running statistics move as the reference's do."""
    orig = O.conv_unit

    def recording(h, sd_, prefix, training):
        out = orig(h, sd_, prefix, training)
        record[prefix] = out.detach()
        return out

    if record is not None:
        O.conv_unit = recording
    try:
        acts = O.down_path(sd, cfg, x, y, down_training)
        outs = O.autoencoder(sd, cfg, x, acts, eps, True)
        ls = O.losses(outs, y, cfg)
        params = {k: v for k, v in sd.items() if v.requires_grad}
        gl = torch.autograd.grad(ls[0], list(params.values()), allow_unused=True)
    finally:
        O.conv_unit = orig
    return ls, {k: g for k, g in zip(params, gl)}, outs


def as_double(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def bn_bias(name: str) -> bool:
    """a convolution bias in front of a training-mode BatchNorm (true gradient zero): every `_op.0.bias` but the VelocityField's 1x1x1 head"""
    return name.endswith("_op.0.bias") and "velocity_field._op.2" not in name


def count_flips(got_units: Dict[str, torch.Tensor], ref_units: Dict[str, torch.Tensor]) -> Tuple[int, int]:
    """(LeakyReLU slope flips, activations) between two recordings of the ConvUnit outputs, over the units both hold"""
    keys = [k for k in ref_units if k in got_units]
    flips = sum(int(((got_units[k].detach().cpu() > 0) != (ref_units[k] > 0)).sum()) for k in keys)
    return flips, sum(ref_units[k].numel() for k in keys)
