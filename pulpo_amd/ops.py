"""torch.autograd.Function wrappers around the libpulpo_hip.so C ABI (include/pulpo_hip.h).

PyTorch supplies device memory, the current HIP stream and the autograd tape; every arithmetic step of the hot path
is a hand-written HIP kernel.  No operator here has a CPU path: tensors must live on a ROCm device.

Layouts: multi-channel activations are torch.channels_last_3d (N,D,H,W,C in memory) — possibly channel slices of a
wider buffer; 1- and 3-channel images / fields are plain contiguous (N,C,D,H,W) like the reference's tensors.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import os
from typing import Optional, Sequence, Tuple

import torch

from ._lib import PulpoHipError, lib

CL = torch.channels_last_3d
LRELU_SLOPE = 0.2


# ------------------------------------------------------------------------------------------------ helpers
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_gpu(*ts: Optional[torch.Tensor], act: bool = False):
    """act: the tensors are multi-channel activations, which may live in HBM as bf16 (ACT_BF16, BASELINE configs 4-5); everything else is fp32"""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise PulpoHipError("pulpo_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.float32 and not (act and t.dtype == torch.bfloat16):
            raise PulpoHipError(f"pulpo_amd operators are fp32 (got {t.dtype})" + (" or bf16 activations" if act else ""))


def _dt(t: torch.Tensor) -> int:
    """dtype code of the typed C entry points (`*_t`): 0 fp32, 1 bf16"""
    return 1 if t.dtype == torch.bfloat16 else 0


def _esize(t: torch.Tensor) -> float:
    return 2.0 if t.dtype == torch.bfloat16 else 4.0


def _dense_grid(t: torch.Tensor) -> bool:
    """spatial dims form a dense voxel grid with a single pixel stride"""
    _, _, D, H, W = t.shape
    ps = t.stride(4)
    return (W == 1 or ps > 0) and (H == 1 or t.stride(3) == W * ps) and (D == 1 or t.stride(2) == H * W * ps)


def grid_strides(t: torch.Tensor) -> Tuple[int, int, int]:
    """(batch, pixel, channel) strides in elements of a (B,C,D,H,W) tensor whose voxels form a dense grid"""
    return t.stride(0), t.stride(4), t.stride(1)


def as_grid(t: torch.Tensor) -> torch.Tensor:
    """any 5-D tensor -> one the conv kernels can address (planar or channels-last, incl. channel slices)"""
    if _dense_grid(t) and (t.shape[1] == 1 or t.stride(1) in (1, t.shape[2] * t.shape[3] * t.shape[4] * t.stride(4))):
        return t
    return t.contiguous(memory_format=CL) if t.shape[1] > 3 else t.contiguous()


def is_cl(t: torch.Tensor) -> bool:
    B, C, D, H, W = t.shape
    return _dense_grid(t) and (t.stride(1) == 1 or C == 1) and t.stride(0) == D * H * W * t.stride(4)


def to_cl(t: torch.Tensor) -> torch.Tensor:
    """channels-last view/copy with cs == 1 and bs == V*ps (what the streaming kernels assume)"""
    if is_cl(t) and (t.shape[1] > 1 or t.stride(4) == 1):
        return t
    if t.shape[1] == 1:
        return t.contiguous()
    return t.contiguous(memory_format=CL)


def new_cl(B: int, C: int, D: int, H: int, W: int, device, dtype=torch.float32) -> torch.Tensor:
    return torch.empty((B, C, D, H, W), device=device, dtype=dtype, memory_format=CL)


def _packed_cl(t: torch.Tensor) -> torch.Tensor:
    """a packed channels-last copy (voxel stride = channel count, 16-byte aligned for C % 4 == 0).  to_cl() hands a channel slice of a wider
    channels-last buffer back as it is - at an unaligned channel offset that is no operand of the vector-load kernels"""
    return torch.empty(t.shape, device=t.device, dtype=t.dtype, memory_format=CL).copy_(t)


def planar(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------------------------- 2-D mode (train.py --ndims 2)
# Slices are run as depth-1 volumes through the same kernels: (B,C,H,W) -> (B,C,1,H,W); 3x3 weights sit in the middle depth slice of a
# 3x3x3 kernel (the other two slices multiply zero padding); 2-channel fields / latents get a leading zero depth channel.  The kernels
# with ndims-dependent arithmetic (warp normalisation, NCC window count, L2_reg, Jacobian, KL_nondiagonal) switch to the reference's
# 2-D form when the depth is 1.  All lifting is done with differentiable torch views / pads on small tensors.
def _is2d(t) -> bool:
    return t is not None and t.dim() == 4


def _lift(t):
    return None if t is None else t.unsqueeze(2)


def _lift_field(f):
    """(B,2,H,W) -> (B,3,1,H,W) with a zero depth component in front"""
    return None if f is None else torch.cat([torch.zeros_like(f[:, :1]), f], dim=1).unsqueeze(2)


def _unlift_field(f5):
    return f5[:, 1:, 0]


def _lift_w3(w):
    """(Cout,Cin,3,3) -> (Cout,Cin,3,3,3): taps in the middle depth slice"""
    return torch.nn.functional.pad(w.unsqueeze(2), (0, 0, 0, 0, 1, 1))


def _colsum(partials: torch.Tensor, nrow: int, ncol: int, scale: float = 1.0, into: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """column sums of [nrow][ncol] fp32 partials (double accumulation); `into` -> added to that tensor in place, returns None"""
    if into is not None:
        lib.call("pulpo_colsum", _ptr(partials), nrow, ncol, _ptr(into), scale, 1, _stream())
        return None
    out = torch.empty(ncol, device=partials.device, dtype=torch.float32)
    lib.call("pulpo_colsum", _ptr(partials), nrow, ncol, _ptr(out), scale, 0, _stream())
    return out


class _BackwardPass:
    """what lives as long as one backward pass.  direct: the conv / BatchNorm backward kernels add parameter gradients straight into the parameters'
    existing .grad storage and hand `None` to autograd (no per-parameter temporary, no AccumulateGrad add kernel: ~170 tiny launches per step);
    side, window: the weight gradients' stream (_on_side_stream) and the CoarseWindow, None = in line; jobs, keep: the finishing jobs (src ptr, dst
    ptr, kind, a, b, c) pending for flush_param_grads() and the buffers they read; bn_parts: see _dgrad_with_bn_reduction"""
    __slots__ = ("direct", "side", "window", "jobs", "keep", "bn_parts")

    def __init__(self, direct: bool = False, side=None, window=None):
        self.direct, self.side, self.window = bool(direct), side, window
        self.jobs, self.keep, self.bn_parts = [], [], {}


# The current pass: a module global, not a thread-local, because autograd runs a device's backward functions on its own thread.  The default one
# serves plain autograd use (gradients are returned to autograd on the caller's stream); backward_pass() installs dp.DataParallelStepper's.
# (bench.py's all-ranks-failed fallback still assigns ops.ASYNC_WGRAD_STREAM / ops.DIRECT_PARAM_GRADS: attributes nobody reads, the pass is over by then)
_DEFAULT_PASS = _PASS = _BackwardPass()


@contextlib.contextmanager
def backward_pass(direct: bool, side=None, window=None, module: Optional[torch.nn.Module] = None):
    """install a pass of its own around one backward pass (the only way to).  Its exit, normal or not, joins the side stream and the window and
    finishes the deferred parameter gradients in one launch; after an exception it first drops them, with `module`'s persistent scratch."""
    global _PASS
    if _PASS is not _DEFAULT_PASS:
        raise PulpoHipError("backward_pass(): another backward pass is installed (passes neither nest nor run concurrently from two threads)")
    _DEFAULT_PASS.bn_parts.clear()               # (sums left for a unit whose backward never ran)
    _PASS = bp = _BackwardPass(direct, side, window)
    if window is not None:
        window.begin()
    try:
        yield bp
    except BaseException:
        reset_param_grad_buffers(module)         # deferred gradient sums of an interrupted backward pass are void
        if window is not None:
            window.held = []                     # (and so are the weight gradients still held back for the coarse window)
        raise
    finally:
        bp.direct = False
        try:
            join_async_wgrad()                   # (also finishes the deferred weight / bias gradients in one launch)
            if window is not None:
                window.begin()                   # (an interrupted pass: no operand stays referenced)
        finally:
            _PASS = _DEFAULT_PASS


def _grad_slot(p: torch.Tensor) -> Optional[torch.Tensor]:
    if not _PASS.direct or not p.is_leaf:         # (lifted 2-D weights are derived tensors: their gradient goes through autograd)
        return None
    if not p.requires_grad:                      # (a frozen parameter may still carry a .grad tensor - frozen after the optimizer was built: never written)
        return None
    g = getattr(p, "grad", None)
    if g is None or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
        return None
    return g


# ------------------------------------------------------------------------------------------------ conv 3x3x3
# Optional live kernel timing (bench.py): when CONV_TRACE is a list, every conv / wgrad launch is bracketed by HIP events
# recorded on the launch stream and (kernel name, algorithmic FLOPs, start, end) is appended.  No synchronisation here.
CONV_TRACE = None
CONV_TRACE_STRIDE = 1          # > 1: bracket only every n-th launch (a stride co-prime with the launches per step samples every layer)
CONV_TRACE_STRIDE_USED = 1     # the stride of the last timed trace (bench.py scales sampled totals with it)
_trace_rng = __import__("random").Random(0)     # which launches are bracketed: an unbiased 1-in-stride draw (a fixed stride can lock onto the
                                                # same launches of every step when the launch count per step is a multiple of it)


def _sampled() -> bool:
    return CONV_TRACE_STRIDE <= 1 or _trace_rng.random() * CONV_TRACE_STRIDE < 1.0


def _trace_begin():
    if CONV_TRACE is None or not _sampled():
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


# HBM-bound kernels (BatchNorm / LeakyReLU passes, warp, VecInt, NCC, pooling / resizing, heads, KL, regulariser, Adam): same bracket,
# algorithmic BYTES instead of FLOP
HBM_TRACE = None


_HBM_SEEN: dict = {}


def _hbm_begin(name: str):
    """brackets the first launches of every kernel class (a class with one launch per step - Adam - must not depend on the draw) and a
    1-in-stride draw of the rest"""
    trace = HBM_TRACE
    if trace is None:
        return None
    if not trace:
        _HBM_SEEN.clear()
    n = _HBM_SEEN[name] = _HBM_SEEN.get(name, 0) + 1
    if n > 2 and not _sampled():
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _hbm_end(start, name: str, nbytes: float):
    if start is None or HBM_TRACE is None:
        return
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    HBM_TRACE.append((name, nbytes, start, end))


def _trace_end(start, name: str, flops: float, nbytes: float = 0.0):
    """nbytes: algorithmic HBM bytes of the launch (operands read once + result written once)"""
    if start is None:
        return
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    CONV_TRACE.append((name, flops, start, end, nbytes))


# Operand precision of the 3x3x3 convolutions: "fp32" (the reference's arithmetic; exact-fp32 MFMA) or "bf16" (BASELINE configs
# 4-5: operands rounded to bf16 while staged, fp32 accumulation; activations, statistics, losses and gradients stay fp32).
# Layers with <= 4 reduction channels (the 2-channel image input) always run the fp32 kernel.
CONV_PRECISION = "fp32"
# bf16 ACTIVATION STORAGE (BASELINE configs 4-5, on top of bf16 operands): the multi-channel activation tensors - a ConvUnit's pre-norm
# output y and its output z, pooled / concatenated / up-sampled feature maps - and their gradients live in HBM as bf16; every kernel
# computes in fp32 (BatchNorm statistics in double) and rounds on the store.  Images, latent samples, displacement fields, losses,
# parameters, their gradients and the optimizer state stay fp32; so do the outputs of the layers with <= 4 reduction channels, which run
# the exact-fp32 kernel.  A definition of this repository (the test suite's CPU checker emulates it), "parity unpinned" against the reference.
ACT_BF16 = False
# None: the library's choice per shape (pulpo_conv3d_k3_algo); "direct" | "wino2": force that forward / data-gradient kernel
# wherever a Winograd kernel would be eligible (A/B runs and the full-size consistency test)
CONV_ALGO = None


def set_conv_precision(precision: str, activations: str = "fp32") -> None:
    """precision: operand type of the 3x3x3 convolutions; activations: storage type of the multi-channel activation tensors ("bf16" only
    together with bf16 operands)"""
    global CONV_PRECISION, ACT_BF16
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"conv precision is {precision}. Not a known option.")
    if activations not in ("fp32", "bf16") or (activations == "bf16" and precision != "bf16"):
        raise ValueError(f"activation storage is {activations} with {precision} operands. Not a known option.")
    CONV_PRECISION = precision
    ACT_BF16 = activations == "bf16"


def act_dtype():
    return torch.bfloat16 if ACT_BF16 else torch.float32


# Deterministic mode (PULPO_DETERMINISTIC=1 / set_deterministic(True)): the backward kernels that add with float atomics - the weight-gradient
# flush of concurrent workgroups, the image-gradient scatter of the warp / VecInt backward, the generic trilinear-resize backward - are replaced
# by their ordered forms (`*_det` entry points: per-split slabs + an ordered sum; 64-bit fixed-point accumulation; a gather): two runs of the same
# build on the same inputs give bit-identical gradients, as the reference's CPU backward does.  Everything else in a step is
# deterministic already (two-stage reductions in fixed order), the `bending` regulariser included (its backward is a gather).  Not covered: the
# `jdet` regulariser's backward (raises in this mode).
DETERMINISTIC = os.environ.get("PULPO_DETERMINISTIC", "0") == "1"


def set_deterministic(on: bool = True) -> None:
    global DETERMINISTIC
    DETERMINISTIC = bool(on)


# The fused BatchNorm-backward passes of a ConvUnit, each with the separate pass it replaces - which stays, for the shapes the fused pass does not
# take, and which False selects everywhere (the test suite's seam: fused and separate passes must agree).
BN_REDUCE_IN_DGRAD = True        # False: the first pass (per-tile sums) as a kernel of its own, not in the consumer's data-gradient / pooling backward
FUSE_INPUT_WGRAD = True          # False: the input layer's second pass writes dy for the plain weight gradient instead of running inside it
POOLED_BN_BACKWARD = True        # False: the gradient of a pooled ConvUnit output is written as a tensor, then the plain passes
FUSE_HEAD_BN = True              # False: a head reads the last ConvUnit's activation (separate BatchNorm and head passes) instead of its pre-norm tensor


def _use_bf16(K: int) -> bool:
    return CONV_PRECISION == "bf16" and K > 4


# Weights written behind torch's back (the fused Adam kernel, a broadcast into the parameter arena) do not move a tensor's version counter:
# whoever does that calls invalidate_weight_packs()
_WEIGHT_EPOCH = 0


def invalidate_weight_packs() -> None:
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    _PACK_REGISTRY.clear()


# id(packed buffer) -> (weakref to the weight, packed buffer, Cin, Cout, dgrad, kind) of every live pack of a LEAF weight that
# pulpo_conv3d_k3_pack_weights_multi can rewrite in place (kinds 0, 2, 3); a pack of another family (Winograd-x) makes the set
# unrefreshable.  Keyed by the pack itself, so every pack of a weight (both orientations, several volume shapes, both precisions) has its
# own entry; the weight is held weakly, so a discarded model's packs go with it (dead entries are pruned as new ones arrive).
_PACK_REGISTRY: dict = {}
_PACK_TABLES: dict = {}
_UNREFRESHABLE_PACKS = False
_registrations = 0


def _register_pack(w: torch.Tensor, wp: torch.Tensor, Cin: int, Cout: int, dgrad: bool, kind: int) -> None:
    global _registrations
    import weakref
    _PACK_REGISTRY[id(wp)] = (weakref.ref(w), wp, Cin, Cout, dgrad, kind)
    _registrations += 1
    if _registrations % 64 == 0:
        for k in [k for k, e in _PACK_REGISTRY.items() if e[0]() is None]:
            del _PACK_REGISTRY[k]


def refresh_weight_packs() -> None:
    """after an update of the parameters behind torch's back (the fused Adam kernel): rewrite every cached weight pack in place with ONE
    launch on the current stream, instead of forgetting them and packing layer by layer (55 small launches on the critical path of the
    next forward and backward pass).  Falls back to invalidate_weight_packs() when a cached pack is of a kind the kernel does not write."""
    global _UNREFRESHABLE_PACKS
    if _UNREFRESHABLE_PACKS or not _PACK_REGISTRY:
        _UNREFRESHABLE_PACKS = False
        invalidate_weight_packs()
        return
    jobs = []
    device = None
    for key, (wref, wp, Cin, Cout, dgrad, kind) in list(_PACK_REGISTRY.items()):
        w = wref()
        cache = getattr(w, "_pulpo_packs", None) if w is not None else None
        if cache is None or cache[0] != (w._version, w.data_ptr(), _WEIGHT_EPOCH) or not any(v is wp for v in cache[1].values()):
            del _PACK_REGISTRY[key]                  # superseded (weight gone, replaced or modified through torch): the next use packs afresh
            continue
        jobs.append((w.data_ptr(), wp.data_ptr(), Cin, Cout, int(dgrad), kind))
        device = w.device
    if not jobs:
        invalidate_weight_packs()
        return
    tkey = tuple(jobs)
    table = _PACK_TABLES.get(tkey)
    if table is None:
        import struct
        raw = b"".join(struct.pack("<QQiiii", *job) for job in tkey)
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        if len(_PACK_TABLES) > 4:
            _PACK_TABLES.clear()
        _PACK_TABLES[tkey] = table
    lib.call("pulpo_conv3d_k3_pack_weights_multi", _ptr(table), len(tkey), _stream())


def _pack_weight(w: torch.Tensor, dgrad: bool, shape=None, both: bool = False) -> torch.Tensor:
    """cached front end of _pack_weight_now: a weight is packed once per (version, orientation, kernel family, precision); `both` = also
    produce the other orientation now (training forward: the data-gradient kernel of the backward pass finds its weights ready, and a
    repeated forward - Monte-Carlo sampling, evaluation loops - packs nothing at all)"""
    if not w.is_leaf:
        # a temporary (the 2-D mode's lifted 3x3 weight, a view, a re-parametrisation): packed per call - a cache on it would die with it,
        # and one that outlived it (the refresh registry) would pin it and every pack made from it
        return _pack_weight_now(w, dgrad, shape, register=False)
    cache = getattr(w, "_pulpo_packs", None)
    ver = (w._version, w.data_ptr(), _WEIGHT_EPOCH)
    if cache is None or cache[0] != ver:
        cache = (ver, {})
        try:
            w._pulpo_packs = cache
        except AttributeError:                       # (non-leaf views cannot carry attributes on some builds: pack uncached)
            return _pack_weight_now(w, dgrad, shape, register=False)
    def key(d):
        return (d, CONV_PRECISION, CONV_ALGO, None if shape is None else tuple(shape))
    if both and key(not dgrad) not in cache[1]:
        cache[1][key(not dgrad)] = _pack_weight_now(w, not dgrad, shape)
    if key(dgrad) not in cache[1]:
        cache[1][key(dgrad)] = _pack_weight_now(w, dgrad, shape)
    return cache[1][key(dgrad)]


def _pack_weight_now(w: torch.Tensor, dgrad: bool, shape=None, register: bool = True) -> torch.Tensor:
    """GEMM-ordered copy of a (Cout, Cin, 3, 3, 3) weight for the forward (dgrad=False) or data-gradient (True) convolution.
    shape = (B, D, H, W) of the volume it will be applied to: large volumes use the Winograd-x kernel, which has its own packing
    (the returned tensor carries the choice in `_pulpo_algo`)."""
    Cout, Cin = w.shape[0], w.shape[1]
    K, N = (Cout, Cin) if dgrad else (Cin, Cout)
    global _UNREFRESHABLE_PACKS
    if _use_bf16(K):
        wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_bf16_elems", K, N), device=w.device, dtype=torch.int16)
        lib.call("pulpo_conv3d_k3_pack_weight_bf16", _ptr(w.contiguous()), _ptr(wp), Cin, Cout, int(dgrad), _stream())
        wp._pulpo_algo = "bf16"
        if register:
            if w.is_contiguous():
                _register_pack(w, wp, Cin, Cout, dgrad, 3)
            else:
                _UNREFRESHABLE_PACKS = True
        return wp
    algo = lib.query("pulpo_conv3d_k3_algo", *shape, K, N) if shape is not None else 0
    if CONV_ALGO is not None and algo != 0:            # diagnostic override; only among the kernels valid for this shape
        algo = {"direct": 0, "wino2": 2, "wino3": algo}[CONV_ALGO]          # ("wino3": wherever the library's own policy picks it)
    # the coarse levels' wide layers (20^3, 10^3 of the 160^3 pyramid): F(2x2x2,3x3x3) as batched GEMMs on the F(2x2x2) pack; forcing "wino2" keeps the (y, x) kernel
    gemm = algo == 2 and CONV_ALGO in (None, "wino3") and bool(lib.query("pulpo_conv3d_k3_wino3g_ok", *shape, K, N))
    if algo == 3 or gemm:
        wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_wino3_floats", K, N), device=w.device, dtype=torch.float32)
        lib.call("pulpo_conv3d_k3_pack_weight_wino3", _ptr(w.contiguous()), _ptr(wp), Cin, Cout, int(dgrad), _stream())
        wp._pulpo_algo = "wino3g" if gemm else "wino3"
        if register:
            if w.is_contiguous():
                _register_pack(w, wp, Cin, Cout, dgrad, 4)
            else:
                _UNREFRESHABLE_PACKS = True
        return wp
    if algo == 2:
        wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_wino2_floats", K, N), device=w.device, dtype=torch.float32)
        lib.call("pulpo_conv3d_k3_pack_weight_wino2", _ptr(w.contiguous()), _ptr(wp), Cin, Cout, int(dgrad), _stream())
        wp._pulpo_algo = "wino2"
        if register:
            if w.is_contiguous():
                _register_pack(w, wp, Cin, Cout, dgrad, 2)
            else:
                _UNREFRESHABLE_PACKS = True
        return wp
    wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_floats", K, N), device=w.device, dtype=torch.float32)
    lib.call("pulpo_conv3d_k3_pack_weight", _ptr(w.contiguous()), _ptr(wp), Cin, Cout, int(dgrad), _stream())
    wp._pulpo_algo = "direct"
    if register:
        if w.is_contiguous():
            _register_pack(w, wp, Cin, Cout, dgrad, 0)
        else:
            _UNREFRESHABLE_PACKS = True
    return wp


def _conv_raw(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, K: int, N: int,
              stats: Optional[torch.Tensor], coef: Optional[torch.Tensor] = None):
    """coef: eval-mode BatchNorm coefficients -> BatchNorm + LeakyReLU are applied by the convolution's store (one kernel per ConvUnit)"""
    B, _, D, H, W = _dims5(x)
    ob, op, oc = (0, 0, 1) if is_blocked(out) else grid_strides(out)
    algo = getattr(wp, "_pulpo_algo", "bf16" if wp.dtype == torch.int16 else "direct")
    if isinstance(x, _BlockedGrad) or is_blocked(x) or is_blocked(out):
        # operand and / or result in the channel-blocked layout: the F(2x2x2,3x3x3) kernel's *_kb entry (the callers have checked the kernel family)
        xt, xb_, xp_, xkb, xblk = _opnd(x)
        ot, ob_, op_, okb, oblk = _opnd(out)
        if algo != "wino3" or (not oblk and not _vec4(out)) or (not xblk and grid_strides(x)[2] != 1):
            raise PulpoHipError("conv3d on channel-blocked tensors: F(2x2x2,3x3x3) kernel, channels-last or blocked fp32 operands only")
        t0 = _trace_begin()
        lib.call("pulpo_conv3d_k3_fwd_wino3_kb", _ptr(xt), xb_, xp_, xkb, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(ot), ob_, op_, okb, _ptr(stats),
                 B, D, H, W, K, N, _stream())
        _trace_end(t0, "conv3d_k3_wino3_mfma<false>", 54.0 * K * N * B * D * H * W, 4.0 * (K + N) * B * D * H * W)
        return
    xb, xp, xc = grid_strides(x)
    bf16 = algo == "bf16"
    vec_ok = _vec4(x, K)
    if algo == "wino3":
        # F(2x2x2,3x3x3): channels-last, 16-byte aligned operand and result (the deep layers' tensors are; anything else is copied into that form)
        if not vec_ok:
            x = _packed_cl(x)
            xb, xp, xc = grid_strides(x)
        if not _vec4(out):
            raise PulpoHipError("conv3d (F(2x2x2,3x3x3) kernel): the result must be channels-last and 16-byte aligned")
        t0 = _trace_begin()
        lib.call("pulpo_conv3d_k3_fwd_wino3", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(out), ob, op, oc, _ptr(stats),
                 B, D, H, W, K, N, _stream())
        _trace_end(t0, "conv3d_k3_wino3_mfma<false>", 54.0 * K * N * B * D * H * W, 4.0 * (K + N) * B * D * H * W)
        return
    if algo == "wino3g":
        # F(2x2x2,3x3x3) as batched GEMMs: any operand / result strides; the transformed operand and the products live in a scratch
        scratch = torch.empty(lib.query("pulpo_conv3d_k3_fwd_wino3g_scratch_floats", B, D, H, W, K, N), device=x.device, dtype=torch.float32)
        t0 = _trace_begin()
        lib.call("pulpo_conv3d_k3_fwd_wino3g", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(out), ob, op, oc, _ptr(stats),
                 _ptr(scratch), B, D, H, W, K, N, _stream())
        _trace_end(t0, f"conv3d_k3_wino3_gemm<{3 if N % 96 == 0 else 2}>", 54.0 * K * N * B * D * H * W, 4.0 * (K + N) * B * D * H * W)
        return
    if algo == "wino2":
        if (D % 4 or D * H * W < 8000) and not vec_ok:     # (volumes below 20^3 - the 10^3 level - run on the pipelined kernel only: channels-last operand)
            x = _packed_cl(x)
            xb, xp, xc = grid_strides(x)
            vec_ok = True
        nscr = lib.query("pulpo_conv3d_k3_fwd_wino2_scratch_floats", B, D, H, W, K, N)
        scratch = torch.empty(nscr, device=x.device, dtype=torch.float32) if nscr else None
        t0 = _trace_begin()
        lib.call("pulpo_conv3d_k3_fwd_wino2", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(out), ob, op, oc, _ptr(stats),
                 _ptr(scratch), B, D, H, W, K, N, _stream())
        kname = f"conv3d_k3_wino2_mfma<{'true' if vec_ok else 'false'}>"
        if vec_ok and t0 is not None and lib.query("pulpo_conv3d_k3_wino2_pipelined", D, H, W, K, xp):
            kname = "conv3d_k3_wino2p_mfma<false>"
        _trace_end(t0, kname, 54.0 * K * N * B * D * H * W, 4.0 * (K + N) * B * D * H * W)
        return
    sfx = "_bf16" if bf16 else ""
    nscr = lib.query(f"pulpo_conv3d_k3_fwd{sfx}_scratch_floats", B, D, H, W, K, N)
    scratch = torch.empty(nscr, device=x.device, dtype=torch.float32) if nscr else None
    t0 = _trace_begin()
    if bf16:
        # the typed entry points: operand and result share one storage type (fp32: rounded while staged; bf16: stored that way)
        if x.dtype != out.dtype:
            raise PulpoHipError(f"conv3d (bf16 operands): input {x.dtype} and output {out.dtype} must share one storage type")
        if coef is None:
            lib.call("pulpo_conv3d_k3_fwd_bf16_t", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(out), ob, op, oc, _dt(x), _ptr(stats), _ptr(scratch),
                     B, D, H, W, K, N, _stream())
        else:
            lib.call("pulpo_conv3d_k3_fwd_bn_lrelu_bf16_t", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(out), ob, op, oc,
                     _dt(x), _ptr(scratch), B, D, H, W, K, N, _stream())
    elif coef is None:
        lib.call("pulpo_conv3d_k3_fwd", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(out), ob, op, oc, _ptr(stats), _ptr(scratch), B, D, H,
                 W, K, N, _stream())
    else:
        lib.call("pulpo_conv3d_k3_fwd_bn_lrelu", _ptr(x), xb, xp, xc, _ptr(wp), _ptr(bias), _ptr(coef), LRELU_SLOPE, _ptr(out), ob, op, oc,
                 _ptr(scratch), B, D, H, W, K, N, _stream())
    if t0 is not None:
        if bf16:
            name = f"conv3d_k3_mfma_bf16<{64 if N % 64 == 0 else 32},{'true' if vec_ok else 'false'}>"
        else:
            cfg = lib.query("pulpo_conv3d_k3_tile_config", K, N)
            name = f"conv3d_k3_mfma<{cfg // 1000},{cfg % 1000},{'true' if vec_ok and cfg // 1000 >= 16 else 'false'}>"
        _trace_end(t0, name, 54.0 * K * N * B * D * H * W, (_esize(x) * K + _esize(out) * N) * B * D * H * W)


# ---- deferred parameter-gradient epilogues (data-parallel stepper): inside a step the weight gradients stay in their packed scratch and
# the conv-bias gradients in their BatchNorm-backward partials until flush_param_grads() finishes ALL of them with one launch
# (pulpo_grad_finish_multi) - instead of a memset + an unpack + a column-sum launch per layer, each of which has to find room on CUs the
# persistent convolution kernels hold.  The scratch buffers persist on the parameter (they are returned all zero by the finishing kernel).
_JOB_TABLES: dict = {}                           # (the device copies of recent job lists: a process-wide cache keyed by pointers, not pass state)


def _persistent_buffer(owner: torch.Tensor, name: str, numel: int, zero: bool) -> torch.Tensor:
    buf = getattr(owner, name, None)
    if buf is None or buf.numel() != numel or buf.device != owner.device:
        buf = (torch.zeros if zero else torch.empty)(numel, device=owner.device, dtype=torch.float32)
        setattr(owner, name, buf)
    return buf


# kind 0 unpacks the weight-gradient scratch `buf` (Cin a, Cout b, padded Cout c) into `dst`; kind 1 adds the column sums of a rows x b columns
# (row length c, 0 = b) of `buf`, from `byte_offset` on, to `dst`
def _defer_grad_job(buf: torch.Tensor, dst: torch.Tensor, kind: int, a: int, b: int, c: int, byte_offset: int = 0) -> None:
    """queue one finishing job for flush_param_grads() and keep its source buffer alive until then"""
    _PASS.jobs.append((buf.data_ptr() + byte_offset, dst.data_ptr(), kind, a, b, c))
    if not (_PASS.keep and _PASS.keep[-1] is buf):
        _PASS.keep.append(buf)


def _pending_src(buf: torch.Tensor) -> bool:
    """is this persistent buffer already the source of a deferred job of the current step?"""
    p_ = buf.data_ptr()
    return any(job[0] == p_ for job in _PASS.jobs)


def flush_param_grads() -> None:
    """finish every deferred weight / bias gradient on the current stream (callers have joined the weight-gradient stream first)"""
    bp = _PASS
    if not bp.jobs:
        return
    key = tuple(bp.jobs)
    table = _JOB_TABLES.get(key)
    if table is None:
        import struct
        raw = b"".join(struct.pack("<QQiiii", *job) for job in key)
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(bp.keep[0].device)
        if len(_JOB_TABLES) > 8:
            _JOB_TABLES.clear()
        _JOB_TABLES[key] = table
    lib.call("pulpo_grad_finish_multi", _ptr(table), len(key), _stream())
    bp.jobs.clear()
    bp.keep.clear()


def reset_param_grad_buffers(module: Optional[torch.nn.Module] = None) -> None:
    """after an interrupted step: forget the pending jobs and drop the persistent scratch buffers (they may hold partial sums)"""
    for pending in (_PASS.jobs, _PASS.keep, _PASS.bn_parts):
        pending.clear()
    if module is not None:
        for p_ in module.parameters():
            for name in ("_pulpo_wgrad_scratch", "_pulpo_dbias_part", "_pulpo_dbias_part_in", "_pulpo_heads_part"):
                if hasattr(p_, name):
                    delattr(p_, name)


# ---- the gradient of a ConvUnit's pre-norm tensor in a channel-BLOCKED layout (round 5).  dy leaves the BatchNorm backward for exactly two readers,
# the unit's data- and weight-gradient convolution (aten::convolution_backward, src/network_blocks.py:23): its layout is nobody else's business.
# Channels-last, a staging item of the F(2x2x2,3x3x3) data-gradient kernel gathers 32 useful bytes from each of four 128-byte voxel lines per
# 8-channel chunk and the kernel waits on those lines (32 -> 32 at 160^3: 0.94 ms, 0.80 with every tap a cache hit); as [C / 8][B][D][H][W][8] the four
# taps are 128 consecutive bytes: 0.80 ms (scripts/blocked_probe.py).  Used where BOTH readers run their F(2x2x2) kernel on a volume of at least
# BLOCKED_DY_MIN_VOXELS voxels (below ~64^3 the tensors live in the caches and the layouts tie).  PULPO_BLOCKED_DY=0: channels-last everywhere.
BLOCKED_DY = os.environ.get("PULPO_BLOCKED_DY", "1") != "0"
BLOCKED_DY_MIN_VOXELS = int(os.environ.get("PULPO_BLOCKED_DY_MIN_VOXELS", str(64 ** 3)))
BLOCKED_DY_HITS = 0              # gradients written in the blocked layout so far (tests look at it)


class _BlockedGrad:
    """fp32 operand in the layout [C / 8][B][D][H][W][8]: element (b, v, c) at  b * bs + (c // 8) * kb + v * ps + c % 8  of `buf`"""
    __slots__ = ("buf", "shape", "bs", "ps", "kb", "dtype", "device")

    def __init__(self, B, C, D, H, W, dev, buf=None):
        self.buf = torch.empty(B * C * D * H * W, device=dev, dtype=torch.float32) if buf is None else buf
        self.shape = (B, C, D, H, W)
        self.ps, self.bs, self.kb = 8, D * H * W * 8, B * D * H * W * 8
        self.dtype, self.device = torch.float32, self.buf.device

    @classmethod
    def of(cls, t6: torch.Tensor):
        """the operand view of a blocked 6-D tensor (is_blocked)"""
        B, C, D, H, W = blocked_shape(t6)
        return cls(B, C, D, H, W, t6.device, buf=t6)

    def to_cl(self) -> torch.Tensor:
        """the same values as a channels-last (B, C, D, H, W) tensor (tests, fallbacks)"""
        B, C, D, H, W = self.shape
        return self.buf.view(C // 8, B, D, H, W, 8).permute(1, 0, 5, 2, 3, 4).reshape(B, C, D, H, W).contiguous(memory_format=CL)


# ---- blocked ACTIVATIONS between the ConvUnits of a ConvSequence (round 5).  The output z of every unit but the last has two readers, the next
# unit's convolution (forward pass) and weight gradient (src/network_blocks.py:40-46) - where both run their F(2x2x2,3x3x3) kernel it is produced as a
# contiguous fp32 tensor of shape (C / 8, B, D, H, W, 8) (`is_blocked`: six dimensions), and autograd carries its gradient in the same shape: the next
# unit's data-gradient kernel writes dz blocked, this unit's BatchNorm backward reads it that way.  A forward hook on such a ConvUnit sees the 6-D
# tensor (blocked_to_cl() gives the usual view).
# OFF by default (PULPO_BLOCKED_Z=1 / ops.BLOCKED_Z = True turns it on): alone on the machine the 32 -> 32 forward convolution at 160^3 gains 15 - 18 %
# (0.95 -> 0.78 ms, profiles/r5_blocked_probe.txt), but inside the training step it already runs at 0.80 ms on channels-last input - the activation has
# just been written and its tail still sits in the 256 MB Infinity Cache - and gains 3 - 5 %, while the data-gradient kernel that now stores a blocked
# dz loses 2.5 % and the weight gradient 1.5 %: 26.53 against 26.55 ms per step, same box (profiles/r5_blocked_z_ab.txt).  The blocked dy above, whose
# producer and consumers are all streaming / staging kernels of the backward pass, keeps 0.14 ms.
BLOCKED_Z = os.environ.get("PULPO_BLOCKED_Z", "0") == "1"
BLOCKED_Z_MIN_VOXELS = int(os.environ.get("PULPO_BLOCKED_Z_MIN_VOXELS", str(64 ** 3)))
BLOCKED_Z_HITS = 0               # activations written in the blocked layout so far (tests look at it)


def is_blocked(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dim() == 6


def blocked_shape(t: torch.Tensor):
    Cb, B, D, H, W, e = t.shape
    if e != 8:
        raise PulpoHipError(f"a six-dimensional activation must be channel-blocked (C / 8, B, D, H, W, 8), got {tuple(t.shape)}")
    return B, Cb * 8, D, H, W


def blocked_to_cl(t: torch.Tensor) -> torch.Tensor:
    """(C / 8, B, D, H, W, 8) -> channels-last (B, C, D, H, W); differentiable"""
    B, C, D, H, W = blocked_shape(t)
    return t.permute(1, 0, 5, 2, 3, 4).reshape(B, C, D, H, W).contiguous(memory_format=CL)


def cl_to_blocked(t: torch.Tensor) -> torch.Tensor:
    B, C, D, H, W = t.shape
    return t.permute(0, 2, 3, 4, 1).reshape(B, D, H, W, C // 8, 8).permute(4, 0, 1, 2, 3, 5).contiguous()


def _opnd(t):
    """(tensor to take the pointer of, batch stride, pixel stride, block stride, blocked?) of a convolution operand / result"""
    if isinstance(t, _BlockedGrad):
        return t.buf, t.bs, t.ps, t.kb, True
    if t.dim() == 6:
        B, C, D, H, W = blocked_shape(t)
        return t, D * H * W * 8, 8, B * D * H * W * 8, True
    b, p, c = grid_strides(t)
    return t, b, p, 8, False


def _dims5(t):
    return t.shape if isinstance(t, _BlockedGrad) else (blocked_shape(t) if t.dim() == 6 else tuple(t.shape))


# The Python predicate of a fused path has to agree with the C entry point's own check, so what the sites ask differently is an argument:
# C - the channel count must be a multiple of four as well; align - the streaming kernels move four-channel groups of the storage type (8 bytes
# of bf16); batch=False - sites that pin the batch stride themselves (== voxels * pixel stride).  A blocked operand keeps a voxel's eight channels together.
def _vec4(t, C: Optional[int] = None, align: int = 16, batch: bool = True) -> bool:
    """may a kernel read or write this operand with 16-byte channel vectors (channel stride 1, pixel and batch stride % 4, pointer % align)?"""
    buf, b, p, _, blk = _opnd(t)
    return (blk or t.stride(1) == 1) and p % 4 == 0 and (not batch or b % 4 == 0) and (C is None or C % 4 == 0) and buf.data_ptr() % align == 0


def _cl_rows4(t: torch.Tensor) -> bool:
    """channels-last with a pixel stride of whole four-channel groups (what the BatchNorm-backward kernels that write a blocked dy read)"""
    return is_cl(t) and t.stride(4) % 4 == 0


def blocked_z_wanted(x, unit_weight, next_weight, training: bool) -> bool:
    """should the ConvUnit with `unit_weight`, applied to x, hand its output to the unit with `next_weight` in the blocked layout?"""
    if not (BLOCKED_Z and training and torch.is_grad_enabled() and CONV_PRECISION == "fp32" and not ACT_BF16 and next_weight.requires_grad
            and isinstance(x, torch.Tensor) and x.dim() in (5, 6) and x.is_cuda):
        return False
    B, _, D, H, W = _dims5(x)
    C, Cn = unit_weight.shape[0], next_weight.shape[0]
    if C % 8 or next_weight.shape[1] != C or D * H * W < BLOCKED_Z_MIN_VOXELS or 4 * B * max(C, Cn) * D * H * W >= 2 ** 31:
        return False
    if lib.query("pulpo_conv3d_k3_wgrad_algo", B, D, H, W, C, Cn, 1) != 3:
        return False
    shape = (B, D, H, W)
    return (getattr(_pack_weight(next_weight, False, shape=shape, both=True), "_pulpo_algo", "") == "wino3"
            and getattr(_pack_weight(next_weight, True, shape=shape), "_pulpo_algo", "") == "wino3")


def _blocked_dy_ok(x, y, weight, wpt, need_dx: bool, need_dw: bool) -> bool:
    B, Cin, D, H, W = _dims5(x)
    Cout = weight.shape[0]
    if not (BLOCKED_DY and need_dx and y.dtype == torch.float32 and Cout % 8 == 0 and D * H * W >= BLOCKED_DY_MIN_VOXELS
            and getattr(wpt, "_pulpo_algo", "") == "wino3" and 4 * B * Cout * D * H * W < 2 ** 31):
        return False
    if need_dw:
        if _use_bf16(Cin) or x.dtype != torch.float32 or lib.query("pulpo_conv3d_k3_wgrad_algo", B, D, H, W, Cin, Cout, 1) != 3:
            return False
        if not is_blocked(x) and not _vec4(x, Cin):
            return False
    return True


def _wgrad_target(Cin: int, Cout: int, into: Optional[torch.Tensor], owner: Optional[torch.Tensor], dev):
    """where a weight-gradient launch puts its result: (dw, the kernels' accumulate mode, packed-sum scratch, deferred?)"""
    # (mode 0 writes dw, 1 adds to it, 2 - deferred: `into` and its `owner` parameter, data-parallel stepper - leaves the packed sums in the
    #  parameter's persistent scratch for flush_param_grads())
    deferred = into is not None and owner is not None
    dw = into if into is not None else torch.empty((Cout, Cin, 3, 3, 3), device=dev, dtype=torch.float32)
    nscr = lib.query("pulpo_conv3d_k3_wgrad_scratch_floats", Cin, Cout)
    scratch = _persistent_buffer(owner, "_pulpo_wgrad_scratch", nscr, zero=True) if deferred else torch.empty(nscr, device=dev, dtype=torch.float32)
    return dw, (2 if deferred else int(into is not None)), scratch, deferred


def _wgrad_raw(x: torch.Tensor, dy: torch.Tensor, Cin: int, Cout: int, into: Optional[torch.Tensor] = None,
               owner: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> Optional[torch.Tensor]:
    """weight gradient; `into` -> accumulated into that (Cout,Cin,3,3,3) tensor in place, returns None.  With `owner` (the weight parameter,
    data-parallel stepper) the accumulation is DEFERRED to flush_param_grads(): the packed sums stay in the parameter's persistent scratch.
    max_workgroups > 0: the fp32 Winograd kernels launch at most that many workgroups (pulpo_conv3d_k3_wgrad_wg; the other kernels ignore it)."""
    B, _, D, H, W = _dims5(x)
    if is_blocked(x) and (_use_bf16(Cin) or lib.query("pulpo_conv3d_k3_wgrad_algo", B, D, H, W, Cin, Cout, 1) != 3):
        x = blocked_to_cl(x)                         # (a blocked operand outside the F(2x2x2,3x3x3) kernel's shapes: a copy - BLOCKED_Z switched between passes)
    dw, mode, scratch, deferred = _wgrad_target(Cin, Cout, into, owner, x.device)
    xblk = is_blocked(x)
    xt, xb, xp, xkb, _ = _opnd(x)
    xc = 1 if xblk else grid_strides(x)[2]
    blocked = isinstance(dy, _BlockedGrad) or xblk
    if blocked and not isinstance(dy, _BlockedGrad):
        dy = to_cl(dy.float())
    db, dp, dc = (dy.bs, dy.ps, 1) if isinstance(dy, _BlockedGrad) else grid_strides(dy)
    t0 = _trace_begin()
    sfx = "_bf16" if _use_bf16(Cin) else ""
    wg, wga = ("_wg", (int(max_workgroups),)) if max_workgroups else ("", ())
    det = ()
    if DETERMINISTIC:
        # one zero-initialised copy of the packed sums per spatial split of the grid (<= ~110 MB, transient), added up in fixed order
        nslab = lib.query("pulpo_conv3d_k3_wgrad_det_slabs", Cin, Cout)
        slabs = torch.empty(nslab * scratch.numel(), device=x.device, dtype=torch.float32)
        det = (_ptr(slabs), nslab)
    if blocked:
        # (_blocked_dy_ok has checked: fp32 operands, channels-last x, the F(2x2x2,3x3x3) weight-gradient kernel takes the shape)
        dyt, _, _, dkb, _ = _opnd(dy)
        lib.call("pulpo_conv3d_k3_wgrad_kb" + wg, _ptr(xt), xb, xp, xkb, _ptr(dyt), db, dp, dkb, _ptr(dw), mode, _ptr(scratch),
                 *(det if det else (None, 0)), B, D, H, W, Cin, Cout, _stream(), *wga)
    else:
        # (one storage type per launch: the bf16 kernels take either - a mixed pair, a user's fp32 input to a bf16-storage unit, is rare -, the others fp32)
        if x.dtype != dy.dtype or (not sfx and x.dtype != torch.float32):
            x, dy = x.float(), dy.float()
            xb, xp, xc = grid_strides(x)
            db, dp, dc = grid_strides(dy)
        if sfx:
            lib.call("pulpo_conv3d_k3_wgrad_bf16_det_t" if det else "pulpo_conv3d_k3_wgrad_bf16_t", _ptr(x), xb, xp, xc, _ptr(dy), db, dp, dc, _dt(x), _ptr(dw),
                     mode, _ptr(scratch), *det, B, D, H, W, Cin, Cout, _stream())
        else:
            lib.call(("pulpo_conv3d_k3_wgrad_det" if det else "pulpo_conv3d_k3_wgrad") + wg, _ptr(x), xb, xp, xc, _ptr(dy), db, dp, dc, _ptr(dw),
                     mode, _ptr(scratch), *det, B, D, H, W, Cin, Cout, _stream(), *wga)
    if deferred and not _pending_src(scratch):
        # (ONE finishing job per scratch: a unit applied twice in a step - shared weights, two forward passes - has accumulated both weight
        #  gradients into the same packed sums by the time the job runs)
        _defer_grad_job(scratch, dw, 0, Cin, Cout, (Cout + 63) // 64 * 64)
    if t0 is not None:
        name = "conv3d_k3_wgrad_bf16"
        if blocked:
            name = "conv3d_k3_wgrad_w3x"
        elif not sfx:
            vec = int(_vec4(x, Cin) and _vec4(dy, Cout))
            name = {0: "conv3d_k3_wgrad_mfma", 2: "conv3d_k3_wgrad_w2", 3: "conv3d_k3_wgrad_w3x"}[lib.query("pulpo_conv3d_k3_wgrad_algo", B, D, H, W, Cin, Cout, vec)]
        _trace_end(t0, name + ("" if deferred else "(+memset,unpack)"), 54.0 * Cin * Cout * B * D * H * W, ((4 if blocked else _esize(x)) * Cin + (4 if blocked else _esize(dy)) * Cout) * B * D * H * W)
    return None if into is not None else dw


# Weight gradients off the critical path.  Inside a data-parallel step the weight gradient goes straight into the gradient arena and
# nothing reads it before the all-reduce, so it need not finish before the backward pass moves on: it is queued on a second HIP
# stream BEHIND this unit's data-gradient kernel, where the matrix-bound persistent kernel (one workgroup per CU) runs next to the
# HBM-bound BatchNorm / LeakyReLU backward passes of the preceding unit on the main stream.  Joined before the gradient exchange
# (dp.DataParallelStepper).  The stream is _PASS.side; None = disabled (plain autograd use: gradients are returned on the caller's stream).
def _on_side_stream(launch, operands) -> None:
    side = _PASS.side
    side.wait_stream(torch.cuda.current_stream())        # after everything queued so far: dy, this unit's data gradient, zero_grad
    with torch.cuda.stream(side):
        launch()
    for t in operands:                           # keep the operands' memory out of the allocator's hands until the side stream is done
        t.record_stream(side)


def _wgrad_on_side_stream(x, dy, Cin, Cout, slot_w, owner):
    _on_side_stream(lambda: _wgrad_raw(x, dy, Cin, Cout, into=slot_w, owner=owner), (x, dy.buf if isinstance(dy, _BlockedGrad) else dy))


def join_async_wgrad():
    """make the current stream wait for every weight gradient queued on the side stream, then finish the deferred parameter gradients"""
    if _PASS.side is not None:
        torch.cuda.current_stream().wait_stream(_PASS.side)
    if _PASS.window is not None:
        _PASS.window.join()
    flush_param_grads()


# ---- The coarse window (round 6).  In the backward pass of a pyramid the levels of at most `coarse_voxels` voxels (20^3 and 10^3 at 160^3: the
# latent levels 3 and 4, then DownPath's two coarsest blocks) are a stretch of ~2.5 ms in which no kernel of the main stream can fill the machine:
# a hundred 5 - 12 us kernels on a few workgroups, data gradients of 270 work items, weight gradients whose split count is capped by their step
# count.  Weight gradients are leaves - nothing reads them before the gradient exchange / Adam - so
#   * the window's own weight gradients go to the side stream instead of in line, and
#   * the last weight gradients produced ABOVE the window (the 40^3 / 80^3 latent levels), as many as fit `defer_flop`, are HELD BACK and queued
#     on the side stream when the window opens,
# all under a workgroup budget (`max_workgroups`, pulpo_conv3d_k3_wgrad_wg): a full-grid F(2x2x2,3x3x3) weight gradient holds every CU whole and
# can only time-slice with the main stream (why "everything on the side stream" lost for fp32), a 192-workgroup one holds 24
# CUs per XCD and leaves the other 8 to the main stream's small kernels (measured: 192 is the best budget, 128 loses to in-line launches, and
# the side stream may overrun the window - profiles/r6_window_ab.txt).  Which jobs to hold is learnt from the previous backward pass (the
# sequence of weight gradients seen above the window; its last entries within the FLOP budget), so the first pass of a model holds nothing.
# _PASS.window, from dp.DataParallelStepper.backward (fp32, non-deterministic, direct parameter gradients); None = off (plain autograd use).
class CoarseWindow:
    ABOVE, INSIDE, BELOW = 0, 1, 2

    def __init__(self, stream, coarse_voxels: int, max_workgroups: int, defer_flop: float, exit_wait: bool):
        self.stream, self.coarse_voxels, self.max_workgroups = stream, int(coarse_voxels), int(max_workgroups)
        self.defer_flop, self.exit_wait = float(defer_flop), bool(exit_wait)
        self._plan_sig, self._plan = None, frozenset()
        self.deferred_last = 0                   # weight gradients held back in the last backward pass (tests / describe())
        self.begin()

    def begin(self) -> None:
        """a backward pass starts"""
        self.state, self.held, self.seen, self.used = self.ABOVE, [], [], False
        self.keep = []                           # operands of launches queued on the side stream the main stream has not waited for yet

    def _budgeted(self, x, dy, Cin, Cout) -> bool:
        """does this weight gradient run a kernel that takes the workgroup budget?"""
        B, _, D, H, W = _dims5(x)
        return (not _use_bf16(Cin) and x.dtype == torch.float32 and dy.dtype == torch.float32
                and lib.query("pulpo_conv3d_k3_wgrad_grid", B, D, H, W, Cin, Cout, self.max_workgroups) > 0)

    def _to_side(self, jobs) -> None:
        side = self.stream
        side.wait_stream(torch.cuda.current_stream())        # after everything queued so far (the operands' producers)
        with torch.cuda.stream(side):
            for x, dy, Cin, Cout, slot_w, owner in jobs:
                _wgrad_raw(x, dy, Cin, Cout, into=slot_w, owner=owner, max_workgroups=self.max_workgroups)
        # The operands stay referenced until the main stream - the stream they were allocated on - has waited for the side stream (the window's
        # exit, or join()): from then on everything the main stream does is ordered behind these launches and the allocator may hand the memory
        # out again.  (Not record_stream(): a block it has marked returns to the pool whenever its event happens to have completed, so which block
        # the next tensors get, and with it the allocator's rounding, would vary from step to step.)
        self.keep.extend(t for x, dy, *_ in jobs for t in (x, dy))
        self.used = True

    def visit(self, voxels: int) -> None:
        """a convolution's backward on a volume of `voxels` voxels per batch element begins: opens / closes the window"""
        if voxels <= self.coarse_voxels:
            if self.state != self.INSIDE:
                if self.state == self.ABOVE:     # the plan of the next pass: the last jobs seen above the window that fit the FLOP budget
                    sig = tuple(self.seen)
                    if sig != self._plan_sig:
                        plan, total = set(), 0.0
                        for key, flop in reversed(sig):
                            if total + flop > self.defer_flop:
                                break
                            plan.add(key)
                            total += flop
                        self._plan_sig, self._plan = sig, frozenset(plan)
                self.deferred_last = len(self.held)
                if self.held:
                    self._to_side(self.held)
                    self.held = []
                self.state = self.INSIDE
        elif self.state == self.INSIDE:
            self.state = self.BELOW
            if self.exit_wait and self.used:     # the full-grid levels that follow do not share the machine with an overrun of the side stream
                torch.cuda.current_stream().wait_stream(self.stream)
                self.keep = []

    def wgrad(self, x, dy, Cin, Cout, slot_w, owner) -> None:
        """the weight gradient of the unit whose backward visit() has just seen"""
        job = (x, dy, Cin, Cout, slot_w, owner)
        if self.state == self.INSIDE:
            self._to_side([job])
            return
        if self.state == self.ABOVE and self._budgeted(x, dy, Cin, Cout):
            B, _, D, H, W = _dims5(x)
            key = id(owner)
            self.seen.append((key, 54.0 * Cin * Cout * B * D * H * W))
            if key in self._plan:
                self.held.append(job)
                return
        _wgrad_raw(x, dy, Cin, Cout, into=slot_w, owner=owner)

    def join(self) -> None:
        """launch what is still held (a pass without a coarse level, a gradient bucket that leaves early) in line and wait for the side stream"""
        for x, dy, Cin, Cout, slot_w, owner in self.held:
            _wgrad_raw(x, dy, Cin, Cout, into=slot_w, owner=owner)
        self.held = []
        if self.used:
            torch.cuda.current_stream().wait_stream(self.stream)
        self.keep = []


# ---- BatchNorm-backward reduction inside the data-gradient convolution.  In a ConvSequence unit u consumes z = lrelu(bn(y)) of unit u-1,
# and the gradient dz that unit u-1's backward receives is exactly what unit u's data-gradient kernel stores: that kernel's epilogue has
# every dz element in registers, so with y of unit u-1 read alongside it also delivers the per-tile sums (sum dbn, sum dbn * xhat) that
# unit u-1 would otherwise compute in a pass of its own over dz and y (pulpo_bn_lrelu_bwd_reduce).  The forward pass hands (y, coef) of
# the producer to the consumer on the tensor z itself (`_pulpo_bn_src`); the backward pass of the consumer leaves the sums here, keyed by
# the producer's y, and the producer takes them only if the gradient it is given IS that kernel's output, untouched (same storage, same
# version: a gradient that autograd accumulated from several consumers is a different tensor or carries a bumped version).  "Here" is
# _PASS.bn_parts: what a unit whose backward never runs leaves there goes with its pass (the default pass's when backward_pass() is next entered).
def _dgrad_with_bn_reduction(bn_src, x, dy, wpt, dx, K: int, N: int) -> bool:
    algo = getattr(wpt, "_pulpo_algo", "")
    if bn_src is None or not BN_REDUCE_IN_DGRAD or algo not in ("wino2", "wino3"):
        return False
    y_prev, coef_prev = bn_src
    B, _, D, H, W = _dims5(dy)
    dyt, db, dp, dkb, blocked = _opnd(dy)
    dc = 1 if blocked else grid_strides(dy)[2]
    dxt, ob, op, okb, oblk = _opnd(dx)
    if (blocked or oblk) and algo != "wino3":
        return False
    yb, yp, _ = grid_strides(y_prev)
    # (the C entry point also needs the gradient operand vectorisable: channels-last, 16-byte aligned, K % 4 == 0 - checked here so that a
    #  consumer unit with an odd channel count falls back to the separate reduction pass instead of raising in the middle of backward)
    vec_ok = blocked or _vec4(dy, K)
    if (not vec_ok or tuple(y_prev.shape) != tuple(_dims5(dx)) or not _vec4(dx) or not _vec4(y_prev) or not lib.query("pulpo_conv3d_k3_dgrad_wino2_bnred_ok", B, D, H, W, K, N)):
        return False
    ntile = lib.query("pulpo_conv3d_k3_stat_tiles", B, D, H, W)
    part = torch.empty(ntile * 2 * N, device=dy.device, dtype=torch.float32)
    t0 = _trace_begin()
    if blocked or oblk:
        lib.call("pulpo_conv3d_k3_dgrad_wino3_bnred_kb", _ptr(dyt), db, dp, dkb, _ptr(wpt), _ptr(dxt), ob, op, okb, _ptr(y_prev), yb, yp, _ptr(coef_prev),
                 LRELU_SLOPE, _ptr(part), B, D, H, W, K, N, _stream())
    else:
        lib.call(f"pulpo_conv3d_k3_dgrad_{algo}_bnred", _ptr(dy), db, dp, dc, _ptr(wpt), _ptr(dx), ob, op, _ptr(y_prev), yb, yp, _ptr(coef_prev), LRELU_SLOPE,
                 _ptr(part), B, D, H, W, K, N, _stream())
    kname = "conv3d_k3_wino3_mfma<true>" if algo == "wino3" else "conv3d_k3_wino2_mfma<true>"
    if algo == "wino2" and t0 is not None and lib.query("pulpo_conv3d_k3_wino2_pipelined", D, H, W, K, dp):
        kname = "conv3d_k3_wino2p_mfma<true>"
    _trace_end(t0, kname, 54.0 * K * N * B * D * H * W, 4.0 * (K + 2 * N) * B * D * H * W)
    _PASS.bn_parts[y_prev.data_ptr()] = (part, ntile, coef_prev.data_ptr(), dx.data_ptr(), dx._version, tuple(dx.shape), tuple(dx.stride()))
    return True


def _take_bn_tile_parts(y: torch.Tensor, coef: torch.Tensor, dz: torch.Tensor):
    entry = _PASS.bn_parts.pop(y.data_ptr(), None)
    if entry is None:
        return None
    part, ntile, coef_ptr, ptr, version, shape, stride = entry
    if coef.data_ptr() != coef_ptr or dz.data_ptr() != ptr or dz._version != version or tuple(dz.shape) != shape or tuple(dz.stride()) != stride:
        return None
    return part, ntile


# ---- producers that write straight into a slice of a wider channels-last buffer (round 5).  PULPoEncoder concatenates the up-sampled
# feedback path's output with the DownPath activation of its level (torch.cat([feedback, down_activation], 1), components/pulpo.py:252): two
# strided copy kernels per level and step (111 us at 80^3).  DownPath allocates the concatenation's buffer up front and its last ConvUnit, like
# the feedback path's later, writes its output into its channel range - every kernel addresses operands through explicit pixel strides, so the
# slices are ordinary operands, and the concatenation is the buffer itself (cat_prewritten).
def _out_slot(out, B, C, D, H, W, dev, dtype):
    """the channel range of `out` = (buffer, first channel) that a ConvUnit writes its result into, or None (no slot, or the shapes do not fit)"""
    if out is None:
        return None
    buf, off = out
    fits = (buf.dim() == 5 and tuple(buf.shape[2:]) == (D, H, W) and buf.shape[0] == B and buf.dtype == dtype and buf.device == dev and off >= 0
            and off + C <= buf.shape[1] and is_cl(buf) and off % 8 == 0 and buf.shape[1] % 8 == 0)
    return buf[:, off:off + C] if fits else None


CAT_PREWRITTEN_HITS = 0          # concatenations that cost nothing so far (tests look at it)


class _CatPrewritten(torch.autograd.Function):
    """cat([a, b], 1) where a and b ARE the two channel ranges of `buf`: the result is the buffer, the gradient is split by position"""

    @staticmethod
    def forward(ctx, a, b, buf):
        ctx.ca = a.shape[1]
        return buf.as_strided(buf.shape, buf.stride(), buf.storage_offset())

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.ca], g[:, ctx.ca:], None


def cat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], dim=1); free when both were produced into the two channel ranges of one buffer (`_pulpo_cat` tags)"""
    ta, tb = getattr(a, "_pulpo_cat", None), getattr(b, "_pulpo_cat", None)
    if ta is not None and tb is not None and ta[0] is tb[0]:
        buf = ta[0]
        es = buf.element_size()
        if (ta[1] == 0 and tb[1] == a.shape[1] and a.shape[1] + b.shape[1] == buf.shape[1] and a.data_ptr() == buf.data_ptr()
                and b.data_ptr() == buf.data_ptr() + es * tb[1] and a.stride() == buf.stride() and b.stride() == buf.stride()
                and a.shape[2:] == buf.shape[2:] and b.shape[2:] == buf.shape[2:] and a.shape[0] == buf.shape[0] == b.shape[0]):
            global CAT_PREWRITTEN_HITS
            CAT_PREWRITTEN_HITS += 1
            return _CatPrewritten.apply(a, b, buf)
    return torch.cat([a, b], dim=1)


# ---- the ConvUnit autograd node.  A Function takes and returns tensors, so everything else about one application travels in a _UnitCall: the
# caller (conv_bn_lrelu, the head wrappers) fills in what the node needs besides the tensors that can ask for a gradient, forward() fills in what
# the caller needs back.  backward() is five stages, each a function of plain values below:
#   1 _bwd_dz_source    the incoming gradients of the node's outputs -> where dz is read from (a _DzSource; None: no gradient arrived)
#   2 _bwd_bn_sums      the first BatchNorm-backward pass - per-tile (sum dbn, sum dbn * xhat) - and its finalize.  The sums come from one of four
#                       places: left behind by the data-gradient convolution (or pooling backward) that PRODUCED dz, if that was the operator behind
#                       this unit (_PASS.bn_parts); the pooled pass; the head's backward; else a pass of its own over dz and y
#   3 _bwd_bn_apply     the second pass writes dy, blocked or channels-last (_bn_apply_entry: the entry point for the source and dy's layout), and the
#                       conv-bias gradient's partial rows - except for the input layer, whose weight gradient forms dy itself (stage 4): no dy
#   4 _bwd_param_grads  the conv-bias gradient (deferred, or column sums now) and the weight gradient, which goes ONE of four ways: fused with the
#                       second pass (_input_layer_param_grads; scratch, accumulate mode and deferral as _wgrad_raw's); to the side stream behind
#                       this unit's data gradient (the job is handed to stage 5); to the coarse window (in line, held back, or on ITS side stream);
#                       in line
#   5 _bwd_data_grad    dx in x's layout - with the producing unit's BatchNorm reduction riding along where it can - then stage 4's side-stream job
class _UnitCall:
    __slots__ = ("bn_src", "out", "pool_after", "pool_only", "blocked_out", "training", "momentum", "eps", "running_mean", "running_var",
                 "num_batches_tracked", "head_nout", "head_eps", "head_params", "y", "coef", "pooled", "pool_only_done")

    def __init__(self, **given):
        assert not set(given) - set(self.__slots__), given
        # (forward() fills in the rest: the pre-norm tensor and coefficient block - the `_pulpo_bn_src` tag -, AvgPool(result) where the same pass
        #  wrote it, and whether that pooled tensor ALONE was returned)
        for name in self.__slots__:
            setattr(self, name, given.get(name))


# where a ConvUnit's backward reads dz, the gradient of its activation - exactly one of
#   dz      a tensor: channels-last, or (`blk`) blocked as the next unit's data-gradient kernel wrote it
#   pooled  (gpool, gskip or None): dz = gskip + avg_pool_backward(gpool), never written
#   head    (nout, the head kernels' pointer operands, the tensors behind them): dz = W^T dpre, never written
_DzSource = collections.namedtuple("_DzSource", "dz blk pooled head", defaults=(None, False, None, None))


# what backward() returns: one entry per argument of _ConvBNLReLU.forward (x, weight, bias, gamma, beta, head_w, head_b, call)
def _unit_grads(dx=None, dw=None, dbias=None, dgamma=None, dbeta=None, head_dw=None, head_db=None):
    return dx, dw, dbias, dgamma, dbeta, head_dw, head_db, None


def _fwd_heads(y, coef, head_w, head_b, head_eps, nout: int, dims):
    # the 1x1x1 head on the pre-norm tensor -> ([field] or [mu, sigma, sample], planar noise)
    _require_gpu(head_w, head_b, head_eps)
    B, Cout, D, H, W = dims
    V = D * H * W
    outs = [torch.empty((B, 3, D, H, W), device=y.device, dtype=torch.float32) for _ in range(1 if nout == 3 else 3)]
    epsc = planar(head_eps) if head_eps is not None else None
    t0 = _hbm_begin("heads_fwd_bn")
    lib.call("pulpo_heads_fwd_bn_t", _ptr(y), y.stride(4), _ptr(coef), LRELU_SLOPE, _ptr(head_w), _ptr(head_b), _ptr(epsc), _ptr(outs[0]),
             _ptr(outs[1]) if nout == 6 else None, _ptr(outs[2]) if nout == 6 else None, nout, B, V, Cout, _stream())
    _hbm_end(t0, "heads_fwd_bn", B * V * (4.0 * Cout + 4.0 * (12 if nout == 6 else 3)))       # read y (+ eps), write mu / sigma / z (or the field)
    return outs, epsc


def _fwd_bn_lrelu_apply(y, coef, call, dims, zdt):
    # z = lrelu(bn(y)) in the form its readers want -> (z or None, AvgPool(z) or None, pool_only?)
    B, Cout, D, H, W = dims
    dev, npix = y.device, B * D * H * W
    # pool_only: nobody reads the un-pooled activation (DownPath levels above the first latent level: only AvgPool(z) goes on) - it is not written
    pool_only = bool(call.pool_only and call.pool_after and lib.query("pulpo_bn_lrelu_apply_pool2_ok", Cout, y.stride(4), Cout, Cout))
    blocked_out = bool(call.blocked_out and call.training and not call.pool_after and not pool_only and zdt == y.dtype == torch.float32 and Cout % 8 == 0)
    z = None if (pool_only or blocked_out) else _out_slot(call.out, B, Cout, D, H, W, dev, zdt)
    if z is None and not pool_only and not blocked_out:
        z = new_cl(B, Cout, D, H, W, dev, zdt)
    pooled = None
    if blocked_out:
        # the next ConvUnit of the sequence reads z through its F(2x2x2,3x3x3) kernels only (blocked_z_wanted): [Cout / 8][B][D][H][W][8]
        global BLOCKED_Z_HITS
        BLOCKED_Z_HITS += 1
        z = torch.empty((Cout // 8, B, D, H, W, 8), device=dev, dtype=torch.float32)
        entry, args = "pulpo_bn_lrelu_apply_kb", (_ptr(y), y.stride(4), _ptr(z), 8, npix * 8, _ptr(coef), npix, Cout, LRELU_SLOPE)
    elif pool_only or (call.pool_after and lib.query("pulpo_bn_lrelu_apply_pool2_ok", Cout, y.stride(4), z.stride(4), Cout)):
        # the caller pools this output next (DownPath): z and AvgPool(z) from one read of y; avg_pool2_skip() picks the pooled tensor up
        pooled = new_cl(B, Cout, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, dev, zdt)
        entry, args = "pulpo_bn_lrelu_apply_pool2_t", (_ptr(y), _dt(y), y.stride(4), _ptr(z), _dt(pooled), z.stride(4) if z is not None else Cout, _ptr(pooled),
                                                       pooled.stride(4), _ptr(coef), B, D, H, W, Cout, LRELU_SLOPE)
    else:
        entry, args = "pulpo_bn_lrelu_apply_t", (_ptr(y), _dt(y), y.stride(4), _ptr(z), _dt(z), z.stride(4), _ptr(coef), npix, Cout, LRELU_SLOPE)
    t0 = _hbm_begin("bn_lrelu_apply")
    lib.call(entry, *args, _stream())
    _hbm_end(t0, "bn_lrelu_apply", (_esize(y) + (0 if pool_only else (2.0 if zdt == torch.bfloat16 else 4.0))) * Cout * npix)      # read y, write z
    return z, pooled, pool_only


class _ConvBNLReLU(torch.autograd.Function):
    """ConvUnit: Conv3d(k3,p1,bias) -> BatchNorm3d -> LeakyReLU(0.2)   (reference src/network_blocks.py:22-26)"""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, head_w, head_b, call: _UnitCall):
        """call.head_nout = 3 / 6 (_conv_bn_lrelu_heads): the unit's activation is read by a 1x1x1 head (head_w [nout][Cout], head_b [nout], call.head_eps)
        and by nothing else - the node returns the head's outputs, and neither the activation nor its gradient is written"""
        _require_gpu(x, act=True)
        _require_gpu(weight, bias, gamma, beta)
        training = call.training
        ctx.bn_src = call.bn_src
        # x: (B, C, D, H, W), or the blocked output (C / 8, B, D, H, W, 8) of the previous ConvUnit of the sequence (is_blocked)
        ctx.dx_blocked = is_blocked(x)
        if not ctx.dx_blocked:
            x = as_grid(x)
        B, Cin, D, H, W = _dims5(x)
        Cout = weight.shape[0]
        dev = x.device
        wp = _pack_weight(weight, dgrad=False, shape=(B, D, H, W), both=bool(training and ctx.needs_input_grad[0]))
        # storage types (ACT_BF16): z - what the next operator reads - is bf16; the pre-norm tensor y is bf16 when the bf16-operand kernel
        # produces it and fp32 behind the exact-fp32 kernel of the <= 4-channel input layers; the kernels take operand and result in ONE type
        half_conv = ACT_BF16 and wp._pulpo_algo == "bf16"
        if ctx.dx_blocked and (wp._pulpo_algo != "wino3" or half_conv or not training):
            x = blocked_to_cl(x)                     # (a blocked activation in front of another kernel family: the producer's check and this call disagree - a copy)
        if x.dtype != (torch.bfloat16 if half_conv else torch.float32):
            x = x.to(torch.bfloat16 if half_conv else torch.float32)
        ydt = torch.bfloat16 if half_conv else torch.float32
        zdt = act_dtype()
        y = new_cl(B, Cout, D, H, W, dev, ydt)
        coef = torch.empty(8 * Cout, device=dev, dtype=torch.float32)      # [4][C] floats + [2][C] doubles
        if training:
            ntile = lib.query("pulpo_conv3d_k3_fwd_bf16_stat_tiles" if wp._pulpo_algo == "bf16" else "pulpo_conv3d_k3_stat_tiles", B, D, H, W)
            stats = torch.empty(ntile * 2 * Cout, device=dev, dtype=torch.float32)
            _conv_raw(x, wp, bias, y, Cin, Cout, stats)
            nsd = lib.query("pulpo_bn_fwd_finalize_scratch_doubles", ntile, Cout)
            scratch = torch.empty(nsd, device=dev, dtype=torch.float64) if nsd else None
            lib.call("pulpo_bn_fwd_finalize", _ptr(stats), ntile, Cout, float(B * D * H * W), _ptr(gamma), _ptr(beta), _ptr(call.running_mean),
                     _ptr(call.running_var), _ptr(call.num_batches_tracked), call.momentum, call.eps, _ptr(coef), _ptr(scratch), _stream())
        else:
            lib.call("pulpo_bn_eval_coef", _ptr(gamma), _ptr(beta), _ptr(call.running_mean), _ptr(call.running_var), call.eps, Cout, _ptr(coef), _stream())
            if not any(ctx.needs_input_grad) and ydt == zdt:
                # inference: conv + folded BatchNorm + LeakyReLU in one kernel, the pre-norm tensor is never written
                zo = _out_slot(call.out, B, Cout, D, H, W, dev, zdt)
                if zo is not None:
                    y = zo
                _conv_raw(x, wp, bias, y, Cin, Cout, None, coef=coef)
                return y
            _conv_raw(x, wp, bias, y, Cin, Cout, None)
        ctx.training = training
        ctx.params = (weight, bias, gamma, beta)      # for a direct pass (their .grad slots)
        ctx.pool_only = False
        ctx.head = (call.head_nout, call.head_params) if call.head_nout else None
        if call.head_nout:
            # (_conv_bn_lrelu_heads has checked: training statistics, fp32 storage, no pooling, no output slot)
            outs, epsc = _fwd_heads(y, coef, head_w, head_b, call.head_eps, call.head_nout, (B, Cout, D, H, W))
            ctx.save_for_backward(x, weight, y, coef, head_w, epsc, outs[1] if call.head_nout == 6 else None)
            return outs[0] if call.head_nout == 3 else tuple(outs)
        z, pooled, pool_only = _fwd_bn_lrelu_apply(y, coef, call, (B, Cout, D, H, W), zdt)
        ctx.save_for_backward(x, weight, y, coef)
        call.y, call.coef, call.pooled, call.pool_only_done = y, coef, pooled, pool_only      # read back by conv_bn_lrelu
        ctx.pool_only = pool_only
        if pool_only:
            ctx.set_materialize_grads(False)
            return pooled
        if pooled is not None:
            # (round 5) z AND AvgPool(z) are outputs of this node: their gradients arrive together, and the backward pass forms
            # dz = gz + avg_pool_backward(gpooled) per element inside the BatchNorm-backward passes instead of writing it
            ctx.set_materialize_grads(False)
            return z, pooled
        return z

    @staticmethod
    def backward(ctx, *grads):
        x, weight, y, coef = ctx.saved_tensors[:4]
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        B, Cin, D, H, W = _dims5(x)
        dims = (B, Cin, weight.shape[0], D, H, W)
        nblk = lib.query("pulpo_bn_bwd_blocks", B * D * H * W, dims[2])
        src = _bwd_dz_source(grads, ctx.head, ctx.pool_only, ctx.saved_tensors, y, dims)
        if src is None:
            return _unit_grads()
        src, totd, slot_w, slot_b, dgamma, dbeta, head_dw, head_db = _bwd_bn_sums(
            src, y, coef, dims, nblk, ctx.training, ctx.params, ctx.needs_input_grad, ctx.head)
        # the data-gradient weights now (cached pack): their kernel family decides dy's layout
        wpt = _pack_weight(weight, dgrad=True, shape=(B, D, H, W)) if need_dx else None
        dy, bias_rows = _bwd_bn_apply(src, x, weight, y, coef, totd, wpt, dims, nblk, (need_dx, need_dw, need_db), ctx.params[1], slot_b)
        dw, dbias, side_job = _bwd_param_grads(src, x, dy, bias_rows, y, coef, totd, dims, (need_dw, need_db), ctx.params, slot_w, slot_b)
        dx = _bwd_data_grad(x, dy, wpt, ctx.bn_src, ctx.dx_blocked, dims, side_job)
        return _unit_grads(dx, dw, dbias, dgamma, dbeta, head_dw, head_db)


def _bwd_dz_source(grads, head, pool_only: bool, saved, y, dims) -> Optional[_DzSource]:
    B, _, Cout, D, H, W = dims
    dev = y.device
    dz, dpool, dsample = (grads + (None, None))[:3]
    if head is not None:                         # (the node's outputs are the head's: the field, or mu / sigma / sample)
        g = [planar(t) if t is not None else None for t in (dz, dpool, dsample)]
        if head[0] == 3 and g[0] is None:
            g[0] = torch.zeros((B, 3, D, H, W), device=dev)
        hw, heps, hsigma = saved[4:7]
        return _DzSource(head=(head[0], (_ptr(hw), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(heps), _ptr(hsigma)), (hw, g, heps, hsigma)))
    if pool_only:                                # (the node's only output is the pooled tensor)
        dz, dpool = None, dz
    dz_blk = is_blocked(dz)                      # the gradient of a blocked activation arrives blocked (the next unit's data-gradient kernel wrote it so)
    if dz_blk and (dz.dtype != torch.float32 or not dz.is_contiguous() or tuple(blocked_shape(dz)) != (B, Cout, D, H, W)):
        dz, dz_blk = blocked_to_cl(dz.float()), False
    if dpool is None:
        if dz is None:
            return None
        return _DzSource(dz if dz_blk else to_cl(dz), dz_blk)
    gp = to_cl(dpool)
    gz = dz
    if gz is not None and gz.dtype != gp.dtype:
        gz = gz.to(gp.dtype)
    grp = 4 * int(_esize(gp))                    # bytes of a four-channel group
    skip_ok = gz is None
    if gz is not None:
        sb, sp, _ = grid_strides(gz)
        skip_ok = _dense_grid(gz) and sb == D * H * W * sp and _vec4(gz, align=grp, batch=False)
    if (Cout // 4 <= 256 and skip_ok and _vec4(gp, Cout, align=grp, batch=False) and _vec4(y, align=4 * int(_esize(y)), batch=False)
            and _dense_grid(y) and POOLED_BN_BACKWARD):
        return _DzSource(pooled=(gp, gz))
    # shapes the fused passes do not take: the gradient as a tensor, then the plain path
    gin = new_cl(B, Cout, D, H, W, dev, gp.dtype)
    add = skip_ok and gz is not None             # (the kernel adds the skip gradient where it can read it in four-channel groups)
    lib.call("pulpo_avgpool2_bwd_t", _ptr(gp), gp.stride(4), _ptr(gz) if add else None, grid_strides(gz)[1] if add else 0, _ptr(gin), gin.stride(4), _dt(gp),
             B, D, H, W, Cout, _stream())
    return _DzSource(to_cl(gin if (add or gz is None) else gin + gz), False)


def _bwd_bn_sums(src: _DzSource, y, coef, dims, nblk: int, training: bool, params, needs, head):
    # -> (src, totd, slot_w, slot_b, dgamma, dbeta, head_dw, head_db)
    B, _, Cout, D, H, W = dims
    dev, npix = y.device, B * D * H * W
    head_dw = head_db = None
    if src.pooled is not None:
        gp, gz = src.pooled
        rows, nrow = torch.empty(nblk * 2 * Cout, device=dev, dtype=torch.float32), nblk
        t0 = _hbm_begin("avgpool2_bwd_bnred")
        lib.call("pulpo_avgpool2_bwd_bnred_t", _ptr(gp), gp.stride(4), _ptr(gz), grid_strides(gz)[1] if gz is not None else 0, None, 0, _dt(gp), _ptr(y), _dt(y),
                 y.stride(4), _ptr(coef), LRELU_SLOPE, _ptr(rows), B, D, H, W, Cout, _stream())
        # read the pooled gradient, the skip gradient and y (the summed gradient is not written)
        _hbm_end(t0, "avgpool2_bwd_bnred", Cout * (_esize(gp) * (gp.numel() // Cout + (npix if gz is not None else 0)) + _esize(y) * npix))
    elif src.head is not None:
        # the head's backward and this unit's first BatchNorm-backward pass in one kernel over y: dz = W^T dpre is formed per element for the sums
        # (and again by the second pass) and never written
        (nout, hparams), V = head, D * H * W
        nrow = lib.query("pulpo_heads_bwd_blocks", B, V, Cout)
        hpart, hslots = _heads_part_rows(hparams, needs[5] and needs[6], nrow, nout, Cout, dev)
        rows = torch.empty(nrow * 2 * Cout, device=dev, dtype=torch.float32)
        t0 = _hbm_begin("heads_bwd_bn")
        lib.call("pulpo_heads_bwd_bn_t", _ptr(y), y.stride(4), _ptr(coef), LRELU_SLOPE, *src.head[1], _ptr(hpart), _ptr(rows), nout, B, V, Cout, _stream())
        _hbm_end(t0, "heads_bwd_bn", B * V * (4.0 * Cout + 4.0 * (15 if nout == 6 else 3)))       # read y and the output gradients (+ eps, sigma)
        head_dw, head_db = _heads_finish_rows(hpart, hslots, hparams, nrow, nout, Cout)
    else:
        tiles = _take_bn_tile_parts(y, coef, src.dz)
        if tiles is not None:
            rows, nrow = tiles
        else:
            if src.blk:                          # (the separate reduction pass reads channels-last: autograd summed several gradients of z - a copy)
                src = _DzSource(blocked_to_cl(src.dz), False)
            dz = src.dz
            rows, nrow = torch.empty(nblk * 2 * Cout, device=dev, dtype=torch.float32), nblk
            t0 = _hbm_begin("bn_lrelu_bwd_reduce")
            lib.call("pulpo_bn_lrelu_bwd_reduce_t", _ptr(dz), _dt(dz), dz.stride(4), _ptr(y), _dt(y), y.stride(4), _ptr(coef), npix, Cout, LRELU_SLOPE,
                     _ptr(rows), _stream())
            _hbm_end(t0, "bn_lrelu_bwd_reduce", (_esize(dz) + _esize(y)) * Cout * npix)                # read dz, y
    if _PASS.window is not None:                 # (the window opens between the two passes: what it held back is queued behind this unit's first pass)
        _PASS.window.visit(D * H * W)
    slot_w, slot_b, slot_g, slot_be = (_grad_slot(t) if need else None for t, need in zip(params, needs[1:5]))
    direct_bn = slot_g is not None and slot_be is not None
    tot = None if direct_bn else torch.empty(2 * Cout, device=dev, dtype=torch.float32)           # dbeta | dgamma
    totd = torch.empty(2 * Cout, device=dev, dtype=torch.float64)          # mean(dbn) | mean(dbn * xhat), kept in double
    # eval-mode BatchNorm is a fixed affine map (dy = scale * dbn): the batch means do not enter
    fin_out = (_ptr(slot_be if direct_bn else tot), _ptr(slot_g) if direct_bn else ctypes.c_void_p(tot.data_ptr() + 4 * Cout), int(direct_bn), _ptr(totd))
    nsd = lib.query("pulpo_bn_bwd_finalize_scratch_doubles", nrow, Cout)
    scratch = torch.empty(nsd, device=dev, dtype=torch.float64) if nsd else None
    lib.call("pulpo_bn_bwd_finalize", _ptr(rows), nrow, Cout, _ptr(coef), float(npix), int(training), *fin_out, _ptr(scratch), _stream())
    dbeta, dgamma = (None, None) if direct_bn else (tot[:Cout], tot[Cout:])
    return src, totd, slot_w, slot_b, dgamma, dbeta, head_dw, head_db


def _dbias_rows(b_p, slot_b, need_db: bool, name: str, nrow: int, Cout: int, dev):
    """the [nrow][Cout] partial rows a kernel leaves the conv-bias gradient in -> (rows, deferred?)"""
    rows = _persistent_buffer(b_p, name, nrow * Cout, zero=False) if (_PASS.direct and need_db and slot_b is not None) else None
    # (inside the stepper: the parameter's persistent buffer, summed by flush_param_grads() - unless this unit has already run a backward pass
    #  in this step and its partials are still waiting there: this pass then takes the immediate path into the same slot)
    if rows is None or _pending_src(rows):
        return torch.empty(nrow * Cout, device=dev, dtype=torch.float32), False
    return rows, True


def _finish_dbias(rows, defer_b: bool, need_db: bool, slot_b, nrow: int, Cout: int):
    if defer_b:
        _defer_grad_job(rows, slot_b, 1, nrow, Cout, 0)
        return None
    return _colsum(rows, nrow, Cout, into=slot_b) if need_db else None


def _bn_apply_entry(src: _DzSource, blocked: bool, dy, y, coef, totd, rows, dims):
    # -> (entry point, arguments, trace name, bytes moved)
    B, _, Cout, D, H, W = dims
    npix = B * D * H * W
    dyo = (_ptr(dy.buf), dy.ps, dy.kb) if blocked else (_ptr(dy), dy.stride(4))
    kb = "_kb" if blocked else ""
    ydt = () if blocked else (_dt(y),)           # (the *_kb entries are fp32 only)
    if src.head is not None:
        nout = src.head[0]
        return (f"pulpo_bn_lrelu_bwd_apply_heads{kb}_t", (_ptr(y), y.stride(4), _ptr(coef), _ptr(totd), LRELU_SLOPE, *src.head[1], *dyo, _ptr(rows), nout,
                                                         B, D * H * W, Cout),
                "bn_lrelu_bwd_apply_heads", npix * (8.0 * Cout + 4.0 * (15 if nout == 6 else 3)))       # read y and the head's planar operands; write dy
    if src.pooled is not None:
        gp, gz = src.pooled
        return (f"pulpo_bn_lrelu_bwd_apply_pooled{kb}_t", (_ptr(gp), gp.stride(4), _ptr(gz), grid_strides(gz)[1] if gz is not None else 0, _dt(gp), _ptr(y), *ydt,
                                                          y.stride(4), _ptr(coef), _ptr(totd), *dyo, LRELU_SLOPE, _ptr(rows), B, D, H, W, Cout),
                "bn_lrelu_bwd_apply", Cout * (_esize(gp) * (gp.numel() // Cout + (npix if gz is not None else 0)) + 2 * _esize(y) * npix))
    dz = src.dz
    nbytes = (_esize(dz) + 2 * _esize(y)) * Cout * npix                # read dz, y; write dy
    if blocked or src.blk:                       # (either side blocked: the entry that takes a block stride for both)
        dzs = (8, npix * 8) if src.blk else (dz.stride(4), 8)
        return ("pulpo_bn_lrelu_bwd_apply_kb_t", (_ptr(dz), _dt(dz), *dzs, _ptr(y), y.stride(4), _ptr(coef), _ptr(totd), *(dyo if blocked else (*dyo, 8)), npix, Cout,
                                                  LRELU_SLOPE, _ptr(rows)), "bn_lrelu_bwd_apply", nbytes)
    return ("pulpo_bn_lrelu_bwd_apply_t", (_ptr(dz), _dt(dz), dz.stride(4), _ptr(y), _dt(y), y.stride(4), _ptr(coef), _ptr(totd), *dyo, npix, Cout, LRELU_SLOPE,
                                           _ptr(rows)), "bn_lrelu_bwd_apply", nbytes)


def _bwd_bn_apply(src: _DzSource, x, weight, y, coef, totd, wpt, dims, nblk: int, needs, b_p, slot_b):
    # -> (dy, (bias rows, their count, deferred?)), or (None, None): the input layer
    B, Cin, Cout, D, H, W = dims
    need_dx, need_dw, need_db = needs
    dev = y.device
    dz_rows4 = src.dz is None or src.blk or _cl_rows4(src.dz)
    # The input layer (image pair -> 32 channels at full resolution): nobody asks for its data gradient, so dy has ONE reader - the weight
    # gradient, which then forms it per element while staging (pulpo_conv3d_k3_wgrad_bn) instead of a pass that reads dz and y and writes dy
    # (0.29 ms at 160^3 x 32 channels).
    if (FUSE_INPUT_WGRAD and src.dz is not None and Cin <= 2 and not need_dx and need_dw and not DETERMINISTIC and y.dtype == torch.float32
            and Cout % 4 == 0 and _cl_rows4(y) and dz_rows4 and x.dtype == torch.float32):
        return None, None
    blocked = _blocked_dy_ok(x, y, weight, wpt, need_dx, need_dw) and dz_rows4 and _cl_rows4(y)
    if blocked:
        global BLOCKED_DY_HITS
        BLOCKED_DY_HITS += 1
        dy = _BlockedGrad(B, Cout, D, H, W, dev)
    else:
        dy = new_cl(B, Cout, D, H, W, dev, y.dtype)        # (the gradient of the pre-norm tensor is stored like the tensor)
    rows, defer_b = _dbias_rows(b_p, slot_b, need_db, "_pulpo_dbias_part", nblk, Cout, dev)
    entry, args, tname, nbytes = _bn_apply_entry(src, blocked, dy, y, coef, totd, rows, dims)
    t0 = _hbm_begin(tname)
    lib.call(entry, *args, _stream())
    _hbm_end(t0, tname, nbytes)
    return dy, (rows, nblk, defer_b)


def _input_layer_param_grads(dz, x, y, coef, totd, dims, need_db: bool, params, slot_w, slot_b):
    # -> (dw, dbias)
    B, Cin, Cout, D, H, W = dims
    w_p, b_p = params[:2]
    dev = x.device
    nrow = lib.query("pulpo_conv3d_k3_wgrad_bn_rows", B, D, H, W, Cout)
    rows, defer_b = _dbias_rows(b_p, slot_b, need_db, "_pulpo_dbias_part_in", nrow, Cout, dev)
    dw, mode, scratch, deferred = _wgrad_target(Cin, Cout, slot_w, w_p, dev)
    xb, xp, xc = grid_strides(x)
    if is_blocked(dz):                           # (the gradient of a blocked activation: the next unit's data-gradient kernel wrote it that way)
        entry, dzo = "pulpo_conv3d_k3_wgrad_bn_kb", (_ptr(dz), D * H * W * 8, 8, B * D * H * W * 8)
    else:
        entry, dzo = "pulpo_conv3d_k3_wgrad_bn", (_ptr(dz), _dt(dz), dz.stride(0), dz.stride(4))

    def launch():
        t0 = _trace_begin()
        lib.call(entry, _ptr(x), xb, xp, xc, *dzo, _ptr(y), y.stride(0), y.stride(4), _ptr(coef), _ptr(totd), LRELU_SLOPE, _ptr(dw), mode, _ptr(scratch),
                 _ptr(rows), B, D, H, W, Cin, Cout, _stream())
        _trace_end(t0, "conv3d_k3_wgrad_smallc(+bn backward)" + ("" if deferred else "(+memset,unpack)"), 54.0 * Cin * Cout * B * D * H * W,
                   (4.0 * Cin + (_esize(dz) + 4.0) * Cout) * B * D * H * W)

    if _PASS.side is not None and deferred:
        _on_side_stream(launch, (x, dz, y, coef, totd))
    else:
        launch()
    if deferred and not _pending_src(scratch):       # (one finishing job per scratch, as in _wgrad_raw)
        _defer_grad_job(scratch, dw, 0, Cin, Cout, (Cout + 63) // 64 * 64)
    return (None if slot_w is not None else dw), _finish_dbias(rows, defer_b, need_db, slot_b, nrow, Cout)


def _bwd_param_grads(src: _DzSource, x, dy, bias_rows, y, coef, totd, dims, needs, params, slot_w, slot_b):
    # -> (dw, dbias, side-stream job or None)
    _, Cin, Cout, _, _, _ = dims
    need_dw, need_db = needs
    if dy is None:
        return (*_input_layer_param_grads(src.dz, x, y, coef, totd, dims, need_db, params, slot_w, slot_b), None)
    rows, nrow, defer_b = bias_rows
    dbias = _finish_dbias(rows, defer_b, need_db, slot_b, nrow, Cout)
    if not need_dw:
        return None, dbias, None
    w_p = params[0]
    if slot_w is not None and _PASS.side is not None:
        return None, dbias, (x, dy, Cin, Cout, slot_w, w_p)
    if slot_w is not None and _PASS.window is not None:
        _PASS.window.wgrad(x, dy, Cin, Cout, slot_w, w_p)
        return None, dbias, None
    return _wgrad_raw(x, dy, Cin, Cout, into=slot_w, owner=w_p if slot_w is not None else None), dbias, None


def _bwd_data_grad(x, dy, wpt, bn_src, dx_blocked: bool, dims, side_job):
    # -> dx (wpt, the packed data-gradient weights, is None where x asks for none)
    B, Cin, Cout, D, H, W = dims
    dx = None
    if wpt is not None:
        # (the bf16-operand kernel takes operand and result in one storage type; every other kernel is fp32)
        dyc = dy if (wpt._pulpo_algo == "bf16" or dy.dtype == torch.float32) else dy.float()
        dx_blk = dx_blocked and wpt._pulpo_algo == "wino3" and dyc.dtype == torch.float32
        if dx_blk:                                   # the input was a blocked activation: its gradient in the same layout, straight from the kernel
            dx = torch.empty((Cin // 8, B, D, H, W, 8), device=x.device, dtype=torch.float32)
        elif is_blocked(x) or not (x.is_contiguous() and Cin <= 3):
            dx = new_cl(B, Cin, D, H, W, x.device, dyc.dtype)
        else:
            dx = torch.empty_like(x, dtype=dyc.dtype)
        if not _dgrad_with_bn_reduction(bn_src, x, dyc, wpt, dx, Cout, Cin):
            _conv_raw(dyc, wpt, None, dx, Cout, Cin, None)
        if dx_blocked and not dx_blk:
            dx = cl_to_blocked(dx.float())
    if side_job is not None:
        _wgrad_on_side_stream(*side_job)
    return dx


def conv_bn_lrelu(x, weight, bias, gamma, beta, running_mean, running_var, training=True, momentum=0.1, eps=1e-5, num_batches_tracked=None,
                  pool_after: bool = False, out=None, pool_only: bool = False, blocked_out: bool = False):
    """ConvUnit forward.  In training mode running_mean / running_var / num_batches_tracked are updated in place by the kernel.
    pool_after: the caller applies avg_pool2_skip() to the result next - where the shapes allow, the pooled tensor is produced by the same
    pass that writes the result and waits on it (`_pulpo_pooled`).
    out: (buffer, first channel) - the result is written into that channel range of a wider channels-last buffer and returned as its slice,
    tagged `_pulpo_cat` (see cat_channels); ignored where the shapes do not fit.
    x may be the blocked output (C / 8, B, D, H, W, 8) of the previous ConvUnit of a sequence; blocked_out: produce this unit's output in that form
    (network_blocks.ConvSequence asks ops.blocked_z_wanted first)."""
    if _is2d(x):
        return conv_bn_lrelu(_lift(x), _lift_w3(weight), bias, gamma, beta, running_mean, running_var, training, momentum, eps,
                             num_batches_tracked).squeeze(2)
    src = getattr(x, "_pulpo_bn_src", None)          # x is the untouched output of another ConvUnit: (y, coef, version at production)
    bn_src = src[:2] if (src is not None and src[2] == x._version and training and torch.is_grad_enabled()) else None
    # pool_only (with pool_after): the caller reads ONLY AvgPool(result) - where the fused pass is available the un-pooled tensor is not written and
    # the call returns (None, pooled); otherwise (result, None) as without the flag
    call = _UnitCall(bn_src=bn_src, out=out, pool_after=pool_after, pool_only=pool_only and pool_after and training and torch.is_grad_enabled(),
                     blocked_out=blocked_out, training=bool(training), momentum=float(momentum), eps=float(eps), running_mean=running_mean,
                     running_var=running_var, num_batches_tracked=num_batches_tracked)
    z = _ConvBNLReLU.apply(x, weight, bias, gamma, beta, None, None, call)
    if call.pool_only_done:                              # the pooled tensor alone came back
        return None, z
    pooled_out = None
    if isinstance(z, tuple):
        z, pooled_out = z
    if call.y is not None:
        z._pulpo_bn_src = (call.y, call.coef, z._version)
        if pooled_out is not None:
            z._pulpo_pooled = (pooled_out, z._version, True)      # (an output of the same autograd node: avg_pool2_skip hands it out as it is)
    if out is not None and z.dim() == 5 and z.data_ptr() == out[0].data_ptr() + out[0].element_size() * out[1] and z.stride() == out[0].stride():
        z._pulpo_cat = (out[0], out[1])
    return (z, None) if pool_only else z


# ---- ConvUnit + 1x1x1 head in one node.  The last ConvUnit in front of a head (PULPoEncoder.sample_merge_block -> mu_sigma, VelocityField's last
# unit -> its 1x1x1 convolution) produces an activation that only the head reads, and the head returns a gradient that only this unit's BatchNorm
# backward reads: the head kernels take the pre-norm tensor and the coefficient block and form both per element (pulpo_heads_fwd_bn_t,
# pulpo_heads_bwd_bn_t, pulpo_bn_lrelu_bwd_apply_heads_t) - ten passes over a C-channel tensor become four, two tensors and two launches per head go.
# ops.FUSE_HEAD_BN = False: the separate passes.
HEAD_BN_HITS = 0                 # heads that ran on the pre-norm tensor so far (tests look at it)


def head_bn_ok(x, training: bool, zdim: int = 3) -> bool:
    """may a ConvUnit applied to x hand (pre-norm tensor, coefficients) to a three-component head instead of its activation?  Training-mode
    statistics, volumes, fp32 activation storage; the CALLER answers for the activation having no other reader (hooks included)"""
    return bool(FUSE_HEAD_BN and training and zdim == 3 and not ACT_BF16 and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() in (5, 6))


def _conv_bn_lrelu_heads(x, unit_args, momentum, eps, Wt, hbias, heps, nout, hparams):
    global HEAD_BN_HITS
    HEAD_BN_HITS += 1
    weight, bias, gamma, beta, running_mean, running_var, num_batches_tracked = unit_args
    src = getattr(x, "_pulpo_bn_src", None)
    bn_src = src[:2] if (src is not None and src[2] == x._version and torch.is_grad_enabled()) else None
    call = _UnitCall(bn_src=bn_src, training=True, momentum=float(momentum), eps=float(eps), running_mean=running_mean, running_var=running_var,
                     num_batches_tracked=num_batches_tracked, head_nout=nout, head_eps=heps, head_params=hparams)
    return _ConvBNLReLU.apply(x, weight, bias, gamma, beta, Wt, hbias, call)


def conv_bn_lrelu_mu_sigma(x, unit_args, momentum, eps, w_mu, b_mu, w_sigma, b_sigma, noise):
    """mu_sigma_sample(conv_bn_lrelu(x, ...), ...) for zdim == 3 where head_bn_ok(): (mu, sigma, z).  unit_args: (weight, bias, gamma, beta,
    running_mean, running_var, num_batches_tracked) of the ConvUnit, in training mode"""
    C = w_mu.shape[1]
    Wt = torch.cat([w_mu.reshape(3, C), w_sigma.reshape(3, C)], dim=0)
    hbias = torch.cat([b_mu, b_sigma], dim=0)
    return _conv_bn_lrelu_heads(x, unit_args, momentum, eps, Wt, hbias, noise, 6, (((w_mu, 0, 3), (w_sigma, 3, 3)), ((b_mu, 0, 3), (b_sigma, 3, 3))))


def conv_bn_lrelu_to3(x, unit_args, momentum, eps, w, b):
    """conv1x1_to3(conv_bn_lrelu(x, ...), w, b) where head_bn_ok()"""
    return _conv_bn_lrelu_heads(x, unit_args, momentum, eps, w.reshape(3, w.shape[1]), b, None, 3, (((w, 0, 3),), ((b, 0, 3),)))


class _Conv3dK3(torch.autograd.Function):
    """bare padded 3x3x3 convolution (no norm / activation); used by tests and by VelocityField-like heads"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu(x, act=True)
        _require_gpu(weight, bias)
        x = as_grid(x.float())                        # (a bare convolution - VelocityField depth 1, tests - keeps fp32 storage)
        B, Cin, D, H, W = x.shape
        Cout = weight.shape[0]
        y = new_cl(B, Cout, D, H, W, x.device)
        _conv_raw(x, _pack_weight(weight, False, shape=(B, D, H, W)), bias, y, Cin, Cout, None)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        B, Cin, D, H, W = x.shape
        Cout = weight.shape[0]
        dy = as_grid(dy.float())
        dw = _wgrad_raw(x, dy, Cin, Cout) if ctx.needs_input_grad[1] else None
        db = dy.sum(dim=(0, 2, 3, 4)) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x) if (x.is_contiguous() and Cin <= 3) else new_cl(B, Cin, D, H, W, x.device)
            _conv_raw(dy, _pack_weight(weight, True, shape=(B, D, H, W)), None, dx, Cout, Cin, None)
        return dx, dw, db


def conv3d_k3(x, weight, bias=None):
    if _is2d(x):
        return conv3d_k3(_lift(x), _lift_w3(weight), bias).squeeze(2)
    return _Conv3dK3.apply(x, weight, bias)


# ------------------------------------------------------------------------------------------------ 1x1x1 heads
class _Heads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, Wt, bias, eps, nout: int, params=None):
        """params: the leaf parameters Wt / bias were assembled from, as ((tensor, first row of Wt, rows), ...) for the weights and
        ((tensor, first element of bias, elements), ...) for the biases: inside the data-parallel stepper their gradients are finished by
        flush_param_grads() straight from the backward kernel's partial rows (no column sum, no split, no AccumulateGrad add per parameter)"""
        _require_gpu(h, act=True)
        _require_gpu(Wt, bias, eps)
        ctx.params = params
        h = to_cl(h)
        B, C, D, H, W = h.shape
        V = D * H * W
        dev = h.device
        outs = [torch.empty((B, 3, D, H, W), device=dev, dtype=torch.float32) for _ in range(1 if nout == 3 else 3)]
        epsc = planar(eps) if eps is not None else None
        t0 = _hbm_begin("heads_fwd")
        lib.call("pulpo_heads_fwd_t", _ptr(h), _dt(h), h.stride(4), _ptr(Wt), _ptr(bias), _ptr(epsc), _ptr(outs[0]), _ptr(outs[1]) if nout == 6 else None,
                 _ptr(outs[2]) if nout == 6 else None, nout, B, V, C, _stream())
        _hbm_end(t0, "heads_fwd", B * V * (_esize(h) * C + 4.0 * (12 if nout == 6 else 3)))       # read h (+ eps), write mu / sigma / z (or the field)
        ctx.nout = nout
        ctx.save_for_backward(h, Wt, epsc, outs[1] if nout == 6 else None)
        return outs[0] if nout == 3 else tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        h, Wt, eps, sigma = ctx.saved_tensors
        nout = ctx.nout
        B, C, D, H, W = h.shape
        V = D * H * W
        dev = h.device
        g = [planar(t) if t is not None else None for t in gs] + [None, None]
        if nout == 3 and g[0] is None:
            g[0] = torch.zeros((B, 3, D, H, W), device=dev)
        dh = new_cl(B, C, D, H, W, dev, h.dtype)
        nblk = lib.query("pulpo_heads_bwd_blocks", B, V, C)
        part, slots = _heads_part_rows(ctx.params, ctx.needs_input_grad[1] and ctx.needs_input_grad[2], nblk, nout, C, dev)
        t0 = _hbm_begin("heads_bwd")
        lib.call("pulpo_heads_bwd_t", _ptr(h), _dt(h), h.stride(4), _ptr(Wt), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(eps), _ptr(sigma), _ptr(dh),
                 dh.stride(4), _ptr(part), nout, B, V, C, _stream())
        _hbm_end(t0, "heads_bwd", B * V * (2 * _esize(h) * C + 4.0 * (15 if nout == 6 else 3)))   # read h, the output gradients (+ eps, sigma), write dh
        dW, db = _heads_finish_rows(part, slots, ctx.params, nblk, nout, C)
        return dh, dW, db, None, None, None


def _heads_part_rows(params, need_wb: bool, nblk: int, nout: int, C: int, dev):
    """(partial rows [nblk][nout * C + nout] for a head's backward kernel, the .grad slots they will be summed into or None).
    Inside the stepper the rows go to a persistent buffer (stable address: the finishing launch's job table is cached) and flush_param_grads()
    adds their column sums to the parameters' .grad; a head applied twice in a step takes the immediate path"""
    rowlen = nout * C + nout
    slots = None
    if params is not None and _PASS.direct and need_wb:
        wparts, bparts = params
        slots = [(_grad_slot(t), off, n) for t, off, n in wparts] + [(_grad_slot(t), off, n) for t, off, n in bparts]
        if not all(sl is not None for sl, _, _ in slots):
            slots = None
    part = _persistent_buffer(params[0][0][0], "_pulpo_heads_part", nblk * rowlen, zero=False) if slots is not None else None
    if part is None or _pending_src(part):
        slots = None
        part = torch.empty(nblk * rowlen, device=dev, dtype=torch.float32)
    return part, slots


def _heads_finish_rows(part, slots, params, nblk: int, nout: int, C: int):
    """(dW, db) of a head from its partial rows - or (None, None) with the column sums queued for flush_param_grads()"""
    rowlen = nout * C + nout
    if slots is not None:
        nw = len(params[0])
        for k, (sl, off, n) in enumerate(slots):
            col0, ncol = (off * C, n * C) if k < nw else (nout * C + off, n)
            _defer_grad_job(part, sl, 1, nblk, ncol, rowlen, byte_offset=4 * col0)
        return None, None
    tot = _colsum(part, nblk, rowlen)
    return tot[: nout * C].view(nout, C), tot[nout * C:]


def mu_sigma_sample(h, w_mu, b_mu, w_sigma, b_sigma, eps):
    """MuSigmaBlock + sampler: returns (mu, sigma, z) planar (B,zdim,D,H,W); eps=None -> z = mu.
    w_*: (zdim, C, 1, 1, 1) conv weights (reference src/network_blocks.py:54-57).  zdim == 3 on volumes / 2 on slices (zdim = ndims,
    models.py:88) is ONE launch of the head kernel; any other zdim runs it over groups of three latent channels, the last group padded with
    zero rows (mu 0, sigma softplus(0), noise 0), which are dropped again."""
    C, zdim = w_mu.shape[1], w_mu.shape[0]
    if _is2d(h) and zdim == 2:
        # 2-D: two latent channels -> rows (0, mu_y, mu_x) / (0, sigma_y, sigma_x) of the three-channel head kernel; the padded channel
        # (mu 0, sigma softplus(0), noise 0 -> sample 0) is dropped again
        z1, zb = w_mu.new_zeros(1, C), b_mu.new_zeros(1)
        Wt = torch.cat([z1, w_mu.reshape(2, C), z1, w_sigma.reshape(2, C)], dim=0)
        bias = torch.cat([zb, b_mu, zb, b_sigma], dim=0)
        mu, sigma, z = _Heads.apply(_lift(h), Wt, bias, _lift_field(eps), 6)
        return _unlift_field(mu), _unlift_field(sigma), _unlift_field(z)
    if zdim != 3 or _is2d(h):
        two_d = _is2d(h)
        h5 = _lift(h) if two_d else h
        e5 = (_lift(eps) if two_d else eps) if eps is not None else None
        mus, sigmas, zs = [], [], []
        for c0 in range(0, zdim, 3):
            n = min(3, zdim - c0)
            pad_w, pad_b = w_mu.new_zeros(3 - n, C), b_mu.new_zeros(3 - n)
            Wt = torch.cat([w_mu[c0:c0 + n].reshape(n, C), pad_w, w_sigma[c0:c0 + n].reshape(n, C), pad_w], dim=0)
            bias = torch.cat([b_mu[c0:c0 + n], pad_b, b_sigma[c0:c0 + n], pad_b], dim=0)
            eg = None
            if e5 is not None:
                eg = e5[:, c0:c0 + n]
                if n < 3:
                    eg = torch.cat([eg, eg.new_zeros((eg.shape[0], 3 - n) + tuple(eg.shape[2:]))], dim=1)
            mu, sigma, z = _Heads.apply(h5, Wt, bias, eg, 6)
            mus.append(mu[:, :n]); sigmas.append(sigma[:, :n]); zs.append(z[:, :n])
        out = [torch.cat(t, dim=1) if len(t) > 1 else t[0].contiguous() for t in (mus, sigmas, zs)]
        return tuple(o.squeeze(2) for o in out) if two_d else tuple(out)
    Wt = torch.cat([w_mu.reshape(3, C), w_sigma.reshape(3, C)], dim=0)
    bias = torch.cat([b_mu, b_sigma], dim=0)
    return _Heads.apply(h, Wt, bias, eps, 6, (((w_mu, 0, 3), (w_sigma, 3, 3)), ((b_mu, 0, 3), (b_sigma, 3, 3))))


def conv1x1_to3(h, w, b):
    """Conv3d(C, 3, kernel_size=1) with planar output (reference src/network_blocks.py:81)"""
    if _is2d(h):
        C = w.shape[1]
        Wt = torch.cat([w.new_zeros(1, C), w.reshape(2, C)], dim=0)
        return _unlift_field(_Heads.apply(_lift(h), Wt, torch.cat([b.new_zeros(1), b]), None, 3))
    return _Heads.apply(h, w.reshape(3, w.shape[1]), b, None, 3, (((w, 0, 3),), ((b, 0, 3),)))


# ------------------------------------------------------------------------------------------------ resampling
class _AvgPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, act=True)
        x = to_cl(x)
        B, C, D, H, W = x.shape
        out = new_cl(B, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, x.device, x.dtype) if C > 1 else \
            torch.empty((B, 1, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=x.device, dtype=x.dtype)
        t0 = _hbm_begin("avgpool2_fwd")
        lib.call("pulpo_avgpool2_fwd_t", _ptr(x), x.stride(4), _ptr(out), out.stride(4), _dt(x), B, D, H, W, C, _stream())
        _hbm_end(t0, "avgpool2_fwd", _esize(x) * C * (x.numel() // C + out.numel() // C))
        ctx.shape = (B, C, D, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, D, H, W = ctx.shape
        g = to_cl(g)
        gin = new_cl(B, C, D, H, W, g.device, g.dtype) if C > 1 else torch.empty((B, 1, D, H, W), device=g.device, dtype=g.dtype)
        lib.call("pulpo_avgpool2_bwd_t", _ptr(g), g.stride(4), None, 0, _ptr(gin), gin.stride(4), _dt(g), B, D, H, W, C, _stream())
        return gin


def avg_pool2(x):
    """AvgPool3d(kernel 2, stride 2, ceil_mode=True)"""
    if _is2d(x):
        return avg_pool2(_lift(x)).squeeze(2)
    return _AvgPool2.apply(x)


class _AvgPool2Skip(torch.autograd.Function):
    """(x, pool(x)) for an activation that is pooled AND used as a skip connection (DownPath: components/pulpo.py:52-59): the backward pass
    forms both gradients' sum in ONE pass (pulpo_avgpool2_bwd_add) instead of a pooling backward plus autograd's accumulation add on a
    strided slice of the concatenation's gradient (101 us at 80^3 x 64 channels at 1 TB/s in torch's generic strided kernel)"""

    @staticmethod
    def forward(ctx, x, ready=None, bn_y=None, bn_coef=None):
        """bn_y / bn_coef: x is the untouched output of a ConvUnit, these are its pre-norm tensor and coefficient block - the backward pass then
        also delivers that unit's BatchNorm-backward partial sums (see _dgrad_with_bn_reduction)"""
        _require_gpu(x, act=True)
        ctx.set_materialize_grads(False)
        ctx.bn = (bn_y, bn_coef) if (bn_y is not None and BN_REDUCE_IN_DGRAD) else None
        xc = to_cl(x)
        B, C, D, H, W = xc.shape
        if ready is not None:                          # AvgPool(x) already written by the pass that wrote x (conv_bn_lrelu(pool_after=True))
            out = ready
        else:
            out = new_cl(B, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2, x.device, x.dtype) if C > 1 else \
                torch.empty((B, 1, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=x.device, dtype=x.dtype)
            lib.call("pulpo_avgpool2_fwd_t", _ptr(xc), xc.stride(4), _ptr(out), out.stride(4), _dt(xc), B, D, H, W, C, _stream())
        ctx.shape = (B, C, D, H, W)
        # (the alias keeps x's exact strides - view_as() would renumber the batch stride of a B = 1 tensor, and torch.cat then no longer
        #  recognises the channels-last layout of its inputs)
        return x.as_strided(x.shape, x.stride(), x.storage_offset()), out

    @staticmethod
    def backward(ctx, gskip, gpool):
        B, C, D, H, W = ctx.shape
        if gpool is None:
            return gskip, None, None, None
        g = to_cl(gpool)
        if gskip is not None and gskip.dtype != g.dtype:
            gskip = gskip.to(g.dtype)
        gin = new_cl(B, C, D, H, W, g.device, g.dtype) if C > 1 else torch.empty((B, 1, D, H, W), device=g.device, dtype=g.dtype)
        grp = 4 * int(_esize(g))                      # bytes of a four-channel group
        skip_ok = False
        if gskip is not None:
            sb, sp, _ = grid_strides(gskip)
            skip_ok = _dense_grid(gskip) and sb == D * H * W * sp and C > 1 and _vec4(gskip, align=grp, batch=False)
        if ctx.bn is not None and C // 4 <= 256 and (gskip is None or skip_ok) and _vec4(g, C, align=grp, batch=False):
            # the producing ConvUnit's first BatchNorm-backward pass rides along: this kernel has every element of its gradient in registers
            y, coef = ctx.bn
            if tuple(y.shape) == (B, C, D, H, W) and _vec4(y, align=4 * int(_esize(y)), batch=False) and _dense_grid(y):
                nblk = lib.query("pulpo_bn_bwd_blocks", B * D * H * W, C)
                part = torch.empty(nblk * 2 * C, device=g.device, dtype=torch.float32)
                t0 = _hbm_begin("avgpool2_bwd_bnred")
                lib.call("pulpo_avgpool2_bwd_bnred_t", _ptr(g), g.stride(4), _ptr(gskip), grid_strides(gskip)[1] if gskip is not None else 0, _ptr(gin),
                         gin.stride(4), _dt(g), _ptr(y), _dt(y), y.stride(4), _ptr(coef), LRELU_SLOPE, _ptr(part), B, D, H, W, C, _stream())
                # read the pooled gradient, the skip gradient and y, write the summed gradient
                _hbm_end(t0, "avgpool2_bwd_bnred", C * (_esize(g) * (g.numel() // C + (2 if gskip is not None else 1) * B * D * H * W) + _esize(y) * B * D * H * W))
                _PASS.bn_parts[y.data_ptr()] = (part, nblk, coef.data_ptr(), gin.data_ptr(), gin._version, tuple(gin.shape), tuple(gin.stride()))
                return gin, None, None, None
        t0 = _hbm_begin("avgpool2_bwd_add") if skip_ok else None
        lib.call("pulpo_avgpool2_bwd_t", _ptr(g), g.stride(4), _ptr(gskip) if skip_ok else None, grid_strides(gskip)[1] if skip_ok else 0, _ptr(gin), gin.stride(4),
                 _dt(g), B, D, H, W, C, _stream())
        _hbm_end(t0, "avgpool2_bwd_add", _esize(g) * C * (g.numel() // C + 2 * B * D * H * W))
        return (gin if (skip_ok or gskip is None) else gskip + gin), None, None, None


def avg_pool2_skip(x):
    """(x, AvgPool(x)) where x goes on to other consumers as well; see _AvgPool2Skip"""
    if _is2d(x):
        return x, avg_pool2(x)
    ready = getattr(x, "_pulpo_pooled", None)
    if ready is not None and ready[1] == x._version and len(ready) > 2:
        return x, ready[0]                            # produced (and differentiated) together with x by the ConvUnit's own autograd node
    src = getattr(x, "_pulpo_bn_src", None)          # x is the untouched output of a ConvUnit: (y, coef, version at production)
    src = src if (src is not None and src[2] == x._version and torch.is_grad_enabled()) else None
    alias, pooled = _AvgPool2Skip.apply(x, ready[0] if (ready is not None and ready[1] == x._version) else None, src[0] if src else None, src[1] if src else None)
    tag = getattr(x, "_pulpo_cat", None)
    if tag is not None:
        alias._pulpo_cat = tag                      # (the skip connection's alias is the same slice of the concatenation buffer)
    return alias, pooled


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, mult: float, add, scale):
        _require_gpu(x, add)
        x = planar(x)
        B, C, Di, Hi, Wi = x.shape
        Do, Ho, Wo = size
        out = torch.empty((B, C, Do, Ho, Wo), device=x.device, dtype=torch.float32)
        addc = planar(add) if add is not None else None
        t0 = _hbm_begin("resize_trilinear_fwd")
        lib.call("pulpo_resize_trilinear_scaled_fwd", _ptr(x), _ptr(addc), _ptr(out), B * C, Di, Hi, Wi, Do, Ho, Wo, *scale, mult, _stream())
        _hbm_end(t0, "resize_trilinear_fwd", 4.0 * (x.numel() + out.numel() * (2 if addc is not None else 1)))
        ctx.dims = (B, C, Di, Hi, Wi, Do, Ho, Wo)
        ctx.mult = mult
        ctx.scale = scale
        ctx.has_add = add is not None
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, Di, Hi, Wi, Do, Ho, Wo = ctx.dims
        g = planar(g)
        gin = None
        if ctx.needs_input_grad[0]:
            gin = torch.empty((B, C, Di, Hi, Wi), device=g.device, dtype=torch.float32)
            t0 = _hbm_begin("resize_trilinear_bwd")
            lib.call("pulpo_resize_trilinear_scaled_bwd_det" if DETERMINISTIC else "pulpo_resize_trilinear_scaled_bwd", _ptr(g), _ptr(gin), B * C, Di, Hi, Wi,
                     Do, Ho, Wo, *ctx.scale, ctx.mult, _stream())
            _hbm_end(t0, "resize_trilinear_bwd", 4.0 * (g.numel() + gin.numel()))
        return gin, None, None, (g if ctx.has_add and ctx.needs_input_grad[3] else None), None


def resize_trilinear(x, size, mult: float = 1.0, add=None, scale_factor: Optional[float] = None):
    """mult * F.interpolate(x, size, 'trilinear', align_corners=False) (+ add).  scale_factor: the call being replaced is
    F.interpolate(x, scale_factor=...) - coordinates are then mapped with 1 / scale_factor on every axis instead of in / out (they differ
    wherever in * scale_factor is not an integer); `size` is still the output size, floor(in * scale_factor)."""
    if _is2d(x):                                       # bilinear = trilinear over a depth-1 volume
        return resize_trilinear(_lift(x), [1] + [int(v) for v in size], mult, _lift(add), scale_factor).squeeze(2)
    step = 0.0 if scale_factor is None else float(torch.tensor(1.0 / float(scale_factor), dtype=torch.float32))     # ATen: static_cast<float>(1.0 / scale)
    scale = (0.0 if x.shape[2] == 1 and int(size[0]) == 1 else step, step, step)       # (the lifted depth axis of a slice keeps its identity mapping)
    return _Resize.apply(x, tuple(int(s) for s in size), float(mult), add, scale)


class _FeedbackUp2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *srcs):
        _require_gpu(*srcs)
        srcs = [planar(s) for s in srcs]
        B, _, Di, Hi, Wi = srcs[0].shape
        chans = [int(s.shape[1]) for s in srcs]
        ctot = sum(chans)
        out = new_cl(B, ctot, 2 * Di, 2 * Hi, 2 * Wi, srcs[0].device, act_dtype())
        n = len(srcs)
        ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
        ch = (ctypes.c_int * n)(*chans)
        t0 = _hbm_begin("feedback_up2_fwd")
        lib.call("pulpo_feedback_up2_fwd_t", ptrs, ch, n, _ptr(out), _dt(out), out.stride(4), B, Di, Hi, Wi, _stream())
        _hbm_end(t0, "feedback_up2_fwd", ctot * B * Di * Hi * Wi * (4.0 + 8 * _esize(out)))             # read the sources, write 8x as many voxels
        ctx.meta = (B, Di, Hi, Wi, chans)
        ctx.keep = srcs      # keep the sources alive until the kernel has been enqueued (same stream: safe afterwards)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Di, Hi, Wi, chans = ctx.meta
        g = to_cl(g)
        n = len(chans)
        gs = [torch.empty((B, c, Di, Hi, Wi), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[i] else None
              for i, c in enumerate(chans)]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in gs])
        ch = (ctypes.c_int * n)(*chans)
        t0 = _hbm_begin("feedback_up2_bwd")
        lib.call("pulpo_feedback_up2_bwd_t", _ptr(g), _dt(g), g.stride(4), ptrs, ch, n, B, Di, Hi, Wi, _stream())
        _hbm_end(t0, "feedback_up2_bwd", sum(chans) * B * Di * Hi * Wi * (4.0 + 8 * _esize(g)))
        return tuple(gs)


def feedback_up2(srcs: Sequence[torch.Tensor]) -> torch.Tensor:
    """cat([interpolate(s, x2) for s in srcs], dim=1) as one channels-last tensor"""
    return _FeedbackUp2.apply(*srcs)


# ------------------------------------------------------------------------------------------------ warp / vecint
class _Warp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, img):
        _require_gpu(df, img)
        df, img = planar(df), planar(img)
        B, _, Dg, Hg, Wg = df.shape
        _, C, Di, Hi, Wi = img.shape
        out = torch.empty((B, C, Dg, Hg, Wg), device=df.device, dtype=torch.float32)
        t0 = _hbm_begin("warp3d_fwd")
        lib.call("pulpo_warp3d_fwd", _ptr(df), _ptr(img), _ptr(out), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "warp3d_fwd", 4.0 * (df.numel() + img.numel() + out.numel()))          # (3 + 2C) V 4
        ctx.save_for_backward(df, img)
        return out

    @staticmethod
    def backward(ctx, g):
        df, img = ctx.saved_tensors
        g = planar(g)
        B, _, Dg, Hg, Wg = df.shape
        _, C, Di, Hi, Wi = img.shape
        gdf = torch.empty_like(df) if ctx.needs_input_grad[0] else None
        gimg = torch.empty_like(img) if ctx.needs_input_grad[1] else None
        t0 = _hbm_begin("warp3d_bwd")
        if DETERMINISTIC and gimg is not None:          # (the displacement gradient alone is a gather: nothing to order)
            ws = torch.empty(lib.query("pulpo_warp3d_bwd_det_ws_bytes", B, C, Di, Hi, Wi), device=df.device, dtype=torch.uint8)
            lib.call("pulpo_warp3d_bwd_det", _ptr(df), _ptr(img), _ptr(g), _ptr(gdf), _ptr(gimg), _ptr(ws), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        else:
            lib.call("pulpo_warp3d_bwd", _ptr(df), _ptr(img), _ptr(g), _ptr(gdf), _ptr(gimg), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "warp3d_bwd", 4.0 * (df.numel() + img.numel() + g.numel() + (gdf.numel() if gdf is not None else 0)
                                          + (2 * gimg.numel() if gimg is not None else 0)))      # (image gradient: zero fill + scatter)
        return gdf, gimg


def warp3d(df, img):
    """SpatialTransformer.forward(df, img)"""
    if _is2d(df):                                      # 2-D SpatialTransformer: channels (y, x) -> (0, y, x), depth-1 grid and image
        return warp3d(_lift_field(df), _lift(img)).squeeze(2)
    return _Warp.apply(df, img)


@torch.no_grad()
def warp_mask(df, mask):
    """a (B,1,...) weight volume under warp3d's warp, for cost-function masking: the same sample positions, the interpolation written so
    that a constant volume comes back exactly (a mask of ones stays a mask of ones; warp3d returns 1 - 1.2e-7 at one voxel in eight).
    No gradient.  Another dtype is converted to fp32."""
    if _is2d(df):
        return warp_mask(_lift_field(df), _lift(mask)).squeeze(2)
    if mask.dim() != 5 or mask.shape[1] != 1 or mask.shape[0] != df.shape[0]:
        raise ValueError(f"warp_mask: a (B,1,D,H,W) weight volume expected for a field of shape {tuple(df.shape)}, got {tuple(mask.shape)}")
    df, mask = planar(df.detach()), planar(mask.detach() if mask.dtype == torch.float32 else mask.detach().float())
    _require_gpu(df, mask)
    B, _, Dg, Hg, Wg = df.shape
    _, _, Di, Hi, Wi = mask.shape
    out = torch.empty((B, 1, Dg, Hg, Wg), device=df.device, dtype=torch.float32)
    lib.call("pulpo_warp_mask_fwd", _ptr(df), _ptr(mask), _ptr(out), B, Dg, Hg, Wg, Di, Hi, Wi, _stream())
    return out


# ------------------------------------------------------------------------------------------------ cubic B-spline interpolation
# Images only: a label map has no cubic interpolant (warp_labels) and a weight volume would overshoot (warp_mask).
INTERPOLATIONS = ("linear", "cubic")


def check_interpolation(interpolation, who: str) -> str:
    """the `interpolation` argument of the public surface: "linear" (trilinear, the default route) or "cubic"; anything else raises"""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"{who}: interpolation is {interpolation!r}; one of {INTERPOLATIONS} expected")
    return interpolation


def _cubic_image(t, name: str, what: str):
    if not isinstance(t, torch.Tensor) or t.dim() not in (4, 5):
        raise ValueError(f"{name}: {what} (B,C,D,H,W) or, for slices, (B,C,H,W) expected, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.requires_grad:
        raise ValueError(f"{name}: the image is data here (no gradient with respect to {what}); detach it")
    if min(t.shape) < 1:
        raise ValueError(f"{name}: {what} of shape {tuple(t.shape)} has an empty extent")


@torch.no_grad()
def bspline_prefilter(img):
    """the cubic B-spline coefficients of an image (B,C,D,H,W) (slices: (B,C,H,W)): per axis of N >= 2 samples the solution of
    s[k] = (c[m(k-1)] + 4 c[k] + c[m(k+1)]) / 6 under the whole-sample mirror m - scipy.ndimage.spline_filter(order=3, mode="mirror").
    What warp3d_cubic(df, coef=...) samples: prefilter once, warp many times.  No autograd (the image is data)."""
    _cubic_image(img, "bspline_prefilter", "img")
    if _is2d(img):
        return bspline_prefilter(_lift(img)).squeeze(2)
    _require_gpu(img)
    img = planar(img.detach())
    B, C, D, H, W = img.shape
    coef = torch.empty_like(img)
    t0 = _hbm_begin("bspline_prefilter")
    lib.call("pulpo_bspline_prefilter", _ptr(img), _ptr(coef), B * C, D, H, W, _stream())
    _hbm_end(t0, "bspline_prefilter", 8.0 * img.numel() * max(1, (D > 1) + (H > 1) + (W > 1)))       # every pass: one read, one write
    return coef


class _WarpCubic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, coef):
        _require_gpu(df, coef)
        df, coef = planar(df), planar(coef)
        B, _, Dg, Hg, Wg = df.shape
        _, C, Di, Hi, Wi = coef.shape
        out = torch.empty((B, C, Dg, Hg, Wg), device=df.device, dtype=torch.float32)
        t0 = _hbm_begin("warp3d_cubic_fwd")
        lib.call("pulpo_warp3d_cubic_fwd", _ptr(df), _ptr(coef), _ptr(out), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "warp3d_cubic_fwd", 4.0 * (df.numel() + coef.numel() + out.numel()))     # (3 + 2C) V 4, as warp3d
        ctx.save_for_backward(df, coef)
        return out

    @staticmethod
    def backward(ctx, g):
        df, coef = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        g = planar(g)
        B, _, Dg, Hg, Wg = df.shape
        _, C, Di, Hi, Wi = coef.shape
        gdf = torch.empty_like(df)
        t0 = _hbm_begin("warp3d_cubic_bwd")
        lib.call("pulpo_warp3d_cubic_bwd", _ptr(df), _ptr(coef), _ptr(g), _ptr(gdf), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "warp3d_cubic_bwd", 4.0 * (df.numel() + coef.numel() + g.numel()))       # (3 + 2C) V 4: gdf replaces out
        return gdf, None


def warp3d_cubic(df, img=None, *, coef=None):
    """warp3d with the cubic B-spline interpolant of the image: the same sample coordinate (clamp included), 64 taps of the coefficients
    instead of 8 corners of the samples; equals scipy.ndimage.map_coordinates(order=3, mode="mirror") at that coordinate.  Exactly one of
    img and coef = bspline_prefilter(img) is given (bit-identical routes; coef lets a caller prefilter once).  df (B,3,Dg,Hg,Wg), image
    (B,C,Di,Hi,Wi) of any size; slices: df (B,2,H,W), image (B,C,H,W).  Differentiable with respect to df only - a gather, deterministic;
    an image that requires grad raises ValueError.  The result may leave the image's range by overshoot at edges: clamp it where a range
    is assumed.  Not for label maps or masks (warp_labels, warp_mask)."""
    if (img is None) == (coef is None):
        raise ValueError("warp3d_cubic: exactly one of img and coef expected")
    src, what = (img, "img") if coef is None else (coef, "coef")
    _cubic_image(src, "warp3d_cubic", what)
    if not isinstance(df, torch.Tensor) or df.dim() != src.dim() or df.shape[1] != df.dim() - 2 or df.shape[0] != src.shape[0]:
        raise ValueError(f"warp3d_cubic: a field (B,3,D,H,W) ((B,2,H,W) for slices) with {what}'s batch expected, got "
                         f"{tuple(df.shape) if isinstance(df, torch.Tensor) else type(df)} for {what} {tuple(src.shape)}")
    if min(df.shape[-2:]) < 2 or (df.dim() == 5 and df.shape[2] < 2 and src.shape[2] != 1):
        raise ValueError(f"warp3d_cubic: grid extents of at least 2 expected (a depth-1 grid goes with a depth-1 image), got {tuple(df.shape)}")
    if _is2d(df):
        return _WarpCubic.apply(_lift_field(df), _lift(bspline_prefilter(src) if coef is None else src)).squeeze(2)
    return _WarpCubic.apply(df, bspline_prefilter(src) if coef is None else src)


class _VecInt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, nsteps: int):
        _require_gpu(v)
        v = planar(v)
        B, _, D, H, W = v.shape
        work = torch.empty((nsteps + 1, B, 3, D, H, W), device=v.device, dtype=torch.float32)
        t0 = _hbm_begin("vecint_fwd")
        lib.call("pulpo_vecint_fwd", _ptr(v), _ptr(work), B, D, H, W, nsteps, _stream())
        _hbm_end(t0, "vecint_fwd", 4.0 * v.numel() * 2 * (nsteps + 1))                       # every step: one read, one write of the field
        ctx.save_for_backward(work)
        ctx.nsteps = nsteps
        return work[nsteps]

    @staticmethod
    def backward(ctx, g):
        (work,) = ctx.saved_tensors
        g = planar(g)
        _, B, _, D, H, W = work.shape
        gin = torch.empty((B, 3, D, H, W), device=g.device, dtype=torch.float32)
        t0 = _hbm_begin("vecint_bwd")
        if DETERMINISTIC:
            nws = lib.query("pulpo_vecint_bwd_det_ws_bytes", B, D, H, W, ctx.nsteps)
            ws = torch.empty(nws, device=g.device, dtype=torch.uint8) if nws else None
            lib.call("pulpo_vecint_bwd_det", _ptr(work), _ptr(g), _ptr(gin), _ptr(ws), B, D, H, W, ctx.nsteps, _stream())
        else:
            ntmp = lib.query("pulpo_vecint_bwd_tmp_floats", B, D, H, W, ctx.nsteps)
            tmp = torch.empty(ntmp, device=g.device, dtype=torch.float32) if ntmp else None
            lib.call("pulpo_vecint_bwd", _ptr(work), _ptr(g), _ptr(gin), _ptr(tmp), B, D, H, W, ctx.nsteps, _stream())
        _hbm_end(t0, "vecint_bwd", 4.0 * gin.numel() * (3 * ctx.nsteps + 2))                 # every step: read the field and the gradient, write a gradient
        return gin, None


def vecint(v, nsteps: int = 7):
    if _is2d(v):
        return _unlift_field(vecint(_lift_field(v), nsteps))
    return _VecInt.apply(v, int(nsteps))


class _VecIntPair(torch.autograd.Function):
    """(VecInt(v), VecInt(-v)) as one node: pulpo_vecint_pair_fwd_work keeps the nsteps + 1 fields of both directions in one buffer, whose
    last pair is the result; the backward pass is one pulpo_vecint_pair_bwd call that takes whichever upstream gradients exist.  The buffer
    hangs on the node itself, not among its saved tensors: the two results are often differentiated in separate passes (one direction's
    loss, then the other's), and a pass releases the saved tensors of the nodes it visits."""

    @staticmethod
    def forward(ctx, v, nsteps: int):
        _require_gpu(v)
        v = planar(v)
        B, _, D, H, W = v.shape
        work = torch.empty((nsteps + 1, 2, B, 3, D, H, W), device=v.device, dtype=torch.float32)
        t0 = _hbm_begin("vecint_pair_fwd_work")
        lib.call("pulpo_vecint_pair_fwd_work", _ptr(v), _ptr(work), B, D, H, W, nsteps, _stream())
        _hbm_end(t0, "vecint_pair_fwd_work", 4.0 * v.numel() * (4 * nsteps + 3))             # v once, both signs out; every step: both fields in and out
        ctx.work = work
        ctx.nsteps = nsteps
        ctx.set_materialize_grads(False)
        return work[nsteps, 0], work[nsteps, 1]

    @staticmethod
    def backward(ctx, gf, gi):
        work = ctx.work
        _, _, B, _, D, H, W = work.shape
        if gf is None and gi is None:
            return None, None
        gf = planar(gf) if gf is not None else None
        gi = planar(gi) if gi is not None else None
        gin = torch.empty((B, 3, D, H, W), device=work.device, dtype=torch.float32)
        t0 = _hbm_begin("vecint_pair_bwd")
        if DETERMINISTIC:
            nws = lib.query("pulpo_vecint_pair_bwd_det_ws_bytes", B, D, H, W, ctx.nsteps)
            ws = torch.empty(nws, device=work.device, dtype=torch.uint8) if nws else None
            lib.call("pulpo_vecint_pair_bwd_det", _ptr(work), _ptr(gf), _ptr(gi), _ptr(gin), _ptr(ws), B, D, H, W, ctx.nsteps, _stream())
        else:
            ntmp = lib.query("pulpo_vecint_pair_bwd_tmp_floats", B, D, H, W, ctx.nsteps)
            if gf is None or gi is None:
                ntmp //= 2                                                                   # one direction's chain: half the buffers
            tmp = torch.empty(ntmp, device=work.device, dtype=torch.float32) if ntmp else None
            lib.call("pulpo_vecint_pair_bwd", _ptr(work), _ptr(gf), _ptr(gi), _ptr(gin), _ptr(tmp), B, D, H, W, ctx.nsteps, _stream())
        ndir = (gf is not None) + (gi is not None)
        _hbm_end(t0, "vecint_pair_bwd", 4.0 * gin.numel() * (3 * ctx.nsteps * ndir + ndir + 1))
        return gin, None


def vecint_pair(v, nsteps: int = 7):
    """(VecInt(v), VecInt(-v)): the integrated field and its inverse (a stationary velocity field's flow is inverted by integrating -v;
    network_blocks.py:160-177).  Under torch.no_grad(), or when v does not require grad, one pulpo_vecint_pair_fwd call that keeps no
    intermediate field (two results + two scratch fields; none of the nsteps + 1 fields per direction that vecint saves for its backward
    pass).  Otherwise one autograd node over the paired kernel chains: both directions advance in the same launches,
    2 (nsteps + 1) fields are kept, and the backward pass writes the gradient of both directions' losses in one call."""
    if torch.is_grad_enabled() and v.requires_grad:
        if _is2d(v):
            fwd, inv = vecint_pair(_lift_field(v), nsteps)
            return _unlift_field(fwd), _unlift_field(inv)
        if v.dim() != 5 or v.shape[1] != 3:
            raise PulpoHipError(f"vecint_pair: velocity field (B,3,D,H,W) or (B,2,H,W) expected, got {tuple(v.shape)}")
        return _VecIntPair.apply(v, int(nsteps))
    if _is2d(v):
        fwd, inv = vecint_pair(_lift_field(v), nsteps)
        return _unlift_field(fwd), _unlift_field(inv)
    _require_gpu(v)
    v = planar(v.detach())
    nsteps = int(nsteps)
    B, C, D, H, W = v.shape
    if C != 3:
        raise PulpoHipError(f"vecint_pair: velocity field (B,3,D,H,W) or (B,2,H,W) expected, got {tuple(v.shape)}")
    fwd, inv = torch.empty_like(v), torch.empty_like(v)
    nscr = lib.query("pulpo_vecint_pair_scratch_floats", B, D, H, W, nsteps)
    scratch = torch.empty(nscr, device=v.device, dtype=torch.float32) if nscr else None
    t0 = _hbm_begin("vecint_pair_fwd")
    lib.call("pulpo_vecint_pair_fwd", _ptr(v), _ptr(fwd), _ptr(inv), _ptr(scratch), B, D, H, W, nsteps, _stream())
    # the one-launch form reads v per direction and writes a result each; the step form reads v once, writes two fields, then every step
    # reads and writes both directions' fields
    fields = 4 if (nsteps and not nscr) else 3 + 4 * nsteps
    _hbm_end(t0, "vecint_pair_fwd", 4.0 * v.numel() * fields)
    return fwd, inv


# ------------------------------------------------------------------------------------------------ losses
# ---- cost-function masking: m = mask * mask2 weights the per-voxel cost, the loss is normalised by M = sum of m.  One
# autograd node per term (_NCC, _SqDiff, _Mind): wa is None -> the unmasked term, a 0-d loss; else the four scalars of pulpo_masked_finish
def _as_masks(img: torch.Tensor, mask, mask2, name: str):
    """the masks of a (B,C,D,H,W) image as contiguous fp32 (B,1,D,H,W) device tensors (another dtype is converted here, once)"""
    if mask is None:
        raise ValueError(f"{name}: mask is required (mask2 is the optional one)")
    want = (img.shape[0], 1) + tuple(img.shape[2:])
    out = []
    for m in (mask, mask2):
        if m is None:
            out.append(None)
            continue
        if tuple(m.shape) != want:
            raise ValueError(f"{name}: mask of shape {tuple(m.shape)} for an image of shape {tuple(img.shape)} (expected {want})")
        m = m.detach()
        if not m.is_cuda:
            raise PulpoHipError("pulpo_amd operators run on the GPU only (got a CPU mask); there is no CPU fallback")
        out.append(planar(m if m.dtype == torch.float32 else m.float()))
    return out[0], out[1]


def _masks_of(img: torch.Tensor, mask, mask2, name: str):
    """_as_masks of a volume, or of a slice (B,C,H,W): its masks are slices (B,1,H,W) and come back lifted to depth 1 like the image will be"""
    if _is2d(img):
        for m in (mask, mask2):
            if m is not None and m.dim() != 4:
                raise ValueError(f"{name}: masks of a (B,C,H,W) image are (B,1,H,W), got {tuple(m.shape)}")
        img, mask, mask2 = _lift(img), _lift(mask), _lift(mask2)
    return _as_masks(img, mask, mask2, name)


def _masked_finish(part: torch.Tensor, nblk: int, scale: float, root: bool, count: float) -> torch.Tensor:
    """(loss, d loss / d sum, M / count, M) of a masked loss from its two-column block partials, on the device"""
    out = torch.empty(4, device=part.device, dtype=torch.float32)
    lib.call("pulpo_masked_finish", _ptr(part), nblk, float(scale), int(root), float(count), _ptr(out), _stream())
    return out


class _NCC(torch.autograd.Function):
    """unmasked (wa is None): the loss scalar; masked: the four scalars of pulpo_masked_finish, the caller takes element 0"""

    @staticmethod
    def forward(ctx, pred, true, wa, wb, win: int, gamma: float):
        _require_gpu(pred, true, wa, wb)
        pred, true = planar(pred), planar(true)
        B, C, D, H, W = pred.shape
        if C != 1:
            raise PulpoHipError("ncc: single-channel volumes expected")
        N = B * D * H * W
        dev = pred.device
        masked = wa is not None
        S = torch.empty(5 * N, device=dev, dtype=torch.float32)
        T = torch.empty(10 * N, device=dev, dtype=torch.float32)
        nblk = lib.query("pulpo_loss_blocks", N)
        part = torch.empty((2 if masked else 1) * nblk, device=dev, dtype=torch.float32)
        name, planes = ("ncc_masked_fwd", (_ptr(wa), _ptr(wb))) if masked else ("ncc_fwd", ())
        t0 = _hbm_begin(name)
        lib.call("pulpo_" + name, _ptr(true), _ptr(pred), *planes, _ptr(S), _ptr(T), _ptr(part), B, D, H, W, win, _stream())
        # 2 images in; three separable passes over 5 box-sum channels (write 5, read 5, write 5, read 5); one read of every mask plane
        _hbm_end(t0, name, 4.0 * (22 + (wa is not None) + (wb is not None)) * N)
        ctx.win, ctx.gamma, ctx.masked = win, gamma, masked
        if not masked:
            ctx.save_for_backward(pred, true, S)
            return _colsum(part, nblk, 1, -gamma / B).reshape(())
        fin = _masked_finish(part, nblk, -gamma * (D * H * W), False, float(N))
        ctx.save_for_backward(pred, true, S, wa, wb, fin)
        return fin

    @staticmethod
    def backward(ctx, g):
        pred, true, S, *rest = ctx.saved_tensors
        B, _, D, H, W = pred.shape
        N = B * D * H * W
        T = torch.empty(6 * N, device=pred.device, dtype=torch.float32)
        gJ = torch.empty_like(pred)
        if ctx.masked:
            wa, wb, fin = rest
            name, planes = "ncc_masked_bwd", (_ptr(wa), _ptr(wb))
            gs, coef = (g[0] * fin[1]).contiguous(), 1.0        # upstream * (-gamma V / M), 0 for an empty mask: device scalars
        else:
            wa = wb = None
            name, planes = "ncc_bwd", ()
            gs, coef = g.contiguous(), -ctx.gamma / B
        t0 = _hbm_begin(name)
        lib.call("pulpo_" + name, _ptr(true), _ptr(pred), _ptr(S), *planes, _ptr(T), _ptr(gs), coef, _ptr(gJ), B, D, H, W, ctx.win, _stream())
        # 2 images + 5 sums in; three passes over 3 channels (write 3, read 3, write 3, read 3); gradient out; one read of every mask plane
        _hbm_end(t0, name, 4.0 * (20 + (wa is not None) + (wb is not None)) * N)
        return gJ, None, None, None, None, None


def ncc_loss(pred, true, win: int = 9, gamma: float = 0.05):
    if _is2d(pred):                                    # depth 1 selects the win x win window count in the kernel
        pred, true = _lift(pred), _lift(true)
    return _NCC.apply(pred, true, None, None, int(win), float(gamma))


def ncc_loss_masked(pred, true, mask, mask2=None, win: int = 9, gamma: float = 0.05):
    """-gamma V sum(m cc) / M with m = mask * mask2 and M = sum(m) (0 for an empty mask): NCC_loss with the per-voxel cost weighted by m,
    the window statistics over all voxels.  Masks: (B,1,...) weights in [0,1], 1 = counted.  Gradient to pred only."""
    wa, wb = _masks_of(pred, mask, mask2, "ncc_loss_masked")
    if _is2d(pred):
        pred, true = _lift(pred), _lift(true)
    return _NCC.apply(pred, true, wa, wb, int(win), float(gamma))[0]


# ---- MIND-SSC: a similarity term between two contrasts.  f_k = exp(-(D_k - min D) / (mean(D - min D) + eps)) over
# the twelve self-similarity-context channels, cost = mean_k (f_k[pred] - f_k[true])^2; voxel-sum, batch-mean like L2_loss.
def _mind_args(name: str, *imgs, dilation, eps):
    for t in imgs:
        if t.dim() == 4:
            raise NotImplementedError(f"{name}: 3-D volumes (B,1,D,H,W) only; the 2-D descriptor (four channels) is not built")
        if t.dim() != 5 or t.shape[1] != 1:
            raise PulpoHipError(f"{name}: single-channel volumes (B,1,D,H,W) expected, got {tuple(t.shape)}")
    if len(imgs) == 2 and imgs[0].shape != imgs[1].shape:
        raise ValueError(f"{name}: pred {tuple(imgs[0].shape)} and true {tuple(imgs[1].shape)} differ in shape")
    return int(dilation), float(eps)


def _mind_bytes(pred, nmask: int, backward: bool) -> float:
    """algorithmic HBM bytes: forward 2 images (+ masks) in; backward 2 images (+ masks) in, 12N out, 12N in, the image once more, N out"""
    N = pred.numel()
    return 4.0 * N * ((2 + nmask + 12 + 12 + 1 + 1) if backward else (2 + nmask))


class _Mind(torch.autograd.Function):
    """unmasked (wa is None): the loss scalar; masked: the four scalars of pulpo_masked_finish"""

    @staticmethod
    def forward(ctx, pred, true, wa, wb, dilation: int, eps: float):
        _require_gpu(pred, true, wa, wb)
        pred, true = planar(pred), planar(true)
        B, _, D, H, W = pred.shape
        nblk = lib.query("pulpo_mind_blocks", B, D, H, W, dilation)
        ncol = 1 if wa is None else 2
        part = torch.empty(max(nblk, 1) * ncol, device=pred.device, dtype=torch.float32)
        nmask = (wa is not None) + (wb is not None)
        t0 = _hbm_begin("mind_fwd")
        lib.call("pulpo_mind_fwd", _ptr(true), _ptr(pred), _ptr(wa), _ptr(wb), _ptr(part), B, D, H, W, dilation, eps, _stream())
        _hbm_end(t0, "mind_fwd", _mind_bytes(pred, nmask, False))
        ctx.dilation, ctx.eps, ctx.masked = dilation, eps, wa is not None
        if wa is None:
            ctx.save_for_backward(pred, true)
            return _colsum(part, nblk, 1, 1.0 / B).reshape(())
        fin = _masked_finish(part, nblk, float(D * H * W), False, float(B * D * H * W))
        ctx.save_for_backward(pred, true, wa, wb, fin)
        return fin

    @staticmethod
    def backward(ctx, g):
        if ctx.masked:
            pred, true, wa, wb, fin = ctx.saved_tensors
            gs, coef = (g[0] * fin[1]).contiguous(), 1.0        # upstream * (V / M), 0 for an empty mask: device scalars
        else:
            (pred, true), wa, wb = ctx.saved_tensors, None, None
            gs, coef = g.contiguous(), 1.0 / pred.shape[0]
        B, _, D, H, W = pred.shape
        scratch = torch.empty(12 * pred.numel(), device=pred.device, dtype=torch.float32)
        gpred = torch.empty_like(pred)
        nmask = (wa is not None) + (wb is not None)
        t0 = _hbm_begin("mind_bwd")
        lib.call("pulpo_mind_bwd", _ptr(true), _ptr(pred), _ptr(wa), _ptr(wb), _ptr(scratch), _ptr(gs), coef, _ptr(gpred), B, D, H, W, ctx.dilation,
                 ctx.eps, _stream())
        _hbm_end(t0, "mind_bwd", _mind_bytes(pred, nmask, True))
        return gpred, None, None, None, None, None


def mind_descriptor(img, dilation: int = 2, eps: float = 1e-5):
    """(B,1,D,H,W) -> (B,12,D,H,W): the MIND-SSC descriptor, in (0,1] with maximum 1 over the channels.  No gradient."""
    dilation, eps = _mind_args("mind_descriptor", img, dilation=dilation, eps=eps)
    _require_gpu(img)
    img = planar(img.detach())
    B, _, D, H, W = img.shape
    out = torch.empty((12, B, D, H, W), device=img.device, dtype=torch.float32)
    lib.call("pulpo_mind_descriptor", _ptr(img), _ptr(out), B, D, H, W, dilation, eps, _stream())
    return out.transpose(0, 1)


def mind_loss(pred, true, dilation: int = 2, eps: float = 1e-5):
    """sum over voxels, mean over the batch of the squared descriptor difference (mean over the 12 channels).  Gradient to pred only."""
    dilation, eps = _mind_args("mind_loss", pred, true, dilation=dilation, eps=eps)
    return _Mind.apply(pred, true.detach(), None, None, dilation, eps)


def mind_loss_masked(pred, true, mask, mask2=None, dilation: int = 2, eps: float = 1e-5):
    """V sum(m cost) / M with m = mask * mask2 and M = sum(m) (0 for an empty mask): mind_loss with the per-voxel cost weighted by m; the
    descriptors are formed from all voxels.  Gradient to pred only."""
    dilation, eps = _mind_args("mind_loss_masked", pred, true, dilation=dilation, eps=eps)      # (3-D only: raises on slices)
    wa, wb = _masks_of(pred, mask, mask2, "mind_loss_masked")
    return _Mind.apply(pred, true.detach(), wa, wb, dilation, eps)[0]


# ---- Mutual information: Mattes MI over a cubic-B-spline Parzen joint histogram of K bins, images expected in [0,1].
# loss = -gamma V mean_b MI_b: NCC_loss's scale.  Pointwise, so slices run as depth-1 volumes.
def _mi_args(name: str, pred, true, bins):
    for t in (pred, true):
        if t.dim() not in (4, 5) or t.shape[1] != 1:
            raise PulpoHipError(f"{name}: single-channel volumes (B,1,D,H,W) or slices (B,1,H,W) expected, got {tuple(t.shape)}")
    if pred.shape != true.shape:
        raise ValueError(f"{name}: pred {tuple(pred.shape)} and true {tuple(true.shape)} differ in shape")
    bins = int(bins)
    if not 4 <= bins <= 64:
        raise ValueError(f"{name}: bins must be in [4, 64], got {bins}")
    return bins


def _mi_forward(pred, true, wa, wb, bins: int, gamma: float):
    """(loss, p, MI, G) of planar device images; the slab is scratch of this call"""
    B = pred.shape[0]
    V = pred.numel() // B
    dev = pred.device
    slab = torch.empty(lib.query("pulpo_mi_scratch_floats", B, V, bins), device=dev, dtype=torch.float32)
    p = torch.empty((B, bins, bins), device=dev, dtype=torch.float64)
    mi = torch.empty(B, device=dev, dtype=torch.float64)
    G = torch.empty((B, bins, bins), device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    nmask = (wa is not None) + (wb is not None)
    t0 = _hbm_begin("mi_fwd")
    lib.call("pulpo_mi_fwd", _ptr(true), _ptr(pred), _ptr(wa), _ptr(wb), _ptr(slab), _ptr(p), _ptr(mi), _ptr(G), _ptr(loss), B, V, bins, float(gamma),
             _stream())
    _hbm_end(t0, "mi_fwd", 4.0 * (2 + nmask) * B * V)                     # 2 images (+ masks) in; the slab and the tables are noise beside them
    return loss, p, mi, G


class _MI(torch.autograd.Function):
    """the loss scalar, masked (wa given) or not: the masks enter the joint histogram, whose own sum normalises it"""

    @staticmethod
    def forward(ctx, pred, true, wa, wb, bins: int, gamma: float):
        _require_gpu(pred, true, wa, wb)
        pred, true = planar(pred), planar(true)
        loss, _, _, G = _mi_forward(pred, true, wa, wb, bins, gamma)
        ctx.bins, ctx.gamma = bins, gamma
        ctx.save_for_backward(pred, true, wa, wb, G)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, true, wa, wb, G = ctx.saved_tensors
        B = pred.shape[0]
        V = pred.numel() // B
        gpred = torch.empty_like(pred)
        nmask = (wa is not None) + (wb is not None)
        t0 = _hbm_begin("mi_bwd")
        lib.call("pulpo_mi_bwd", _ptr(true), _ptr(pred), _ptr(wa), _ptr(wb), _ptr(G), _ptr(g.contiguous()), -ctx.gamma * V / B, _ptr(gpred), B, V,
                 ctx.bins, _stream())
        _hbm_end(t0, "mi_bwd", 4.0 * (3 + nmask) * B * V)                 # 2 images (+ masks) in, the gradient out
        return gpred, None, None, None, None, None


def mi_loss(pred, true, bins: int = 32, gamma: float = 0.05):
    """-gamma V mean_b MI_b, MI_b the Mattes mutual information of pred_b and true_b over a bins x bins cubic-B-spline Parzen histogram
    (images in [0,1], values outside are clamped).  Volumes or slices.  Gradient to pred only."""
    bins = _mi_args("mi_loss", pred, true, bins)
    if _is2d(pred):
        pred, true = _lift(pred), _lift(true)
    return _MI.apply(pred, true.detach(), None, None, bins, float(gamma))


def mi_loss_masked(pred, true, mask, mask2=None, bins: int = 32, gamma: float = 0.05):
    """mi_loss with every voxel's histogram weight multiplied by m = mask * mask2 ((B,1,...) weights in [0,1]); the histogram is normalised
    by M = sum(m), V stays the voxel count; 0 with a zero gradient for an empty mask.  Gradient to pred only."""
    bins = _mi_args("mi_loss_masked", pred, true, bins)
    wa, wb = _masks_of(pred, mask, mask2, "mi_loss_masked")
    if _is2d(pred):
        pred, true = _lift(pred), _lift(true)
    return _MI.apply(pred, true.detach(), wa, wb, bins, float(gamma))


def joint_histogram(a, b, bins: int = 32, mask=None, mask2=None):
    """(p (B,K,K) float64, MI (B,) float64): the normalised Parzen joint histogram of a (rows) and b (columns) and its mutual information
    per batch element, as mi_loss forms them.  No gradient."""
    bins = _mi_args("joint_histogram", a, b, bins)
    if mask is None:
        mask, mask2 = mask2, None
    wa, wb = _masks_of(a, mask, mask2, "joint_histogram") if mask is not None else (None, None)
    if _is2d(a):
        a, b = _lift(a), _lift(b)
    _require_gpu(a, b, wa, wb)
    _, p, mi, _ = _mi_forward(planar(a.detach()), planar(b.detach()), wa, wb, bins, 0.0)
    return p, mi


class _KL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, mu1, sigma1):
        _require_gpu(mu, sigma, mu1, sigma1)
        mu, sigma = planar(mu), planar(sigma)
        mu1 = planar(mu1) if mu1 is not None else None
        sigma1 = planar(sigma1) if sigma1 is not None else None
        n = mu.numel()
        nblk = lib.query("pulpo_loss_blocks", n)
        part = torch.empty(nblk, device=mu.device, dtype=torch.float32)
        t0 = _hbm_begin("kl_fwd")
        lib.call("pulpo_kl_fwd", _ptr(mu), _ptr(sigma), _ptr(mu1), _ptr(sigma1), n, _ptr(part), _stream())
        _hbm_end(t0, "kl_fwd", 4.0 * n * (2 + (mu1 is not None) + (sigma1 is not None)))
        ctx.save_for_backward(mu, sigma, mu1, sigma1)
        return _colsum(part, nblk, 1, 0.5 / mu.shape[0]).reshape(())

    @staticmethod
    def backward(ctx, g):
        mu, sigma, mu1, sigma1 = ctx.saved_tensors
        gmu, gsg = torch.empty_like(mu), torch.empty_like(sigma)
        g = g.contiguous()
        t0 = _hbm_begin("kl_bwd")
        lib.call("pulpo_kl_bwd", _ptr(mu), _ptr(sigma), _ptr(mu1), _ptr(sigma1), _ptr(g), 1.0 / mu.shape[0], _ptr(gmu), _ptr(gsg), mu.numel(),
                 _stream())
        _hbm_end(t0, "kl_bwd", 4.0 * mu.numel() * (4 + (mu1 is not None) + (sigma1 is not None)))
        return gmu, gsg, None, None


def kl_diag(mu, sigma, mu1=None, sigma1=None):
    """KL[N(mu, sigma^2) || N(mu1, sigma1^2)] (sum over features, mean over batch); mu1/sigma1 None = N(0,1).
    Gradients flow to (mu, sigma) only: the prior is a constant in the reference (pulpo.py:330-341)."""
    if _is2d(mu):
        return kl_diag(_lift(mu), _lift(sigma), _lift(mu1), _lift(sigma1))
    return _KL.apply(mu, sigma, mu1, sigma1)


def kl_std_normal(mu, sigma):
    return _KL.apply(mu, sigma, None, None)


class _L2Reg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, lamb: float):
        _require_gpu(df)
        df = planar(df)
        B, C, D, H, W = df.shape
        n = df.numel()
        nblk = lib.query("pulpo_loss_blocks", n)
        part = torch.empty(nblk, device=df.device, dtype=torch.float32)
        t0 = _hbm_begin("l2reg_fwd")
        lib.call("pulpo_l2reg_fwd", _ptr(df), B * C, D, H, W, _ptr(part), _stream())
        _hbm_end(t0, "l2reg_fwd", 4.0 * n)
        coef = lamb * D * H * W / float(B * C * max(D - 1, 1) * (H - 1) * (W - 1))      # D == 1: the 2-D form (no depth difference)
        ctx.save_for_backward(df)
        ctx.coef = coef
        return _colsum(part, nblk, 1, coef).reshape(())

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        B, C, D, H, W = df.shape
        gdf = torch.empty_like(df)
        g = g.contiguous()
        t0 = _hbm_begin("l2reg_bwd")
        lib.call("pulpo_l2reg_bwd", _ptr(df), _ptr(g), ctx.coef, _ptr(gdf), B * C, D, H, W, _stream())
        _hbm_end(t0, "l2reg_bwd", 8.0 * df.numel())
        return gdf, None


def l2_reg(df, lamb: float = 0.0):
    if _is2d(df):
        return l2_reg(_lift(df), lamb)
    return _L2Reg.apply(df, float(lamb))


class _Bending(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, lamb: float):
        df = planar(df)
        B, C, D, H, W = df.shape
        n = df.numel()
        nblk = lib.query("pulpo_bending_blocks", B * C, D, H, W)
        part = torch.empty(nblk, device=df.device, dtype=torch.float32)
        t0 = _hbm_begin("bending_fwd")
        lib.call("pulpo_bending_fwd", _ptr(df), B * C, D, H, W, _ptr(part), _stream())
        _hbm_end(t0, "bending_fwd", 4.0 * n)
        coef = lamb * D * H * W / float(B * C * max(D - 2, 1) * (H - 2) * (W - 2))      # D == 1: the 2-D form (interior 1..H-2, 1..W-2)
        ctx.save_for_backward(df)
        ctx.coef = coef
        return _colsum(part, nblk, 1, coef).reshape(())

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        B, C, D, H, W = df.shape
        gdf = torch.empty_like(df)
        g = g.contiguous()
        t0 = _hbm_begin("bending_bwd")
        lib.call("pulpo_bending_bwd", _ptr(df), _ptr(g), ctx.coef, _ptr(gdf), B * C, D, H, W, _stream())
        _hbm_end(t0, "bending_bwd", 8.0 * df.numel())
        return gdf, None


def bending_reg(df, lamb: float = 0.0):
    """lamb * D*H*W * mean over (batch, components, INTERIOR voxels) of the bending-energy density
    u_xx^2 + u_yy^2 + u_zz^2 + 2 u_xy^2 + 2 u_xz^2 + 2 u_yz^2 of a displacement field in voxels, central differences (DESIGN.md section 3o;
    no counterpart in the reference).  On L2_reg's scale, but an affine field costs nothing.  df (B,C,D,H,W), or (B,C,H,W) / a depth of 1 for
    the 2-D form (no z term); every other extent at least 3.  The gradient is a gather without atomics: bit-identical from run to run, in
    deterministic mode and out of it.  No double backward."""
    _require_gpu(df)
    if df.dim() not in (4, 5):
        raise ValueError(f"bending_reg: a field (B,C,D,H,W) or (B,C,H,W) expected, got shape {tuple(df.shape)}")
    if _is2d(df):
        df = _lift(df)
    if min(df.shape[3:]) < 3 or df.shape[2] in (0, 2) or df.shape[0] * df.shape[1] < 1:
        raise ValueError(f"bending_reg: every extent other than a depth of 1 must be at least 3 (central differences at interior voxels), got "
                         f"shape {tuple(df.shape)}")
    return _Bending.apply(df, float(lamb))


class _WeightedSum(torch.autograd.Function):
    """(sum_i w_i t_i, [w_0 t_0, ..., w_{n-1} t_{n-1}]) (optionally * scale): the per-level weighting and summation of the Hierarchical*
    losses as ONE launch (and one in the backward pass) instead of a mul + an add kernel per level and their autograd counterparts"""

    @staticmethod
    def forward(ctx, terms, weights_dev, scale):
        _require_gpu(terms, weights_dev)
        n = terms.numel()
        levels = torch.empty(n, device=terms.device, dtype=torch.float32)
        total = torch.empty((), device=terms.device, dtype=torch.float32)
        lib.call("pulpo_weighted_sum_fwd", _ptr(terms), _ptr(weights_dev), n, 1.0 if scale is None else float(scale), int(scale is not None),
                 _ptr(levels), _ptr(total), _stream())
        ctx.save_for_backward(weights_dev)
        ctx.scale = 1.0 if scale is None else float(scale)
        ctx.set_materialize_grads(False)
        return total, levels

    @staticmethod
    def backward(ctx, gtotal, glevels):
        (weights_dev,) = ctx.saved_tensors
        n = weights_dev.numel()
        if gtotal is None and glevels is None:
            return None, None, None
        gt = torch.empty(n, device=weights_dev.device, dtype=torch.float32)
        lib.call("pulpo_weighted_sum_bwd", _ptr(gtotal.contiguous() if gtotal is not None else None),
                 _ptr(glevels.contiguous() if glevels is not None else None), _ptr(weights_dev), n, ctx.scale, _ptr(gt), _stream())
        return gt, None, None


_WEIGHT_VECTORS: dict = {}


def weighted_sum(terms, weights, scale=None):
    """terms: list of 0-d device tensors, weights: list of python floats -> (sum, [w_i * term_i]) as 0-d views of one device vector.
    scale (optional) multiplies the sum and every level term afterwards (models.py:161-162: kl_loss * beta)."""
    dev = terms[0].device
    key = (tuple(float(w) for w in weights), dev)
    wd = _WEIGHT_VECTORS.get(key)
    if wd is None:
        if len(_WEIGHT_VECTORS) > 64:
            _WEIGHT_VECTORS.clear()
        wd = _WEIGHT_VECTORS[key] = torch.tensor(key[0], device=dev, dtype=torch.float32)
    total, levels = _WeightedSum.apply(torch.stack([t.reshape(()).float() for t in terms]), wd, scale)
    return total, [levels[i] for i in range(len(terms))]


# ------------------------------------------------------------------------------------------------ alternative losses / metrics
class _SqDiff(torch.autograd.Function):
    """unmasked (wa is None): L2_loss, the spatial sum of squared differences, mean over batch and channels; masked: the four scalars of
    pulpo_masked_finish - (L2_masked or, with root, RMSE_masked; d value / d sum; MaskFrac; M), DESIGN.md section 3i"""

    @staticmethod
    def forward(ctx, a, b, wa, wb, root: bool):
        _require_gpu(a, b, wa, wb)
        a, b = planar(a), planar(b)
        B, C = a.shape[0], a.shape[1]
        n = a.numel()
        V = n // (B * C)
        nblk = lib.query("pulpo_metric_blocks", n)
        ctx.masked = wa is not None
        if not ctx.masked:
            part = torch.empty(nblk, device=a.device, dtype=torch.float32)
            lib.call("pulpo_sqdiff_fwd", _ptr(a), _ptr(b), n, _ptr(part), _stream())
            ctx.save_for_backward(a, b)
            ctx.coef = 1.0 / (B * C)
            return _colsum(part, nblk, 1, ctx.coef).reshape(())
        part = torch.empty(2 * nblk, device=a.device, dtype=torch.float32)
        lib.call("pulpo_sqdiff_masked_fwd", _ptr(a), _ptr(b), _ptr(wa), _ptr(wb), _ptr(part), B, C, V, _stream())
        fin = _masked_finish(part, nblk, (1.0 if root else float(V)) / C, root, float(B * V))
        ctx.save_for_backward(a, b, wa, wb, fin)
        return fin

    @staticmethod
    def backward(ctx, g):
        a, b, *rest = ctx.saved_tensors
        ga = torch.empty_like(a)
        if ctx.masked:
            wa, wb, fin = rest
            B, C = a.shape[0], a.shape[1]
            gs = (g[0] * fin[1]).contiguous()
            lib.call("pulpo_sqdiff_masked_bwd", _ptr(a), _ptr(b), _ptr(wa), _ptr(wb), _ptr(gs), 1.0, _ptr(ga), B, C, a.numel() // (B * C), _stream())
        else:
            lib.call("pulpo_sqdiff_bwd", _ptr(a), _ptr(b), _ptr(g.contiguous()), ctx.coef, _ptr(ga), a.numel(), _stream())
        return ga, None, None, None, None


def l2_loss(inp, target):
    if _is2d(inp):
        inp, target = _lift(inp), _lift(target)
    return _SqDiff.apply(inp, target, None, None, False)


def _sqdiff_masked(inp, target, mask, mask2, root: bool, name: str):
    wa, wb = _masks_of(inp, mask, mask2, name)
    if _is2d(inp):
        inp, target = _lift(inp), _lift(target)
    if inp.shape != target.shape:
        raise ValueError(f"{name}: input {tuple(inp.shape)} and target {tuple(target.shape)} differ in shape")
    return _SqDiff.apply(inp, target, wa, wb, root)


def l2_loss_masked(inp, target, mask, mask2=None):
    """V sum(m (inp - target)^2) / (C M), m = mask * mask2 broadcast over the channels, M = sum(m) (0 for an empty mask): L2_loss with
    the per-voxel cost weighted by m.  Gradient to inp only."""
    return _sqdiff_masked(inp, target, mask, mask2, False, "l2_loss_masked")[0]


def rmse_masked(inp, target, mask, mask2=None):
    """(sqrt(L2_masked / V), MaskFrac = M / (B V)) as 0-d device tensors"""
    fin = _sqdiff_masked(inp, target, mask, mask2, True, "rmse_masked")
    return fin[0], fin[2].detach()


SIMILARITY_TERMS = ("ncc", "mse", "mind", "mi")


def similarity(kind: str, pred, true, mask=None, mask2=None, *, win: int = 9, gamma: float = 0.05, dilation: int = 2, eps: float = 1e-5,
               bins: int = 32):
    """the similarity term `kind` between pred and true: the one place that maps (term, masks) to an operator.  No mask: ncc_loss (window win,
    factor gamma) / l2_loss / mind_loss (dilation, eps; gamma does not apply: on MSE's scale already) / mi_loss (bins, factor gamma as for
    NCC); with either mask of the pair, in either argument: the masked form, cost weighted by mask * mask2.  An unknown kind raises
    ValueError before anything touches the device."""
    if kind not in SIMILARITY_TERMS:
        raise ValueError(f"similarity: term {kind!r} - one of {SIMILARITY_TERMS} expected")
    if mask is None:
        mask, mask2 = mask2, None
    if kind == "ncc":
        return ncc_loss(pred, true, win, gamma) if mask is None else ncc_loss_masked(pred, true, mask, mask2, win, gamma)
    if kind == "mse":
        return l2_loss(pred, true) if mask is None else l2_loss_masked(pred, true, mask, mask2)
    if kind == "mi":
        return mi_loss(pred, true, bins, gamma) if mask is None else mi_loss_masked(pred, true, mask, mask2, bins, gamma)
    return mind_loss(pred, true, dilation, eps) if mask is None else mind_loss_masked(pred, true, mask, mask2, dilation, eps)


class _Dice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, tgt, dice_factor: float):
        _require_gpu(inp, tgt)
        inp, tgt = planar(inp), planar(tgt)
        nplanes = inp.shape[0] * inp.shape[1]
        V = inp.numel() // nplanes
        nb = lib.query("pulpo_dice_blocks", V)
        part = torch.empty(nplanes * nb * 3, device=inp.device, dtype=torch.float32)
        numden = torch.empty(2 * nplanes, device=inp.device, dtype=torch.float64)
        loss = torch.empty((), device=inp.device, dtype=torch.float32)
        lib.call("pulpo_dice_fwd", _ptr(inp), _ptr(tgt), nplanes, V, dice_factor, _ptr(part), _ptr(numden), _ptr(loss), _stream())
        ctx.save_for_backward(inp, tgt, numden)
        ctx.meta = (nplanes, V, dice_factor)
        return loss

    @staticmethod
    def backward(ctx, g):
        inp, tgt, numden = ctx.saved_tensors
        nplanes, V, df = ctx.meta
        ginp = torch.empty_like(inp)
        lib.call("pulpo_dice_bwd", _ptr(inp), _ptr(tgt), _ptr(numden), _ptr(g.contiguous()), nplanes, V, df, _ptr(ginp), _stream())
        return ginp, None, None


def soft_dice_loss(inp, target, dice_factor=1):
    if _is2d(inp):
        return soft_dice_loss(_lift(inp), _lift(target), dice_factor)
    return _Dice.apply(inp, target, float(dice_factor))


def jacobian_det(df, normalize: bool = True):
    """determinant of the Jacobian of x + u(x), (B,3,D,H,W) -> (B,D,H,W); evaluation metric, not differentiable here"""
    if _is2d(df):                                      # (B,2,H,W) -> (B,H,W)
        return jacobian_det(_lift(df), normalize)[:, 0]
    _require_gpu(df)
    d = planar(df.detach())
    B, C, D, H, W = d.shape
    if C != (2 if D == 1 else 3):
        raise PulpoHipError("jacobian_det: displacement field (B,3,D,H,W) or, for slices, (B,2,1,H,W) expected")
    out = torch.empty((B, D, H, W), device=d.device, dtype=torch.float32)
    lib.call("pulpo_jacdet_fwd", _ptr(d), _ptr(out), None, B, D, H, W, int(bool(normalize)), _stream())
    return out


class _JDetStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, lamb: float, normalize: bool):
        _require_gpu(df)
        df = planar(df)
        B, C, D, H, W = df.shape
        n = B * D * H * W
        jd = torch.empty((B, D, H, W), device=df.device, dtype=torch.float32)
        part = torch.empty(2 * lib.query("pulpo_metric_blocks", n), device=df.device, dtype=torch.float64)     # block sums of J - 1, (J - 1)^2
        stat = torch.empty(2, device=df.device, dtype=torch.float64)
        loss = torch.empty((), device=df.device, dtype=torch.float32)
        lib.call("pulpo_jacdet_fwd", _ptr(df), _ptr(jd), _ptr(part), B, D, H, W, int(normalize), _stream())
        lib.call("pulpo_jdetstd_finalize", _ptr(part), n, lamb, _ptr(stat), _ptr(loss), _stream())
        ctx.save_for_backward(df, jd, stat)
        ctx.meta = (lamb, normalize)
        return loss

    @staticmethod
    def backward(ctx, g):
        df, jd, stat = ctx.saved_tensors
        lamb, normalize = ctx.meta
        B, _, D, H, W = df.shape
        if DETERMINISTIC:
            raise PulpoHipError("the `jdet` regulariser's backward scatters with float atomics and has no deterministic form (PULPO_DETERMINISTIC covers "
                                "the default training path: ncc / mse / dice + the L2 or the bending regulariser)")
        gdf = torch.empty_like(df)
        lib.call("pulpo_jdetstd_bwd", _ptr(df), _ptr(jd), _ptr(stat), _ptr(g.contiguous()), lamb, _ptr(gdf), B, D, H, W, int(normalize), _stream())
        return gdf, None, None


def jdet_std(df, lamb: float = 0.0, normalize: bool = True):
    if _is2d(df):
        return jdet_std(_lift(df), lamb, normalize)
    return _JDetStd.apply(df, float(lamb), bool(normalize))


class _KLNonDiag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, prior_lambda: float):
        _require_gpu(mu, sigma)
        mu, sigma = planar(mu), planar(sigma)
        B, C, D, H, W = mu.shape
        part = torch.empty(4 * lib.query("pulpo_metric_blocks", mu.numel()), device=mu.device, dtype=torch.float32)
        loss = torch.empty((), device=mu.device, dtype=torch.float32)
        lib.call("pulpo_kl_nondiag_fwd", _ptr(mu), _ptr(sigma), B * C, D, H, W, prior_lambda, _ptr(part), _ptr(loss), _stream())
        ctx.save_for_backward(mu, sigma)
        ctx.lam = prior_lambda
        return loss

    @staticmethod
    def backward(ctx, g):
        mu, sigma = ctx.saved_tensors
        B, C, D, H, W = mu.shape
        gmu, gsg = torch.empty_like(mu), torch.empty_like(sigma)
        lib.call("pulpo_kl_nondiag_bwd", _ptr(mu), _ptr(sigma), _ptr(g.contiguous()), B * C, D, H, W, ctx.lam, _ptr(gmu), _ptr(gsg), _stream())
        return gmu, gsg, None


def kl_nondiagonal(mu, sigma, prior_lambda: float = 20.0):
    if _is2d(mu):
        return kl_nondiagonal(_lift(mu), _lift(sigma), prior_lambda)
    return _KLNonDiag.apply(mu, sigma, float(prior_lambda))


# ------------------------------------------------------------------------------------------------ optimizer
# ------------------------------------------------------------------------------------------------ MC uncertainty
class StreamingMoments:
    """running per-voxel mean / unbiased std over Monte-Carlo samples (evaluate.py:222-251 keeps all N samples instead).
    update() folds one (B, C, D, H, W) sample in; std_map() = torch.mean(torch.std(stack, axis=0), axis=<channel>) -> (B, D, H, W)."""

    def __init__(self) -> None:
        self.count = 0
        self._mean = None
        self._m2 = None

    def update(self, sample: torch.Tensor) -> None:
        _require_gpu(sample)
        s = sample.detach().contiguous()
        if self._mean is None:
            self._mean, self._m2 = torch.empty_like(s), torch.empty_like(s)
        elif s.shape != self._mean.shape:
            raise ValueError(f"StreamingMoments: sample shape {tuple(s.shape)} differs from {tuple(self._mean.shape)}")
        self.count += 1
        lib.call("pulpo_mc_moments_update", _ptr(s), _ptr(self._mean), _ptr(self._m2), s.numel(), self.count, _stream())

    def mean(self) -> torch.Tensor:
        if self._mean is None:
            raise ValueError("StreamingMoments: no samples")
        return self._mean

    def m2(self) -> torch.Tensor:
        """the running sum of squared deviations from the mean (Welford's M2): var = M2 / (count - 1)"""
        if self._m2 is None:
            raise ValueError("StreamingMoments: no samples")
        return self._m2

    def std_map(self, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self._m2 is None:
            raise ValueError("StreamingMoments: no samples")
        B, C = self._m2.shape[0], self._m2.shape[1]
        V = self._m2[0, 0].numel()
        out = torch.empty((B,) + tuple(self._m2.shape[2:]), device=self._m2.device, dtype=torch.float32)
        sc = None
        if scale is not None:
            _require_gpu(scale)
            sc = scale.detach().expand((B, 1) + tuple(self._m2.shape[2:])).contiguous()
        lib.call("pulpo_mc_moments_std", _ptr(self._m2), _ptr(sc), _ptr(out), B, C, V, self.count, _stream())
        return out


def adam_step(p, g, m, v, lr: float, step: int, beta1=0.9, beta2=0.999, eps=1e-8, gscale: float = 1.0):
    _require_gpu(p, g, m, v)
    t0 = _hbm_begin("adam_step")
    lib.call("pulpo_adam_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, int(step), gscale, _stream())
    _hbm_end(t0, "adam_step", 28.0 * p.numel())               # read p, g, m, v; write p, m, v
    refresh_weight_packs()                       # the kernel rewrote parameters through raw pointers: the cached packs follow, in one launch


def anchored_adam_step(p, g, m, v, lr: float, step: int, mean=None, prec=None, loss_out=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """Adam over a flat arena of velocity fields (pulpo_amd.refine) in one launch.  With `mean` the gradient used is
    g + a (p - mean), a = prec (per element) or 1, and `loss_out` (a 1-element fp32 tensor, optional) receives 0.5 sum a (p - mean)^2 at the
    iterate before the update; mean=None is adam_step's arithmetic bit for bit.  The arena holds no network parameter: no weight pack is
    refreshed.  Every tensor flat, contiguous and 16-byte aligned (the library checks)."""
    _require_gpu(p, g, m, v, mean, prec, loss_out)
    if prec is not None and mean is None:
        raise ValueError("anchored_adam_step: prec needs mean")
    n = p.numel()
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("mean", mean), ("prec", prec)):
        if t is not None and (t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"anchored_adam_step: {name} must be contiguous with {n} elements")
    part = None
    if mean is not None and loss_out is not None:
        if loss_out.numel() != 1:
            raise ValueError("anchored_adam_step: loss_out is one fp32 element")
        nblk = lib.query("pulpo_loss_blocks", n)
        part = torch.empty(nblk, device=p.device, dtype=torch.float32)
    t0 = _hbm_begin("anchored_adam_step")
    lib.call("pulpo_anchored_adam_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(mean), _ptr(prec), n, lr, beta1, beta2, eps, int(step), _ptr(part),
             _stream())
    _hbm_end(t0, "anchored_adam_step", (28.0 + 4.0 * (mean is not None) + 4.0 * (prec is not None)) * n)       # read p, g, m, v (mean, prec); write p, m, v
    if part is not None:
        lib.call("pulpo_colsum", _ptr(part), nblk, 1, _ptr(loss_out), 1.0, 0, _stream())


# ------------------------------------------------------------------------------------------------ evaluation scalars (evaluate.py)
def rmse(inp, target):
    """sqrt(MSELoss(inp, target)) as a 0-d device tensor (evaluate.py:315-319)"""
    _require_gpu(inp, target)
    a, b = inp.detach().contiguous(), target.detach().expand_as(inp).contiguous()
    n = a.numel()
    part = torch.empty(lib.query("pulpo_metric_blocks", n), device=a.device, dtype=torch.float32)
    out = torch.empty((), device=a.device, dtype=torch.float32)
    lib.call("pulpo_rmse", _ptr(a), _ptr(b), n, _ptr(part), _ptr(out), _stream())
    return out


def dsc(inp, target):
    """dice similarity coefficient of two (soft) segmentation maps (evaluate.py:321-327), 0-d device tensor"""
    _require_gpu(inp, target)
    a, b = inp.detach().contiguous(), target.detach().expand_as(inp).contiguous()
    nplanes = a.shape[0] * a.shape[1]
    V = a.numel() // nplanes
    part = torch.empty(nplanes * lib.query("pulpo_dice_blocks", V) * 3, device=a.device, dtype=torch.float32)
    out = torch.empty((), device=a.device, dtype=torch.float32)
    lib.call("pulpo_dsc", _ptr(a), _ptr(b), nplanes, V, _ptr(part), _ptr(out), _stream())
    return out


def percent_leq0(x):
    """100 * (x <= 0).sum() / x.numel() as a 0-d device tensor (the 'JDetLeq0' metric, evaluate.py:1441-1446)"""
    _require_gpu(x)
    a = x.detach().contiguous()
    n = a.numel()
    part = torch.empty(lib.query("pulpo_metric_blocks", n), device=a.device, dtype=torch.float32)
    out = torch.empty((), device=a.device, dtype=torch.float32)
    lib.call("pulpo_percent_leq0", _ptr(a), n, _ptr(part), _ptr(out), _stream())
    return out


@torch.no_grad()
def field_quality(df, normalize: bool = True):
    """(mean, unbiased std, 100 * count(J <= 0) / numel) of jacobian_det(df, normalize) as 0-d device tensors, in one pass that reads the
    field once and stores no determinant map (evaluate.py:1440-1449: JDetStd with lamb = 1 and JDetLeq0).  The determinant is
    jacobian_det's bit for bit; deterministic.  df (B,3,D,H,W) or (B,2,H,W).  Evaluation only: no autograd."""
    if _is2d(df):
        return field_quality(_lift(df), normalize)
    _require_gpu(df)
    d = planar(df.detach())
    B, C, D, H, W = d.shape
    if C != (2 if D == 1 else 3):
        raise PulpoHipError("field_quality: displacement field (B,3,D,H,W) or, for slices, (B,2,1,H,W) expected")
    ws = torch.empty(lib.query("pulpo_field_quality_ws_bytes", B, D, H, W), device=d.device, dtype=torch.uint8)
    out = torch.empty(3, device=d.device, dtype=torch.float32)
    lib.call("pulpo_field_quality", _ptr(d), _ptr(out), _ptr(ws), B, D, H, W, int(bool(normalize)), _stream())
    return out[0], out[1], out[2]


def warp_landmarks(lm, df):
    """lm.long() - df[:, :, lm[0,:,0], lm[0,:,1], lm[0,:,2]].transpose(-2, -1)   (evaluate.py:410-423, src/components/utils.py:15-25)
    lm: (1, n_landmarks, ndims); df: (n_samples, ndims, ...) -> (n_samples, n_landmarks, ndims) float.  Out-of-range landmarks raise
    IndexError like the reference's tensor indexing (one host read of a device flag: an evaluation-time helper)."""
    _require_gpu(df)
    nd = df.dim() - 2
    if lm.dim() != 3 or lm.shape[0] != 1 or lm.shape[2] != nd or df.shape[1] != nd or nd not in (2, 3):
        raise PulpoHipError(f"warp_landmarks: lm (1, n, ndims) and df (samples, ndims, ...) expected, got {tuple(lm.shape)} and {tuple(df.shape)}")
    d = df.detach().contiguous()
    l = lm.detach().to(device=d.device, dtype=torch.float32).contiguous()
    nlm, ns = int(lm.shape[1]), int(d.shape[0])
    D, H, W = (1, *d.shape[2:]) if nd == 2 else d.shape[2:]
    out = torch.empty((ns, nlm, nd), device=d.device, dtype=torch.float32)
    flag = torch.empty(1, device=d.device, dtype=torch.int32)
    lib.call("pulpo_warp_landmarks", _ptr(l), _ptr(d), _ptr(out), nlm, ns, nd, int(D), int(H), int(W),
             ctypes.cast(flag.data_ptr(), ctypes.POINTER(ctypes.c_int)), _stream())
    if int(flag.item()):
        raise IndexError("warp_landmarks: landmark index out of bounds of the displacement field")
    return out


@torch.no_grad()
def inverse_consistency(a, b):
    """(mean, max) over all voxels of ||b(p) + a(p + b(p))||_2 in voxel units as 0-d device tensors: how far the composition a o b is from
    the identity (a = final field, b = its inverse: the sanity number of a diffeomorphic model next to JDetLeq0).  a sampled geometrically
    - position clamped to [0, S - 1], trilinear, a zero field is the identity - not with SpatialTransformer's normalisation.  One pass,
    no composed field; deterministic.  a, b (B,3,D,H,W) or (B,2,H,W) of one shape.  Evaluation only: no autograd."""
    _require_gpu(a, b)
    if tuple(a.shape) != tuple(b.shape):
        raise PulpoHipError(f"inverse_consistency: fields of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    if _is2d(a):
        a, b = _lift(a), _lift(b)
    a, b = planar(a.detach()), planar(b.detach())
    B, C, D, H, W = a.shape
    if C != (2 if D == 1 else 3):
        raise PulpoHipError("inverse_consistency: displacement fields (B,3,D,H,W) or, for slices, (B,2,H,W) expected")
    ws = torch.empty(lib.query("pulpo_inverse_consistency_ws_bytes", B, D, H, W), device=a.device, dtype=torch.uint8)
    out = torch.empty(2, device=a.device, dtype=torch.float32)
    t0 = _hbm_begin("inverse_consistency")
    lib.call("pulpo_inverse_consistency", _ptr(a), _ptr(b), _ptr(out), _ptr(ws), B, D, H, W, _stream())
    _hbm_end(t0, "inverse_consistency", 4.0 * (a.numel() + b.numel()))                  # both fields read once (the gather hits in cache)
    return out[0], out[1]


def transport_points(pts, field):
    """pts + field(pts): points carried by a displacement field sampled trilinearly at their own fractional positions (geometric
    sampling, as inverse_consistency).  With the inverse field of vecint_pair / combine_dfs_bidirectional this moves landmarks of the moving
    image onto the fixed image exactly; warp_landmarks' long(lm) - df[long(lm)] is its first-order approximation at a truncated position.
    pts: (1, n, ndims) voxel coordinates; field: (n_samples, ndims, ...) -> (n_samples, n, ndims).  A point outside [0, S - 1] raises
    IndexError like warp_landmarks (one host read of a device flag: an evaluation-time helper)."""
    _require_gpu(field)
    nd = field.dim() - 2
    if pts.dim() != 3 or pts.shape[0] != 1 or pts.shape[2] != nd or field.shape[1] != nd or nd not in (2, 3):
        raise PulpoHipError(f"transport_points: pts (1, n, ndims) and field (samples, ndims, ...) expected, got {tuple(pts.shape)} and {tuple(field.shape)}")
    d = field.detach().contiguous()
    p = pts.detach().to(device=d.device, dtype=torch.float32).contiguous()
    npts, ns = int(pts.shape[1]), int(d.shape[0])
    D, H, W = (1, *d.shape[2:]) if nd == 2 else d.shape[2:]
    out = torch.empty((ns, npts, nd), device=d.device, dtype=torch.float32)
    flag = torch.empty(1, device=d.device, dtype=torch.int32)
    t0 = _hbm_begin("transport_points")
    lib.call("pulpo_transport_points", _ptr(p), _ptr(d), _ptr(out), npts, ns, nd, int(D), int(H), int(W),
             ctypes.cast(flag.data_ptr(), ctypes.POINTER(ctypes.c_int)), _stream())
    _hbm_end(t0, "transport_points", 4.0 * (p.numel() + out.numel() + 8 * nd * npts * ns))      # the points, the results, 8 corners per component
    if int(flag.item()):
        raise IndexError("transport_points: point outside the displacement field")
    return out


# ------------------------------------------------------------------------------------------------ label maps (MC segmentation uncertainty)
# Evaluation-time operators: no autograd (call them under torch.no_grad(); the outputs carry no graph).  Label maps are uint8 or int32.
_LABEL_DT = {torch.uint8: 0, torch.int32: 1}


def _require_labels(*ts: Optional[torch.Tensor]):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise PulpoHipError("pulpo_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
        if t.dtype not in _LABEL_DT:
            raise PulpoHipError(f"label maps are uint8 or int32 (got {t.dtype})")


def _int_ptr(t: Optional[torch.Tensor], i: int = 0):
    return None if t is None else ctypes.cast(t.data_ptr() + 4 * i, ctypes.POINTER(ctypes.c_int))


def _check_labels(labels: torch.Tensor, num_classes: int, flag: torch.Tensor, i: int) -> None:
    lib.call("pulpo_labels_check", _ptr(labels), _LABEL_DT[labels.dtype], labels.numel(), int(num_classes), _int_ptr(flag, i), _stream())


def _raise_on_flag(flag: torch.Tensor, what: str) -> None:
    if int(flag.max().item()):                     # one host read
        raise IndexError(f"{what}: label outside [0, num_classes)")


def _warp_labels_raw(df, labels, C: int, target, onehot, amax, dice, mean, m2, k: int, flag, fi: int):
    """df (B,3,Dg,Hg,Wg) planar fp32, labels (B,1,Di,Hi,Wi), target (B,1,Dg,Hg,Wg) of the labels' dtype: one pulpo_warp_labels launch"""
    B, _, Dg, Hg, Wg = df.shape
    Di, Hi, Wi = labels.shape[2:]
    ws = torch.empty(lib.query("pulpo_warp_labels_ws_bytes", B, C), device=df.device, dtype=torch.uint8) if target is not None else None
    lib.call("pulpo_warp_labels", _ptr(df), _ptr(labels), _LABEL_DT[labels.dtype], C, _ptr(target), _ptr(onehot), _ptr(amax), _ptr(dice),
             _ptr(mean), _ptr(m2), int(k), _ptr(ws), _int_ptr(flag, fi), B, Dg, Hg, Wg, int(Di), int(Hi), int(Wi), _stream())


def _lift_labels(df, labels, target):
    """2-D inputs -> the depth-1 3-D form of warp3d; label maps as contiguous (B,1,D,H,W), the target in the labels' dtype"""
    if _is2d(df):
        df, labels, target = _lift_field(df), _lift(labels), _lift(target)
    df, labels = planar(df.detach()), labels.contiguous()
    if labels.dim() != 5 or labels.shape[1] != 1 or labels.shape[0] != df.shape[0]:
        raise PulpoHipError(f"label map (B, 1, ...) expected for a field of shape {tuple(df.shape)}, got {tuple(labels.shape)}")
    if target is not None:
        target = target.to(labels.dtype).contiguous()
        if tuple(target.shape) != (df.shape[0], 1) + tuple(df.shape[2:]):
            raise PulpoHipError(f"target label map (B, 1) + the field's grid expected, got {tuple(target.shape)}")
    return df, labels, target


@torch.no_grad()
def warp_labels(df, labels, num_classes: int, target=None, onehot: bool = False, argmax: bool = False):
    """warp3d(df, one_hot(labels, num_classes)) without the one-hot maps (SpatialTransformer on a segmentation, evaluate.py:252-274).
    df (B, 3, D, H, W) fp32 (2-D: (B, 2, H, W)); labels (B, 1, ...) uint8 / int32 on the moving map's grid, which may differ from the field's.
    Returns the requested outputs in this order - onehot: the warped one-hot map (B, C, grid) fp32; argmax: its arg-max label map
    (B, 1, grid) in the labels' dtype, the lowest class on ties; target (B, 1, grid): per-class Dice (B, C) of the warped one-hot map against
    one_hot(target) (Evaluate.dsc per class, evaluate.py:321-327) - a single tensor when one output is requested.  A label outside
    [0, num_classes) raises IndexError (one host read).  Evaluation only: no autograd."""
    if not (onehot or argmax or target is not None):
        raise ValueError("warp_labels: request at least one of onehot, argmax, target")
    return _warp_labels(df, labels, num_classes, target, onehot, argmax, True)


def _warp_labels(df, labels, num_classes: int, target, onehot: bool, argmax: bool, check: bool):
    """warp_labels; check=False skips the label-range pass and its host read (for maps the caller has range-checked already)"""
    _require_gpu(df)
    _require_labels(labels, target)
    is2d = _is2d(df)
    df, labels, target = _lift_labels(df, labels, target)
    B, C = df.shape[0], int(num_classes)
    grid = tuple(df.shape[2:])
    dev = df.device
    oh = torch.empty((B, C) + grid, device=dev, dtype=torch.float32) if onehot else None
    am = torch.empty((B, 1) + grid, device=dev, dtype=labels.dtype) if argmax else None
    dice = torch.empty((B, C), device=dev, dtype=torch.float32) if target is not None else None
    flag = torch.zeros(3, device=dev, dtype=torch.int32)
    if check:
        _check_labels(labels, C, flag, 1)
        if target is not None:
            _check_labels(target, C, flag, 2)
    _warp_labels_raw(df, labels, C, target, oh, am, dice, None, None, 1, flag, 0)
    if check:
        _raise_on_flag(flag, "warp_labels")
    out = [t.squeeze(2) if is2d else t for t in (oh, am) if t is not None] + ([dice] if dice is not None else [])
    return out[0] if len(out) == 1 else tuple(out)


@torch.no_grad()
def warp_labels_soft_dice(df, labels, num_classes: int, target):
    """The level Dice of Evaluate.performance (evaluate.py:1427, 1454-1455) without a one-hot tensor: for p = warp3d(df, one_hot(labels)) and
    t = F.interpolate(one_hot(target), size=grid of df, tri/bilinear, align_corners=False), dice_bc = (2 sum(p t) + 1e-6) / (sum(t^2) +
    sum(p^2) + 1e-6) with sums over the grid (Soft_dice_loss, src/losses.py:137-145).  df (B,3,D,H,W) fp32 (2-D: (B,2,H,W)); labels and target
    (B,1,...) uint8 / int32 label maps, each on a grid of its own (the full-resolution maps for every level's field).  Returns (dice_bc (B, C),
    their mean as a 0-d tensor = 1 - level_dice / num_pixels).  Deterministic.  A label outside [0, num_classes) raises IndexError (one
    host read).  Evaluation only: no autograd."""
    _require_gpu(df)
    _require_labels(labels, target)
    if target is None:
        raise ValueError("warp_labels_soft_dice: a target label map is required")
    if _is2d(df):
        df, labels, target = _lift_field(df), _lift(labels), _lift(target)
    df, labels, target = planar(df.detach()), labels.contiguous(), target.to(labels.dtype).contiguous()
    B, C = df.shape[0], int(num_classes)
    for name, t in (("label", labels), ("target", target)):
        if t.dim() != 5 or t.shape[1] != 1 or t.shape[0] != B:
            raise PulpoHipError(f"{name} map (B, 1, ...) expected for a field of shape {tuple(df.shape)}, got {tuple(t.shape)}")
    dev = df.device
    dice = torch.empty((B, C), device=dev, dtype=torch.float32)
    mean = torch.empty((), device=dev, dtype=torch.float32)
    flag = torch.zeros(3, device=dev, dtype=torch.int32)
    _check_labels(labels, C, flag, 1)
    _check_labels(target, C, flag, 2)
    ws = torch.empty(lib.query("pulpo_warp_labels_ws_bytes", B, C), device=dev, dtype=torch.uint8)
    lib.call("pulpo_warp_labels_soft_dice", _ptr(df), _ptr(labels), _ptr(target), _LABEL_DT[labels.dtype], C, _ptr(dice), _ptr(mean), _ptr(ws),
             _int_ptr(flag, 0), B, *[int(v) for v in df.shape[2:]], *[int(v) for v in labels.shape[2:]], *[int(v) for v in target.shape[2:]], _stream())
    _raise_on_flag(flag, "warp_labels_soft_dice")
    return dice, mean


class LabelMoments(StreamingMoments):
    """StreamingMoments of warp3d(df, one_hot(labels, C)) without a per-sample C-channel tensor: update(df, labels) folds the warped one-hot
    map in (the arithmetic of StreamingMoments.update, so N updates equal StreamingMoments over the N warped one-hot maps); mean() and
    std_map() are StreamingMoments'.  update(..., target=...) also returns that sample's per-class Dice (B, C), from the same pass.
    Evaluation only: no autograd."""

    def __init__(self, num_classes: int) -> None:
        super().__init__()
        self.num_classes = int(num_classes)
        self._checked = None

    @torch.no_grad()
    def update(self, df, labels, target=None):
        _require_gpu(df)
        _require_labels(labels, target)
        shape2d = (df.shape[0], self.num_classes) + tuple(df.shape[2:]) if _is2d(df) else None
        df, labels, target = _lift_labels(df, labels, target)
        B, C = df.shape[0], self.num_classes
        shape = shape2d or (B, C) + tuple(df.shape[2:])
        if self._mean is None:
            self._mean = torch.empty(shape, device=df.device, dtype=torch.float32)
            self._m2 = torch.empty_like(self._mean)
        elif tuple(self._mean.shape) != tuple(shape):
            raise ValueError(f"LabelMoments: sample shape {tuple(shape)} differs from {tuple(self._mean.shape)}")
        flag = torch.zeros(3, device=df.device, dtype=torch.int32)
        # the whole label map is range-checked (one host read) whenever it is a map not seen before; the samples of a Monte-Carlo loop
        # share one map and then run without a host synchronisation
        key = (labels.data_ptr(), tuple(labels.shape), labels.dtype, None if target is None else (target.data_ptr(), tuple(target.shape)))
        check = key != self._checked
        if check:
            _check_labels(labels, C, flag, 1)
            if target is not None:
                _check_labels(target, C, flag, 2)
            _raise_on_flag(flag, "LabelMoments.update")
            self._checked = key
        dice = torch.empty((B, C), device=df.device, dtype=torch.float32) if target is not None else None
        self.count += 1
        _warp_labels_raw(df, labels, C, target, None, None, dice, self._mean, self._m2, self.count, flag, 0)
        return dice


@torch.no_grad()
def labels_from_onehot(seg, dtype: Optional[torch.dtype] = None):
    """(B, C, ...) fp32 one-hot (or soft) segmentation -> (B, 1, ...) label map: arg-max over C, the lowest class on ties.  Converts the
    reference's one-hot loader output (src/data/OASIS/oasis.py:17,78) once per pair.  dtype: uint8 (default for C <= 256) or int32.
    Evaluation only: no autograd."""
    _require_gpu(seg)
    s = seg.detach().contiguous()
    B, C = int(s.shape[0]), int(s.shape[1])
    dtype = dtype or (torch.uint8 if C <= 256 else torch.int32)
    if dtype not in _LABEL_DT:
        raise PulpoHipError(f"label maps are uint8 or int32 (got {dtype})")
    out = torch.empty((B, 1) + tuple(s.shape[2:]), device=s.device, dtype=dtype)
    lib.call("pulpo_labels_from_onehot", _ptr(s), _ptr(out), _LABEL_DT[dtype], B, C, s[0, 0].numel(), _stream())
    return out


@torch.no_grad()
def map_ncc(a, b):
    """Evaluate.ncc(a, b) (evaluate.py:334-353: zero-normed, population std, eps 1e-15) of two maps of equal size, accumulated in double
    on the device with a deterministic two-stage reduction; returns a 0-d float64 device tensor.  Evaluation only: no autograd."""
    _require_gpu(a, b)
    x, y = a.detach().contiguous(), b.detach().contiguous()
    if x.numel() != y.numel():
        raise PulpoHipError(f"map_ncc: maps of {x.numel()} and {y.numel()} elements")
    n = x.numel()
    part = torch.empty(5 * lib.query("pulpo_map_ncc_blocks", n), device=x.device, dtype=torch.float64)
    out = torch.empty((), device=x.device, dtype=torch.float64)
    lib.call("pulpo_map_ncc", _ptr(x), _ptr(y), n, _ptr(part), _ptr(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------ Dice term from label maps
def _label_map5(t: torch.Tensor, B: int, name: str) -> torch.Tensor:
    if t.dim() != 5 or t.shape[1] != 1 or t.shape[0] != B:
        raise PulpoHipError(f"{name} map (B, 1, ...) with B = {B} expected, got {tuple(t.shape)}")
    return t.contiguous()


class _LabelDice(torch.autograd.Function):
    """(loss, dice (B, C)) of a field (B,3,Dg,Hg,Wg) or (B,2,H,W) and two contiguous (B,1,D,H,W) label maps of one dtype; saves the planar field,
    the maps and the (B, C, 2) coefficient table - nothing C times the volume.  The gradient has the caller's channel count, contiguous."""

    @staticmethod
    def forward(ctx, df, labels, target, C: int, dice_factor: float, flag):
        ctx.two_d = _is2d(df)
        df = planar(_lift_field(df) if ctx.two_d else df)
        B = df.shape[0]
        dev = df.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dice = torch.empty((B, C), device=dev, dtype=torch.float32)
        coef = torch.empty((B, C, 2), device=dev, dtype=torch.float32)
        ws = torch.empty(lib.query("pulpo_warp_labels_ws_bytes", B, C), device=dev, dtype=torch.uint8)
        dims = [int(v) for v in (*df.shape[2:], *labels.shape[2:], *target.shape[2:])]
        lib.call("pulpo_label_dice_fwd", _ptr(df), _ptr(labels), _ptr(target), _LABEL_DT[labels.dtype], C, dice_factor, _ptr(loss), _ptr(dice),
                 _ptr(coef), _ptr(ws), _int_ptr(flag, 0), B, *dims, _stream())
        ctx.save_for_backward(df, labels, target, coef)
        ctx.meta = (C, dims)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    def backward(ctx, g, _gdice):
        df, labels, target, coef = ctx.saved_tensors
        C, dims = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        ddf = torch.empty_like(df)
        gup = g.detach().to(torch.float32).contiguous()                 # read on the device, like pulpo_dice_bwd's gscale: no host synchronisation
        t0 = _hbm_begin("label_dice_bwd")
        lib.call("pulpo_label_dice_bwd", _ptr(df), _ptr(labels), _ptr(target), _LABEL_DT[labels.dtype], C, _ptr(coef), _ptr(gup), _ptr(ddf),
                 df.shape[0], *dims, _stream())
        # the field read and its gradient written once; a label byte per voxel of either map when the grids agree
        _hbm_end(t0, "label_dice_bwd", 4.0 * 2 * df.numel() + labels.element_size() * (labels.numel() + target.numel()))
        return (_unlift_field(ddf).contiguous() if ctx.two_d else ddf), None, None, None, None, None


def label_dice_loss(df, labels, num_classes: int, target, dice_factor=1, check: bool = True, return_dice: bool = False):
    """Soft_dice_loss(warp3d(df, one_hot(labels)), F.interpolate(one_hot(target), size = df's grid), dice_factor) (src/losses.py:137-145, the Dice
    term of HierarchicalReconstructionLoss) from integer label maps: no one-hot tensor in the forward pass, the backward pass or the saved
    state.  df (B,3,D,H,W) fp32 (2-D: (B,2,H,W)); labels and target (B,1,...) uint8 / int32, each on a grid of its own.  Differentiable with
    respect to df only; the gradient is one gather per grid voxel, without atomics: two calls give the same bits.  check=True range-checks both
    maps (one host read) and raises IndexError for a label outside [0, num_classes); check=False reads nothing back (a label out of range then
    counts for no class) and can be captured into a HIP graph.  return_dice: also the per-class Dice (B, C), ops.warp_labels_soft_dice's values."""
    _require_gpu(df)
    _require_labels(labels, target)
    if target is None or labels is None:
        raise ValueError("label_dice_loss: a moving and a target label map are required")
    if df.dim() not in (4, 5) or df.shape[1] != df.dim() - 2:
        raise PulpoHipError(f"label_dice_loss: field (B,3,D,H,W) or (B,2,H,W) expected, got {tuple(df.shape)}")
    if _is2d(df):
        labels, target = _lift(labels), _lift(target)
    B, C = int(df.shape[0]), int(num_classes)
    labels = _label_map5(labels.detach(), B, "label")
    target = _label_map5(target.detach().to(labels.dtype), B, "target")
    flag = torch.zeros(3, device=df.device, dtype=torch.int32)
    if check:
        _check_labels(labels, C, flag, 1)
        _check_labels(target, C, flag, 2)
    loss, dice = _LabelDice.apply(df, labels, target, C, float(dice_factor), flag)
    if check:
        _raise_on_flag(flag, "label_dice_loss")
    return (loss, dice) if return_dice else loss


@torch.no_grad()
def labels_soft_map(labels, num_classes: int, pool2: bool = False, size=None):
    """A pooled or resized one-hot map from an integer label map, without the full-resolution one-hot volume.  labels (B,1,...) uint8 / int32.
    pool2=True: (B, C, ceil(S / 2)) fp32 equal to avg_pool2(one_hot(labels)) bit for bit; size=(...): (B, C, size) fp32 =
    F.interpolate(one_hot(labels), size, tri/bilinear, align_corners=False).  Exactly one of the two.  A label outside [0, num_classes) counts
    for no class.  No autograd, no host read."""
    if bool(pool2) == (size is not None):
        raise ValueError("labels_soft_map: give exactly one of pool2=True and size=")
    _require_labels(labels)
    two_d = _is2d(labels)
    lab = _label_map5(_lift(labels) if two_d else labels, int(labels.shape[0]), "label")
    B, C = int(lab.shape[0]), int(num_classes)
    D, H, W = (int(v) for v in lab.shape[2:])
    if pool2:
        out = torch.empty((B, C, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), device=lab.device, dtype=torch.float32)
        lib.call("pulpo_labels_pool2", _ptr(lab), _LABEL_DT[lab.dtype], C, _ptr(out), B, D, H, W, _stream())
    else:
        size = tuple(int(s) for s in size)
        if len(size) != (2 if two_d else 3) or min(size) < 1:
            raise ValueError(f"labels_soft_map: a size of {2 if two_d else 3} extents >= 1 expected, got {size}")
        Do, Ho, Wo = ((1,) + size) if two_d else size
        out = torch.empty((B, C, Do, Ho, Wo), device=lab.device, dtype=torch.float32)
        lib.call("pulpo_labels_resize", _ptr(lab), _LABEL_DT[lab.dtype], C, _ptr(out), B, D, H, W, Do, Ho, Wo, _stream())
    return out.squeeze(2) if two_d else out


# ------------------------------------------------------------------------------------------------ boundary metrics
EDT_INF = 1 << 29          # edt_sq of an item without a feature voxel (PULPO_EDT_INF)


@torch.no_grad()
def edt_sq(mask):
    """Exact squared Euclidean distance transform, in voxels: out[p] = min over the set voxels q of |p - q|^2 as int32 of the mask's shape.
    mask (B, 1, D, H, W) or (B, 1, H, W), bool or uint8 (non-zero = set).  A batch item without a set voxel gets EDT_INF everywhere.
    Extents up to 1024 per axis.  Evaluation only: no autograd."""
    if not mask.is_cuda:
        raise PulpoHipError("pulpo_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise PulpoHipError(f"edt_sq: the mask is bool or uint8 (got {mask.dtype})")
    if mask.dim() not in (4, 5) or mask.shape[1] != 1:
        raise PulpoHipError(f"edt_sq: mask (B, 1, D, H, W) or (B, 1, H, W) expected, got {tuple(mask.shape)}")
    m = mask.detach().contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    m5 = _lift(m) if _is2d(m) else m
    out = torch.empty(m5.shape, device=m.device, dtype=torch.int32)
    B, _, D, H, W = (int(v) for v in m5.shape)
    lib.call("pulpo_edt_sq", _ptr(m5), _int_ptr(out), B, D, H, W, _stream())
    return out.squeeze(2) if _is2d(m) else out


def _surface_distances(lab_a, lab_b, C: int, percentile: float, return_hist: bool, check: bool):
    """surface_distances; check=False skips the host read of the label-range flag (for maps the caller has range-checked already)"""
    _require_labels(lab_a, lab_b)
    if tuple(lab_a.shape) != tuple(lab_b.shape) or lab_a.dim() not in (4, 5) or lab_a.shape[1] != 1:
        raise PulpoHipError(f"surface_distances: two label maps (B, 1, ...) on one grid expected, got {tuple(lab_a.shape)} and {tuple(lab_b.shape)}")
    nd = 2 if _is2d(lab_a) else 3
    if nd == 2:
        lab_a, lab_b = _lift(lab_a), _lift(lab_b)
    a = lab_a.detach().contiguous()
    B, _, D, H, W = (int(v) for v in a.shape)
    dev = a.device
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    b = lab_b.detach().contiguous()
    if b.dtype != a.dtype:                            # mixed dtypes run as int32: narrowing would wrap a label above 255 into range
        a, b = a.to(torch.int32), b.to(torch.int32)
    bins = int(lib.query("pulpo_surface_distances_bins", D, H, W))
    nbytes = int(lib.query("pulpo_surface_distances_ws_bytes", B, C, D, H, W))
    if bins <= 0 or nbytes <= 0:
        raise PulpoHipError(f"surface_distances: num_classes >= 1 and extents 1 ... 1024 per axis expected, got C = {C}, grid {(D, H, W)}")
    out = torch.empty((B, C, 5), device=dev, dtype=torch.float32)
    hist = torch.empty((B, C, 2, bins), device=dev, dtype=torch.int32) if return_hist else None
    # the workspace ends with room for the histograms, which a caller that passes its own leaves off
    ws = torch.empty(nbytes - (hist.numel() * 4 if return_hist else 0), device=dev, dtype=torch.uint8)
    lib.call("pulpo_surface_distances", _ptr(a), _ptr(b), _LABEL_DT[a.dtype], C, float(percentile), _ptr(out), _int_ptr(hist), _ptr(ws),
             _int_ptr(flag), B, D, H, W, nd, _stream())
    if check:
        _raise_on_flag(flag, "surface_distances")
    counts = ws[:8 * B * C].view(torch.int32).view(B, C, 2).clone()          # the exact int32 counts the workspace starts with
    res = {"hd": out[..., 0], "hd_pct": out[..., 1], "assd": out[..., 2], "n_a": counts[..., 0], "n_b": counts[..., 1]}
    if return_hist:
        res["hist"] = hist
    return res


@torch.no_grad()
def surface_distances(lab_a, lab_b, num_classes: int, percentile: float = 95.0, return_hist: bool = False):
    """Boundary distances between two label maps (B, 1, ...) uint8 / int32 on one grid, per batch item and class, in voxels.  The surface
    S_c(L) of class c is the set of its voxels with a face neighbour (6 in 3-D, 4 in 2-D) outside the class, the outside of the volume
    included; d_AB = the distances of the voxels of S_c(A) to S_c(B), d_BA the mirror.  Returns a dict of (B, C) tensors:
      hd      max(max d_AB, max d_BA)                                         (Hausdorff distance)
      hd_pct  max(percentile(d_AB), percentile(d_BA)), numpy's linear rule    (HD95 for percentile = 95)
      assd    (sum d_AB + sum d_BA) / (n_a + n_b)                             (average symmetric surface distance)
      n_a, n_b  the surface voxel counts (int32)
    hd, hd_pct and assd are NaN for a class absent from either map.  return_hist adds hist (B, C, 2, bins) int32, the counts of d_AB^2
    ([:, :, 0]) and d_BA^2, bins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1.  Exact integer arithmetic up to the final square roots: bit-identical
    from call to call.  A label outside [0, num_classes) raises IndexError (one host read).  Evaluation only: no autograd."""
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"surface_distances: percentile {percentile} outside [0, 100]")
    return _surface_distances(lab_a, lab_b, int(num_classes), float(percentile), return_hist, True)



# ------------------------------------------------------------------------------------------------ affine pre-alignment
def _theta3(theta, name: str):
    """(theta as (B,3,4), was 2-D): a (B,2,3) slice transform is lifted with an identity depth row and column, by differentiable torch ops on
    its six entries"""
    if theta.dim() != 3 or tuple(theta.shape[1:]) not in ((3, 4), (2, 3)):
        raise ValueError(f"{name}: theta (B,3,4) or, for slices, (B,2,3) expected, got {tuple(theta.shape)}")
    if theta.shape[1] == 3:
        return theta, False
    lifted = torch.nn.functional.pad(theta, (1, 0, 1, 0))
    corner = torch.zeros(3, 4, device=theta.device, dtype=theta.dtype)
    corner[0, 0] = 1.0
    return lifted + corner, True


def _size3(size, two_d: bool, name: str):
    size = tuple(int(s) for s in size)
    if len(size) != (2 if two_d else 3) or min(size) < 1:
        raise ValueError(f"{name}: a size of {2 if two_d else 3} extents >= 1 expected for this theta, got {size}")
    return ((1,) + size) if two_d else size


@torch.no_grad()
def affine_field(theta, size):
    """the displacement field an affine stands for: theta (B,3,4) = [M | t] in voxel units of the grid `size` = (D,H,W), about the grid's
    centre c = (size - 1) / 2, sends voxel v to p = c + M (v - c) + t; the result (B,3,D,H,W) is d = p - v under SpatialTransformer's
    convention (warp3d(d, img) samples img where v + d(v) points).  (B,2,3) with size (H,W) gives (B,2,H,W).  The bridge to every operator
    that takes a field (warp_labels, warp_mask, warp_landmarks, field_quality, ...).  No autograd: affine_warp carries theta's gradient."""
    theta, two_d = _theta3(theta.detach(), "affine_field")
    D, H, W = _size3(size, two_d, "affine_field")
    _require_gpu(theta)
    theta = theta.contiguous()
    B = theta.shape[0]
    out = torch.empty((B, 3, D, H, W), device=theta.device, dtype=torch.float32)
    t0 = _hbm_begin("affine_field")
    lib.call("pulpo_affine_field", _ptr(theta), _ptr(out), B, D, H, W, _stream())
    _hbm_end(t0, "affine_field", 4.0 * out.numel())
    return _unlift_field(out) if two_d else out


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, img, size):
        _require_gpu(theta, img)
        theta, img = theta.contiguous(), planar(img)
        B, C, Di, Hi, Wi = img.shape
        Dg, Hg, Wg = size
        out = torch.empty((B, C, Dg, Hg, Wg), device=img.device, dtype=torch.float32)
        t0 = _hbm_begin("affine_warp_fwd")
        lib.call("pulpo_affine_warp_fwd", _ptr(theta), _ptr(img), _ptr(out), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "affine_warp_fwd", 4.0 * (img.numel() + out.numel()))                   # the image read once, the result written: no field
        ctx.save_for_backward(theta, img)
        ctx.size = size
        return out

    @staticmethod
    def backward(ctx, g):
        theta, img = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = planar(g)
        B, C, Di, Hi, Wi = img.shape
        Dg, Hg, Wg = ctx.size
        ws = torch.empty(lib.query("pulpo_affine_warp_bwd_ws_bytes", B, Dg, Hg, Wg), device=img.device, dtype=torch.uint8)
        gtheta = torch.empty((B, 3, 4), device=img.device, dtype=torch.float32)
        t0 = _hbm_begin("affine_warp_bwd")
        lib.call("pulpo_affine_warp_bwd", _ptr(theta), _ptr(img), _ptr(g), _ptr(gtheta), _ptr(ws), B, C, Dg, Hg, Wg, Di, Hi, Wi, _stream())
        _hbm_end(t0, "affine_warp_bwd", 4.0 * (img.numel() + g.numel()))                     # the image and the upstream gradient read once
        return gtheta, None, None


def affine_warp(theta, img, size=None):
    """warp3d(affine_field(theta, size), img) in one kernel that never writes the field: bit-identical to that route, a quarter of its
    bytes.  theta (B,3,4) on the output grid `size` (default: img's own), img (B,C,Di,Hi,Wi); slices: theta (B,2,3), img (B,C,H,W).
    Differentiable with respect to theta only (deterministic: ordered double sums, no float atomics); the image is data - an img that
    requires grad raises ValueError."""
    if img.requires_grad:
        raise ValueError("affine_warp: the image is data here (no gradient with respect to img); detach it, or use warp3d(affine_field(theta, size), img)")
    theta3, two_d = _theta3(theta, "affine_warp")
    if two_d != _is2d(img) or img.dim() not in (4, 5) or img.shape[0] != theta.shape[0]:
        raise ValueError(f"affine_warp: theta {tuple(theta.shape)} and img {tuple(img.shape)} do not go together")
    img5 = _lift(img) if two_d else img
    size3 = _size3(img.shape[2:] if size is None else size, two_d, "affine_warp")
    out = _AffineWarp.apply(theta3, img5, size3)
    return out.squeeze(2) if two_d else out


@torch.no_grad()
def affine_compose(theta, df, image_size=None):
    """"affine first, deformable second" as one field on df's grid: warp3d(affine_compose(theta, df), img) equals
    warp3d(df, affine_warp(theta, img)) up to the second interpolation of that two-step route, so a segmentation, a mask or landmarks of
    the original moving image are carried through both transforms with one interpolation.  theta (B,3,4) in the frame of the image grid
    `image_size` (default: df's own grid), df (B,3,Dg,Hg,Wg); slices: theta (B,2,3), df (B,2,H,W).  No autograd."""
    theta, two_d = _theta3(theta.detach(), "affine_compose")
    if two_d != _is2d(df) or df.dim() not in (4, 5) or df.shape[0] != theta.shape[0] or df.shape[1] != df.dim() - 2:
        raise ValueError(f"affine_compose: theta {tuple(theta.shape)} and df {tuple(df.shape)} do not go together")
    Di, Hi, Wi = _size3(df.shape[2:] if image_size is None else image_size, two_d, "affine_compose")
    df5 = planar(_lift_field(df.detach()) if two_d else df.detach())
    _require_gpu(theta, df5)
    theta = theta.contiguous()
    B, _, Dg, Hg, Wg = df5.shape
    out = torch.empty_like(df5)
    t0 = _hbm_begin("affine_compose")
    lib.call("pulpo_affine_compose", _ptr(theta), _ptr(df5), _ptr(out), B, Dg, Hg, Wg, Di, Hi, Wi, _stream())
    _hbm_end(t0, "affine_compose", 8.0 * out.numel())
    return _unlift_field(out) if two_d else out


# ------------------------------------------------------------------------------------------------ training augmentation
# Augmentation is data: no autograd, and a source that requires grad is refused.  Every refusal below is a ValueError raised before anything is
# launched (and before a GPU is needed).
_INTENSITY_KEYS = ("gamma", "gain", "offset", "sigma", "bias", "seed", "clip")
_AUG_BIAS_MAX_NODES = 4096


def bspline_lattice_size(size, spacing: int):
    """extents of the control lattice of a grid: ceil((S - 1) / s) + 3 per axis"""
    return tuple(-(-(int(S) - 1) // int(spacing)) + 3 for S in size)


def _aug_lattice(phi, spacing, two_d: bool, size3, B: int, name: str):
    """phi as (B,3,Gz,Gy,Gx) (slices: (B,2,Gy,Gx) lifted with a zero depth component and Gz = 1), checked against the grid"""
    if spacing is None or int(spacing) != spacing or int(spacing) < 2:
        raise ValueError(f"{name}: an integer lattice spacing >= 2 voxels expected with phi, got {spacing!r}")
    nd = 2 if two_d else 3
    if phi.dim() != nd + 2 or phi.shape[1] != nd:
        raise ValueError(f"{name}: phi (B,{nd}," + ",".join("G" * nd) + f") expected for {nd}-D arguments, got {tuple(phi.shape)}")
    if phi.shape[0] != B:
        raise ValueError(f"{name}: phi has batch size {phi.shape[0]}, the other arguments {B}")
    want = bspline_lattice_size(size3[3 - nd:], spacing)
    if tuple(phi.shape[2:]) != want:
        raise ValueError(f"{name}: a lattice of ceil((S - 1) / s) + 3 = {want} nodes expected for the grid {tuple(size3[3 - nd:])} at spacing {spacing}, "
                         f"got {tuple(phi.shape[2:])}")
    phi = phi.detach()
    return _lift_field(phi) if two_d else phi


def _per_sample_column(v, B: int, default: float, dev, name: str):
    if v is None:
        v = default
    if torch.is_tensor(v):
        if v.numel() != B:
            raise ValueError(f"augment: intensity[{name!r}] holds {v.numel()} values for a batch of {B}")
        return v.detach().reshape(B).to(device=dev, dtype=torch.float32)
    return float(v)


@torch.no_grad()
def augment(img=None, mask=None, labels=None, *, theta=None, phi=None, spacing=None, intensity=None, fill: float = 0.0, fill_label: int = 0):
    """One random spatial map per sample, evaluated once per output voxel and applied to every source given, in ONE launch that writes neither a
    sampling grid nor a field.  Output voxel v samples the sources at p = c + M (q - c) + t, q = v + e(v): theta (B,3,4) = [M | t] in voxel
    units about the grid's centre c (None: the identity), e the cubic B-spline free-form deformation of the control lattice phi
    (B,3,Gz,Gy,Gx) of integer `spacing` s >= 2 voxels with G = ceil((S - 1) / s) + 3 nodes per axis (None: e = 0).
    img (B,C,D,H,W) fp32 and mask (B,Cm,D,H,W) fp32: trilinear in voxel units, corners outside the volume contribute `fill`
    (grid_sample(align_corners=True, padding_mode="zeros")); labels (B,1,D,H,W) uint8 / int32: the nearest voxel floor(p + 0.5), fill_label
    outside.  The identity returns every source bit for bit.  Slices: (B,C,H,W) sources with theta (B,2,3) and phi (B,2,Gy,Gx).
    intensity (the image only, after sampling, every piece optional): a dict of per-sample tensors (B,) or floats - r = clamp(r,0,1)^gamma;
    r *= exp(beta), beta the trilinear interpolation of the log-bias lattice `bias` (B,Lz,Ly,Lx) spanning the volume; r = gain r + offset;
    r += sigma n, n a standard normal that is a pure function of `seed` (an int, or one int64 on the device) and the element's index
    (Philox4x32-10); clip: clamp(r,0,1).  Returns a tuple, in the order of the sources given.  Deterministic, no autograd."""
    given = [(n, t) for n, t in (("img", img), ("mask", mask), ("labels", labels)) if t is not None]
    if not given:
        raise ValueError("augment: give at least one of img, mask, labels")
    first = given[0][1]
    if first.dim() not in (4, 5):
        raise ValueError(f"augment: (B,C,D,H,W) or (B,C,H,W) sources expected, got {tuple(first.shape)}")
    two_d = first.dim() == 4
    B, grid = first.shape[0], tuple(first.shape[2:])
    for n, t in given:
        if t.dim() != first.dim():
            raise ValueError("augment: 2-D and 3-D arguments do not mix")
        if t.shape[0] != B or tuple(t.shape[2:]) != grid:
            raise ValueError(f"augment: {n} {tuple(t.shape)} does not share the batch size and grid of {given[0][0]} {tuple(first.shape)}")
        if t.requires_grad:
            raise ValueError(f"augment: {n} requires grad; augmentation is data (detach it)")
    for n, t in (("img", img), ("mask", mask)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"augment: {n} is fp32 (got {t.dtype})")
    if labels is not None:
        if labels.is_floating_point() or labels.dtype not in _LABEL_DT:
            raise ValueError(f"augment: label maps are uint8 or int32 (got {labels.dtype}); a float map goes in as mask")
        if labels.shape[1] != 1:
            raise ValueError(f"augment: a label map (B,1,...) expected, got {tuple(labels.shape)}")
    size3 = ((1,) + grid) if two_d else grid
    theta3 = None
    if theta is not None:
        if theta.dim() != 3 or tuple(theta.shape[1:]) != ((2, 3) if two_d else (3, 4)):
            raise ValueError(f"augment: theta (B,2,3) for slices, (B,3,4) for volumes expected, got {tuple(theta.shape)} for {first.dim() - 2}-D sources")
        if theta.shape[0] != B:
            raise ValueError(f"augment: theta has batch size {theta.shape[0]}, the sources {B}")
        theta3 = _theta3(theta.detach(), "augment")[0]
    phi5 = _aug_lattice(phi, spacing, two_d, size3, B, "augment") if phi is not None else None
    cfg = dict(intensity or {})
    unknown = [k for k in cfg if k not in _INTENSITY_KEYS]
    if unknown:
        raise ValueError(f"augment: unknown intensity keys {unknown} (known: {_INTENSITY_KEYS})")
    active = any(cfg.get(k) is not None for k in ("gamma", "gain", "offset", "sigma", "bias")) or bool(cfg.get("clip"))
    if active and img is None:
        raise ValueError("augment: the intensity transform applies to img, which is missing")
    bias = cfg.get("bias")
    if bias is not None:
        if bias.dim() != first.dim() - 1 or bias.shape[0] != B:
            raise ValueError(f"augment: a log-bias lattice (B,{'Ly,Lx' if two_d else 'Lz,Ly,Lx'}) expected, got {tuple(bias.shape)}")
        if bias[0].numel() > _AUG_BIAS_MAX_NODES or bias[0].numel() < 1:
            raise ValueError(f"augment: a log-bias lattice of 1 to {_AUG_BIAS_MAX_NODES} nodes expected, got {bias[0].numel()}")
    if cfg.get("sigma") is not None and cfg.get("seed") is None:
        raise ValueError("augment: intensity['sigma'] needs intensity['seed']")
    dev = first.device
    cols = [_per_sample_column(cfg.get(k), B, d, dev, k) for k, d in (("gamma", 1.0), ("gain", 1.0), ("offset", 0.0), ("sigma", 0.0))]

    _require_gpu(img, mask, theta3, phi5, bias)
    _require_labels(labels)
    iflags = (1 if cfg.get("gamma") is not None else 0) | (2 if cfg.get("gain") is not None or cfg.get("offset") is not None else 0) \
        | (4 if cfg.get("sigma") is not None else 0) | (8 if cfg.get("clip") else 0)
    iparams = seed = None
    if iflags & 7:
        if any(torch.is_tensor(c) for c in cols):
            iparams = torch.stack([c if torch.is_tensor(c) else torch.full((B,), c, device=dev, dtype=torch.float32) for c in cols], dim=1).contiguous()
        else:
            iparams = torch.tensor([cols] * B, dtype=torch.float32).to(dev)
    if iflags & 4:
        seed = cfg["seed"]
        if not torch.is_tensor(seed):
            s = int(seed) & ((1 << 64) - 1)
            seed = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64).to(dev)
        elif seed.dtype != torch.int64 or seed.numel() != 1 or not seed.is_cuda:
            raise PulpoHipError("augment: intensity['seed'] is an int or one int64 on the device")
    lift = (lambda t: None if t is None else t.unsqueeze(2)) if two_d else (lambda t: t)
    img5 = None if img is None else planar(lift(img))
    mask5 = None if mask is None else planar(lift(mask))
    lab5 = None if labels is None else lift(labels).contiguous()
    bias4 = None if bias is None else (bias.detach().unsqueeze(1) if two_d else bias.detach()).contiguous()
    theta3 = None if theta3 is None else theta3.contiguous()
    phi5 = None if phi5 is None else planar(phi5)
    D, H, W = size3
    outs = [None if t is None else torch.empty_like(t) for t in (img5, mask5, lab5)]
    Gz, Gy, Gx = phi5.shape[2:] if phi5 is not None else (0, 0, 0)
    Lz, Ly, Lx = bias4.shape[1:] if bias4 is not None else (0, 0, 0)
    nbytes = 2.0 * sum(t.numel() * t.element_size() for t in (img5, mask5, lab5) if t is not None)      # the sources read once, the results written
    t0 = _hbm_begin("augment_apply")
    lib.call("pulpo_augment_apply", _ptr(theta3), _ptr(phi5), int(spacing) if phi5 is not None else 0, int(Gz), int(Gy), int(Gx),
             _ptr(img5), _ptr(outs[0]), img5.shape[1] if img5 is not None else 0, _ptr(mask5), _ptr(outs[1]), mask5.shape[1] if mask5 is not None else 0,
             _ptr(lab5), _ptr(outs[2]), _LABEL_DT[lab5.dtype] if lab5 is not None else 0, _ptr(iparams), iflags, _ptr(bias4), int(Lz), int(Ly), int(Lx),
             _ptr(seed), float(fill), int(fill_label), B, D, H, W, _stream())
    _hbm_end(t0, "augment_apply", nbytes)
    return tuple(o.squeeze(2) if two_d else o for o in outs if o is not None)


@torch.no_grad()
def bspline_field(phi, size, spacing: int, theta=None):
    """the displacement the augmentation's spatial map stands for, as a dense tensor: e (B,3,D,H,W), the cubic B-spline free-form deformation of
    the control lattice phi (B,3,Gz,Gy,Gx) on the grid `size` at integer spacing s >= 2 (ops.augment's definition), or p - v when an affine
    theta (B,3,4) is given - from the fused kernel's own coordinate code, bit for bit.  Slices: phi (B,2,Gy,Gx), size (H,W), theta (B,2,3) ->
    (B,2,H,W).  No autograd."""
    if phi.dim() not in (4, 5):
        raise ValueError(f"bspline_field: phi (B,3,Gz,Gy,Gx) or (B,2,Gy,Gx) expected, got {tuple(phi.shape)}")
    two_d = phi.dim() == 4
    size3 = _size3(size, two_d, "bspline_field")
    B = phi.shape[0]
    theta3 = None
    if theta is not None:
        if theta.dim() != 3 or tuple(theta.shape[1:]) != ((2, 3) if two_d else (3, 4)) or theta.shape[0] != B:
            raise ValueError(f"bspline_field: theta {tuple(theta.shape)} and phi {tuple(phi.shape)} do not go together")
        theta3 = _theta3(theta.detach(), "bspline_field")[0]
    phi5 = _aug_lattice(phi, spacing, two_d, size3, B, "bspline_field")
    _require_gpu(phi5, theta3)
    phi5 = planar(phi5)
    theta3 = None if theta3 is None else theta3.contiguous()
    D, H, W = size3
    out = torch.empty((B, 3, D, H, W), device=phi5.device, dtype=torch.float32)
    t0 = _hbm_begin("bspline_field")
    lib.call("pulpo_bspline_field", _ptr(phi5), _ptr(theta3), _ptr(out), int(spacing), *(int(g) for g in phi5.shape[2:]), B, D, H, W, _stream())
    _hbm_end(t0, "bspline_field", 4.0 * out.numel())
    return _unlift_field(out) if two_d else out


@torch.no_grad()
def philox4x32(counters, key):
    """raw Philox4x32-10 words: counters (N,4) and key (2,) as int32 bit patterns (or int64 values below 2^32) on the device -> (N,4) int32
    bit patterns.  The generator behind ops.augment's noise, exposed so that it can be held to the published vectors."""
    if counters.dim() != 2 or counters.shape[1] != 4 or counters.shape[0] < 1:
        raise ValueError(f"philox4x32: counters (N,4) expected, got {tuple(counters.shape)}")
    key = torch.as_tensor(key, device=counters.device)
    if key.numel() != 2:
        raise ValueError(f"philox4x32: a key of two words expected, got {tuple(key.shape)}")
    if not counters.is_cuda:
        raise PulpoHipError("pulpo_amd operators run on the GPU only (got a CPU tensor); there is no CPU fallback")
    c32, k32 = counters.to(torch.int32).contiguous(), key.reshape(2).to(torch.int32).contiguous()
    out = torch.empty_like(c32)
    lib.call("pulpo_philox4x32", _ptr(c32), _ptr(k32), _ptr(out), c32.shape[0], _stream())
    return out
