"""Launch log of the ConvUnit training step: every `lib.call` of a scenario as one text line, compared with tests/golden/convunit_launches.txt
(tests/test_gpu_launch_log.py; scripts/record_launch_log.py writes the fixture).  The log pins WHAT the Python side hands the kernels - entry point,
null-ness of every pointer, every integer and float, the stream - so a restructuring of pulpo_amd/ops.py that changes a launch shows up as a
one-line diff; it says nothing about what the kernels compute."""
import ctypes
import gc
import os
import re

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convunit_launches.txt")


class LaunchLog:
    """context manager: swaps `lib.call` on the shared _Lib instance for a recorder (the call still runs) and restores it; `lib.query` is not
    recorded.  `lines`: entry point, then each argument - pointers as p / 0, ints in decimal, floats by repr - then the stream current at the
    call as s0, s1, ... in order of first appearance."""

    def __init__(self):
        self.lines, self._streams = [], {}

    def _render(self, a) -> str:
        if a is None:
            return "0"
        if isinstance(a, (ctypes.c_void_p, ctypes.c_char_p)):
            return "p" if a.value else "0"
        if isinstance(a, (ctypes.Array, ctypes._Pointer, bytes)):
            return "p"
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, int):
            return str(a)
        if isinstance(a, float):
            return repr(a)
        raise TypeError(f"launch log: argument of type {type(a).__name__}")

    def __enter__(self):
        from pulpo_amd._lib import lib
        self._lib, call = lib, lib.call

        def record(name, *args):
            s = self._streams.setdefault(torch.cuda.current_stream().cuda_stream, len(self._streams))
            self.lines.append(" ".join([name] + [self._render(a) for a in args] + [f"s{s}"]))
            return call(name, *args)

        lib.call = record                          # (an instance attribute in front of the method)
        return self

    def __exit__(self, *exc):
        del self._lib.call
        return False


def _step_case(size: int = 32, n0: int = 32):
    """model factory and batch of tests/test_gpu_wgrad_budget.py::_make_step_case (T3 / L2, B = 1, seeds 9 and 0, FixedNoiseSampler)"""
    import src.models as models
    import src.network_blocks as nb
    from oracle import pulpo_oracle as O
    gen = torch.Generator().manual_seed(9)
    S = size
    x, y = torch.rand(1, 1, S, S, S, generator=gen).cuda(), torch.rand(1, 1, S, S, S, generator=gen).cuda()
    eps = [torch.randn(1, 3, S // 2, S // 2, S // 2, generator=gen).cuda(), torch.randn(1, 3, S // 4, S // 4, S // 4, generator=gen).cuda()]
    empty = torch.empty((0,))

    def make():
        torch.manual_seed(0)
        m = models.PULPo(3, 2, 0.1, [S, S, S], feedback=list(O.FEEDBACK_DEFAULT), n0=n0).cuda().train()
        for l in range(2):
            m.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        return m

    return make, (x, y, empty, empty, empty, empty, empty, empty)


_DY = dict(BLOCKED_DY_MIN_VOXELS=32 ** 3)
# scenario -> (module attributes of pulpo_amd.ops set for its duration, entry points its log exists to cover: regular expressions, each must match
# the whole name of some launch)
SCENARIOS = {
    "a": (_DY, [r"pulpo_conv3d_k3_wgrad_bn", r"pulpo_conv3d_k3_dgrad_\w+_bnred(_kb)?", r"pulpo_avgpool2_bwd_bnred_t", r"pulpo_heads_bwd_bn_t",
                r"pulpo_conv3d_k3_wgrad_kb"]),
    "b": (dict(_DY, BLOCKED_Z=True, BLOCKED_Z_MIN_VOXELS=32 ** 3), [r"pulpo_bn_lrelu_apply_kb"]),
    "c": (dict(_DY, BN_REDUCE_IN_DGRAD=False, POOLED_BN_BACKWARD=False, FUSE_INPUT_WGRAD=False, FUSE_HEAD_BN=False, BLOCKED_DY=False), []),
    "d": (_DY, [r"pulpo_conv3d_k3_wgrad\w*_det\w*"]),
    "e": (_DY, [r"pulpo_\w+_bf16_t"]),
    "f": (_DY, [r"pulpo_grad_finish_multi"]),
    "g": (_DY, []),
}
# what scenario c (every fused pass off) must NOT launch: scenario a's list and b's
FUSED_ENTRIES = SCENARIOS["a"][1] + SCENARIOS["b"][1]


def missing_entries(name: str, lines):
    """what the scenario exists to cover and its log does not show (empty = the log still tests what it was recorded for)"""
    names = [line.split(" ", 1)[0] for line in lines]
    out = [pat for pat in SCENARIOS[name][1] if not any(re.fullmatch(pat, n) for n in names)]
    if name == "c":
        out += [f"not {pat}" for pat in FUSED_ENTRIES if any(re.fullmatch(pat, n) for n in names)]
    if name == "f" and not any(line.endswith(" s1") for line in lines):
        out.append("a launch on s1")
    if name == "g" and not any(line.startswith("pulpo_conv3d_k3_fwd_bn_lrelu") or (line.split()[0] in ("pulpo_conv3d_k3_fwd_wino2", "pulpo_conv3d_k3_fwd_wino3")
                                                                                     and line.split()[7] == "p") for line in lines):
        out.append("a convolution that applies BatchNorm + LeakyReLU in its store (non-null coef)")
    return out


def run_scenario(name: str, size: int = 32, n0: int = 32, digest: bool = False):
    """the launch log of one scenario (a list of lines); digest=True: (lines, SHA-256 over the bytes of all parameter gradients in
    named_parameters() order)"""
    from pulpo_amd import dp, ops
    attrs = SCENARIOS[name][0]
    saved = {k: getattr(ops, k) for k in attrs}
    det, prec = ops.DETERMINISTIC, (ops.CONV_PRECISION, "bf16" if ops.ACT_BF16 else "fp32")
    make, batch = _step_case(size, n0)
    gc.collect()
    ops.invalidate_weight_packs()              # (the stepper rewrites every live weight pack of the process in one launch: none of an earlier test's)
    ops.reset_param_grad_buffers()
    model = make()
    try:
        for k, v in attrs.items():
            setattr(ops, k, v)
        if name == "d":
            ops.set_deterministic(True)
        if name == "e":
            ops.set_conv_precision("bf16", "bf16")
        with LaunchLog() as log:
            if name == "f":
                stepper = dp.DataParallelStepper(model, lr=0.0, coarse_window=True, coarse_voxels=8 ** 3, max_workgroups=64, defer_flop=1e30,
                                                 exit_wait=True)
                for _ in range(2):                 # (the second step holds weight gradients back: the first learns which)
                    stepper.step(batch)
            elif name == "g":
                # (frozen parameters, as a deployed model's: autograd reports needs_input_grad from requires_grad even under no_grad, and the
                #  ConvUnit node keeps the pre-norm tensor - two kernels - for any input that may ask for a gradient)
                model.eval().requires_grad_(False)
                with torch.no_grad():
                    model(batch[0], batch[1])
            else:
                model.training_step(batch, 0).backward()
            torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.set_deterministic(det)
        ops.set_conv_precision(*prec)
    if not digest:
        return log.lines
    import hashlib
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        if p.grad is not None:
            h.update(p.grad.detach().cpu().contiguous().numpy().tobytes())
    return log.lines, h.hexdigest()


def read_golden(path: str = GOLDEN):
    """{scenario: (size, n0, lines)} of the fixture: `# <scenario> <size> <n0>` heads a section, `##` lines are the file's header"""
    out, cur = {}, None
    with open(path) as f:
        for line in f.read().splitlines():
            if line.startswith("##") or not line:
                continue
            if line.startswith("# "):
                _, name, size, n0 = line.split()
                cur = []
                out[name] = (int(size), int(n0), cur)
            else:
                cur.append(line)
    return out
