"""Bidirectional training measured on the GPU.

    python scripts/bidir_bench.py [--reps 40] [--steps 8] [--no-step] [--out profiles/bidir_bench.txt]

1. The paired autograd node against the route it replaces, at the pyramid shapes 80^3, 40^3, 20^3 and 10^3, B = 1, nsteps = 7: forward and
   backward of  (fwd * a + inv * b).sum()  through ops.vecint_pair(v) and through (ops.vecint(v), ops.vecint(-v)), same process, after a
   warm-up, the routes alternating, device events around each call: median ms over --reps with the 10 % / 90 % quantiles.  The two-call route
   is timed TWICE in the same alternation (columns "2 calls" and "again"): the ratio of its two medians is the run-to-run spread that a
   difference between the routes has to exceed to mean anything.  The gradients of the two routes are compared on the same inputs.
2. The 160^3 T5 / L4 training step (bench.py's model and data, eager dp.DataParallelStepper) with bidirectional off and on, alternating
   blocks of --steps steps, median ms per step.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fns, reps: int):
    """[(median, p10, p90)] in ms per function: warm-up, then alternating calls, device events around each"""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    out = []
    for t in ts:
        t = sorted(t)
        out.append((statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]))
    return out


def node_bench(ops, reps: int, lines) -> None:
    nsteps = 7
    g = torch.Generator(device="cuda").manual_seed(0)
    lines.append(f"{'size':>6} | {'pair ms':>8} [{'p10':>7} {'p90':>7}] | {'2 calls ms':>10} [{'p10':>7} {'p90':>7}] | {'again ms':>8} | {'2 calls / pair':>14} | "
                 f"{'spread':>6} | grad rel_l2")
    for S in (80, 40, 20, 10):
        v = (1.5 * torch.randn((1, 3, S, S, S), device="cuda", generator=g)).requires_grad_(True)
        a, b = (torch.randn((1, 3, S, S, S), device="cuda", generator=g) for _ in range(2))

        def pair():
            fwd, inv = ops.vecint_pair(v, nsteps)
            return torch.autograd.grad((fwd * a + inv * b).sum(), [v])[0]

        def two():
            return torch.autograd.grad((ops.vecint(v, nsteps) * a + ops.vecint(-v, nsteps) * b).sum(), [v])[0]

        gp, gt = pair(), two()
        err = float((gp - gt).norm() / gt.norm())
        assert err < 1e-5, err                                   # faster and different is not faster
        (tp, p10, p90), (tt, t10, t90), (ta, _, _) = timed([pair, two, two], reps)
        spread = max(tt, ta) / min(tt, ta) - 1.0
        lines.append(f"{S:>3}^3  | {tp:8.3f} [{p10:7.3f} {p90:7.3f}] | {tt:10.3f} [{t10:7.3f} {t90:7.3f}] | {ta:8.3f} | {min(tt, ta) / tp:13.2f}x | "
                     f"{100 * spread:5.1f}% | {err:.1e}")


def step_bench(steps: int, lines) -> None:
    from pulpo_amd import dp, synthetic
    from pulpo_amd.models import PULPo
    size, T, L = [160, 160, 160], 5, 4
    feedback = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
    x, y = synthetic.oasis_like_pair(size, 1, 1234, "cuda")
    e = torch.empty((0,), device="cuda")
    batch = (x, y, e, e, e, e, e, e)
    steppers = {}
    for flag in (False, True):
        torch.manual_seed(0)
        model = PULPo(T, L, 0.1, size, feedback=feedback, n0=32, bidirectional=flag).to("cuda").train()
        steppers[flag] = dp.DataParallelStepper(model)
        for _ in range(3):                                       # warm-up: code objects, weight packs, arena
            steppers[flag].step(batch)
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(3):                                           # alternating blocks
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                steppers[flag].step(batch)
            torch.cuda.synchronize()
            ts[flag].append((time.perf_counter() - t0) * 1e3 / steps)
    off, on = statistics.median(ts[False]), statistics.median(ts[True])
    lines.append("")
    lines.append(f"160^3 T5/L4 step (eager stepper, oasis-like pair, B = 1), 3 alternating blocks of {steps} steps, ms per step:")
    lines.append(f"  bidirectional off {off:8.2f}  (blocks {', '.join(f'{t:.2f}' for t in ts[False])})")
    lines.append(f"  bidirectional on  {on:8.2f}  (blocks {', '.join(f'{t:.2f}' for t in ts[True])})   on / off {on / off:.3f}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="skip the 160^3 step")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bidir_bench: needs a ROCm GPU (no CPU path)")
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    lines = [f"ops.vecint_pair (one paired node) against vecint(v) + vecint(-v): forward + backward, B = 1, nsteps = 7, reps = {args.reps}, "
             f"{torch.cuda.get_device_name(0)}"]
    node_bench(ops, args.reps, lines)
    if not args.no_step:
        step_bench(args.steps, lines)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
