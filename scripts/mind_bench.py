"""ops.mind_loss beside ops.ncc_loss, forward + backward, on the GPU.

    python scripts/mind_bench.py [--reps 30] [--step-limit 120] [--out profiles/mind_bench.txt]

At 160^3, 80^3, 40^3 and 20^3 (the levels of the 160^3 pyramid; NCC windows 9, 7, 5, 3), B = 1, dilation 2: one process, after a
warm-up, the routes alternating; median ms over --reps with the 10 % / 90 % quantiles (device events around a forward + backward pair,
and around the MIND forward alone, which splits the pair).  Bytes counted per pair (N voxels, fp32; the estimates of ops._Mind and
ops._NCC):
  mind   4 (2 + 28) N    forward 2 images in; backward 2 images in, G 12 N out and 12 N in, the image once more, the gradient out
  ncc    4 (22 + 20) N
Every size runs under its own time limit (SIGALRM with the default action ends the process, also inside a blocked device call), and the
first failure ends the script: nothing is started on the GPU after it.  The two backward runs of MIND are compared bit for bit before
anything is timed.
"""
from __future__ import annotations

import argparse
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(routes, reps: int):
    """[(median, p10, p90)] in ms per route: warm-up, then alternating calls, GPU events around each"""
    for _ in range(3):
        for f in routes:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in routes]
    for _ in range(reps):
        for i, f in enumerate(routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))

    def stats(t):
        t = sorted(t)
        return statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]

    return [stats(t) for t in ts]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dilation", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds allowed per size")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("mind_bench: at least 20 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("mind_bench: needs a ROCm GPU (no CPU path)")
    signal.alarm(args.step_limit)                       # library load and the first kernel launches count as a step
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    d = args.dilation
    lines = [f"ops.mind_loss (dilation {d}) beside ops.ncc_loss, forward + backward, B = 1, reps = {args.reps}, {torch.cuda.get_device_name(0)}",
             f"{'size':>6} | {'mind ms':>8} [{'p10':>7} {'p90':>7}] {'GB/s':>6} {'fwd ms':>7} {'bwd ms':>7} | {'win':>3} {'ncc ms':>8} [{'p10':>7} {'p90':>7}] {'GB/s':>6} | "
             f"{'mind/ncc':>8}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for S, win in ((160, 9), (80, 7), (40, 5), (20, 3)):
        signal.alarm(args.step_limit)
        shape = (1, 1, S, S, S)
        pred = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
        true = torch.rand(shape, device=dev, generator=g)
        N = pred.numel()

        def pair(loss_fn):
            def run():
                pred.grad = None
                loss_fn().backward()
            return run

        mind = pair(lambda: ops.mind_loss(pred, true, d))
        ncc = pair(lambda: ops.ncc_loss(pred, true, win, 0.05))

        def mind_fwd():
            with torch.no_grad():
                ops.mind_loss(pred, true, d)

        mind()
        g0 = pred.grad.clone()
        mind()
        assert torch.equal(pred.grad, g0) and bool(torch.isfinite(g0).all()), "two MIND backward runs differ"
        (t0, a0, b0), (t1, a1, b1), (tf, _, _) = timed([mind, ncc, mind_fwd], args.reps)
        by_mind, by_ncc = 4.0 * (2 + 28) * N, 4.0 * (22 + 20) * N
        lines.append(f"{S:>4}^3 | {t0:8.3f} [{a0:7.3f} {b0:7.3f}] {by_mind / t0 / 1e6:6.0f} {tf:7.3f} {t0 - tf:7.3f} | {win:>3} {t1:8.3f} [{a1:7.3f} {b1:7.3f}] "
                     f"{by_ncc / t1 / 1e6:6.0f} | {t0 / t1:8.2f}")
        del pred, true, g0
        torch.cuda.empty_cache()
    signal.alarm(0)
    lines.append("fwd ms: the MIND forward alone (no_grad); bwd ms: pair - fwd.  GB/s: counted bytes / median.  mind/ncc: ratio of the pair medians")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
