"""ops.ncc_loss_masked against ops.ncc_loss, forward + backward, on the GPU.

    python scripts/masked_bench.py [--reps 30] [--out profiles/masked_bench.txt]

At 160^3 with window 9 and 80^3 with window 7 (the two finest levels of the 160^3 pyramid), B = 1, with one mask and with two: same
process, after a warm-up, the three routes alternating; median ms over --reps with the 10 % / 90 % quantiles (device events around a
forward + backward pair).  Bytes counted per pair (N voxels, fp32; the estimates of ops._NCC):
  unmasked   4 (22 + 20) N
  masked     that + 8 N per mask plane (one read in the forward D pass, one in the backward abc kernel)
so the byte ratio is 1.048 with one mask and 1.095 with two.  The masked pair also launches pulpo_masked_finish in place of
pulpo_colsum and one device-scalar product in the backward pass.  The unmasked and the all-ones masked results are compared before
anything is timed.
"""
from __future__ import annotations

import argparse
import os
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
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("masked_bench: at least 20 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("masked_bench: needs a ROCm GPU (no CPU path)")
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    gamma = 0.05
    lines = [f"ops.ncc_loss_masked against ops.ncc_loss, forward + backward, B = 1, reps = {args.reps}, {torch.cuda.get_device_name(0)}",
             f"{'size':>6} {'win':>3} | {'unmasked ms':>11} [{'p10':>7} {'p90':>7}] {'GB/s':>6} | {'1 mask ms':>10} [{'p10':>7} {'p90':>7}] {'ratio':>6} {'bytes':>6} | "
             f"{'2 masks ms':>10} [{'p10':>7} {'p90':>7}] {'ratio':>6} {'bytes':>6}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for S, win in ((160, 9), (80, 7)):
        shape = (1, 1, S, S, S)
        pred = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
        true = torch.rand(shape, device=dev, generator=g)
        wa, wb = torch.rand(shape, device=dev, generator=g), torch.rand(shape, device=dev, generator=g)
        N = pred.numel()

        def pair(loss_fn):
            def run():
                pred.grad = None
                loss_fn().backward()
            return run

        plain = pair(lambda: ops.ncc_loss(pred, true, win, gamma))
        one = pair(lambda: ops.ncc_loss_masked(pred, true, wa, None, win, gamma))
        two = pair(lambda: ops.ncc_loss_masked(pred, true, wa, wb, win, gamma))
        # faster and different is not faster: a mask of ones is the unmasked loss
        plain()
        g0 = pred.grad.clone()
        pair(lambda: ops.ncc_loss_masked(pred, true, torch.ones_like(wa), None, win, gamma))()
        err = float((pred.grad - g0).abs().max() / g0.abs().max())
        assert err <= 1e-6, err
        (t0, a0, b0), (t1, a1, b1), (t2, a2, b2) = timed([plain, one, two], args.reps)
        bytes0 = 4.0 * (22 + 20) * N
        r1, r2 = (bytes0 + 8.0 * N) / bytes0, (bytes0 + 16.0 * N) / bytes0
        lines.append(f"{S:>4}^3 {win:>3} | {t0:11.3f} [{a0:7.3f} {b0:7.3f}] {bytes0 / t0 / 1e6:6.0f} | {t1:10.3f} [{a1:7.3f} {b1:7.3f}] {t1 / t0:6.3f} {r1:6.3f} | "
                     f"{t2:10.3f} [{a2:7.3f} {b2:7.3f}] {t2 / t0:6.3f} {r2:6.3f}")
        del pred, true, wa, wb, g0
        torch.cuda.empty_cache()
    lines.append("ratio: masked median / unmasked median of the same run; bytes: the ratio of the counted bytes (accepted: bytes + 0.05)")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
