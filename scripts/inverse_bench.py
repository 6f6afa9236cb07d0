"""ops.vecint_pair(v) against the two ops.vecint calls it replaces (vecint(v), vecint(-v)) under no_grad, on the GPU.

    python scripts/inverse_bench.py [--reps 30] [--out profiles/inverse_bench.txt]

At 80^3 and 160^3, B = 1, nsteps = 7, same process, after a warm-up, alternating the two routes: median ms over --reps with the 10 % / 90 %
quantiles, and the peak device memory each route adds on top of the input field (torch.cuda.max_memory_allocated).  Also, per size, one
ops.inverse_consistency(fwd, inv) call, timed the same way beside a device copy of its two operands.
Bytes counted per route (n = 3 D H W 4 bytes, one field):
  vecint_pair        (3 + 4 nsteps) n: the scaling pass reads v and writes both directions, every step reads and writes both directions
  two vecint calls   2 (2 + 2 nsteps) n + 2 n: per direction a scaling pass and nsteps steps, each one field read and one written, and the
                     negation of v in front of the second call
Both routes move the same bytes per squaring step; the pair works on 4 fields where the two calls spread over 16.
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


def timed_pair(new, old, reps: int):
    """(new, old) -> ((median, p10, p90), (median, p10, p90)) in ms: warm-up, then alternating calls, GPU events around each"""
    for f in (new, old, new, old):
        f()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for i, f in enumerate((new, old)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))

    def stats(t):
        t = sorted(t)
        return statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]

    return stats(ts[0]), stats(ts[1])


def peak_added(fn) -> float:
    """MiB of device memory fn() adds at its peak (its results alive)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
    del keep
    return peak


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inverse_bench: needs a ROCm GPU (no CPU path)")
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    nsteps = 7
    lines = [f"ops.vecint_pair against two ops.vecint calls, B = 1, nsteps = {nsteps}, reps = {args.reps}, {torch.cuda.get_device_name(0)}",
             f"{'size':>11} | {'pair ms':>8} [{'p10':>7} {'p90':>7}] {'GB/s':>6} {'MiB':>8} | {'2 calls ms':>10} [{'p10':>7} {'p90':>7}] {'GB/s':>6} {'MiB':>8} | {'speed':>6}"]
    cons = []
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for S in (80, 160):
            v = 2.0 * torch.randn((1, 3, S, S, S), device=dev, generator=g)
            n = v.numel() * 4
            pair = lambda: ops.vecint_pair(v, nsteps)
            two = lambda: (ops.vecint(v, nsteps), ops.vecint(-v, nsteps))
            (tp, p10, p90), (tt, t10, t90) = timed_pair(pair, two, args.reps)
            fwd, inv = pair()
            a, b = two()
            e_f = float((fwd - a).norm() / a.norm())
            e_i = float((inv - b).norm() / b.norm())
            assert e_f < 1e-5 and e_i < 1e-5, (e_f, e_i)                      # faster and different is not faster
            del a, b
            bp, bt = (3 + 4 * nsteps) * n, (2 * (2 + 2 * nsteps) + 2) * n
            m_pair, m_two = peak_added(pair), peak_added(two)
            lines.append(f"{S:>3}^3{'':>6} | {tp:8.3f} [{p10:7.3f} {p90:7.3f}] {bp / tp / 1e6:6.0f} {m_pair:8.1f} | {tt:10.3f} [{t10:7.3f} {t90:7.3f}] "
                         f"{bt / tt / 1e6:6.0f} {m_two:8.1f} | {tt / tp:5.2f}x")
            dst = torch.empty(2 * v.numel(), device=dev)
            src = torch.cat([fwd.reshape(-1), inv.reshape(-1)])
            (tc, c10, c90), (tcp, _, _) = timed_pair(lambda: ops.inverse_consistency(fwd, inv), lambda: dst.copy_(src), args.reps)
            mean, mx = ops.inverse_consistency(fwd, inv)
            cons.append(f"{S:>3}^3: inverse_consistency {tc:7.3f} ms [{c10:7.3f} {c90:7.3f}], {2 * n / tc / 1e6:5.0f} GB/s of its two operands; a device copy of "
                        f"them {tcp:7.3f} ms; mean {float(mean):.4f}, max {float(mx):.3f} voxels (randn * 2 velocity: not a smooth field)")
            del fwd, inv, dst, src
            torch.cuda.empty_cache()
    report = "\n".join(lines + [""] + cons)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
