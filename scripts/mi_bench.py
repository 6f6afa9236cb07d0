"""ops.mi_loss beside ops.ncc_loss, ops.mind_loss and the dense ATen statement of the same term, on the GPU.

    python scripts/mi_bench.py [--reps 30] [--size 160] [--step-limit 120] [--out profiles/mi_bench.txt]

At size^3, B = 1, K = 32 and 64: one process, after a warm-up, the routes alternating; median ms over --reps with the 10 % / 90 % quantiles
(device events around a forward + backward pair, and around the forward alone, which splits the pair).  The ATen form materialises the two
V x K weight tensors (torch.where over the two spline pieces) and contracts them with an einsum, forward and backward by autograd: what a
user would write without the kernels.  Every step runs under its own time limit (SIGALRM with the default action ends the process, also
inside a blocked device call), and the first failure ends the script: nothing is started on the GPU after it.  Two fused runs are compared
bit for bit, and the fused value against the ATen one, before anything is timed.
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


def aten_mi_loss(pred, true, bins: int, gamma: float = 0.05):
    """the definition with dense weight tensors, fp32"""
    def weights(v):
        u = v.reshape(-1).clamp(0.0, 1.0) * (bins - 3) + 1.0
        a = (u.unsqueeze(1) - torch.arange(bins, device=v.device, dtype=v.dtype)).abs()
        return torch.where(a < 1, 2.0 / 3.0 - a * a + a * a * a / 2, torch.where(a < 2, (2.0 - a) ** 3 / 6, torch.zeros_like(a)))

    V = pred.numel()
    p = torch.einsum("va,vc->ac", weights(pred), weights(true)) / V
    pa, pb = p.sum(1, keepdim=True), p.sum(0, keepdim=True)
    return -gamma * V * (p * (torch.log(p + 1e-12) - torch.log(pa * pb + 1e-12))).sum()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds allowed per step")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("mi_bench: at least 20 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("mi_bench: needs a ROCm GPU (no CPU path)")
    signal.alarm(args.step_limit)                       # library load and the first kernel launches count as a step
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    S = args.size
    shape = (1, 1, S, S, S)
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
    # another "contrast" of the same image plus noise: a pair with mutual information (that of two independent noise images is some 1e-5,
    # a difference of logarithms no fp32 evaluation can be compared on)
    true = (4.0 * pred.detach() * (1.0 - pred.detach()) + 0.1 * torch.rand(shape, device=dev, generator=g)).clamp(0.0, 1.0)
    sparse = (pred.detach() * (torch.rand(shape, device=dev, generator=g) < 0.1)).requires_grad_(True)      # 90 % of the voxels exactly 0
    lines = [f"ops.mi_loss beside ops.ncc_loss (win 9), ops.mind_loss (dilation 2) and the dense ATen form, {S}^3, B = 1, reps = {args.reps}, "
             f"{torch.cuda.get_device_name(0)}",
             f"{'route':>22} | {'pair ms':>8} [{'p10':>7} {'p90':>7}] | {'fwd ms':>8} [{'p10':>7} {'p90':>7}] | {'bwd ms':>7}"]

    def pair(loss_fn, leaf=pred):
        def run():
            leaf.grad = None
            loss_fn().backward()
        return run

    def fwd(loss_fn):
        def run():
            with torch.no_grad():
                loss_fn()
        return run

    def row(name, p, f):
        lines.append(f"{name:>22} | {p[0]:8.3f} [{p[1]:7.3f} {p[2]:7.3f}] | {f[0]:8.3f} [{f[1]:7.3f} {f[2]:7.3f}] | {p[0] - f[0]:7.3f}")

    ratios = []
    for K in (32, 64):
        signal.alarm(args.step_limit)
        fused, aten = (lambda K=K: ops.mi_loss(pred, true, K)), (lambda K=K: aten_mi_loss(pred, true, K))
        fused_sparse = lambda K=K: ops.mi_loss(sparse, true, K)
        pair(fused)()
        g0, v0 = pred.grad.clone(), float(fused().detach())
        pair(fused)()
        assert torch.equal(pred.grad, g0) and bool(torch.isfinite(g0).all()), "two fused backward runs differ"
        pair(aten)()
        v1 = float(aten().detach())
        rel = float((pred.grad - g0).norm() / g0.norm())
        assert abs(v0 - v1) <= 1e-3 * abs(v1) and rel <= 1e-3, (v0, v1, rel)
        res = timed([pair(fused), fwd(fused), pair(fused_sparse, sparse), fwd(fused_sparse), pair(aten), fwd(aten)], args.reps)
        row(f"mi K={K} fused", res[0], res[1])
        row(f"mi K={K} fused, 90% zeros", res[2], res[3])
        row(f"mi K={K} ATen dense", res[4], res[5])
        ratios.append(f"K={K}: ATen / fused forward {res[5][0] / res[1][0]:.1f}x, pair {res[4][0] / res[0][0]:.1f}x; value {v0:.6g} against {v1:.6g}, "
                      f"gradient relative L2 {rel:.2g}")
        del g0
        torch.cuda.empty_cache()
    signal.alarm(args.step_limit)
    ncc, mind = (lambda: ops.ncc_loss(pred, true, 9, 0.05)), (lambda: ops.mind_loss(pred, true, 2))
    res = timed([pair(ncc), fwd(ncc), pair(mind), fwd(mind)], args.reps)
    row("ncc win 9", res[0], res[1])
    row("mind dilation 2", res[2], res[3])
    signal.alarm(0)
    lines.extend(ratios)
    lines.append("pair: forward + backward; fwd: the forward alone (no_grad); bwd ms: pair - fwd, of the medians")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
