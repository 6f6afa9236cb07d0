"""ops.affine_warp beside the route through the existing operators, and affine.fit box to box, on the GPU.

    python scripts/affine_bench.py [--reps 30] [--step-limit 120] [--out profiles/affine_bench.txt]

At 160^3 and 80^3, C = 1, B = 1, one process, after a warm-up, the routes alternating; median ms over --reps with the 10 % / 90 %
quantiles (device events around each call):
  fused fwd      ops.affine_warp(theta, img)                                   counted 8 N bytes: the image in, the result out
  composed fwd   ops.warp3d(ops.affine_field(theta, size), img)                counted 32 N: the field out (12 N), then 3 + 2 planes of 4 N
  fused f+b      forward + backward: gtheta from the gradient kernel           counted 16 N: forward, then the image and the gradient in
  composed f+b   forward + ops.warp3d's backward, gtheta by torch reductions of gdf (twelve sums over the field)
                                                                               counted 92 N: forward 32, warp backward 36 (field,
                                                                               image, gradient in, gdf out), the reductions read gdf 12 N
                                                                               and the 12 N coordinate planes
  copy           a device copy of the fused route's bytes (4 N in, 4 N out) in the same run: the rate the counted GB/s is set against
Before anything is timed the fused forward is compared with the composed one bit for bit (C = 1) and the two gtheta with each other.
Then affine.fit with its defaults at 160^3 on synthetic.affine_pair, box to box (host clock around a synchronised call), its corner error,
and the split of its device time by kernel class from the ops.HBM_TRACE brackets of a second, traced call.
Every stage runs under its own time limit (SIGALRM with the default action ends the process, also inside a blocked device call), and the
first failure ends the script: nothing is started on the GPU after it.
"""
from __future__ import annotations

import argparse
import os
import signal
import statistics
import sys
import time

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
    ap.add_argument("--step-limit", type=int, default=120, help="seconds allowed per stage")
    ap.add_argument("--fit-size", type=int, default=160)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("affine_bench: at least 20 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("affine_bench: needs a ROCm GPU (no CPU path)")
    signal.alarm(args.step_limit)                       # library load and the first kernel launches count as a stage
    from pulpo_amd import affine, ops, synthetic
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"ops.affine_warp beside warp3d(affine_field), C = 1, B = 1, reps = {args.reps}, {torch.cuda.get_device_name(0)}",
             f"{'size':>6} {'route':>13} | {'ms':>8} [{'p10':>7} {'p90':>7}] {'counted GB/s':>12} {'of copy':>8} | {'vs composed':>11}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for S in (160, 80):
        signal.alarm(args.step_limit)
        size = (S, S, S)
        img = ops.resize_trilinear(torch.rand((1, 1, S // 8, S // 8, S // 8), device=dev, generator=g), size).contiguous()
        gout = torch.randn((1, 1, S, S, S), device=dev, generator=g)
        theta = synthetic.default_theta_gen(1, dev)
        N = img.numel()
        u = torch.stack(torch.meshgrid(*[torch.arange(s, device=dev, dtype=torch.float32) - (s - 1) / 2 for s in size], indexing="ij"))
        src, dst = torch.empty(N, device=dev), torch.empty(N, device=dev)

        def fused_fwd():
            with torch.no_grad():
                return ops.affine_warp(theta, img)

        def composed_fwd():
            with torch.no_grad():
                return ops.warp3d(ops.affine_field(theta, size), img)

        def fused_fb():
            leaf = theta.clone().requires_grad_(True)
            ops.affine_warp(leaf, img).backward(gout)
            return leaf.grad

        def composed_fb():
            df = ops.affine_field(theta, size).requires_grad_(True)
            ops.warp3d(df, img).backward(gout)
            gdf = df.grad[0]
            return torch.cat([torch.einsum("adhw,jdhw->aj", gdf, u), gdf.flatten(1).sum(1, keepdim=True)], dim=1).unsqueeze(0)

        def copy():
            dst.copy_(src)

        assert torch.equal(fused_fwd(), composed_fwd()), "the fused forward differs from warp3d(affine_field)"
        ga, gb = fused_fb(), composed_fb()
        dev_g = float((ga - gb).abs().max() / gb.abs().max())
        assert torch.equal(fused_fb(), ga) and dev_g < 1e-3, f"gtheta: two calls differ, or the routes disagree ({dev_g:.3g})"
        stats = timed([fused_fwd, composed_fwd, fused_fb, composed_fb, copy], args.reps)
        counted = [8.0 * N, 32.0 * N, 16.0 * N, 92.0 * N, 8.0 * N]
        copy_rate = counted[4] / stats[4][0]
        for k, name in enumerate(("fused fwd", "composed fwd", "fused f+b", "composed f+b", "copy")):
            t, a, b = stats[k]
            rate = counted[k] / t
            versus = "" if k in (1, 3, 4) else f"{stats[k + 1][0] / t:10.2f}x"
            lines.append(f"{S:>4}^3 {name:>13} | {t:8.3f} [{a:7.3f} {b:7.3f}] {rate / 1e6:12.0f} {rate / copy_rate:8.2f} | {versus:>11}")
        lines.append(f"{S:>4}^3 gtheta: fused against torch reductions of warp3d's gdf, largest difference {dev_g:.2g} of the largest entry")
        del img, gout, u, src, dst
        torch.cuda.empty_cache()
    # ---- the fitter, box to box
    signal.alarm(args.step_limit)
    S = args.fit_size
    size = (S, S, S)
    x, y, want = synthetic.affine_pair(size, 1, 3, dev)
    affine.fit(x, y, iters=(2, 2, 2))                   # warm-up: every kernel of the loop at every level
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = affine.fit(x, y)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    start = float(affine.corner_error(affine.identity(1, dev), want, size))
    end = float(affine.corner_error(res["theta"], want, size))
    h = res["history"]
    n_it = h.shape[0] - 1
    lines.append("")
    lines.append(f"affine.fit defaults (dof 12, NCC, lr {affine.DEFAULT_LR}, iterations {affine.DEFAULT_ITERS}, windows {affine.DEFAULT_WIN}) at {S}^3 on "
                 f"synthetic.affine_pair: {statistics.median(times):.1f} ms box to box (3 calls: {', '.join(f'{t:.1f}' for t in times)}), "
                 f"{n_it} iterations; corner error {start:.2f} -> {end:.2f} voxels; loss at the finest level {float(h[-1 - affine.DEFAULT_ITERS[-1], 0]):.1f} -> {float(h[-1, 0]):.1f}")
    signal.alarm(args.step_limit)
    ops.CONV_TRACE_STRIDE, ops.HBM_TRACE = 1, []
    affine.fit(x, y)
    torch.cuda.synchronize()
    trace, ops.HBM_TRACE = ops.HBM_TRACE, None
    by = {}
    for name, nbytes, a, b in trace:
        t, n, by_ = by.get(name, (0.0, 0, 0.0))
        by[name] = (t + a.elapsed_time(b), n + 1, by_ + nbytes)
    total = sum(t for t, _, _ in by.values())
    lines.append(f"device time inside the HBM_TRACE brackets of one traced call: {total:.1f} ms (the rest of the box-to-box time is the host: "
                 f"launches, autograd, the few-element torch ops)")
    lines.append(f"{'kernel class':>22} | {'launches':>8} {'ms':>8} {'share':>6} {'counted GB/s':>12}")
    for name, (t, n, nb) in sorted(by.items(), key=lambda kv: -kv[1][0]):
        lines.append(f"{name:>22} | {n:8d} {t:8.2f} {100 * t / total:5.1f}% {nb / t / 1e6:12.0f}")
    signal.alarm(0)
    lines.append("ms: median of device events around one call; counted GB/s: the bytes the route must move (docstring) / median; of copy: that rate over")
    lines.append("the device copy's in the same run; vs composed: composed median / fused median.  One synthetic pair; traced brackets cover every launch.")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
