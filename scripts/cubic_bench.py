"""The cubic B-spline kernels (ops.bspline_prefilter, ops.warp3d_cubic forward and backward) beside the trilinear warp
(ops.warp3d forward and its field-gradient backward), on the GPU.

    python scripts/cubic_bench.py [--reps 30] [--out profiles/cubic_bench.txt]

At 80^3 and 160^3, B = 1, C = 1, one process, after a warm-up, the five variants and a device copy alternating: median ms over --reps with
the 10 % / 90 % quantiles.  The field is smooth noise of 2 voxels (a 4^3 lattice interpolated up), the image uniform noise.
Bytes counted (V voxels, 4 bytes each):
  prefilter          8 V per pass, three passes: every pass reads and writes the volume once (the anticausal sweep reads the causal values
                     again - from L2 where the plane set fits - and that second trip is not counted)
  cubic / warp3d     (3 + 2 C) V 4: the field and the image (or coefficients) once, the result once; the backward reads the upstream
                     gradient in place of writing the result and writes the 3-component field gradient, (6 + 2 C) V 4
Each variant's floor is its bytes at the rate of the device copy measured in the same loop (2 V 4 bytes moved).
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


def timed(fns, reps: int):
    """{name: fn} -> {name: (median, p10, p90)} in ms: warm-up, then the variants alternating, GPU events around each call"""
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))

    def stats(t):
        t = sorted(t)
        return statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]

    return {k: stats(t) for k, t in ts.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cubic_bench: needs a ROCm GPU (no CPU path)")
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    C = 1
    lines = [f"cubic B-spline kernels beside the trilinear warp, B = 1, C = {C}, reps = {args.reps}, {torch.cuda.get_device_name(0)}",
             f"{'size':>6} {'variant':>16} | {'ms':>8} [{'p10':>7} {'p90':>7}] | {'MB':>7} {'GB/s':>6} | {'ms / floor':>10} | {'/ warp3d':>8}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for S in (80, 160):
        V = S ** 3
        img = torch.rand((1, C, S, S, S), device=dev, generator=g)
        lat = torch.randn((1, 3, 4, 4, 4), device=dev, generator=g)
        df = 2.0 * torch.nn.functional.interpolate(lat, size=(S, S, S), mode="trilinear", align_corners=True).contiguous()
        gout = torch.randn((1, C, S, S, S), device=dev, generator=g)
        coef = ops.bspline_prefilter(img)
        dst = torch.empty_like(img)

        def backward_of(warp):
            leaf = df.clone().requires_grad_(True)
            out = warp(leaf)

            def run():
                leaf.grad = None
                out.backward(gout, retain_graph=True)
            return run

        fns = {
            "copy": lambda: dst.copy_(img),
            "prefilter": lambda: ops.bspline_prefilter(img),
            "cubic fwd": lambda: ops.warp3d_cubic(df, coef=coef),          # (nothing here requires grad: no graph is recorded)
            "warp3d fwd": lambda: ops.warp3d(df, img),
            "cubic bwd": backward_of(lambda f: ops.warp3d_cubic(f, coef=coef)),
            "warp3d bwd": backward_of(lambda f: ops.warp3d(f, img)),
        }
        nbytes = {"copy": 8.0 * V, "prefilter": 24.0 * V, "cubic fwd": 4.0 * (3 + 2 * C) * V, "warp3d fwd": 4.0 * (3 + 2 * C) * V,
                  "cubic bwd": 4.0 * (6 + 2 * C) * V, "warp3d bwd": 4.0 * (6 + 2 * C) * V}
        t = timed(fns, args.reps)
        rate = nbytes["copy"] / t["copy"][0]                                   # bytes per ms of the device copy in this loop
        against = {"cubic fwd": "warp3d fwd", "cubic bwd": "warp3d bwd"}
        for k in fns:
            med, p10, p90 = t[k]
            ratio = f"{med / t[against[k]][0]:7.2f}x" if k in against else f"{'':>8}"
            lines.append(f"{S:>3}^3 {k:>16} | {med:8.4f} [{p10:7.4f} {p90:7.4f}] | {nbytes[k] / 1e6:7.1f} {nbytes[k] / med / 1e6:6.0f} | "
                         f"{med / (nbytes[k] / rate):9.1f}x | {ratio}")
        del img, df, gout, coef, dst, fns
        torch.cuda.empty_cache()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
