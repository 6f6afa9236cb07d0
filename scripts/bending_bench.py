"""The bending-energy kernels beside the L2 regulariser's, and the training step with either regulariser, on the GPU.

    python scripts/bending_bench.py [--reps 30] [--batch 10] [--steps 20] [--rounds 3] [--out profiles/bending_bench.txt]

Kernels: B = 1, C = 3 at 160^3, 80^3, 40^3 and 20^3, one process, the library's entry points called directly on preallocated buffers.
After a warm-up the four kernels alternate; one sample is a device-event bracket around --batch back-to-back launches of one kernel
divided by --batch (a single launch of 10 - 50 us between two events measures the events as much as the kernel), the figure is the median
of --reps samples with the 10 % / 90 % quantiles.  Where a launch takes less device time than the host needs to enqueue it the figure is
the enqueue rate, not the kernel: about 4 us per launch here, which is what the l2reg kernels show at 40^3 and 20^3.
  l2reg_fwd / bending_fwd    counted 4 n bytes: the field read once
  l2reg_bwd / bending_bwd    counted 8 n bytes: the field read once, the gradient written once
Each figure is set against its byte floor at 8 TB/s and each bending kernel against its l2reg counterpart of the same run.
Before anything is timed the bending value and gradient at 3 x 40^3 are compared with torch's float64 evaluation of the definition.
Step: the 160^3 / total_levels 5 / latent_levels 4 / n0 = 32 training step of bench.py (dp.DataParallelStepper, batch 1, fp32) with
regularizer="L2" and regularizer="bending", each model built --rounds times in the order L2, bending, L2, bending, ...; the script times its
own loop (host clock around --steps steps that end in a device synchronise, after 3 warm-up steps) and reports every run and the medians.
Every stage runs under its own time limit (SIGALRM with the default action ends the process, also inside a blocked device call), and the
first failure ends the script: nothing is started on the GPU after it."""
from __future__ import annotations

import argparse
import ctypes
import gc
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FEEDBACK = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
HBM_TBS = 8.0


def quantiles(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]


def timed(routes, reps: int, batch: int):
    """[(median, p10, p90)] in us per launch and route: warm-up, then alternating samples of `batch` back-to-back launches"""
    for _ in range(3):
        for f in routes:
            for _ in range(batch):
                f()
    torch.cuda.synchronize()
    ts = [[] for _ in routes]
    for _ in range(reps):
        for i, f in enumerate(routes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                f()
            b.record()
            b.synchronize()
            ts[i].append(1e3 * a.elapsed_time(b) / batch)
    return [quantiles(t) for t in ts]


def kernel_routes(lib, df, gdf, one, stream):
    """the four launches on preallocated buffers, straight through the C ABI"""
    _, C, D, H, W = df.shape
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    n = df.numel()
    p_l2 = torch.empty(lib.query("pulpo_loss_blocks", n), device=df.device)
    p_be = torch.empty(lib.query("pulpo_bending_blocks", C, D, H, W), device=df.device)
    keep = (p_l2, p_be)
    l2f, l2b = lib.raw("pulpo_l2reg_fwd"), lib.raw("pulpo_l2reg_bwd")
    bef, beb = lib.raw("pulpo_bending_fwd"), lib.raw("pulpo_bending_bwd")

    def must(rc):
        if rc != 0:
            raise SystemExit(f"bending_bench: a launch failed with code {rc}")

    return [("l2reg_fwd", 4.0 * n, lambda: must(l2f(vp(df), C, D, H, W, vp(p_l2), stream))),
            ("bending_fwd", 4.0 * n, lambda: must(bef(vp(df), C, D, H, W, vp(p_be), stream))),
            ("l2reg_bwd", 8.0 * n, lambda: must(l2b(vp(df), vp(one), 1.0, vp(gdf), C, D, H, W, stream))),
            ("bending_bwd", 8.0 * n, lambda: must(beb(vp(df), vp(one), 1.0, vp(gdf), C, D, H, W, stream)))], keep


def accuracy(ops, say):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bending_ref as BR
    u = torch.randn(1, 3, 40, 40, 40, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    x = u.clone().requires_grad_(True)
    loss = ops.bending_reg(x, 0.025)
    g, = torch.autograd.grad(loss, [x])
    ref, rg = BR.bending_ref(u.double(), 0.025), BR.bending_grad_ref(u.double(), 0.025)
    el = abs(float(loss.detach()) - float(ref)) / abs(float(ref))
    eg = float(((g.double() - rg).abs() / (1e-7 * max(1.0, float(rg.abs().max())) + 1e-4 * rg.abs())).max())
    say(f"check at 3 x 40^3 against float64: loss relative error {el:.2e} (bound 1e-5), gradient error / bound {eg:.3f}")
    if not (el <= 1e-5 and eg <= 1.0):
        raise SystemExit("bending_bench: the kernels disagree with the float64 definition; nothing timed")


def step_time(models, dp, synthetic, regularizer: str, steps: int):
    torch.manual_seed(0)
    size = [160, 160, 160]
    model = models.PULPo(5, 4, 0.1, size, feedback=FEEDBACK, n0=32, regularizer=regularizer).to("cuda").train()
    stepper = dp.DataParallelStepper(model)
    x, y = synthetic.uniform_pair(size, 1, 1234, torch.device("cuda"))
    empty = torch.empty((0,), device="cuda")
    batch = (x, y, empty, empty, empty, empty, empty, empty)
    for _ in range(3):
        stepper.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = stepper.step(batch)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    reg = float(model.logged["train/regularization_loss"].detach())
    if not torch.isfinite(torch.as_tensor(loss)).all():
        raise SystemExit(f"bending_bench: the {regularizer} step's loss is not finite")
    del stepper, model, batch, x, y
    gc.collect()
    torch.cuda.empty_cache()
    return ms, reg


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--stage-limit", type=int, default=150, help="seconds per stage")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bending_bench: at least 20 samples")
    if not torch.cuda.is_available():
        raise SystemExit("bending_bench: needs a ROCm GPU (no CPU path)")
    from pulpo_amd import dp, ops, synthetic
    from pulpo_amd._lib import lib
    import src.models as models
    lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"bending_bench on {torch.cuda.get_device_name(0)}: {args.reps} samples of {args.batch} launches, median [p10, p90] us per launch; "
        f"floor = counted bytes at {HBM_TBS:.0f} TB/s")
    signal.alarm(args.stage_limit)
    accuracy(ops, say)
    signal.alarm(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = torch.ones((), device="cuda")
    ratios = {}
    for s in (160, 80, 40, 20):
        signal.alarm(args.stage_limit)
        df = torch.randn(1, 3, s, s, s, device="cuda", generator=torch.Generator(device="cuda").manual_seed(s))
        gdf = torch.empty_like(df)
        routes, keep = kernel_routes(lib, df, gdf, one, stream)
        res = timed([r[2] for r in routes], args.reps, args.batch)
        say(f"3 x {s}^3")
        t = {}
        for (name, nbytes, _), (med, lo, hi) in zip(routes, res):
            floor = nbytes / (HBM_TBS * 1e12) * 1e6
            t[name] = med
            say(f"  {name:12s} {med:8.2f} [{lo:7.2f}, {hi:7.2f}] us   floor {floor:6.2f} us   floor / time {floor / med:5.2f}   "
                f"{nbytes / med * 1e-6:7.3f} TB/s counted")
        ratios[s] = (t["bending_fwd"] / t["l2reg_fwd"], t["bending_bwd"] / t["l2reg_bwd"])
        say(f"  bending / l2reg: fwd {ratios[s][0]:.2f} x, bwd {ratios[s][1]:.2f} x")
        signal.alarm(0)
        del df, gdf, routes, keep
    f, b = ratios[160]
    say(f"target at 3 x 160^3 (each bending kernel <= 2 x its l2reg counterpart): fwd {f:.2f} x {'met' if f <= 2.0 else 'MISSED'}, "
        f"bwd {b:.2f} x {'met' if b <= 2.0 else 'MISSED'}")
    if not args.no_step:
        got = {"L2": [], "bending": []}
        for reg in ("L2", "bending") * args.rounds:
            signal.alarm(args.stage_limit)
            ms, val = step_time(models, dp, synthetic, reg, args.steps)
            signal.alarm(0)
            got[reg].append(ms)
            say(f"step 160^3 / T5 / L4 / n0 32, regularizer={reg!r}: {ms:.2f} ms per step over {args.steps} steps (regularisation term {val:.4g})")
        l2, be = statistics.median(got["L2"]), statistics.median(got["bending"])
        say(f"step, medians of {args.rounds} runs: L2 {l2:.2f} ms, bending {be:.2f} ms, difference {be - l2:+.2f} ms ({100 * (be - l2) / l2:+.2f} %); "
            f"spread of the runs of one regulariser: L2 {max(got['L2']) - min(got['L2']):.2f} ms, "
            f"bending {max(got['bending']) - min(got['bending']):.2f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
