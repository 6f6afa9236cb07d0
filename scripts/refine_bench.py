"""pulpo_amd.refine on the GPU at the benchmark's configuration: time per iteration, the step-size sweep behind
refine.DEFAULT_LR, and the fused parameter-side launch beside the per-level composition it replaces.

    python scripts/refine_bench.py [--size 160 160 160] [--levels 5 4] [--repeats 7] [--iters 40] [--step-limit 300] [--out profiles/refine_bench.txt]

One process, synthetic.oasis_like_pair, an untrained model in eval mode (the loop has no network in it: the weights only set the start).
  1. ms per iteration, box to box: refine(individual_dfs=<the prediction>, iters=K) between two device synchronisations minus the same call with
     iters=0 (arena set-up, the closing forward pass, the output warps), over K; --repeats times after a warm-up call: median [min, max].
  2. where the time goes: a run of its own with ops.HBM_TRACE on (device events around every HBM-bound launch), ms per iteration and
     kernel class; what the brackets do not cover (torch's own small kernels, launch gaps) is the remainder to the box-to-box figure.
  3. the sweep: the objective after 10 / 25 / 50 iterations for lr in {0.01, 0.03, 0.1, 0.3}, from the model's prediction and from zero
     fields; `rise` = the largest increase of the total between consecutive iterations over the total drop.  The default lr is the best
     objective after 50 iterations among the settings with rise <= 1 % in BOTH starts (ranked by the sum over the two starts), the smaller on a tie.
  4. the parameter side alone, on the refinement's own arena: one ops.anchored_adam_step launch (+ its column sum) against, per level,
     torch ops for the anchor's gradient and value + ops.adam_step (which also re-packs the model's convolution weights, as it must after a
     step on parameters); alternating, device events around each, median [p10, p90] over 30 calls.
  5. for scale, the training step (dp.DataParallelStepper) of the same model and pair in the same process.
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

FEEDBACK = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
LRS = (0.01, 0.03, 0.1, 0.3)


def wall(fn) -> float:
    """ms between two device synchronisations around fn()"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(routes, reps: int):
    """[(median, p10, p90)] in ms per route: warm-up, then alternating calls, device events around each"""
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
    out = []
    for t in ts:
        t = sorted(t)
        out.append((statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]))
    return out


def rise_share(total: torch.Tensor) -> float:
    """largest increase between consecutive rows over the drop from the first row to the lowest"""
    drop = float(total[0] - total.min())
    return float((total[1:] - total[:-1]).clamp_min(0).max()) / drop if drop > 0 else float("inf")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[160, 160, 160])
    ap.add_argument("--levels", type=int, nargs=2, default=[5, 4], help="total_levels latent_levels")
    ap.add_argument("--n0", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40, help="iterations per timed call")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds allowed per stage")
    ap.add_argument("--no-train-step", action="store_true", help="skip stage 5")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("refine_bench: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench: needs a ROCm GPU (no CPU path)")
    signal.alarm(args.step_limit)                       # library load, model construction and the first launches count as a stage
    from pulpo_amd import dp, ops, synthetic
    from pulpo_amd._lib import lib
    from pulpo_amd.models import PULPo
    from pulpo_amd.refine import DEFAULT_LR, _views, arena_layout, refine
    lib.load()
    dev = torch.device("cuda", 0)
    T, L = args.levels
    size = list(args.size)
    torch.manual_seed(0)
    model = PULPo(T, L, 0.1, size, feedback=FEEDBACK, n0=args.n0).to(dev).eval()
    x, y = synthetic.oasis_like_pair(size, 1, 1234, dev)
    with torch.no_grad():
        pred = {l: t.clone() for l, t in model.predict_deterministic(x, y)[1].items()}
    zero = {l: torch.zeros_like(t) for l, t in pred.items()}
    shapes = [tuple(pred[l].shape) for l in range(L)]
    offsets, total = arena_layout(shapes)
    lines = [f"pulpo_amd.refine at {'x'.join(map(str, size))} / T{T} / L{L} / n0 {args.n0}, B = 1, synthetic.oasis_like_pair, untrained model in eval mode, "
             f"{torch.cuda.get_device_name(0)}",
             f"level fields {[tuple(s[2:]) for s in shapes]}: arena of {total} floats ({4 * total / 1e6:.2f} MB)", ""]

    # ---- 1. box to box
    K = args.iters
    refine(model, x, y, individual_dfs=pred, iters=3)                                                   # warm-up: every shape of the loop
    t_k = [wall(lambda: refine(model, x, y, individual_dfs=pred, iters=K)) for _ in range(args.repeats)]
    t_0 = [wall(lambda: refine(model, x, y, individual_dfs=pred, iters=0)) for _ in range(args.repeats)]
    base = statistics.median(t_0)
    per = sorted((t - base) / K for t in t_k)
    per_iter = statistics.median(per)
    lines += [f"1. per iteration, box to box (refine(iters={K}) - refine(iters=0), {args.repeats} repeats): median {per_iter:.3f} ms [min {per[0]:.3f}, max {per[-1]:.3f}]",
              f"   refine(iters=0): median {base:.3f} ms [min {min(t_0):.3f}, max {max(t_0):.3f}]  (arena set-up, one forward pass, the output warps)"]
    t_a = sorted((wall(lambda: refine(model, x, y, individual_dfs=pred, iters=K, anchor=0.1)) - base) / K for _ in range(args.repeats))
    lines += [f"   with anchor=0.1: median {statistics.median(t_a):.3f} ms [min {t_a[0]:.3f}, max {t_a[-1]:.3f}]", ""]

    # ---- 2. the split (a run of its own: the brackets slow the host)
    signal.alarm(args.step_limit)
    n_it = 10
    ops.HBM_TRACE, stride = [], ops.CONV_TRACE_STRIDE
    ops.CONV_TRACE_STRIDE = 1
    t_traced = wall(lambda: refine(model, x, y, individual_dfs=pred, iters=n_it, anchor=0.1))
    trace, ops.HBM_TRACE = ops.HBM_TRACE, None
    ops.CONV_TRACE_STRIDE = stride
    torch.cuda.synchronize()
    by = {}
    for name, nbytes, a, b in trace:
        e = by.setdefault(name, [0, 0.0, 0.0])
        e[0] += 1
        e[1] += a.elapsed_time(b)
        e[2] += nbytes
    lines.append(f"2. HBM-bound launches of refine(iters={n_it}, anchor=0.1), {n_it + 1} forward and {n_it} backward passes, per iteration (traced call: {t_traced / n_it:.3f} ms per iteration):")
    lines.append(f"   {'kernel class':<24} {'launches':>8} {'ms':>8} {'GB/s':>7}")
    covered = 0.0
    for name, (cnt, ms, nb) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        covered += ms
        lines.append(f"   {name:<24} {cnt / n_it:8.1f} {ms / n_it:8.3f} {nb / ms / 1e6 if ms > 0 else 0:7.0f}")
    lines += [f"   bracketed total {covered / n_it:.3f} ms per iteration; box to box (1.) {per_iter:.3f} ms", ""]

    # ---- 3. the sweep
    signal.alarm(args.step_limit)
    lines.append("3. step-size sweep, total objective (similarity + regulariser) after 0 / 10 / 25 / 50 iterations; rise = largest single increase / total drop")
    lines.append(f"   {'start':<11} {'lr':>5} {'0':>12} {'10':>12} {'25':>12} {'50':>12} {'rise':>8}")
    table = {}
    for tag, start in (("prediction", pred), ("zero", zero)):
        for lr in LRS:
            h = refine(model, x, y, individual_dfs=start, iters=50, lr=lr)["history"][:, 0].double().cpu()
            table[(tag, lr)] = (float(h[50]), rise_share(h))
            lines.append(f"   {tag:<11} {lr:5.2f} {float(h[0]):12.4f} {float(h[10]):12.4f} {float(h[25]):12.4f} {float(h[50]):12.4f} {100 * rise_share(h):7.2f}%")
    ok = [lr for lr in LRS if all(table[(tag, lr)][1] <= 0.01 for tag in ("prediction", "zero"))]
    if ok:
        best = min(ok, key=lambda lr: (sum(table[(tag, lr)][0] for tag in ("prediction", "zero")), lr))
        lines.append(f"   settings with rise <= 1 % in both starts: {ok}; best sum of the two objectives after 50 iterations: lr = {best}"
                     f"   (refine.DEFAULT_LR is {DEFAULT_LR})")
    else:
        lines.append(f"   no setting keeps the rise within 1 % in both starts (refine.DEFAULT_LR is {DEFAULT_LR})")
    lines.append("")

    # ---- 4. the parameter side alone
    signal.alarm(args.step_limit)
    g = torch.Generator(device="cuda").manual_seed(0)
    arena, grad, mean = (torch.randn(total, device=dev, generator=g) for _ in range(3))
    prec = torch.rand(total, device=dev, generator=g) + 0.1
    m, v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    val = torch.zeros(1, device=dev)
    lv = lambda t: _views(t, offsets, shapes)
    P, G, M_, V, MU, PR = lv(arena), lv(grad), lv(m), lv(v), lv(mean), lv(prec)

    def fused():
        ops.anchored_adam_step(arena, grad, m, v, 0.1, 1, mean=mean, prec=prec, loss_out=val)

    def fused_plain():
        ops.anchored_adam_step(arena, grad, m, v, 0.1, 1)

    def composed():
        acc = None
        for l in range(L):
            d = P[l] - MU[l]
            ad = PR[l] * d
            s = 0.5 * torch.sum(ad * d)
            acc = s if acc is None else acc + s
            ops.adam_step(P[l].view(-1), (G[l] + ad).view(-1), M_[l].view(-1), V[l].view(-1), 0.1, 1)
        val.copy_(acc.reshape(1))

    def composed_plain():
        for l in range(L):
            ops.adam_step(P[l].view(-1), G[l].view(-1), M_[l].view(-1), V[l].view(-1), 0.1, 1)

    with torch.no_grad():
        (tf, f10, f90), (tc, c10, c90), (tp, p10, p90), (tq, q10, q90) = alternating([fused, composed, fused_plain, composed_plain], 30)
    lines += [f"4. parameter side alone on the {total}-float arena ({L} levels), median ms [p10, p90] over 30 alternating calls:",
              f"   anchored: one ops.anchored_adam_step + column sum   {tf:7.3f} [{f10:7.3f}, {f90:7.3f}]   ({36.0 * total / tf / 1e6:.0f} GB/s of 36 bytes per element)",
              f"             {L} x (torch anchor + ops.adam_step)        {tc:7.3f} [{c10:7.3f}, {c90:7.3f}]   ratio {tc / tf:.1f}",
              f"   no anchor: one ops.anchored_adam_step              {tp:7.3f} [{p10:7.3f}, {p90:7.3f}]",
              f"             {L} x ops.adam_step                         {tq:7.3f} [{q10:7.3f}, {q90:7.3f}]   ratio {tq / tp:.1f}",
              "   (ops.adam_step ends in refresh_weight_packs(): with this model's packs registered it re-packs every convolution weight per call)", ""]
    del arena, grad, mean, prec, m, v

    # ---- 5. the training step, for scale
    if not args.no_train_step:
        signal.alarm(args.step_limit)
        model.train()
        stepper = dp.DataParallelStepper(model, lr=1e-4)
        empty = torch.empty((0,), device=dev)
        batch = (x, y, empty, empty, empty, empty, empty, empty)
        for _ in range(2):
            stepper.step(batch)
        ts = sorted(wall(lambda: stepper.step(batch)) for _ in range(args.repeats))
        lines += [f"5. training step of the same model and pair (dp.DataParallelStepper, fp32), {args.repeats} steps: median {statistics.median(ts):.2f} ms "
                  f"[min {ts[0]:.2f}, max {ts[-1]:.2f}]; one refinement iteration is {100 * per_iter / statistics.median(ts):.1f} % of it", ""]
    signal.alarm(0)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
