"""The Dice term of the training step from label maps against the one-hot route it stands beside, on the GPU.

    python scripts/label_dice_bench.py [--reps 20] [--only operator|step] [--out profiles/label_dice_bench.txt]

Same process, the two routes alternating, medians with the 10 % / 90 % quantiles after a warm-up.
  operator   ops.label_dice_loss forward + backward          against  ops.warp3d(df, one_hot) + ops.soft_dice_loss forward + backward (gradient
             at 160^3 and 192 x 224 x 160, C in {5, 36},              of the field only; the one-hot maps are built outside the timed region)
             uint8 labels in 8^3 regions, all grids alike
             Bytes of the backward kernel: 24 V (three displacement planes read, three gradient planes written) + 2 V label bytes; reported as
             the share of that floor at the device-to-device copy rate measured in the same run (the kernel timed alone, 10 launches between two HIP events).
  step       the 160^3 / T5 / L4 / n0 = 32 training step of bench.py with recon_loss = ["ncc", "dice"], C = 36: a batch of uint8 label maps
             against the same batch as float one-hot maps; ms per step (zero_grad + forward + backward + Adam, dp.DataParallelStepper) and
             torch.cuda.max_memory_allocated of each, the peak measured from a fresh model in a fresh allocator state.
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
import torch.nn.functional as F  # noqa: E402

FEEDBACK = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
LINES = []


def say(line: str = "") -> None:
    print(line, flush=True)
    LINES.append(line)


def stats(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[(9 * len(t)) // 10]


def timed(fns, reps: int):
    """[(median, p10, p90) ms per function]: two warm-up rounds, then `reps` alternating rounds, GPU events around each call"""
    for _ in range(2):
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
    return [stats(t) for t in ts]


def copy_rate(reps: int) -> float:
    """bytes/s of a 2 GiB device-to-device copy (read + write counted)"""
    src = torch.empty(1 << 29, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    (ms, _, _), = timed([lambda: dst.copy_(src)], reps)
    return 2.0 * src.numel() * 4 / (ms * 1e-3)


def one_hot(lab, C):
    return F.one_hot(lab[:, 0].long(), C).permute(0, 4, 1, 2, 3).float().contiguous()


def block_labels(C, size, gen, dev):
    coarse = torch.randint(0, C, (1, 1) + tuple((s + 7) // 8 for s in size), device=dev, generator=gen)
    lab = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4)[:, :, :size[0], :size[1], :size[2]]
    return lab.to(torch.uint8).contiguous()


def bwd_kernel_ms(df, lab, tgt, C: int, reps: int) -> float:
    """median ms of one pulpo_label_dice_bwd launch: `reps` boxes of 10 launches between two GPU events, on the coefficients of a forward call"""
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    dev = df.device
    f32 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    loss, dice, coef, ddf, gup = f32(), f32(1, C), f32(1, C, 2), torch.empty_like(df), torch.ones((), device=dev)
    ws = torch.empty(lib.query("pulpo_warp_labels_ws_bytes", 1, C), device=dev, dtype=torch.uint8)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    dims = [int(v) for v in (*df.shape[2:], *lab.shape[2:], *tgt.shape[2:])]
    P, st = ops._ptr, ops._stream()
    lib.call("pulpo_label_dice_fwd", P(df), P(lab), P(tgt), 0, C, 1.0, P(loss), P(dice), P(coef), P(ws), ops._int_ptr(flag), 1, *dims, st)

    def box():
        for _ in range(10):
            lib.call("pulpo_label_dice_bwd", P(df), P(lab), P(tgt), 0, C, P(coef), P(gup), P(ddf), 1, *dims, st)

    (ms, _, _), = timed([box], reps)
    return ms / 10


def operator(reps: int, dev) -> None:
    from pulpo_amd import ops
    bw = copy_rate(reps)
    say(f"device-to-device copy: {bw / 1e9:.0f} GB/s (the byte floor is counted at this rate); reps: {reps}")
    say(f"{'grid':>13} {'C':>3} | {'label fwd+bwd ms':>16} [{'p10':>7} {'p90':>7}] | {'one-hot fwd+bwd':>16} [{'p10':>7} {'p90':>7}] | {'speed':>6} | "
        f"{'bwd kernel ms':>13} {'floor ms':>8} {'share':>6}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for size in ((160, 160, 160), (192, 224, 160)):
        V = size[0] * size[1] * size[2]
        for C in (5, 36):
            lab, tgt = block_labels(C, size, gen, dev), block_labels(C, size, gen, dev)
            df = (2.0 * torch.randn((1, 3) + size, device=dev, generator=gen)).requires_grad_(True)
            oh, toh = one_hot(lab, C), one_hot(tgt, C)

            def label_route():
                df.grad = None
                ops.label_dice_loss(df, lab, C, tgt, check=False).backward()

            def onehot_route():
                df.grad = None
                ops.soft_dice_loss(ops.warp3d(df, oh), toh, 1).backward()

            new, old = timed([label_route, onehot_route], reps)
            label_route()
            g_new = df.grad.clone()
            onehot_route()
            err = float((g_new - df.grad).abs().max() / df.grad.abs().max())
            assert err < 1e-3, err                                              # faster and different is not faster
            tb = bwd_kernel_ms(df.detach(), lab, tgt, C, reps)
            floor = (24 * V + 2 * V) / bw * 1e3
            say(f"{'x'.join(map(str, size)):>13} {C:>3} | {new[0]:16.3f} [{new[1]:7.3f} {new[2]:7.3f}] | {old[0]:16.3f} [{old[1]:7.3f} {old[2]:7.3f}] | "
                f"{old[0] / new[0]:5.1f}x | {tb:13.3f} {floor:8.3f} {floor / tb:6.2f}   (gradients agree to {err:.1e} of max)")
            del oh, toh
            torch.cuda.empty_cache()


def step(reps: int, dev) -> None:
    from pulpo_amd import dp, synthetic
    from src.models import PULPo
    size, T, L, C = [160, 160, 160], 5, 4, 36
    gen = torch.Generator(device="cuda").manual_seed(1)
    x, y = synthetic.uniform_pair(size, 1, 1234, dev)
    seg_x, seg_y = block_labels(C, tuple(size), gen, dev), block_labels(C, tuple(size), gen, dev)
    empty = torch.empty((0,), device=dev)
    onehot_bytes = 2 * C * size[0] * size[1] * size[2] * 4

    def fresh():
        torch.manual_seed(0)
        model = PULPo(T, L, 0.1, size, feedback=FEEDBACK, n0=32, recon_loss=["ncc", "dice"], segs=True, num_classes=C).to(dev).train()
        return dp.DataParallelStepper(model)

    def batch(kind):
        if kind == "label":
            return (x, y, seg_x, seg_y, empty, empty, empty, empty)
        return (x, y, one_hot(seg_x, C), one_hot(seg_y, C), empty, empty, empty, empty)

    peak, loss = {}, {}
    for kind in ("label", "one-hot"):
        st = fresh()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        b = batch(kind)
        for _ in range(3):
            loss[kind] = float(st.step(b))
        torch.cuda.synchronize()
        peak[kind] = torch.cuda.max_memory_allocated()
        del st, b
        torch.cuda.empty_cache()
    st = fresh()
    bl, bo = batch("label"), batch("one-hot")
    new, old = timed([lambda: st.step(bl), lambda: st.step(bo)], reps)
    say(f"\nstep 160^3 T{T} L{L} n0=32 recon_loss=[ncc, dice] C={C}, B=1 (loss of the third step: label {loss['label']:.6g}, one-hot {loss['one-hot']:.6g})")
    say(f"  label batch    {new[0]:8.2f} ms [{new[1]:8.2f} {new[2]:8.2f}]   peak memory {peak['label'] / 2 ** 20:9.1f} MiB")
    say(f"  one-hot batch  {old[0]:8.2f} ms [{old[1]:8.2f} {old[2]:8.2f}]   peak memory {peak['one-hot'] / 2 ** 20:9.1f} MiB")
    drop = peak["one-hot"] - peak["label"]
    say(f"  peak memory drop {drop / 2 ** 20:9.1f} MiB; the two one-hot inputs are {onehot_bytes / 2 ** 20:.1f} MiB "
        f"({'at least' if drop >= onehot_bytes else 'LESS THAN'} that; {(drop - onehot_bytes) / 2 ** 20:+.1f} MiB beyond)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, choices=["operator", "step"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    try:
        if args.only in (None, "operator"):
            operator(args.reps, dev)
        if args.only in (None, "step"):
            step(args.reps, dev)
    finally:
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
