"""The two kernels of the deterministic evaluation harness (pulpo_amd.evaluation) against the composed routes they replace, on the GPU.

    python scripts/performance_bench.py [--reps 20] [--labels blocks|iid]

At 160^3 and 192 x 224 x 160 (the T6 / L5 shape), one pair (B = 1), same process, alternating new / composed per case.
  field_quality    ops.field_quality(df)                                  against  jacobian_det + jdet_std + percent_leq0
  soft Dice        ops.warp_labels_soft_dice(df, labels, C, target)       against  warp3d on the one-hot map + resize_trilinear of the one-hot
                   C in {5, 36}, uint8 labels, at level 0 (grid = map)             target (skipped at grid = map, as HierarchicalReconstructionLoss
                   and at level 1 (grid = map / 2)                                 does) + soft_dice_loss; the one-hot inputs are built outside the
                                                                                   timed region
--labels blocks (default): every 8^3 block of a map carries one random class, regions like a parcellation's; iid: every voxel its own class,
the worst case of the class exchange (a wave then meets up to C classes).
Bytes counted (V voxels of the grid, M = min(map voxels, 8 V) label or one-hot elements gathered, l = 1 byte per label):
  field_quality    12 V (the field, once)                 composed  36 V: 16 V (field read, map written) twice - jdet_std recomputes the map -
                                                                    and 4 V (percent_leq0 reads it)
  soft Dice        12 V + 2 l M                           composed  12 V + 4 C M + 4 C V (warp3d), 4 C M + 4 C V (resize, grid != map), 8 C V (Dice)
Reported: median ms over --reps with the 10 % / 90 % quantiles, GB/s of the counted bytes, the fraction of the byte floor (counted bytes at
the device-to-device copy rate measured in the same run), and for the soft Dice the peak device memory each route adds on top of the label
maps (the composed route's two one-hot inputs included).
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


def copy_rate(reps: int) -> float:
    """bytes/s of a 2 GiB device-to-device copy (read + write counted)"""
    src = torch.empty(1 << 29, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    (ms, _, _), _ = timed_pair(lambda: dst.copy_(src), lambda: None, reps)
    return 2.0 * src.numel() * 4 / (ms * 1e-3)


def peak_added(fn) -> float:
    """MiB of device memory fn() adds at its peak"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def one_hot(lab, C):
    return F.one_hot(lab[:, 0].long(), C).permute(0, 4, 1, 2, 3).float().contiguous()


def row(name, size, extra, new, old, bn, bo, bw):
    (tn, n10, n90), (to, o10, o90) = new, old
    print(f"{name:>13} {'x'.join(map(str, size)):>13} {extra:>14} | {tn:8.3f} [{n10:7.3f} {n90:7.3f}] {bn / tn / 1e6:6.0f} {bn / bw / (tn * 1e-3):5.2f} | "
          f"{to:8.3f} [{o10:7.3f} {o90:7.3f}] {bo / to / 1e6:6.0f} {bo / bw / (to * 1e-3):5.2f} | {bn / bo:6.3f} {to / tn:6.1f}x")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--labels", default="blocks", choices=["blocks", "iid"])
    args = ap.parse_args()
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    bw = copy_rate(args.reps)
    print(f"device-to-device copy: {bw / 1e9:.0f} GB/s (the byte floor below is counted at this rate); labels: {args.labels}; reps: {args.reps}")
    print(f"{'kernel':>13} {'grid':>13} {'case':>14} | {'new ms':>8} [{'p10':>7} {'p90':>7}] {'GB/s':>6} {'floor':>5} | {'route ms':>8} [{'p10':>7} {'p90':>7}] "
          f"{'GB/s':>6} {'floor':>5} | {'bytes':>6} {'speed':>7}")
    g = torch.Generator(device="cuda").manual_seed(0)

    def labels(C, size):
        if args.labels == "iid":
            return torch.randint(0, C, (1, 1) + size, device=dev, generator=g).to(torch.uint8)
        coarse = torch.randint(0, C, (1, 1) + tuple(s // 8 for s in size), device=dev, generator=g)
        return coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4).to(torch.uint8).contiguous()

    memory = []
    with torch.no_grad():
        for size in ((160, 160, 160), (192, 224, 160)):
            Vm = size[0] * size[1] * size[2]
            # ---- field quality, at the full size and at the level below
            for grid in (size, tuple(s // 2 for s in size)):
                V = grid[0] * grid[1] * grid[2]
                df = 2.0 * torch.randn((1, 3) + grid, device=dev, generator=g)

                def composed_fq():
                    ops.percent_leq0(ops.jacobian_det(df, True))
                    ops.jdet_std(df, 1.0, True)

                new, old = timed_pair(lambda: ops.field_quality(df, True), composed_fq, args.reps)
                row("field_quality", grid, "", new, old, 12 * V, 36 * V, bw)
            # ---- soft Dice, level 0 (grid = map) and level 1 (grid = map / 2)
            for C in (5, 36):
                lab, tgt = labels(C, size), labels(C, size)
                for grid in (size, tuple(s // 2 for s in size)):
                    V = grid[0] * grid[1] * grid[2]
                    M = min(Vm, 8 * V)
                    df = 2.0 * torch.randn((1, 3) + grid, device=dev, generator=g)
                    oh, toh = one_hot(lab, C), one_hot(tgt, C)

                    def composed_dice(oh=oh, toh=toh):
                        t = toh if grid == size else ops.resize_trilinear(toh, grid)
                        return ops.soft_dice_loss(ops.warp3d(df, oh), t, 1)

                    new, old = timed_pair(lambda: ops.warp_labels_soft_dice(df, lab, C, tgt), composed_dice, args.reps)
                    b_new = 12 * V + 2 * M
                    b_old = 12 * V + 4 * C * M + 4 * C * V + (4 * C * M + 4 * C * V if grid != size else 0) + 8 * C * V
                    row("soft Dice", grid, f"C={C} map {size[0]}", new, old, b_new, b_old, bw)
                    fused, route = float(ops.warp_labels_soft_dice(df, lab, C, tgt)[1]), 1.0 - float(composed_dice()) / V
                    assert abs(fused - route) <= 1e-5 * abs(route), (fused, route)                 # faster and different is not faster
                    del oh, toh
                    m_new = peak_added(lambda: ops.warp_labels_soft_dice(df, lab, C, tgt))
                    m_old = peak_added(lambda: composed_dice(one_hot(lab, C), one_hot(tgt, C)))
                    memory.append(f"{'x'.join(map(str, grid)):>13} C={C:>2} map {'x'.join(map(str, size))}: peak added memory {m_new:9.2f} MiB new, "
                                  f"{m_old:9.1f} MiB composed (one-hot inputs included)")
                    torch.cuda.empty_cache()
    print("\nsoft Dice, device memory added on top of the two label maps and the field")
    print("\n".join(memory))


if __name__ == "__main__":
    main()
