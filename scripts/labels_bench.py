"""Label-map warp (pulpo_warp_labels) against the one-hot route, on the GPU.

    python scripts/labels_bench.py [--reps 20] [--samples 4] [--labels blocks|iid]

For 160^3 and 192 x 224 x 160, C in {4, 36}, uint8 labels, one pair (B = 1).  --labels blocks (default): every 8^3 block of the map carries
one random class, a map with regions like a parcellation's; iid: every voxel its own random class, the worst case of the Dice exchange
(a wave then meets up to C distinct classes).
  fused   one pulpo_warp_labels launch per sample: Dice sums alone, then Dice sums + the per-class Welford update (LabelMoments.update)
  route   the same results from a one-hot map (the one-hot input is built once and not timed): warp3d(df, one_hot) + dsc, then
          + StreamingMoments.update
Bytes counted per sample (V voxels, l = 1 byte per label):
  fused Dice     12 V (field) + l V (label gathers, the corners shared between neighbours served from cache) + l V (target)
  route Dice     12 V + 4 C V (one-hot gathers) + 4 C V (warped map written) + 8 C V (dsc reads map and one-hot target)
  + moments      fused + 16 C V (mean, M2 read and written); route + 20 C V (sample read, mean, M2 read and written)
Reported: median ms over --reps, GB/s of the counted bytes, and the fraction of the byte floor (counted bytes at the device-to-device copy
rate measured in the same run).  Then the added per-sample cost inside mc_uncertainty (seg_x / seg_y extras against none) on the
flagship model (T5 / L4, n0 = 32), eval mode, --samples samples.
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

FEEDBACK = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]     # bench.py's


def timed(fn, reps: int) -> float:
    """median wall time of fn() in ms, GPU events around each call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def copy_rate(reps: int) -> float:
    """bytes/s of a 2 GiB device-to-device copy (read + write counted)"""
    src = torch.empty(1 << 29, device="cuda", dtype=torch.float32)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), reps)
    return 2.0 * src.numel() * 4 / (ms * 1e-3)


def byte_model(V: int, C: int, moments: bool):
    fused = 12 * V + 2 * V + (16 * C * V if moments else 0)
    route = 12 * V + 16 * C * V + (20 * C * V if moments else 0)
    return fused, route


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--labels", default="blocks", choices=["blocks", "iid"])
    args = ap.parse_args()
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    bw = copy_rate(args.reps)
    print(f"device-to-device copy: {bw / 1e9:.0f} GB/s (the byte floor below is counted at this rate)")
    print(f"{'size':>13} {'C':>3} {'what':>16} {'fused ms':>9} {'GB/s':>6} {'floor':>6} {'route ms':>9} {'GB/s':>6} {'floor':>6} {'speed-up':>8}")
    g = torch.Generator(device="cuda").manual_seed(0)

    def labels(C, size):
        if args.labels == "iid":
            return torch.randint(0, C, (1, 1) + size, device=dev, generator=g).to(torch.uint8)
        coarse = torch.randint(0, C, (1, 1) + tuple(s // 8 for s in size), device=dev, generator=g)
        return coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4).to(torch.uint8).contiguous()

    print(f"labels: {args.labels}")
    for size in ((160, 160, 160), (192, 224, 160)):
        V = size[0] * size[1] * size[2]
        df = 2.0 * torch.randn((1, 3) + size, device=dev, generator=g)
        for C in (4, 36):
            lab, tgt = labels(C, size), labels(C, size)
            oh = F.one_hot(lab[:, 0].long(), C).permute(0, 4, 1, 2, 3).float().contiguous()
            toh = F.one_hot(tgt[:, 0].long(), C).permute(0, 4, 1, 2, 3).float().contiguous()
            dice = torch.empty((1, C), device=dev)
            mean, m2 = torch.empty((1, C) + size, device=dev), torch.empty((1, C) + size, device=dev)
            flag = torch.zeros(3, device=dev, dtype=torch.int32)
            sm = ops.StreamingMoments()
            state = {"k": 0}

            def fused_dice():
                ops._warp_labels_raw(df, lab, C, tgt, None, None, dice, None, None, 1, flag, 0)

            def fused_mom():
                state["k"] += 1
                ops._warp_labels_raw(df, lab, C, tgt, None, None, dice, mean, m2, state["k"], flag, 0)

            def route_dice():
                ops.dsc(ops.warp3d(df, oh), toh)

            def route_mom():
                w = ops.warp3d(df, oh)
                ops.dsc(w, toh)
                sm.update(w)

            with torch.no_grad():
                for what, f, r, mom in (("dice", fused_dice, route_dice, False), ("dice + moments", fused_mom, route_mom, True)):
                    tf, tr = timed(f, args.reps), timed(r, args.reps)
                    bf, br = byte_model(V, C, mom)
                    print(f"{'x'.join(map(str, size)):>13} {C:>3} {what:>16} {tf:9.3f} {bf / tf / 1e6:6.0f} {bf / bw / (tf * 1e-3):6.2f} "
                          f"{tr:9.3f} {br / tr / 1e6:6.0f} {br / bw / (tr * 1e-3):6.2f} {tr / tf:7.1f}x")
            del oh, toh, mean, m2
            torch.cuda.empty_cache()

    # added per-sample cost inside mc_uncertainty
    import src.models as models
    from pulpo_amd.uncertainty import mc_uncertainty
    N = args.samples
    print(f"\nmc_uncertainty, flagship model (T5/L4, n0 = 32), eval, N = {N}: added cost of seg_x / seg_y per sample")
    for size in ((160, 160, 160), (192, 224, 160)):
        torch.manual_seed(0)
        model = models.PULPo(5, 4, 0.1, list(size), feedback=FEEDBACK, n0=32).to(dev).eval()
        x, y = torch.rand((1, 1) + size, device=dev, generator=g), torch.rand((1, 1) + size, device=dev, generator=g)
        plain = timed(lambda: mc_uncertainty(model, x, y, N), 3)
        for C in (4, 36):
            sx, sy = labels(C, size), labels(C, size)
            ext = timed(lambda: mc_uncertainty(model, x, y, N, seg_x=sx, seg_y=sy, num_classes=C), 3)
            print(f"{'x'.join(map(str, size)):>13} C={C:>2}: {plain:8.1f} ms without, {ext:8.1f} ms with -> {(ext - plain) / N:6.2f} ms per sample "
                  f"({(ext - plain) / plain * 100:5.1f} %)")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
