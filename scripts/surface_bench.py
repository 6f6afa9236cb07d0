"""Distance transform and surface distances (pulpo_edt_sq, pulpo_surface_distances) against their byte floor, on the GPU.

    python scripts/surface_bench.py [--reps 20] [--perf-reps 5] [--no-model]

For 160^3 and 192 x 224 x 160, C in {4, 36}, uint8 labels, one pair (B = 1).  Labels: every 8^3 block of the fixed map carries one random
class, a map with regions like a parcellation's; the moving map is that map warped (arg-max) through a field of the size
synthetic.oasis_like_pair uses (U[-3, 3] voxels on a size/16 lattice, up-sampled), and is scored against the unwarped map.
Bytes counted (V voxels, l = 1 byte per label, bins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1), the implementation's own passes:
  edt_sq              V (mask) + 4 V (row pass out) + 8 V (pass along H, in place) + 8 V (pass along D)                       = 21 V
  surface_distances   per class and direction: l V + 4 V (row pass) + 8 V (along H) + 4 V + l V (along D, evaluated on the other
                      map's surface: nothing written but histogram counts) = 16 V + 2 l V; two directions, C classes; + the histograms
                      zeroed and read once (16 C bins)
Reported: median ms over --reps after a warm-up call, GB/s of the counted bytes, the byte floor (counted bytes at the device-to-device
copy rate measured in the same run) and the ratio of the measured time to it.  Then the added time of performance(surface=True) over
performance with segmentations on the flagship model (T5 / L4, n0 = 32), eval mode.  With scipy, the host time of ONE class's two
transforms (scipy.ndimage.distance_transform_edt of the two surfaces), for scale.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--perf-reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="skip the performance() part")
    args = ap.parse_args()
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    bw = copy_rate(args.reps)
    print(f"device-to-device copy: {bw / 1e9:.0f} GB/s (the byte floor below is counted at this rate)")
    g = torch.Generator(device="cuda").manual_seed(0)

    def block_labels(C, size):
        coarse = torch.randint(0, C, (1, 1) + tuple(s // 8 for s in size), device=dev, generator=g)
        return coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4).to(torch.uint8).contiguous()

    def field(size):
        lattice = (torch.rand((1, 3) + tuple(max(s // 16, 2) for s in size), device=dev, generator=g) * 2 - 1) * 3.0
        return ops.resize_trilinear(lattice, list(size)).contiguous()

    print(f"{'size':>13} {'C':>3} {'what':>18} {'ms':>9} {'GB/s':>6} {'floor ms':>9} {'ms / floor':>10}   surface voxels (a, b)")
    host = []
    for size in ((160, 160, 160), (192, 224, 160)):
        V = size[0] * size[1] * size[2]
        bins = sum((s - 1) ** 2 for s in size) + 1
        df = field(size)
        for C in (4, 36):
            fixed = block_labels(C, size)
            moving = ops.warp_labels(df, fixed, C, argmax=True)
            mask = (moving == 1)
            with torch.no_grad():
                t_edt = timed(lambda: ops.edt_sq(mask), args.reps)
                t_sd = timed(lambda: ops.surface_distances(moving, fixed, C), args.reps)
                res = ops.surface_distances(moving, fixed, C)
            b_edt = 21 * V
            b_sd = C * 2 * (16 * V + 2 * V) + 16 * C * bins
            n_a, n_b = int(res["n_a"].sum()), int(res["n_b"].sum())
            for what, t, nb in (("edt_sq", t_edt, b_edt), ("surface_distances", t_sd, b_sd)):
                floor = nb / bw * 1e3
                print(f"{'x'.join(map(str, size)):>13} {C:>3} {what:>18} {t:9.3f} {nb / t / 1e6:6.0f} {floor:9.3f} {t / floor:10.1f}   "
                      + (f"{n_a}, {n_b}" if what == "surface_distances" else ""))
            if C == 4:
                host.append((size, moving.cpu().numpy()[0, 0], fixed.cpu().numpy()[0, 0]))
        del df
        torch.cuda.empty_cache()

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        print("\nhost, scipy.ndimage.distance_transform_edt: ONE class (class 1 of the C = 4 maps), its two surfaces' transforms")
        for size, a, b in host:
            t0 = time.perf_counter()
            for lab in (a, b):
                m = lab == 1
                s = m & ~ndimage.binary_erosion(m)
                ndimage.distance_transform_edt(~s)
            print(f"{'x'.join(map(str, size)):>13}: {time.perf_counter() - t0:6.2f} s for one class (the device rows above cover all C classes)")

    if args.no_model:
        return
    import src.models as models
    from pulpo_amd.evaluation import performance
    print("\nperformance(), flagship model (T5/L4, n0 = 32), eval: added time of surface=True over the call with segmentations alone")
    for size in ((160, 160, 160), (192, 224, 160)):
        torch.manual_seed(0)
        model = models.PULPo(5, 4, 0.1, list(size), feedback=FEEDBACK, n0=32).to(dev).eval()
        x, y = torch.rand((1, 1) + size, device=dev, generator=g), torch.rand((1, 1) + size, device=dev, generator=g)
        for C in (4, 36):
            sy = block_labels(C, size)
            sx = ops.warp_labels(field(size), sy, C, argmax=True)
            plain = timed(lambda: performance(model, x, y, seg_x=sx, seg_y=sy, num_classes=C), args.perf_reps)
            surf = timed(lambda: performance(model, x, y, seg_x=sx, seg_y=sy, num_classes=C, surface=True), args.perf_reps)
            print(f"{'x'.join(map(str, size)):>13} C={C:>2}: {plain:8.1f} ms without, {surf:8.1f} ms with -> {surf - plain:6.2f} ms added "
                  f"({(surf - plain) / plain * 100:5.1f} %)")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
