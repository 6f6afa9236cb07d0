"""ops.augment beside its byte floor and beside the same transform written in ATen, and the 160^3 training step with and without an
AugmentedLoader, on the GPU.

    python scripts/augment_bench.py [--reps 30] [--size 160] [--step-limit 120] [--out profiles/augment_bench.txt]

One sample (B = 1) of --size^3 with an image, a float mask and a uint8 label map, and the full transform: an affine (rotations of 10 degrees,
scales of 10 %, shifts of 4 voxels), an elastic part (lattice spacing 16, N(0, 1.5^2) voxels) and every intensity piece (gamma, a 4^3 log-bias
lattice, gain / offset, noise, clip).  One process, after a warm-up, the routes alternating; median ms over --reps with the 10 % / 90 %
quantiles (device events around each call):
  fused    ops.augment(img, mask, labels, ...): one launch; counted bytes = those of its own ops._hbm_end accounting (the sources read once,
           the results written once: 18 N for N voxels)
  floor    the counted bytes over the device-copy rate, measured in the same run the way scripts/bn_bandwidth.py measures it (Tensor.copy_ between
           two 32 x 160^3 fp32 tensors, read + write counted); `small copy` is the same between two tensors of the fused route's own size
  ATen     the usual chain: the lattice expanded by three dense matrix products, a dense sampling grid, grid_sample per tensor (bilinear twice,
           nearest on a float copy of the labels), pow / exp of an interpolated bias lattice / randn_like / clamp
Before anything is timed the two routes are compared: image without the noise term, mask, and the share of label voxels that differ (positions
that round differently in the two fp32 coordinate chains).
Then the 160^3 / T5 / L4 / n0 = 32 training step (dp.DataParallelStepper, B = 1, NCC) on a batch with label maps and masks: stepper.step(batch)
against stepper.step(augmenter(batch)), alternating; and the augmenter's call alone.  Nothing of the step itself changed with the augmentation:
the plain figure is what the parent commit's step measures on the same box.
Every stage runs under its own time limit (SIGALRM with the default action ends the process), and the first failure ends the script: nothing
is started on the GPU after it.
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
import torch.nn.functional as F  # noqa: E402

FEEDBACK = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
LINES = []


def say(line: str = "") -> None:
    print(line, flush=True)
    LINES.append(line)


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


def bspline_matrix(S: int, G: int, s: int, dev):
    """(S, G) fp32: row z holds the four cubic B-spline basis values of voxel z at columns z // s + l"""
    z = torch.arange(S, device=dev)
    i = z // s
    u = z.float() / s - i.float()
    m = 1 - u
    basis = (m ** 3 / 6, (3 * u ** 3 - 6 * u ** 2 + 4) / 6, (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) / 6, u ** 3 / 6)
    A = torch.zeros(S, G, device=dev)
    for l, w in enumerate(basis):
        ok = i + l < G
        A[z[ok], (i + l)[ok]] = w[ok]
    return A


def operator(args, dev) -> None:
    from pulpo_amd import ops
    from pulpo_amd.augment import Augmenter
    S = args.size
    size = (S, S, S)
    N = S ** 3
    aug = Augmenter(size, seed=1, rotate_deg=10.0, scale=0.1, translate_vox=4.0, elastic_spacing=16, elastic_std_vox=1.5, gamma=0.3, gain=0.1,
                    offset=0.05, noise_std=0.05, bias_std=0.3, bias_nodes=4)
    m = Augmenter.to_device(aug.draw(1), dev)["x"]
    theta, phi, s, cfg = m["theta"], m["phi"], m["spacing"], m["intensity"]
    g = torch.Generator(device="cuda").manual_seed(0)
    img = ops.resize_trilinear(torch.rand((1, 1, S // 8, S // 8, S // 8), device=dev, generator=g), size).contiguous()
    mask = (torch.rand((1, 1) + size, device=dev, generator=g) > 0.3).float()
    lab = torch.randint(0, 36, (1, 1) + size, device=dev, generator=g, dtype=torch.uint8)
    mats = [bspline_matrix(S, G, s, dev) for G in phi.shape[2:]]
    base = torch.stack(torch.meshgrid(*[torch.arange(S, device=dev, dtype=torch.float32) for _ in range(3)], indexing="ij")).unsqueeze(0)
    c = (S - 1) / 2

    def fused(intensity=cfg):
        return ops.augment(img, mask, lab, theta=theta, phi=phi, spacing=s, intensity=intensity)

    def aten(noise: bool = True):
        e = torch.einsum("bcijk,zi,yj,xk->bczyx", phi, *mats)
        q = base + e - c
        p = torch.einsum("bij,bjzyx->bizyx", theta[:, :, :3], q) + theta[:, :, 3].view(1, 3, 1, 1, 1) + c
        grid = (p * (2.0 / (S - 1)) - 1).flip(1).permute(0, 2, 3, 4, 1)
        r = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        mk = F.grid_sample(mask, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        lb = F.grid_sample(lab.float(), grid, mode="nearest", padding_mode="zeros", align_corners=True).to(torch.uint8)
        r = r.clamp(0, 1).pow(cfg["gamma"].view(1, 1, 1, 1, 1))
        r = r * torch.exp(F.interpolate(cfg["bias"].unsqueeze(1), size=size, mode="trilinear", align_corners=True))
        r = cfg["gain"].view(1, 1, 1, 1, 1) * r + cfg["offset"].view(1, 1, 1, 1, 1)
        if noise:
            r = r + cfg["sigma"].view(1, 1, 1, 1, 1) * torch.randn_like(r)
        return r.clamp(0, 1), mk, lb

    quiet = {k: v for k, v in cfg.items() if k not in ("sigma", "seed")}
    fi, fm, fl = fused(quiet)
    ai, am, al = aten(noise=False)
    d_img, d_mask = float((fi - ai).abs().max()), float((fm - am).abs().max())
    d_lab = float((fl != al).float().mean())
    assert d_img < 1e-3 and d_mask < 1e-3 and d_lab < 1e-2, (d_img, d_mask, d_lab)           # faster and different is not faster
    say(f"routes agree: image (noise off) to {d_img:.1e}, mask to {d_mask:.1e}, {100 * d_lab:.3f} % of the label voxels differ")

    ops.CONV_TRACE_STRIDE, ops.HBM_TRACE = 1, []
    fused()
    torch.cuda.synchronize()
    trace, ops.HBM_TRACE = ops.HBM_TRACE, None
    assert [t[0] for t in trace] == ["augment_apply"], [t[0] for t in trace]
    counted = trace[0][1]
    big_a, big_b = torch.empty(32 * 160 ** 3, device=dev).normal_(), torch.empty(32 * 160 ** 3, device=dev)
    small_a, small_b = torch.empty(int(counted) // 8, device=dev).normal_(), torch.empty(int(counted) // 8, device=dev)
    stats = timed([fused, aten, lambda: big_b.copy_(big_a), lambda: small_b.copy_(small_a)], args.reps)
    rate = 8.0 * big_a.numel() / stats[2][0]             # bytes per ms
    rate_small = 8.0 * small_a.numel() / stats[3][0]
    floor, floor_small = counted / rate, counted / rate_small
    say(f"ops.augment at {S}^3, B = 1: image + mask + uint8 labels, affine + elastic (s = {s}) + gamma / bias / gain / noise / clip; reps = {args.reps}, "
        f"{torch.cuda.get_device_name(0)}")
    say(f"{'route':>12} | {'ms':>8} [{'p10':>7} {'p90':>7}] | {'counted MB':>10} {'GB/s':>7}")
    for name, (t, a, b), nb in (("fused", stats[0], counted), ("ATen", stats[1], None), ("copy 524 MB", stats[2], 8.0 * big_a.numel()),
                                ("small copy", stats[3], 8.0 * small_a.numel())):
        tail = f"{nb / 1e6:10.1f} {nb / t / 1e6:7.0f}" if nb is not None else f"{'':>10} {'':>7}"
        say(f"{name:>12} | {t:8.3f} [{a:7.3f} {b:7.3f}] | {tail}")
    say(f"byte floor of the fused route: {counted / 1e6:.1f} MB ({counted / N:.0f} bytes per voxel) at the 524 MB copy's rate {rate / 1e6:.0f} GB/s = {floor:.3f} ms "
        f"(fused = {stats[0][0] / floor:.2f} x floor); at the rate of a copy of its own size {rate_small / 1e6:.0f} GB/s = {floor_small:.3f} ms "
        f"({stats[0][0] / floor_small:.2f} x)")
    say(f"fused against ATen: {stats[1][0] / stats[0][0]:.1f} x faster")
    assert stats[0][0] <= stats[1][0], "the fused operator is slower than the ATen route"
    # which of its parts the fused kernel pays for: the same call with pieces left out
    parts = timed([lambda: ops.augment(img, mask, lab), lambda: ops.augment(img, mask, lab, theta=theta),
                   lambda: ops.augment(img, mask, lab, theta=theta, phi=phi, spacing=s), lambda: fused(quiet), fused], args.reps)
    say("fused, by transform: " + ", ".join(f"{n} {t[0]:.3f} ms" for n, t in zip(("identity", "affine", "affine + elastic", "+ intensity without noise", "full"), parts)))


def step(args, dev) -> None:
    from pulpo_amd import dp, synthetic
    from pulpo_amd.augment import Augmenter
    from src.models import PULPo
    size = [160, 160, 160]
    x, y = synthetic.oasis_like_pair(size, 1, 1234, dev)
    g = torch.Generator(device="cuda").manual_seed(2)
    seg = torch.randint(0, 36, (1, 1, *size), device=dev, generator=g, dtype=torch.uint8)
    mask = torch.ones((1, 1, *size), device=dev)
    empty = torch.empty((0,), device=dev)
    batch = (x, y, seg, seg.clone(), empty, empty, mask, mask.clone())
    aug = Augmenter(size, seed=3, rotate_deg=10.0, scale=0.1, translate_vox=4.0, elastic_spacing=16, elastic_std_vox=1.5, gamma=0.3, gain=0.1, offset=0.05,
                    noise_std=0.05, bias_std=0.3)
    torch.manual_seed(0)
    model = PULPo(5, 4, 0.1, size, feedback=FEEDBACK, n0=32).to(dev).train()
    st = dp.DataParallelStepper(model)
    for _ in range(3):
        st.step(batch)
    plain, with_aug, alone = timed([lambda: st.step(batch), lambda: st.step(aug(batch)), lambda: aug(batch)], args.reps)
    say(f"\nstep 160^3 T5 L4 n0=32 NCC, B = 1, batch with uint8 label maps and float masks (2 x (image + mask + labels) augmented per step)")
    say(f"  stepper.step(batch)              {plain[0]:8.2f} ms [{plain[1]:8.2f} {plain[2]:8.2f}]   (the step is unchanged: the parent commit's figure on this box)")
    say(f"  stepper.step(augmenter(batch))   {with_aug[0]:8.2f} ms [{with_aug[1]:8.2f} {with_aug[2]:8.2f}]   (+{with_aug[0] - plain[0]:.2f} ms, {100 * (with_aug[0] / plain[0] - 1):.1f} %)")
    say(f"  augmenter(batch) alone           {alone[0]:8.2f} ms [{alone[1]:8.2f} {alone[2]:8.2f}]   (device events around the call: the draw on the host, "
        f"one staged copy, two launches)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds allowed per stage")
    ap.add_argument("--only", default=None, choices=["operator", "step"])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a ROCm GPU (no CPU path)")
    signal.alarm(args.step_limit)
    from pulpo_amd._lib import lib
    lib.load()
    dev = torch.device("cuda", 0)
    if args.only in (None, "operator"):
        signal.alarm(args.step_limit)
        operator(args, dev)
        torch.cuda.empty_cache()
    if args.only in (None, "step"):
        signal.alarm(args.step_limit)
        step(args, dev)
    signal.alarm(0)
    say("ms: median of device events around one call, routes alternating in one process after a warm-up; [p10 p90] the 10 % / 90 % quantiles.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
