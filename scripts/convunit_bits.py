"""The bits of the ConvUnit kernels, for an A/B of two trees that must compute the same thing (a refactor of the convolution epilogues, the
BatchNorm passes or the 1x1x1 heads).

    python scripts/convunit_bits.py --out a.npz              (on the GPU, from the tree it is started from)
    python scripts/convunit_bits.py --compare a.npz b.npz    (anywhere: array by array with numpy.array_equal, exit status 1 on a difference)

With fixed seeds, through ops._conv_raw: the forward convolution with its statistics rows at test_gpu_pyramid_convunit.STAT_CASES (its own
_call_fwd: every kernel family through the C ABI) and at FORMS (default selection, the operand forms of the step), the data gradient at FORMS,
the data gradient with the BatchNorm-backward reduction at BNRED_CASES (output and rows), the eval-mode fused store at one ragged shape per
Winograd family (from C5 / C2 / C3: the general path and the pipelined kernel's edge masks run) and at the direct kernel's shapes, the round-2
F(2x2,3x3) kernel's plain and eval-mode store through its own entry point (default selection never picks it for an eval-mode store), the
bf16-operand kernel with fp32 and with bf16 storage at one C3 layer, and the five head kernels at test_gpu_heads_bn.CASES.  Only names that an
older tree has (pulpo_amd.ops, lib.call on existing entry points), so the same file runs from there.  None of these kernels adds with
atomics: two trees that evaluate the same float expressions in the same order give equal files.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)


def compare(a_path: str, b_path: str) -> int:
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for name in names:
        if name not in a.files or name not in b.files:
            verdict = "only in " + (a_path if name in a.files else b_path)
        else:
            verdict = "equal" if a[name].shape == b[name].shape and np.array_equal(a[name], b[name], equal_nan=True) else "DIFFERENT"
        bad += verdict != "equal"
        print(f"{verdict:<10} {name}  {tuple(a[name].shape) if name in a.files else ''}")
    print(f"{len(names)} arrays compared with numpy.array_equal, {bad} not equal")
    return 1 if bad else 0


def collect() -> dict:
    import torch
    import test_gpu_heads_bn as TH
    import test_gpu_pyramid_convunit as T
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev, CL, vp, st = "cuda", torch.channels_last_3d, T.vp, ops._stream()
    out = {}

    def keep(name, t):
        # (bf16 tensors as their fp32 values; large outputs as they are - the file stays on the GPU machine's disk)
        out[name] = t.detach().float().cpu().numpy()

    def tag(B, K, N, size):
        return f"B{B}-{K}to{N}-{'x'.join(map(str, size))}"

    def coef_of(g, C):
        mean = torch.randn(C, device=dev, generator=g).double() * 0.3
        rstd = torch.rand(C, device=dev, generator=g).double() + 0.5
        return T.coef_block(mean, rstd, torch.rand(C, device=dev, generator=g).double() + 0.5, torch.randn(C, device=dev, generator=g).double() * 0.5)

    def raw(name, x, w, b, dgrad, stats_rows, coef, dtype=torch.float32):
        """one convolution through ops._conv_raw with the default selection: output, statistics rows"""
        B, _, D, H, W = x.shape
        K, N = (w.shape[0], w.shape[1]) if dgrad else (w.shape[1], w.shape[0])
        wp = ops._pack_weight_now(w, dgrad, (B, D, H, W), register=False)
        y = ops.new_cl(B, N, D, H, W, dev, dtype)
        stats = torch.zeros(stats_rows * 2 * N, device=dev) if stats_rows else None
        ops._conv_raw(x, wp, b, y, K, N, stats, coef)
        keep(name + "/out", y)
        if stats is not None:
            keep(name + "/rows", stats)

    # ---- forward + statistics rows, every family through the C ABI
    for fam, B, Cin, Cout, size, _ in T.STAT_CASES:
        g = T.gen(Cin + Cout + size[0])
        x, w, b, _ = T.conv_data(g, B, Cin, Cout, size, fam == "b")
        x = x.contiguous(memory_format=CL) if Cin > 4 else x
        nrow = lib.query("pulpo_conv3d_k3_fwd_bf16_stat_tiles" if fam == "b" else "pulpo_conv3d_k3_stat_tiles", B, *size)
        stats = torch.zeros(nrow * 2 * Cout, device=dev)
        y, _ = T._call_fwd(ops, fam, x, w, b, stats)
        keep(f"stat/{fam}/{tag(B, Cin, Cout, size)}/out", y)
        keep(f"stat/{fam}/{tag(B, Cin, Cout, size)}/rows", stats)

    # ---- forward (with rows) and data gradient at the operand forms, through ops._conv_raw
    for B, Cin, Cout, size, form, *_ in T.FORMS:
        if not isinstance(form, str):
            continue                                     # (the 2^31-byte gate cases: 5 GB buffers, the same kernels as "aligned" / "unaligned")
        g = T.gen(B * 1000 + Cin * 10 + Cout + size[0] + size[2])
        x, w, b, dy = T.conv_data(g, B, Cin, Cout, size, False)
        xo, dyo = T.operand(x, form, g), T.operand(dy, form, g)
        if form == "unaligned":                          # (what ops.conv3d_k3 hands to _conv_raw where the kernels cannot take the slice)
            xo, dyo = ops.as_grid(xo), ops.as_grid(dyo)
        nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
        name = f"form/{form}/{tag(B, Cin, Cout, size)}"
        try:
            raw(name + "/fwd", xo, w, b, False, nrow, None)
            raw(name + "/dgrad", dyo, w, None, True, 0, None)
        except Exception as e:                           # an operand form _conv_raw refuses is refused by both trees: recorded as such
            out[name + "/refused"] = np.array([len(str(e)) > 0])

    # ---- data gradient with the BatchNorm-backward reduction
    for entry, B, K, N, size in T.BNRED_CASES:
        g = T.gen(K + N + size[0] + B)
        dy, w, _, _ = T.conv_data(g, B, K, N, size, False)
        dy, w = dy + 1.0, w + 1.0 / (27 * K)
        wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()
        ybn = (torch.randn(B, N, *size, device=dev, generator=g) * 1.5 + 0.3).contiguous(memory_format=CL)
        coef = coef_of(g, N)
        kind = "wino2" if entry == "wino2" else "wino3"
        wp = torch.empty(lib.query(f"pulpo_conv3d_k3_packed_{kind}_floats", K, N), device=dev)
        lib.call(f"pulpo_conv3d_k3_pack_weight_{kind}", vp(wt), vp(wp), N, K, 1, st)
        dyc = dy.contiguous(memory_format=CL)
        dx = torch.zeros((B, *size, N), device=dev).permute(0, 4, 1, 2, 3)
        nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
        part = torch.zeros(nrow * 2 * N, device=dev)
        ds, xs, ys = ops.grid_strides(dyc), ops.grid_strides(dx), ops.grid_strides(ybn)
        if entry == "wino3_kb":
            V = size[0] * size[1] * size[2]
            dkb = dy.reshape(B, K // 8, 8, *size).permute(1, 0, 3, 4, 5, 2).contiguous()
            lib.call("pulpo_conv3d_k3_dgrad_wino3_bnred_kb", vp(dkb), V * 8, 8, B * V * 8, vp(wp), vp(dx), xs[0], xs[1], 8, vp(ybn), ys[0], ys[1], vp(coef), 0.2,
                     vp(part), B, *size, K, N, st)
        else:
            lib.call(f"pulpo_conv3d_k3_dgrad_{entry}_bnred", vp(dyc), *ds, vp(wp), vp(dx), xs[0], xs[1], vp(ybn), ys[0], ys[1], vp(coef), 0.2, vp(part),
                     B, *size, K, N, st)
        keep(f"bnred/{entry}/{tag(B, K, N, size)}/out", dx)
        keep(f"bnred/{entry}/{tag(B, K, N, size)}/rows", part)

    # ---- eval-mode fused store (and, without it, the plain store with rows) at ragged shapes of every family and a whole-tile shape each
    ragged = [T.C5[18], T.C5[15], T.C2[11], T.C5[24], T.C3[8], T.C2[5], T.C5[21], T.C5[28], T.C3[0]]
    for i, (B, Cin, Cout, size, *_fam) in enumerate(ragged):
        if size[0] >= 96:
            size = (size[0] // 4, size[1] // 4 + 1, size[2] // 4 + 3)      # (the full-resolution input layer's kernels at a small ragged volume)
        g = T.gen(900 + i)
        x, w, b, dy = T.conv_data(g, B, Cin, Cout, size, False)
        x = x.contiguous(memory_format=CL) if Cin > 4 else x
        nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
        fam = T.family(B, size, Cin, Cout)
        name = f"ragged/{fam}/{tag(B, Cin, Cout, size)}"
        raw(name + "/fwd", x, w, b, False, nrow, None)
        raw(name + "/eval", x, w, b, False, 0, coef_of(g, Cout))
        raw(name + "/dgrad", dy.contiguous(memory_format=CL), w, None, True, 0, None)

    # ---- the round-2 F(2x2,3x3) kernel (default selection passes it only what the pipelined kernel refuses): eval-mode fused store and plain store
    # with rows through its entry point, channels-last with K % 8 != 0 (vector staging) and planar (scalar staging), ragged and whole tiles
    for i, (B, Cin, Cout, size, planar_x) in enumerate([(1, 20, 32, (24, 28, 20), False), (2, 32, 48, (24, 28, 20), True), (1, 20, 32, (24, 24, 24), False)]):
        g = T.gen(950 + i)
        x, w, b, _ = T.conv_data(g, B, Cin, Cout, size, False)
        x = x.contiguous() if planar_x else x.contiguous(memory_format=CL)
        wp = torch.empty(lib.query("pulpo_conv3d_k3_packed_wino2_floats", Cin, Cout), device=dev)
        lib.call("pulpo_conv3d_k3_pack_weight_wino2", vp(w.contiguous()), vp(wp), Cin, Cout, 0, st)
        n = lib.query("pulpo_conv3d_k3_fwd_wino2_scratch_floats", B, *size, Cin, Cout)
        scr = torch.zeros(n, device=dev) if n else None
        nrow = lib.query("pulpo_conv3d_k3_stat_tiles", B, *size)
        for mode, coef in (("fwd", None), ("eval", coef_of(g, Cout))):
            y = torch.zeros((B, *size, Cout), device=dev).permute(0, 4, 1, 2, 3)
            stats = torch.zeros(nrow * 2 * Cout, device=dev) if coef is None else None
            lib.call("pulpo_conv3d_k3_fwd_wino2", vp(x), *ops.grid_strides(x), vp(wp), vp(b), vp(coef), 0.2, vp(y), *ops.grid_strides(y), vp(stats), vp(scr),
                     B, *size, Cin, Cout, st)
            keep(f"wino2/{'planar' if planar_x else 'cl'}/{tag(B, Cin, Cout, size)}/{mode}/out", y)
            if stats is not None:
                keep(f"wino2/{'planar' if planar_x else 'cl'}/{tag(B, Cin, Cout, size)}/{mode}/rows", stats)

    # ---- bf16-operand kernel, fp32 and bf16 storage
    B, Cin, Cout, size = T.C3[11][:4]
    g = T.gen(4096)
    x, w, b, _ = T.conv_data(g, B, Cin, Cout, size, True)
    nrow = lib.query("pulpo_conv3d_k3_fwd_bf16_stat_tiles", B, *size)
    for act in ("fp32", "bf16"):
        ops.set_conv_precision("bf16", activations=act)
        try:
            dt = torch.bfloat16 if act == "bf16" else torch.float32
            xb = x.to(dt).contiguous(memory_format=CL)
            raw(f"bf16/{act}/{tag(B, Cin, Cout, size)}/fwd", xb, w, b, False, nrow, None, dt)
            raw(f"bf16/{act}/{tag(B, Cin, Cout, size)}/eval", xb, w, b, False, 0, coef_of(g, Cout), dt)
        finally:
            ops.set_conv_precision("fp32")

    # ---- the five head kernels
    for B, C, size, nout, with_eps, off in TH.CASES:
        D, H, W = size
        V, npix = D * H * W, B * D * H * W
        g = T.gen(7 * C + 3 * D + B + nout)
        name = f"heads/B{B}-C{C}-{'x'.join(map(str, size))}-nout{nout}-eps{int(with_eps)}-off{off}"
        y = TH._like(B, C, size, off, 0.0)
        y.copy_(torch.randn(B, C, *size, device=dev, generator=g) * 1.5 + 0.3)
        coef = coef_of(g, C).contiguous()
        Wt = torch.randn(nout, C, device=dev, generator=g) / C ** 0.5
        hb = torch.randn(nout, device=dev, generator=g)
        eps = torch.randn(B, 3, *size, device=dev, generator=g) if with_eps else None
        gs = [torch.randn(B, 3, *size, device=dev, generator=g) for _ in range(3 if nout == 6 else 1)] + [None] * (0 if nout == 6 else 2)
        totd = torch.randn(2 * C, device=dev, generator=g).double() * 0.01
        yps = y.stride(4)
        z = TH._like(B, C, size, off, 0.0)
        lib.call("pulpo_bn_lrelu_apply", vp(y), yps, vp(z), z.stride(4), vp(coef), npix, C, 0.2, st)
        zeros = lambda: torch.zeros((B, 3, *size), device=dev)
        o_sep, o_fus = [zeros() for _ in range(3)], [zeros() for _ in range(3)]
        lib.call("pulpo_heads_fwd", vp(z), z.stride(4), vp(Wt), vp(hb), vp(eps), *(vp(t) for t in o_sep), nout, B, V, C, st)
        lib.call("pulpo_heads_fwd_bn_t", vp(y), yps, vp(coef), 0.2, vp(Wt), vp(hb), vp(eps), *(vp(t) for t in o_fus), nout, B, V, C, st)
        sigma = o_sep[1] if nout == 6 else None
        hblk = lib.query("pulpo_heads_bwd_blocks", B, V, C)
        rowlen = nout * C + nout
        dz = TH._like(B, C, size, off, 0.0)
        p_sep, p_fus, bnpart = torch.zeros(hblk * rowlen, device=dev), torch.zeros(hblk * rowlen, device=dev), torch.zeros(hblk * 2 * C, device=dev)
        lib.call("pulpo_heads_bwd", vp(z), z.stride(4), vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma), vp(dz), dz.stride(4), vp(p_sep), nout, B, V, C, st)
        lib.call("pulpo_heads_bwd_bn_t", vp(y), yps, vp(coef), 0.2, vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma), vp(p_fus), vp(bnpart),
                 nout, B, V, C, st)
        ablk = lib.query("pulpo_bn_bwd_blocks", npix, C)
        dyt, p2 = TH._like(B, C, size, off, 0.0), torch.zeros(ablk * C, device=dev)
        lib.call("pulpo_bn_lrelu_bwd_apply_heads_t", vp(y), yps, vp(coef), vp(totd), 0.2, vp(Wt), vp(gs[0]), vp(gs[1]), vp(gs[2]), vp(eps), vp(sigma), vp(dyt),
                 dyt.stride(4), vp(p2), nout, B, V, C, st)
        for k in range(3 if nout == 6 else 1):
            keep(f"{name}/fwd{k}", o_sep[k])
            keep(f"{name}/fwd_bn{k}", o_fus[k])
        for label, t in (("bwd/dh", dz), ("bwd/rows", p_sep), ("bwd_bn/rows", p_fus), ("bwd_bn/bnrows", bnpart), ("apply_heads/dy", dyt), ("apply_heads/rows", p2)):
            keep(f"{name}/{label}", t)
    torch.cuda.synchronize()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the arrays of this tree to this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), default=None, help="compare two such files")
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(*args.compare))
    if not args.out:
        raise SystemExit("convunit_bits: --out FILE.npz or --compare A.npz B.npz")
    arrays = collect()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    print(f"convunit_bits: {len(arrays)} arrays from {ROOT} -> {args.out}")


if __name__ == "__main__":
    main()
