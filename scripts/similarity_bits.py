"""The bits of the similarity terms, for an A/B of two trees that must compute the same thing (a refactor of the NCC / MSE / MIND operators).

    python scripts/similarity_bits.py --out a.npz              (on the GPU, from the tree it is started from)
    python scripts/similarity_bits.py --compare a.npz b.npz    (anywhere: array by array with numpy.array_equal, exit status 1 on a difference)

With fixed seeds: value and gradient (upstream 1.7) of ops.ncc_loss, ncc_loss_masked (one and two masks), l2_loss, l2_loss_masked, rmse_masked
(with its MaskFrac), mind_loss and mind_loss_masked at every entry of test_gpu_masks.CASES (one channel; the MIND terms where every extent is
at least 2, which the kernel asks for), the squared-difference terms at test_gpu_masks.SQ_CASES with 1 and 3 channels, and all but MIND at
the 2-D shape (2, 1, 20, 130).  Only public names of pulpo_amd.ops are used, so the same file runs from an older tree.  None of these kernels
adds with atomics: two trees that evaluate the same float expressions in the same order give equal files.
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
            verdict = "equal" if a[name].shape == b[name].shape and np.array_equal(a[name], b[name]) else "DIFFERENT"
        bad += verdict != "equal"
        print(f"{verdict:<10} {name}  {tuple(a[name].shape) if name in a.files else ''}")
    print(f"{len(names)} arrays compared with numpy.array_equal, {bad} not equal")
    return 1 if bad else 0


def collect() -> dict:
    import torch
    import test_gpu_masks as T
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    dev = "cuda"
    gamma = 0.05
    out = {}

    def record(name, fn, x):
        xg = x.clone().requires_grad_(True)
        res = fn(xg)
        val, extra = (res[0], res[1:]) if isinstance(res, tuple) else (res, ())
        grad, = torch.autograd.grad(val, [xg], grad_outputs=torch.tensor(1.7, device=dev))
        out[name + "/value"] = val.detach().cpu().numpy()
        out[name + "/grad"] = grad.cpu().numpy()
        for i, e in enumerate(extra):
            out[f"{name}/extra{i}"] = e.detach().cpu().numpy()

    def sqdiff_terms(tag, a, b, m1, m2):
        record(f"l2_loss/{tag}", lambda x: ops.l2_loss(x, b), a)
        record(f"l2_loss_masked(1)/{tag}", lambda x: ops.l2_loss_masked(x, b, m1), a)
        record(f"l2_loss_masked(2)/{tag}", lambda x: ops.l2_loss_masked(x, b, m1, m2), a)
        record(f"rmse_masked(1)/{tag}", lambda x: ops.rmse_masked(x, b, m1), a)
        record(f"rmse_masked(2)/{tag}", lambda x: ops.rmse_masked(x, b, m1, m2), a)

    def ncc_terms(tag, p, t, m1, m2, win):
        record(f"ncc_loss/{tag}", lambda x: ops.ncc_loss(x, t, win, gamma), p)
        record(f"ncc_loss_masked(1)/{tag}", lambda x: ops.ncc_loss_masked(x, t, m1, None, win, gamma), p)
        record(f"ncc_loss_masked(2)/{tag}", lambda x: ops.ncc_loss_masked(x, t, m1, m2, win, gamma), p)

    def planes(seed, n, *shape):
        g = torch.Generator(device=dev).manual_seed(seed)
        return [torch.rand(*shape, device=dev, generator=g) for _ in range(n)]

    for i, (B, size, win) in enumerate(T.CASES):
        p, t, m1, m2 = planes(100 + i, 4, B, 1, *size)
        tag = f"{B}x{'x'.join(map(str, size))}/w{win}"
        ncc_terms(tag, p, t, m1, m2, win)
        sqdiff_terms(tag + "/C1", p, t, m1, m2)
        if min(size) >= 2:
            record(f"mind_loss/{tag}", lambda x: ops.mind_loss(x, t), p)
            record(f"mind_loss_masked(1)/{tag}", lambda x: ops.mind_loss_masked(x, t, m1), p)
            record(f"mind_loss_masked(2)/{tag}", lambda x: ops.mind_loss_masked(x, t, m1, m2), p)
    for i, (B, size) in enumerate(T.SQ_CASES):
        for C in (1, 3):
            a, b = planes(200 + 10 * i + C, 2, B, C, *size)
            m1, m2 = planes(300 + 10 * i + C, 2, B, 1, *size)
            sqdiff_terms(f"{B}x{'x'.join(map(str, size))}/C{C}", a, b, m1, m2)
    p, t, m1, m2 = planes(400, 4, 2, 1, 20, 130)
    ncc_terms("2-D 2x20x130/w7", p, t, m1, m2, 7)
    sqdiff_terms("2-D 2x20x130/C1", p, t, m1, m2)
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
        raise SystemExit("similarity_bits: --out FILE.npz or --compare A.npz B.npz")
    arrays = collect()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    print(f"similarity_bits: {len(arrays)} arrays from {ROOT} -> {args.out}")


if __name__ == "__main__":
    main()
