"""CPU-side tests of cost-function masking: the float64 definitions of tests/masked_ref.py against the unmasked
references of tests/pyramid_ref.py and against their own properties, and the argument checks of the masked entry points of
pulpo_amd/csrc/losses.hip and metrics.hip."""
import ctypes

import pytest
import torch

import masked_ref as M
import pyramid_ref as R

CASES = [(2, (6, 7, 9), 5), (1, (1, 10, 12), 3), (1, (5, 4, 11), 9)]


def _pair(B, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 1, *size, generator=g, dtype=torch.float64), torch.rand(B, 1, *size, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("B,size,win", CASES)
def test_a_mask_of_ones_is_the_unmasked_loss(B, size, win):
    p, t = _pair(B, size)
    ones = torch.ones_like(p)
    tight = dict(rtol=1e-12, atol=0.0)
    torch.testing.assert_close(M.ncc_masked_ref(p, t, ones, None, win, 0.05), R.ncc_ref(p, t, win, 0.05), **tight)
    torch.testing.assert_close(M.ncc_masked_ref(p, t, ones, ones, win, 0.05), R.ncc_ref(p, t, win, 0.05), **tight)
    torch.testing.assert_close(M.ncc_masked_grad_ref(p, t, ones, None, win, 0.05), R.ncc_grad_ref(p, t, win, 0.05), rtol=1e-11, atol=1e-14)
    a, b = torch.cat([p, t, p * t], 1), torch.cat([t, p * p, p], 1)
    spatial = tuple(range(2, a.dim()))
    torch.testing.assert_close(M.l2_masked_ref(a, b, ones), ((a - b) ** 2).sum(spatial).mean(), **tight)       # L2_loss, src/losses.py:79-83
    rmse, frac = M.rmse_masked_ref(a, b, ones)
    torch.testing.assert_close(rmse, ((a - b) ** 2).mean().sqrt(), **tight)
    assert float(frac) == 1.0


@pytest.mark.parametrize("B,size,win", CASES)
def test_closed_form_gradient_is_the_gradient_of_the_masked_loss(B, size, win):
    p, t = _pair(B, size, 1)
    g = torch.Generator().manual_seed(2)
    w1, w2 = torch.rand(p.shape, generator=g, dtype=torch.float64), M.ball(B, size).double()
    assert 0 < float((w1 * w2).sum()) < p.numel()
    pg = p.clone().requires_grad_(True)
    auto, = torch.autograd.grad(M.ncc_masked_ref(pg, t, w1, w2, win, 0.05), [pg])
    closed = M.ncc_masked_grad_ref(p, t, w1, w2, win, 0.05)
    torch.testing.assert_close(closed, auto, rtol=1e-9, atol=1e-12 * float(auto.abs().max()))


def test_a_zero_mask_gives_zero():
    p, t = _pair(2, (5, 6, 7))
    zero = torch.zeros_like(p)
    assert float(M.ncc_masked_ref(p, t, zero, None, 5, 0.05)) == 0.0
    assert float(M.ncc_masked_ref(p, t, torch.ones_like(p), zero, 5, 0.05)) == 0.0
    assert not bool(M.ncc_masked_grad_ref(p, t, zero, None, 5, 0.05).any())
    assert float(M.l2_masked_ref(p, t, zero)) == 0.0
    rmse, frac = M.rmse_masked_ref(p, t, zero)
    assert float(rmse) == 0.0 and float(frac) == 0.0


@pytest.mark.parametrize("win", [3, 5])
def test_voxels_out_of_the_masks_reach_do_not_change_the_loss(win):
    """pred changed only at voxels farther than win // 2 from every voxel with m > 0 (all of them, which includes those that are that
    far away along every axis): the window sums change there, but no counted voxel's window reaches them"""
    B, size = 2, (12, 14, 16)
    p, t = _pair(B, size, 3)
    mask = torch.zeros_like(p)
    mask[:, :, 2:5, 3:6, 4:8] = 0.75
    far = M.outside_reach(mask, None, win)
    near = ~far
    assert int(far.sum()) > 100 and int(near.sum()) == B * (3 + 2 * (win // 2)) ** 2 * (4 + 2 * (win // 2))
    every_axis = torch.zeros_like(far)
    every_axis[:, :, 5 + win // 2:, 6 + win // 2:, 8 + win // 2:] = True
    assert bool(far[every_axis].all())
    g = torch.Generator().manual_seed(4)
    moved = torch.where(far, torch.rand(p.shape, generator=g, dtype=torch.float64), p)
    assert float((moved - p).abs().max()) > 0.5
    base = float(M.ncc_masked_ref(p, t, mask, None, win, 0.05))
    # (pyramid_ref's box sums are differences of prefix sums: a far value enters a window's sum and leaves it again, to 1e-16 of the prefix)
    assert abs(float(M.ncc_masked_ref(moved, t, mask, None, win, 0.05)) - base) <= 1e-12 * abs(base)
    assert not bool(M.ncc_masked_grad_ref(p, t, mask, None, win, 0.05)[far].any())
    # ... and one voxel inside the reach does change it
    inside = p.clone()
    inside[0, 0, 5 + win // 2 - 1, 4, 5] += 0.25
    assert abs(float(M.ncc_masked_ref(inside, t, mask, None, win, 0.05)) - base) > 1e-6 * abs(base)


def test_header_declares_the_masked_entry_points():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    want = {"pulpo_ncc_masked_fwd": 13, "pulpo_ncc_masked_bwd": 15, "pulpo_sqdiff_masked_fwd": 9, "pulpo_sqdiff_masked_bwd": 11, "pulpo_masked_finish": 7,
            "pulpo_warp_mask_fwd": 11}
    for name, nargs in want.items():
        assert name in protos, name
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, (name, len(argtypes))
    assert header_abi_version() >= 7
    # the unmasked entry points keep their prototypes
    assert len(protos["pulpo_ncc_fwd"][1]) == 11 and len(protos["pulpo_ncc_bwd"][1]) == 13
    assert len(protos["pulpo_sqdiff_fwd"][1]) == 5 and len(protos["pulpo_sqdiff_bwd"][1]) == 7


def test_entry_points_reject_null_pointers_and_bad_sizes():
    from pulpo_amd._lib import lib
    fwd, bwd, sfwd, sbwd, fin = (lib.raw(n) for n in ("pulpo_ncc_masked_fwd", "pulpo_ncc_masked_bwd", "pulpo_sqdiff_masked_fwd",
                                                        "pulpo_sqdiff_masked_bwd", "pulpo_masked_finish"))
    assert lib.query("pulpo_abi_version") >= 7
    p = ctypes.c_void_p(256)                        # never dereferenced: every call below fails its argument check first
    ok = (1, 8, 8, 8, 9)
    # ncc_masked_fwd(I, J, wa, wb, S, T, partial, B, D, H, W, win, stream): wb is the one nullable pointer
    for k in (0, 1, 2, 4, 5, 6):
        args = [p] * 7
        args[k] = None
        assert fwd(*args, *ok, None) != 0, k
    assert b"ncc_masked_fwd" in lib.raw("pulpo_last_error")()
    for bad in ((0, 8, 8, 8, 9), (1, 0, 8, 8, 9), (1, 8, -1, 8, 9), (1, 8, 8, 0, 9), (1, 8, 8, 8, 8), (1, 8, 8, 8, 0), (1, 8, 8, 8, -3), (1, 8, 8, 8, 33)):
        assert fwd(p, p, p, p, p, p, p, *bad, None) != 0, bad
        assert fwd(p, p, p, None, p, p, p, *bad, None) != 0, bad
    # ncc_masked_bwd(I, J, S, wa, wb, T, gscale, coef, gJ, B, D, H, W, win, stream): wb and gscale nullable
    for k in (0, 1, 2, 3, 5):
        args = [p] * 7
        args[k] = None
        assert bwd(*args, 1.0, p, *ok, None) != 0, k
    assert bwd(p, p, p, p, p, p, p, 1.0, None, *ok, None) != 0
    assert b"ncc_masked_bwd" in lib.raw("pulpo_last_error")()
    for bad in ((0, 8, 8, 8, 9), (1, 0, 8, 8, 9), (1, 8, 0, 8, 9), (1, 8, 8, -2, 9), (1, 8, 8, 8, 4), (1, 8, 8, 8, 35)):
        assert bwd(p, p, p, p, None, p, None, 1.0, p, *bad, None) != 0, bad
    # sqdiff_masked_fwd(a, b, wa, wb, partial, B, C, V, stream)
    for k in (0, 1, 2, 4):
        args = [p] * 5
        args[k] = None
        assert sfwd(*args, 1, 3, 512, None) != 0, k
    for bad in ((0, 3, 512), (1, 0, 512), (1, 3, 0), (-1, 3, 512), (1, 3, -7)):
        assert sfwd(p, p, p, None, p, *bad, None) != 0, bad
    assert b"sqdiff_masked_fwd" in lib.raw("pulpo_last_error")()
    # sqdiff_masked_bwd(a, b, wa, wb, gscale, coef, ga, B, C, V, stream)
    for k in (0, 1, 2):
        args = [p] * 5
        args[k] = None
        assert sbwd(*args, 1.0, p, 1, 3, 512, None) != 0, k
    assert sbwd(p, p, p, p, p, 1.0, None, 1, 3, 512, None) != 0
    for bad in ((0, 3, 512), (1, 0, 512), (1, 3, 0)):
        assert sbwd(p, p, p, None, None, 1.0, p, *bad, None) != 0, bad
    assert b"sqdiff_masked_bwd" in lib.raw("pulpo_last_error")()
    # masked_finish(partial, nblk, scale, root, count, out, stream)
    assert fin(None, 4, 1.0, 0, 64.0, p, None) != 0 and fin(p, 4, 1.0, 0, 64.0, None, None) != 0
    assert fin(p, 0, 1.0, 0, 64.0, p, None) != 0 and fin(p, -1, 1.0, 0, 64.0, p, None) != 0 and fin(p, 4, 1.0, 0, 0.0, p, None) != 0
    assert b"masked_finish" in lib.raw("pulpo_last_error")()
    # warp_mask_fwd(df, mask, out, B, Dg, Hg, Wg, Di, Hi, Wi, stream)
    wm = lib.raw("pulpo_warp_mask_fwd")
    assert wm(None, p, p, 1, 8, 8, 8, 8, 8, 8, None) != 0 and wm(p, None, p, 1, 8, 8, 8, 8, 8, 8, None) != 0
    assert wm(p, p, None, 1, 8, 8, 8, 8, 8, 8, None) != 0
    for bad in ((0, 8, 8, 8, 8, 8, 8), (1, 0, 8, 8, 8, 8, 8), (1, 8, 1, 8, 8, 8, 8), (1, 8, 8, 1, 8, 8, 8), (1, 8, 8, 8, 0, 8, 8), (1, 8, 8, 8, 8, -1, 8),
                (1, 8, 8, 8, 8, 8, 0), (1, 1, 8, 8, 2, 8, 8), (1, 2048, 1024, 1024, 8, 8, 8)):
        assert wm(p, p, p, *bad, None) != 0, bad
    assert b"warp_mask_fwd" in lib.raw("pulpo_last_error")()


def test_similarity_refuses_unknown_terms():
    """before anything asks for a GPU: CPU tensors, which every known term refuses with PulpoHipError"""
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    p, t = _pair(1, (4, 5, 6))
    for kind in ("dice", "", "NCC", None):
        with pytest.raises(ValueError):
            ops.similarity(kind, p.float(), t.float())
        with pytest.raises(ValueError):
            ops.similarity(kind, p.float(), t.float(), torch.ones_like(p), None, win=5)
    with pytest.raises(PulpoHipError):
        ops.similarity("ncc", p.float(), t.float(), win=5)
