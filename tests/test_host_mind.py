"""CPU-side tests of the MIND-SSC similarity term: the properties of the float64 definition of tests/mind_ref.py,
and the public surface of the feature (names, argument checks, hyper-parameters) as far as it exists without a GPU."""
import inspect

import pytest
import torch

import mind_ref as M

# ================================================================================================ the reference's own properties
def test_channels_are_the_stated_offset_pairs():
    """twelve channels, channel k built from offsets PAIRS[k]: a hand evaluation of D_k at one interior voxel of a small volume"""
    assert M.PAIRS == ((0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (3, 5))
    d, eps = 2, 1e-5
    img = M.noise(1, (7, 8, 9), 3)
    f = M.descriptor(img, d, eps)
    assert f.shape == (1, 12, 7, 8, 9)
    I = img[0, 0]
    p = (3, 4, 4)
    e = [(-d, 0, 0), (d, 0, 0), (0, -d, 0), (0, d, 0), (0, 0, -d), (0, 0, d)]
    lim = [s - 1 for s in I.shape]
    cl = lambda q: tuple(min(max(v, 0), h) for v, h in zip(q, lim))
    Dk = []
    for a, b in M.PAIRS:
        acc = 0.0
        for qz in (-1, 0, 1):
            for qy in (-1, 0, 1):
                for qx in (-1, 0, 1):
                    r = cl((p[0] + qz, p[1] + qy, p[2] + qx))
                    ia, ib = cl(tuple(r[i] + e[a][i] for i in range(3))), cl(tuple(r[i] + e[b][i] for i in range(3)))
                    acc += float(I[ia] - I[ib]) ** 2
        Dk.append(acc / 27)
    Dk = torch.tensor(Dk, dtype=torch.float64)
    m = Dk - Dk.min()
    want = torch.exp(-m / (m.mean() + eps))
    torch.testing.assert_close(f[0, :, p[0], p[1], p[2]], want, rtol=1e-12, atol=0.0)


def test_clamping_is_applied_to_the_box_tap_first():
    """at a corner voxel: c(c(p + q) + d e), not c(p + q + d e)"""
    d = 2
    img = M.noise(1, (5, 5, 6), 4)
    I = img[0, 0]
    lim = [s - 1 for s in I.shape]
    cl = lambda q: tuple(min(max(v, 0), h) for v, h in zip(q, lim))
    a, b = (0, 0, -d), (0, d, 0)                        # channel 11 = (+y, -x) ... PAIRS[10] = (3, 4): +y and -x
    acc = 0.0
    for qz in (-1, 0, 1):
        for qy in (-1, 0, 1):
            for qx in (-1, 0, 1):
                r = cl((qz, qy, qx))
                acc += float(I[cl((r[0], r[1] + d, r[2]))] - I[cl((r[0], r[1], r[2] - d))]) ** 2
    nb = [M._shift(img, dim, s * d) for dim, s in M.OFFSETS]
    D10 = M._box3((nb[3] - nb[4]) ** 2)[0, 0, 0, 0, 0]
    torch.testing.assert_close(D10, torch.tensor(acc / 27, dtype=torch.float64), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_descriptor_range_and_inverted_contrast(d):
    img = M.noise(2, (6, 7, 9), 1, smooth=1)
    f = M.descriptor(img, d)
    assert float(f.max(dim=1).values.min()) == 1.0 and float(f.min()) > 0.0          # the arg-min channel is exp(0)
    torch.testing.assert_close(M.descriptor(1.0 - img, d), f, rtol=0.0, atol=1e-12)
    assert float(M.loss(1.0 - img, img, d)) <= 1e-24


def test_zero_volume_gives_a_descriptor_of_ones():
    z = torch.zeros(1, 1, 4, 5, 6, dtype=torch.float64)
    f = M.descriptor(z)
    assert bool(torch.isfinite(f).all()) and bool((f == 1.0).all())
    half = M.noise(1, (6, 6, 8), 2)
    half[..., :4] = 0.0                                                              # a zero half-volume stays finite
    assert bool(torch.isfinite(M.descriptor(half)).all())
    g = M.grad(half, M.noise(1, (6, 6, 8), 3))
    assert bool(torch.isfinite(g).all())


def test_aligned_beats_shifted_under_inverted_contrast_and_mse_does_not():
    a, inv, sh = M.shifted_pair()
    aligned, shifted = float(M.loss(a, inv, 2)), float(M.loss(sh, inv, 2))
    assert shifted > 100.0 and shifted > M.SHIFT_FACTOR * aligned, (aligned, shifted)
    a32, inv32, sh32 = a.float(), inv.float(), sh.float()
    assert float(M.loss(sh32, inv32, 2)) > M.SHIFT_FACTOR * float(M.loss(a32, inv32, 2))
    mse = lambda p, t: float(((p - t) ** 2).sum())
    assert mse(sh, inv) < mse(a, inv), "MSE was expected to prefer the misaligned pair"


def test_masked_reference():
    p, t = M.noise(2, (5, 6, 7), 1), M.noise(2, (5, 6, 7), 2)
    ones = torch.ones_like(p)
    torch.testing.assert_close(M.loss_masked(p, t, ones), M.loss(p, t), rtol=1e-12, atol=0.0)
    assert float(M.loss_masked(p, t, torch.zeros_like(p))) == 0.0
    assert not bool(M.grad(p, t, mask=torch.zeros_like(p)).any())
    w = torch.rand(p.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    torch.testing.assert_close(M.loss_masked(p, t, w, ones), M.loss_masked(p, t, w), rtol=1e-12, atol=0.0)


# ================================================================================================ the public surface
def test_names_exist():
    from pulpo_amd import evaluation, losses, ops, synthetic
    for mod, names in ((losses, ("MIND_loss", "MIND_loss_masked")), (ops, ("mind_loss", "mind_loss_masked", "mind_descriptor")),
                       (synthetic, ("multimodal_pair",))):
        for n in names:
            assert callable(getattr(mod, n)), n
    assert evaluation.MIND_METRICS == ("MIND",)
    for fn in (evaluation.level_scores, evaluation.performance):
        params = inspect.signature(fn).parameters
        assert params["mind"].default is False and params["mind_dilation"].default == 2 and params["mind_eps"].default == 1e-5
    import src.losses as shim
    assert shim.MIND_loss is losses.MIND_loss


def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    for n in ("pulpo_mind_blocks", "pulpo_mind_descriptor", "pulpo_mind_fwd", "pulpo_mind_bwd"):
        assert n in protos, n
    assert len(protos["pulpo_mind_fwd"][1]) == 12 and len(protos["pulpo_mind_bwd"][1]) == 15 and len(protos["pulpo_mind_descriptor"][1]) == 9
    assert header_abi_version() == 8


def test_cpu_tensors_and_2d_inputs_are_refused():
    from pulpo_amd import losses, ops
    from pulpo_amd._lib import PulpoHipError
    a, b = torch.rand(1, 1, 4, 5, 6), torch.rand(1, 1, 4, 5, 6)
    for call in (lambda: ops.mind_loss(a, b), lambda: losses.MIND_loss(a, b), lambda: ops.mind_descriptor(a),
                 lambda: ops.mind_loss_masked(a, b, torch.ones_like(a)), lambda: losses.MIND_loss_masked(a, b, torch.ones_like(a))):
        with pytest.raises(PulpoHipError):
            call()
    a2, b2 = torch.rand(1, 1, 5, 6), torch.rand(1, 1, 5, 6)
    for call in (lambda: ops.mind_loss(a2, b2), lambda: losses.MIND_loss(a2, b2), lambda: ops.mind_descriptor(a2),
                 lambda: ops.mind_loss_masked(a2, b2, torch.ones_like(a2))):
        with pytest.raises(NotImplementedError, match="3-D"):
            call()


def test_library_refuses_bad_arguments():
    """null pointers, d < 1, an extent < 2, eps <= 0: the library's error code, no launch"""
    import ctypes
    from pulpo_amd._lib import lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd, desc = lib.raw("pulpo_mind_fwd"), lib.raw("pulpo_mind_bwd"), lib.raw("pulpo_mind_descriptor")
    good = (1, 4, 5, 6, 2, 1e-5)
    for shape in ((1, 4, 5, 6, 0, 1e-5), (1, 1, 5, 6, 2, 1e-5), (1, 4, 5, 1, 2, 1e-5), (0, 4, 5, 6, 2, 1e-5), (1, 4, 5, 6, 2, 0.0), (1, 4, 5, 6, 2, -1.0),
                  (1, 4, 5, 6, 50, 1e-5)):
        assert fwd(p, p, None, None, p, *shape, None) != 0, shape
        assert bwd(p, p, None, None, p, None, 1.0, p, *shape, None) != 0, shape
        assert desc(p, p, *shape, None) != 0, shape
    assert fwd(None, p, None, None, p, *good, None) != 0 and fwd(p, None, None, None, p, *good, None) != 0
    assert fwd(p, p, None, None, None, *good, None) != 0 and fwd(p, p, None, p, p, *good, None) != 0          # mask2 without mask
    assert bwd(p, p, None, None, None, None, 1.0, p, *good, None) != 0 and bwd(p, p, None, None, p, None, 1.0, None, *good, None) != 0
    assert desc(None, p, *good, None) != 0 and desc(p, None, *good, None) != 0
    assert lib.query("pulpo_mind_blocks", 1, 4, 5, 6, 0) == 0 and lib.query("pulpo_mind_blocks", 1, 1, 5, 6, 2) == 0
    assert lib.query("pulpo_mind_blocks", 1, 20, 24, 20, 2) == 3 * 3 * 1 and lib.query("pulpo_mind_blocks", 2, 160, 160, 160, 2) == 2048


def test_loss_module_and_model_take_the_new_hyperparameters():
    from pulpo_amd import losses
    import src.models as models
    rec = losses.HierarchicalReconstructionLoss(["mind"], {0: 1.0, 1: 8.0}, False, 3, {0: 5, 1: 3})
    assert (rec.mind_dilation, rec.mind_eps) == (2, 1e-5)
    rec = losses.HierarchicalReconstructionLoss(["ncc", "mind"], {0: 1.0}, False, 3, {0: 9}, mind_dilation=3, mind_eps=1e-4)
    assert (rec.mind_dilation, rec.mind_eps) == (3, 1e-4)
    names = list(inspect.signature(losses.HierarchicalReconstructionLoss.__init__).parameters)
    assert names == ["self", "recon_loss", "weight_dict", "similarity_pyramid", "ndims", "window_size", "mind_dilation", "mind_eps"]
    fb = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=fb, n0=2, recon_loss=["mind"], mind_dilation=3)
    assert m.hparams.mind_dilation == 3 and m.hparams.mind_eps == 1e-5 and m.hparams.recon_loss == ["mind"]
    assert m.hierarchical_recon_loss.mind_dilation == 3
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=fb, n0=2)
    assert m.hparams.mind_dilation == 2 and m.hparams.recon_loss == ["ncc"]
    assert list(inspect.signature(models.PULPo.__init__).parameters)[-2:] == ["mind_dilation", "mind_eps"]
