"""CPU-side tests of the mutual-information similarity term: the properties of the float64 definition of
tests/mi_ref.py, its stored float32 distances, and the public surface of the feature as far as it exists without a GPU."""
import inspect

import pytest
import torch

import affine_ref as AR
import mi_ref as M

FB = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]


# ================================================================================================ the reference's own properties
@pytest.mark.parametrize("K", [4, 16, 32, 33, 64])
def test_weights_sum_to_one_and_touch_four_bins(K):
    v = torch.cat([torch.linspace(-0.3, 1.3, 257, dtype=torch.float64), torch.tensor([0.0, 1.0], dtype=torch.float64)])
    w = M.weights(v, K)
    assert w.shape == (259, K)
    torch.testing.assert_close(w.sum(1), torch.ones(259, dtype=torch.float64), rtol=0.0, atol=1e-14)
    assert int((w > 0).sum(1).max()) <= 4 and int((w > 0).sum(1).min()) >= 3 and float(w.min()) >= 0.0
    ends = torch.tensor([1.0, 4.0, 1.0], dtype=torch.float64) / 6
    w0, w1 = M.weights(torch.tensor([0.0], dtype=torch.float64), K)[0], M.weights(torch.tensor([1.0], dtype=torch.float64), K)[0]
    torch.testing.assert_close(w0[:3], ends, rtol=0.0, atol=1e-15)
    torch.testing.assert_close(w1[K - 3:], ends, rtol=0.0, atol=1e-15)
    assert float(w0[3:].abs().sum()) == 0.0 and float(w1[:K - 3].abs().sum()) == 0.0
    # values outside [0,1] are clamped
    torch.testing.assert_close(M.weights(torch.tensor([-0.2, 1.7], dtype=torch.float64), K), torch.stack([w0, w1]), rtol=0.0, atol=0.0)


def test_inverted_contrast_has_the_same_mi():
    a = AR.head_image((24, 24, 24), 3)
    same, inv = float(M.mi(a, a)[0]), float(M.mi(1.0 - a, a)[0])
    print(f"FIGURE MI(a, a) {same:.4f}, MI(1 - a, a) {inv:.4f}")
    assert abs(same - inv) <= 1e-12 and same > 0.5


def test_aligned_beats_moved_under_another_contrast():
    y = AR.head_image((24, 24, 24), 3)
    fixed = M.remap(y)
    aligned, moved = float(M.mi(y, fixed)[0]), float(M.mi(torch.roll(y, 2, dims=4), fixed)[0])
    print(f"FIGURE MI aligned {aligned:.3f}, moved by 2 voxels {moved:.3f}")
    assert aligned >= 1.5 * moved and moved > 0.0


def test_independent_noise_has_no_mi():
    g = torch.Generator().manual_seed(1)
    a, b = (torch.rand(1, 1, 24, 24, 24, generator=g, dtype=torch.float64) for _ in range(2))
    val = float(M.mi(a, b)[0])
    print(f"FIGURE MI of independent noise {val:.4f}")
    assert 0.0 <= val < 0.05


def test_constant_image():
    c = torch.full((1, 1, 5, 6, 7), 0.3, dtype=torch.float64)
    t = M.smooth(1, (5, 6, 7), 2)
    assert abs(float(M.mi(c, t)[0])) <= 1e-12
    val, g = M.grad(c, t)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(val))
    val, g = M.grad(t, c)
    assert bool(torch.isfinite(g).all()) and abs(float(val)) <= 1e-9


def test_masked_reference():
    p, t = M.make_pair(2, (5, 6, 7), "smooth")
    ones, zeros = torch.ones_like(p), torch.zeros_like(p)
    torch.testing.assert_close(M.loss_masked(p, t, ones), M.loss(p, t), rtol=1e-13, atol=0.0)
    torch.testing.assert_close(M.grad(p, t, mask=ones)[1], M.grad(p, t)[1], rtol=1e-10, atol=1e-14)
    val, g = M.grad(p, t, mask=zeros)
    assert float(val) == 0.0 and not bool(g.any()) and bool(torch.isfinite(g).all())
    assert not bool(M.histogram(p, t, 32, zeros).any())
    w, w2 = M.make_masks(2, (5, 6, 7), "ball_x_rand")
    torch.testing.assert_close(M.loss_masked(p, t, w, w2), M.loss_masked(p, t, w * w2), rtol=1e-13, atol=0.0)
    assert float((M.loss_masked(p, t, w, w2) - M.loss_masked(p, t, w)).abs()) > 1e-6
    # V stays the voxel count, the histogram is normalised by the mask's weight
    torch.testing.assert_close(M.loss_masked(p, t, 0.5 * ones), M.loss(p, t), rtol=1e-13, atol=0.0)


def test_gradient_outside_the_range_is_zero_and_passes_at_the_ends():
    p, t, *_, g = M.case(2, (7, 9, 11), 32, "edges", None)
    out = (p < 0) | (p > 1)
    assert int(out.sum()) > 0 and not bool(g[out].any())
    ends = (p == 0) | (p == 1)
    assert int(ends.sum()) > 0 and bool(g[ends].abs().max() > 0)


def test_bounds_are_the_fp32_references_own_error():
    """mi_ref.P_OWN / LOSS_OWN / GRAD_OWN, which the GPU tests' bounds are 8 x, are what a float32 CPU run of mi_ref gives against float64
    on the GPU tests' cases: re-measured, at most 25 % above the constants and not below a fifth of them"""
    p, l, g = M.own_figures()
    print(f"FIGURE fp32 reference: p {p:.3g}, loss {l:.3g} relative, gradient {g:.3g} relative L2")
    assert 0.2 * M.P_OWN <= p <= 1.25 * M.P_OWN, p
    assert 0.2 * M.LOSS_OWN <= l <= 1.25 * M.LOSS_OWN, l
    assert 0.2 * M.GRAD_OWN <= g <= 1.25 * M.GRAD_OWN, g


# ================================================================================================ the public surface
def test_names_exist():
    from pulpo_amd import affine, evaluation, losses, ops, refine
    for mod, names in ((losses, ("MI_loss", "MI_loss_masked")), (ops, ("mi_loss", "mi_loss_masked", "joint_histogram"))):
        for n in names:
            assert callable(getattr(mod, n)), n
    assert evaluation.MI_METRICS == ("MI",)
    for fn in (evaluation.level_scores, evaluation.performance):
        params = inspect.signature(fn).parameters
        assert params["mi"].default is False and params["mi_bins"].default == 32
    import src.losses as shim
    assert shim.MI_loss is losses.MI_loss and shim.MI_loss_masked is losses.MI_loss_masked
    assert "mi" in ops.SIMILARITY_TERMS and "mi" in refine.RECON_TERMS and "mi" in affine.LOSSES
    for names in (ops.SIMILARITY_TERMS, refine.RECON_TERMS, affine.LOSSES):
        assert "nmi" not in names
    for fn, default in ((ops.mi_loss, 32), (ops.mi_loss_masked, 32), (ops.joint_histogram, 32), (losses.MI_loss, 32), (ops.similarity, 32)):
        assert inspect.signature(fn).parameters["bins"].default == default
    assert inspect.signature(ops.mi_loss).parameters["gamma"].default == 0.05
    assert affine.DEFAULT_MI_BINS == (16, 16, 32)


def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    for n in ("pulpo_mi_blocks", "pulpo_mi_scratch_floats", "pulpo_mi_fwd", "pulpo_mi_bwd"):
        assert n in protos, n
    assert len(protos["pulpo_mi_fwd"][1]) == 14 and len(protos["pulpo_mi_bwd"][1]) == 12
    assert header_abi_version() == 8


def test_cpu_tensors_are_refused():
    from pulpo_amd import affine, losses, ops
    from pulpo_amd._lib import PulpoHipError
    a, b = torch.rand(1, 1, 4, 5, 6), torch.rand(1, 1, 4, 5, 6)
    a2, b2 = torch.rand(1, 1, 5, 6), torch.rand(1, 1, 5, 6)
    for call in (lambda: ops.mi_loss(a, b), lambda: losses.MI_loss(a, b), lambda: ops.joint_histogram(a, b),
                 lambda: ops.mi_loss_masked(a, b, torch.ones_like(a)), lambda: losses.MI_loss_masked(a, b, torch.ones_like(a)),
                 lambda: ops.mi_loss(a2, b2), lambda: ops.similarity("mi", a, b), lambda: ops.similarity("mi", a2, b2, torch.ones_like(a2)),
                 lambda: affine.fit(a, b, loss="mi", levels=1, iters=(1,))):
        with pytest.raises(PulpoHipError):
            call()
    for bins in (3, 65, 0):
        with pytest.raises(ValueError, match="bins"):
            ops.mi_loss(a, b, bins)
    with pytest.raises(ValueError, match="shape"):
        ops.mi_loss(a, torch.rand(1, 1, 4, 5, 7))


def test_library_refuses_bad_arguments():
    """null pointers, K outside [4, 64], B < 1, V < 1, mask2 without mask: the library's error code, no launch"""
    import ctypes
    from pulpo_amd._lib import lib
    buf = (ctypes.c_double * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.raw("pulpo_mi_fwd"), lib.raw("pulpo_mi_bwd")
    good = (1, 210, 32)

    def f(*ptrs, shape=good):
        return fwd(*ptrs, *shape, 0.05, None)

    def b(*ptrs, shape=good):
        return bwd(*ptrs[:5], None, 1.0, ptrs[5], *shape, None)

    for shape in ((1, 210, 3), (1, 210, 65), (1, 210, 0), (0, 210, 32), (-1, 210, 32), (1, 0, 32), (1, -5, 32)):
        assert f(p, p, None, None, p, p, p, p, p, shape=shape) != 0, shape
        assert b(p, p, None, None, p, p, shape=shape) != 0, shape
    for k in (0, 1, 4, 5, 6, 7, 8):                                         # every required pointer of mi_fwd
        ptrs = [p, p, None, None, p, p, p, p, p]
        ptrs[k] = None
        assert f(*ptrs) != 0, k
    for k in (0, 1, 4, 5):
        ptrs = [p, p, None, None, p, p]
        ptrs[k] = None
        assert b(*ptrs) != 0, k
    assert f(p, p, None, p, p, p, p, p, p) != 0 and b(p, p, None, p, p, p) != 0              # mask2 without mask
    assert "mi_fwd" in lib.raw("pulpo_last_error")().decode() or "mi_bwd" in lib.raw("pulpo_last_error")().decode()
    q = lib.query
    assert q("pulpo_mi_blocks", 0, 210) == 0 and q("pulpo_mi_blocks", 1, 0) == 0
    assert q("pulpo_mi_scratch_floats", 1, 210, 3) == 0 and q("pulpo_mi_scratch_floats", 1, 210, 65) == 0
    # a function of the shape only; the slab stays a few MiB at 160^3
    assert q("pulpo_mi_blocks", 1, 210) == 1 and q("pulpo_mi_blocks", 2, 693) == 2 and q("pulpo_mi_blocks", 2, 9600) == 20
    assert q("pulpo_mi_blocks", 1, 160 ** 3) == 256 and q("pulpo_mi_blocks", 3, 160 ** 3) == 3 * 85 and q("pulpo_mi_blocks", 300, 160 ** 3) == 300
    assert q("pulpo_mi_scratch_floats", 1, 160 ** 3, 32) == 256 * 32 * 32 and q("pulpo_mi_scratch_floats", 1, 160 ** 3, 33) == 256 * 64 * 64
    assert q("pulpo_mi_scratch_floats", 1, 160 ** 3, 64) * 4 <= 4 << 20


def test_term_names_are_checked_before_the_device():
    from pulpo_amd import affine, ops, refine
    import src.models as models
    a = torch.rand(1, 1, 16, 16, 16)
    for kind in ("nmi", "MI", "mutual_information"):
        with pytest.raises(ValueError):
            ops.similarity(kind, a, a)
        with pytest.raises(ValueError, match="loss"):
            affine.fit(a, a, loss=kind)
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2)
    with pytest.raises(ValueError, match="recon_loss"):
        refine.refine(m, a, a, recon_loss=["nmi"])
    assert refine._recon_list(m, ["mi"]) == ["mi"] and refine._recon_list(m, ["ncc", "mi"]) == ["ncc", "mi"]
    for bad in (3, 65, (16, 16), (16, 16, 100)):
        with pytest.raises(ValueError, match="mi_bins"):
            affine.fit(a, a, loss="mi", mi_bins=bad)


def test_loss_module_and_model_take_the_term():
    from pulpo_amd import losses, refine
    import src.models as models
    rec = losses.HierarchicalReconstructionLoss(["mi"], {0: 1.0, 1: 8.0}, False, 3, {0: 5, 1: 3})
    assert rec.mi_bins == 32
    rec.mi_bins = 16
    assert rec.mi_bins == 16 and losses.HierarchicalReconstructionLoss.mi_bins == 32
    names = list(inspect.signature(losses.HierarchicalReconstructionLoss.__init__).parameters)
    assert names == ["self", "recon_loss", "weight_dict", "similarity_pyramid", "ndims", "window_size", "mind_dilation", "mind_eps"]
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2, recon_loss=["mi"])
    assert m.hparams.recon_loss == ["mi"] and m.hierarchical_recon_loss.mi_bins == 32
    m.hierarchical_recon_loss.mi_bins = 16
    assert m.hierarchical_recon_loss.mi_bins == 16 and models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2).hierarchical_recon_loss.mi_bins == 32
    assert list(inspect.signature(models.PULPo.__init__).parameters)[-2:] == ["mind_dilation", "mind_eps"]
    sig = inspect.signature(refine.refine).parameters
    assert "mi_bins" not in sig and "bins" not in sig
