"""CPU-side tests of the bending-energy regulariser: the properties of the float64 definition of tests/bending_ref.py,
and the public surface of the feature (names, header, argument checks, the model's hyper-parameter) as far as it exists without a GPU."""
import inspect

import pytest
import torch

import bending_ref as BR

FB = ["samples", "velocity_fields", "individual_dfs", "combined_dfs", "final_dfs", "transformed"]


def _coords(size):
    return torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in size], indexing="ij")


# ================================================================================================ the reference's own properties
def test_affine_field_costs_nothing():
    """a random affine displacement field of 12 x 14 x 16 at lamb = 0.025: rounding only in float64, where the first differences cost ~1"""
    g = torch.Generator().manual_seed(0)
    theta = torch.eye(3, 4, dtype=torch.float64).unsqueeze(0) + 0.1 * torch.randn(1, 3, 4, generator=g, dtype=torch.float64)
    u = BR.affine_field(theta, (12, 14, 16))
    assert u.shape == (1, 3, 12, 14, 16) and float(u.abs().max()) > 0.5
    assert float(BR.bending_ref(u, 0.025)) <= 1e-20
    assert float(BR.bending_ref(u.float(), 0.025)) <= 1e-9
    first = sum(float((u.diff(dim=d) ** 2).mean()) for d in (2, 3, 4))
    assert 0.025 * 12 * 14 * 16 * first > 0.1


def test_hand_values():
    """u = x^2: u_xx = 2, e = 4;  u = x y: u_xy = 1, e = 2;  the same for slices"""
    z, y, x = _coords((5, 6, 7))
    for u, e in ((x * x, 4.0), (y * y, 4.0), (z * z, 4.0), (x * y, 2.0), (x * z, 2.0), (y * z, 2.0), (x * x + y * z, 6.0)):
        d = BR.density(u.reshape(1, 1, 5, 6, 7))
        assert d.shape == (1, 1, 3, 4, 5)
        torch.testing.assert_close(d, torch.full_like(d, e), rtol=0.0, atol=1e-12)
        assert abs(float(BR.bending_ref(u.reshape(1, 1, 5, 6, 7), 0.5)) - 0.5 * 5 * 6 * 7 * e) <= 1e-9
    y2, x2 = _coords((6, 7))
    for u, e in ((x2 * x2, 4.0), (x2 * y2, 2.0)):
        d4, d5 = BR.density(u.reshape(1, 1, 6, 7)), BR.density(u.reshape(1, 1, 1, 6, 7))
        assert d4.shape == (1, 1, 4, 5) and d5.shape == (1, 1, 1, 4, 5)
        torch.testing.assert_close(d4, torch.full_like(d4, e), rtol=0.0, atol=1e-12)
        assert torch.equal(d5[:, :, 0], d4)
        assert abs(float(BR.bending_ref(u.reshape(1, 1, 1, 6, 7), 0.5)) - 0.5 * 6 * 7 * e) <= 1e-9
    with pytest.raises(ValueError, match="at least 3"):
        BR.density(torch.zeros(1, 1, 2, 6, 7, dtype=torch.float64))


def test_hessian_row_has_the_25_taps_of_radius_2():
    """the gradient is linear in u: its derivative with respect to u at one voxel is the Hessian's row.  Away from the border: the axis offsets
    +-1 and +-2, the in-plane diagonals (+-2, +-2) and the centre"""
    n, c = 11, 5
    u = torch.zeros(1, 1, n, n, n, dtype=torch.float64)
    u[0, 0, c, c, c] = 1.0
    row = BR.bending_grad_ref(u, 1.0)[0, 0]
    nz = torch.nonzero(row) - c
    assert nz.shape[0] == 25 and int(nz.abs().max()) == 2
    want = set()
    for a in range(3):
        for s in (-2, -1, 1, 2):
            o = [0, 0, 0]
            o[a] = s
            want.add(tuple(o))
        for b in range(a + 1, 3):
            for sa in (-2, 2):
                for sb in (-2, 2):
                    o = [0, 0, 0]
                    o[a], o[b] = sa, sb
                    want.add(tuple(o))
    want.add((0, 0, 0))
    assert {tuple(int(v) for v in o) for o in nz} == want
    assert abs(float(row.sum())) <= 1e-12                       # constants cost nothing


# ================================================================================================ the public surface
def test_names_exist():
    from pulpo_amd import evaluation, losses, ops
    assert callable(ops.bending_reg) and callable(losses.Bending_reg)
    import src.losses as shim
    assert shim.Bending_reg is losses.Bending_reg
    assert evaluation.BENDING_METRICS == ("BendingE",)
    for fn in (evaluation.level_scores, evaluation.performance):
        assert inspect.signature(fn).parameters["bending"].default is False
    assert inspect.signature(ops.bending_reg).parameters["lamb"].default == 0.0
    assert inspect.signature(losses.Bending_reg).parameters["lamb"].default == 0


def test_header_declares_the_entry_points_without_an_abi_bump():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    for n in ("pulpo_bending_blocks", "pulpo_bending_fwd", "pulpo_bending_bwd"):
        assert n in protos, n
    assert len(protos["pulpo_bending_blocks"][1]) == 4
    assert len(protos["pulpo_bending_fwd"][1]) == len(protos["pulpo_l2reg_fwd"][1]) == 7
    assert len(protos["pulpo_bending_bwd"][1]) == len(protos["pulpo_l2reg_bwd"][1]) == 9
    assert header_abi_version() == 8


def test_library_refuses_bad_arguments():
    """null pointers, nplanes < 1, H < 3, W < 3, D == 2, D < 1: the library's error code, no launch"""
    import ctypes
    from pulpo_amd._lib import lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.raw("pulpo_bending_fwd"), lib.raw("pulpo_bending_bwd")
    good = (3, 4, 5, 6)
    for shape in ((0, 4, 5, 6), (-1, 4, 5, 6), (3, 4, 2, 6), (3, 4, 5, 2), (3, 2, 5, 6), (3, 0, 5, 6), (3, -1, 5, 6), (3, 1, 2, 6), (3, 1, 5, 1)):
        assert fwd(p, *shape, p, None) != 0, shape
        assert bwd(p, None, 1.0, p, *shape, None) != 0, shape
        assert lib.query("pulpo_bending_blocks", *shape) == 0, shape
    assert fwd(None, *good, p, None) != 0 and fwd(p, *good, None, None) != 0
    assert bwd(None, None, 1.0, p, *good, None) != 0 and bwd(p, None, 1.0, None, *good, None) != 0
    assert b"bending" in lib.raw("pulpo_last_error")()
    # one workgroup per 16 x 32 (y, x) tile of a plane and march of 16, 8 or 4 planes: the longest march that leaves 1024 workgroups, else 4
    assert lib.query("pulpo_bending_blocks", 3, 4, 5, 6) == 3 and lib.query("pulpo_bending_blocks", 2, 1, 20, 24) == 2 * 2
    assert lib.query("pulpo_bending_blocks", 3, 160, 160, 160) == 3 * 10 * 10 * 5 and lib.query("pulpo_bending_blocks", 3, 128, 128, 128) == 3 * 16 * 8 * 4
    assert lib.query("pulpo_bending_blocks", 1, 17, 17, 33) == 5 * 2 * 2 and lib.query("pulpo_bending_blocks", 3, 80, 80, 80) == 3 * 20 * 5 * 3


def test_cpu_tensors_and_small_extents_are_refused():
    from pulpo_amd import losses, ops
    from pulpo_amd._lib import PulpoHipError
    for u in (torch.rand(1, 3, 4, 5, 6), torch.rand(1, 2, 5, 6)):
        for call in (lambda: ops.bending_reg(u, 0.1), lambda: losses.Bending_reg(u, 0.1)):
            with pytest.raises(PulpoHipError):
                call()
    with pytest.raises(NotImplementedError):
        losses.Bending_reg(torch.rand(4, 5, 6), 0.1)


def test_model_takes_the_regularizer():
    from pulpo_amd import losses
    import src.models as models
    m = models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2, regularizer="bending")
    assert m.hparams.regularizer == "bending" and m.hierarchical_regularization.regularizer is losses.Bending_reg
    assert models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2).hierarchical_regularization.regularizer is losses.L2_reg
    assert models.PULPo(2, 2, 0.1, [16, 20], feedback=FB, n0=2, regularizer="bending").hparams.regularizer == "bending"
    with pytest.raises(ValueError, match="L2.*jdet.*bending"):
        models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=FB, n0=2, regularizer="nope")
    with pytest.raises(ValueError, match="at least 3"):                  # levels 16, 2 -> the level-1 field has an extent of 2
        models.PULPo(4, 2, 0.1, [16, 16, 16], feedback=FB, n0=2, regularizer="bending")
    models.PULPo(4, 2, 0.1, [16, 16, 16], feedback=FB, n0=2)             # (L2 takes that pyramid)
    assert list(inspect.signature(models.PULPo.__init__).parameters)[-2:] == ["mind_dilation", "mind_eps"]
    with pytest.raises(Exception) as e:                                  # CPU tensors: the first operator of the step refuses them
        m.training_step((torch.rand(1, 1, 16, 16, 16), torch.rand(1, 1, 16, 16, 16), None, None, None, None, None, None), 0)
    assert "GPU" in str(e.value) or "CPU" in str(e.value)
