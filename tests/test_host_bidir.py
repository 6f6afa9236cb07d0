"""CPU-side tests of bidirectional training: the new entry points of the C ABI and their argument checks, the
model's flag, and the symmetry the feature exists for, shown on the float64 reference of tests/bidir_ref.py."""
import ctypes
import inspect

import pytest
import torch

import bidir_ref as BR
import pyramid_ref as R
from oracle import pulpo_oracle as O

FB = list(O.FEEDBACK_DEFAULT)


def test_entry_points_are_exported_and_reject_bad_arguments():
    from pulpo_amd._lib import header_abi_version, lib, parse_header
    protos = parse_header()
    I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert protos["pulpo_vecint_pair_fwd_work"] == (I, [P, P, I, I, I, I, I, P])
    assert protos["pulpo_vecint_pair_bwd"] == (I, [P, P, P, P, P, I, I, I, I, I, P])
    assert protos["pulpo_vecint_pair_bwd_det"] == (I, [P, P, P, P, P, I, I, I, I, I, P])
    assert protos["pulpo_vecint_pair_bwd_tmp_floats"] == (Z, [I] * 5) == protos["pulpo_vecint_pair_bwd_det_ws_bytes"]
    assert header_abi_version() == 8 == lib.query("pulpo_abi_version")          # additions only: no prototype changed, nothing removed
    err = lambda: lib.raw("pulpo_last_error")()
    p = P(256)                                      # never dereferenced: every call below fails its argument check first
    fwd, bwd, det = (lib.raw(n) for n in ("pulpo_vecint_pair_fwd_work", "pulpo_vecint_pair_bwd", "pulpo_vecint_pair_bwd_det"))
    assert fwd(None, p, 1, 8, 8, 8, 7, None) != 0 and fwd(p, None, 1, 8, 8, 8, 7, None) != 0
    for bad in ((0, 8, 8, 8, 7), (1, 0, 8, 8, 7), (1, 8, 1, 8, 7), (1, 8, 8, -3, 7), (1, 8, 8, 8, -1), (1, 8, 8, 8, 31)):
        assert fwd(p, p, *bad, None) != 0, bad
    assert b"vecint_pair_fwd_work" in err()
    for f, name in ((bwd, b"vecint_pair_bwd"), (det, b"vecint_pair_bwd_det")):
        assert f(None, p, p, p, p, 1, 8, 8, 8, 7, None) != 0 and f(p, p, p, None, p, 1, 8, 8, 8, 7, None) != 0
        assert f(p, None, None, p, p, 1, 8, 8, 8, 7, None) != 0          # one upstream gradient may be absent, not both
        for bad in ((0, 8, 8, 8, 7), (1, 0, 8, 8, 7), (1, 8, 1, 8, 7), (1, 8, 8, 0, 7), (1, 8, 8, 8, -1)):
            assert f(p, p, p, p, p, *bad, None) != 0, bad
        assert name in err()
        assert f(p, p, None, p, None, 1, 8, 8, 8, 7, None) != 0          # the steps need their scratch
        assert name in err() and (b"scratch" in err() or b"workspace" in err())
    # the size queries: pulpo_vecint_bwd's buffers for both directions; the deterministic chain's workspace and two more fields
    n = 3 * 12 * 10 * 14
    q = lambda name, *a: lib.query(name, *a)
    assert q("pulpo_vecint_pair_bwd_tmp_floats", 2, 12, 10, 14, 7) == 7 * 2 * 2 * n == 2 * q("pulpo_vecint_bwd_tmp_floats", 2, 12, 10, 14, 7)
    assert q("pulpo_vecint_pair_bwd_tmp_floats", 1, 6, 12, 14, 7) == 2 * 2 * 3 * 6 * 12 * 14          # plain scatter: two buffers, both directions
    assert q("pulpo_vecint_pair_bwd_tmp_floats", 1, 12, 10, 14, 0) == 0 == q("pulpo_vecint_pair_bwd_tmp_floats", 0, 12, 10, 14, 7)
    assert q("pulpo_vecint_pair_bwd_det_ws_bytes", 2, 12, 10, 14, 7) == q("pulpo_vecint_bwd_det_ws_bytes", 2, 12, 10, 14, 7) + 2 * 4 * 2 * n
    assert q("pulpo_vecint_pair_bwd_det_ws_bytes", 2, 12, 10, 14, 0) == 0


def test_public_surface():
    from pulpo_amd import evaluation, losses, ops, refine
    from pulpo_amd.components.pulpo import Autoencoder, SVFDecoder
    import src.models as models
    p = inspect.signature(models.PULPo.__init__).parameters["bidirectional"]
    assert p.default is False
    assert inspect.signature(models.PULPo.refine).parameters["bidirectional"].default is None
    assert inspect.signature(refine.refine_interpolated).parameters["bidirectional"].default is None
    assert inspect.signature(refine.Objective.__init__).parameters["bidirectional"].default is None
    assert inspect.signature(evaluation.performance).parameters["inverse_image"].default is False
    assert evaluation.INVERSE_IMAGE_METRICS == ("RMSE_inv", "Dice_inv")
    assert inspect.signature(Autoencoder.forward).parameters["y"].default is None
    assert inspect.signature(SVFDecoder.forward).parameters["inverse_image"].default is None
    assert inspect.signature(losses.HierarchicalReconstructionLoss.forward).parameters["inverse"].default is None
    assert inspect.signature(losses.HierarchicalRegularization.forward).parameters["dfs_inv"].default is None
    assert hasattr(ops, "_VecIntPair")
    with pytest.raises(Exception, match="no CPU|GPU|cuda|CUDA"):                # no CPU fallback: the paired node refuses host tensors too
        ops.vecint_pair(torch.zeros(1, 3, 8, 8, 8, requires_grad=True))


@pytest.mark.parametrize("size", [[16, 16, 16], [12, 14, 16]])
def test_flag_changes_no_parameter(size):
    """same state_dict keys and shapes either way, the flag among the hyper-parameters, and a state dict of one loads into the other"""
    import src.models as models
    make = lambda **kw: models.PULPo(3, 2, 0.1, size, feedback=FB, n0=4, **kw)
    torch.manual_seed(0)
    off = make()
    on = make(bidirectional=True)
    assert on.hparams["bidirectional"] is True and off.hparams["bidirectional"] is False and on.bidirectional and not off.bidirectional
    sd_off, sd_on = off.state_dict(), on.state_dict()
    assert list(sd_off.keys()) == list(sd_on.keys())
    assert all(sd_off[k].shape == sd_on[k].shape and sd_off[k].dtype == sd_on[k].dtype for k in sd_off)
    on.load_state_dict(sd_off)
    off.load_state_dict(on.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), sd_off.values()))


def _fields(cfg, seed, amp=2.0):
    """smooth float64 combined velocity fields on the latent levels' grids"""
    sizes = cfg.level_sizes()
    return {l: R.vecint_field("smooth", 1, sizes[cfg.offset + l], amp=amp / (l + 1), seed=seed + l).double() for l in range(cfg.latent_levels)}


@pytest.mark.parametrize("size,recon", [((16, 16, 16), ("ncc",)), ((12, 14, 16), ("ncc", "mse"))])
def test_objective_is_symmetric_and_reduces_to_the_unidirectional_one(size, recon):
    """J(x, y, v) == J(y, x, -v) to 1e-12 relative in float64, with final <-> final_inv and y_hat <-> x_hat exchanged exactly; the same
    objective is half the sum of the two unidirectional ones; with the inverse terms dropped it is the oracle's own loss block"""
    cfg = O.Cfg(3, 2, list(size), n0=4)
    gen = torch.Generator().manual_seed(3)
    x, y = torch.rand(1, 1, *size, generator=gen).double(), torch.rand(1, 1, *size, generator=gen).double()
    v = _fields(cfg, 5)
    a = BR.objective(cfg, x, y, v, recon)
    b = BR.objective(cfg, y, x, {l: -t for l, t in v.items()}, recon)
    for key in ("rec", "reg", "total"):
        assert abs(float(a[key]) - float(b[key])) <= 1e-12 * abs(float(a[key])), key
    for l in v:
        assert torch.equal(a["final"][l], b["final_inv"][l]) and torch.equal(a["final_inv"][l], b["final"][l])
        assert torch.equal(a["y_hat"][l], b["x_hat"][l]) and torch.equal(a["x_hat"][l], b["y_hat"][l])
        assert float((a["final"][l] + a["final_inv"][l]).abs().max()) > 1e-3          # the inverse integral is not the negated field
    one = BR.objective(cfg, x, y, v, recon, bidirectional=False)
    other = BR.objective(cfg, y, x, {l: -t for l, t in v.items()}, recon, bidirectional=False)
    assert one["x_hat"] is None and one["final_inv"] is None
    for key in ("rec", "reg"):
        assert abs(float(a[key]) - 0.5 * (float(one[key]) + float(other[key]))) <= 1e-12 * abs(float(a[key])), key
    assert abs(float(one["rec"]) - float(other["rec"])) > 1e-6 * abs(float(one["rec"]))          # the one-sided objective is NOT symmetric
    if recon == ("ncc",):
        outs = (None, None, None, None, None, None, one["final"], one["y_hat"])
        mus = {l: torch.zeros(1, 3, 2, 2, 2, dtype=torch.float64) for l in v}
        _, _, rec, reg, _, rec_l, reg_l = O.losses((mus, {l: torch.ones_like(m) for l, m in mus.items()}) + outs[2:], y, cfg)
        assert abs(float(rec) - float(one["rec"])) <= 1e-12 * abs(float(rec)) and abs(float(reg) - float(one["reg"])) <= 1e-12 * abs(float(reg))
        assert all(abs(float(rec_l[l]) - float(one["rec_levels"][l])) <= 1e-12 * abs(float(rec_l[l])) for l in v)


def test_pair_chain_is_the_oracle_on_both_signs():
    v = R.vecint_field("smooth", 2, (6, 7, 5), amp=3.0, seed=2).double()
    chain = BR.pair_chain(v, 4)
    assert len(chain) == 5 and torch.equal(chain[0][0], v / 16) and torch.equal(chain[0][1], -v / 16)
    torch.testing.assert_close(chain[-1][0], O.vecint(v, 4), rtol=0, atol=1e-14)
    torch.testing.assert_close(chain[-1][1], O.vecint(-v, 4), rtol=0, atol=1e-14)
