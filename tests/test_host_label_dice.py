"""The Dice term from label maps, the parts that need no GPU: the float64 definition (tests/label_dice_ref.py) has the gradient autograd
says it has, the C prototypes are declared, the model takes the number of classes and refuses integer maps without it, the operators
refuse contradictory arguments, and HierarchicalReconstructionLoss(dice_terms=...) is the plain weighted chain."""
import inspect

import pytest
import torch

import label_dice_ref as L


def test_definition_gradient_by_gradcheck():
    """torch.autograd.gradcheck of the float64 definition with respect to the field on a 4 x 5 x 3 grid (maps on grids of their own), at
    sample coordinates away from the cell borders, where the trilinear gradient jumps"""
    gen = torch.Generator().manual_seed(7)
    grid, lab_size, tgt_size, C = (4, 5, 3), (5, 4, 6), (8, 10, 6), 4
    df, clamped = L.make_field(1, grid, lab_size, gen, slab=False)
    L.assert_floor_agrees(df, lab_size, clamped)
    labels, target = L.make_labels(1, lab_size, C, torch.uint8, gen, False), L.make_labels(1, tgt_size, C, torch.uint8, gen, True)
    d = df.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda f: L.label_dice_loss(f, labels, C, target, 2), (d,), eps=1e-6, atol=1e-6, rtol=1e-5)
    g, = torch.autograd.grad(L.label_dice_loss(d, labels, C, target), [d])
    assert float(g.abs().max()) > 0


def test_definition_clamped_axis_has_zero_gradient():
    gen = torch.Generator().manual_seed(8)
    grid, C = (4, 5, 3), 4
    df, clamped = L.make_field(1, grid, grid, gen)
    L.assert_floor_agrees(df, grid, clamped)
    assert all(bool(clamped[:, a].any()) for a in range(3))
    labels, target = L.make_labels(1, grid, C, torch.uint8, gen, False), L.make_labels(1, grid, C, torch.uint8, gen, True)
    d = df.double().requires_grad_(True)
    g, = torch.autograd.grad(L.label_dice_loss(d, labels, C, target), [d])
    assert bool((g[clamped] == 0).all()) and bool((g[~clamped] != 0).any())


def test_prototypes_are_declared():
    from pulpo_amd._lib import header_abi_version, parse_header
    protos = parse_header()
    for name, nargs in (("pulpo_label_dice_fwd", 22), ("pulpo_label_dice_bwd", 19), ("pulpo_labels_pool2", 9), ("pulpo_labels_resize", 12)):
        assert name in protos, name
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))
    assert header_abi_version() == 8


def _model(**kw):
    import src.models as models
    from oracle import pulpo_oracle as O
    return models.PULPo(3, 2, 0.1, [16, 16, 16], feedback=list(O.FEEDBACK_DEFAULT), n0=2, recon_loss=["ncc", "dice"], segs=True, **kw)


def test_num_classes_hyperparameter():
    import src.models as models
    p = inspect.signature(models.PULPo.__init__).parameters["num_classes"]
    assert p.default is None
    m = _model(num_classes=3)
    assert m.num_classes == 3 and m.hparams.num_classes == 3
    assert _model().num_classes is None


def test_integer_segmentations_need_num_classes():
    m = _model()
    lab = torch.zeros(1, 1, 16, 16, 16, dtype=torch.uint8)
    dfs = {0: torch.zeros(1, 3, 16, 16, 16), 1: torch.zeros(1, 3, 4, 4, 4)}
    assert m._label_maps(lab, lab) and not m._label_maps(lab.float(), lab.float())
    with pytest.raises(ValueError, match="num_classes"):
        m.label_dice_terms(dfs, lab, lab)
    with pytest.raises(ValueError):
        m._label_maps(lab, lab.float())                      # one label map, one one-hot map


def test_labels_soft_map_wants_exactly_one_form():
    from pulpo_amd import ops
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.labels_soft_map(lab, 3)
    with pytest.raises(ValueError):
        ops.labels_soft_map(lab, 3, pool2=True, size=(2, 2, 2))


def test_dice_terms_stand_in_for_the_dice_term(monkeypatch):
    """CPU scalars: with dice_terms the level term is (w ncc_l + w dice_terms[l]) / 2, everything else as before"""
    from pulpo_amd import losses
    w = {0: 4.0, 1: 8.0}
    rec = losses.HierarchicalReconstructionLoss(["ncc", "dice"], dict(w), False, 3, {0: 5, 1: 3})
    ncc = {0: torch.tensor(-0.3), 1: torch.tensor(-0.7)}
    level_of_window = {5: 0, 3: 1}
    monkeypatch.setattr(losses.ops, "similarity", lambda kind, pred, true, mask=None, mask2=None, *, win, **kw: ncc[level_of_window[win]])
    dice = {0: torch.tensor(1.25), 1: torch.tensor(0.5)}
    y = torch.zeros(1, 1, 2, 2, 2)
    total, levels = rec(dict.fromkeys(w, y), y, dict.fromkeys(w), None, dice_terms=dice)
    want = {l: (w[l] * ncc[l] + w[l] * dice[l]) / 2 for l in w}
    for l in w:
        assert torch.equal(levels[l], want[l])
    assert torch.equal(total, 0.0 + want[0] + want[1])
    assert "dice_terms" in inspect.signature(rec.forward).parameters and inspect.signature(rec.forward).parameters["dice_terms"].default is None
