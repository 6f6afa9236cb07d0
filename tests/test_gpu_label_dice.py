"""The Dice term of the training step from integer label maps on the GPU: ops.label_dice_loss and its field
gradient against the float64 one-hot definition (tests/label_dice_ref.py) under the rule of tests/test_gpu_pyramid_metrics.py, the
bit-exact invariants (the per-class Dice of ops.warp_labels_soft_dice, two calls, the pooled map), ops.labels_soft_map, the range check,
the training step with label maps against the oracle's step on one_hot(labels), a descent, and the step as a HIP graph."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import label_dice_ref as L
from oracle import pulpo_oracle as O
from test_gpu_pyramid_metrics import FLOOR, UP, check_scalar, check_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
FB = list(O.FEEDBACK_DEFAULT)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    return models, nb


# ================================================================================================ the operator against float64
# (B, C, field grid, label grid, target grid, dtype): the golden-sized case; three different grids with the OASIS class count; slices;
# 67,200 voxels (a block tail and 263 blocks)
CASES = [
    (2, 5, (9, 10, 11), (9, 10, 11), (9, 10, 11), torch.uint8),
    (1, 36, (12, 10, 9), (7, 13, 8), (24, 20, 18), torch.int32),
    (2, 5, (17, 19), (17, 19), (17, 19), torch.uint8),
    (1, 5, (40, 42, 40), (40, 42, 40), (40, 42, 40), torch.uint8),
]


def _case(B, C, grid, lab_size, tgt_size, dtype):
    """built on the CPU; the input condition is asserted before anything reaches the GPU"""
    gen = torch.Generator().manual_seed(sum(grid) + C)
    df, clamped = L.make_field(B, grid, lab_size, gen)
    L.assert_floor_agrees(df, lab_size, clamped)
    assert all(bool(clamped[:, a].any()) for a in range(len(grid)))
    labels, target = L.make_labels(B, lab_size, C, dtype, gen, False), L.make_labels(B, tgt_size, C, dtype, gen, True)
    assert not bool((labels == C - 1).any() | (target == C - 1).any() | (labels == C - 2).any()) and bool((target == C - 2).any())
    if B > 1:
        assert set(labels[0].unique().tolist()) != set(labels[1].unique().tolist())
    return df.to(DEV), clamped.to(DEV), labels.to(DEV), target.to(DEV)


@pytest.mark.parametrize("dice_factor", [1, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[2])) + f"-C{c[1]}")
def test_label_dice_loss_and_gradient_vs_float64(ops, case, dice_factor):
    """loss, per-class Dice and field gradient (upstream gradient 1.7) of ops.label_dice_loss against the float64 definition, the bound the
    larger of 4 x the fp32 evaluation's own deviation and 1e-6 of max|ref|; the clamped axes of the slab have a gradient of exactly 0, the
    absent class a Dice of exactly 1.
    Observed on the MI355X, error / bound: loss 0.005 ... 0.06, Dice 0.01 ... 0.06, gradient 0.15 ... 0.31 (its bound 2.6e-6 ... 4.2e-5 of
    max|ref|: the fp32 reference's own sums over the grid are what deviates)."""
    B, C, grid, lab_size, tgt_size, dtype = case
    df, clamped, labels, target = _case(*case)
    d = df.clone().requires_grad_(True)
    loss, dice = ops.label_dice_loss(d, labels, C, target, dice_factor, return_dice=True)
    assert not dice.requires_grad and tuple(dice.shape) == (B, C)
    g, = torch.autograd.grad(loss, [d], grad_outputs=torch.tensor(UP, device=DEV))
    assert g.shape == df.shape and g.is_contiguous()

    def ref(dtype_):
        x = df.to(dtype_).requires_grad_(True)
        val = L.label_dice_loss(x, labels, C, target, dice_factor)
        gr, = torch.autograd.grad(val, [x], grad_outputs=torch.tensor(UP, dtype=dtype_, device=DEV))
        return val.detach(), gr, L.dice_per_class(x.detach(), labels, C, target)

    l64, g64, d64 = ref(torch.float64)
    l32, g32, d32 = ref(torch.float32)
    name = f"label_dice {grid} C{C} f{dice_factor}"
    check_scalar(name + " loss", loss.detach(), l64, l32)
    check_tensor(name + " dice", dice, d64, d32)
    check_tensor(name + " grad", g, g64, g32)
    assert bool((g[clamped] == 0).all()), "a clamped coordinate has a gradient of exactly 0"
    assert bool((g64[clamped] == 0).all())
    assert bool((dice[:, C - 1] == 1).all()), "a class in neither map: Dice exactly 1"
    assert bool((dice[:, C - 2] < 1e-3).all()), "a class in the target only"
    assert float(g.abs().max()) > 0


def test_label_dice_gradient_layout_follows_the_caller(ops):
    """a non-contiguous 3-D field and a (B,2,H,W) field get their gradient in their own shape; the values are the contiguous call's"""
    case = CASES[0]
    df, _, labels, target = _case(*case)
    base = ops.label_dice_loss(df.clone().requires_grad_(True), labels, case[1], target)
    wide = torch.zeros(2, 4, *case[2], device=DEV)
    wide[:, :3] = df
    wide.requires_grad_(True)
    loss = ops.label_dice_loss(wide[:, :3], labels, case[1], target)
    assert torch.equal(loss, base)
    g, = torch.autograd.grad(loss, [wide])
    assert g.shape == wide.shape and bool((g[:, 3] == 0).all()) and float(g[:, :3].abs().max()) > 0


# ================================================================================================ bit-exact invariants
@pytest.mark.parametrize("case", CASES[:3], ids=lambda c: "x".join(map(str, c[2])))
def test_dice_equals_warp_labels_soft_dice_and_two_calls_agree(ops, case):
    B, C, grid, lab_size, tgt_size, dtype = case
    df, _, labels, target = _case(*case)
    runs = []
    for _ in range(2):
        d = df.clone().requires_grad_(True)
        loss, dice = ops.label_dice_loss(d, labels, C, target, return_dice=True)
        g, = torch.autograd.grad(loss, [d])
        runs.append((loss.detach(), dice, g))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    dice_eval, mean_eval = ops.warp_labels_soft_dice(df, labels, C, target)
    assert torch.equal(runs[0][1], dice_eval)
    V = float(np.prod(grid))
    np.testing.assert_allclose(float(runs[0][0]), (1.0 - float(mean_eval)) * V, rtol=1e-5)


@pytest.mark.parametrize("shape", [(6, 5, 7), (9, 6), (16, 16, 16)], ids=str)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32], ids=["u8", "i32"])
def test_labels_soft_map_pool2_is_exact(ops, shape, dtype):
    B, C = 2, 5
    gen = torch.Generator().manual_seed(sum(shape))
    lab = L.make_labels(B, shape, C, dtype, gen, True).to(DEV)
    got = ops.labels_soft_map(lab, C, pool2=True)
    oh = L.one_hot(lab, C, torch.float32)
    assert got.shape == (B, C) + tuple((s + 1) // 2 for s in shape) and got.dtype == torch.float32
    assert torch.equal(got, ops.avg_pool2(oh).contiguous())
    pool = F.avg_pool3d if len(shape) == 3 else F.avg_pool2d
    # (count_include_pad=True with no padding: ceil-mode edge windows are divided by their in-bounds count)
    ref64 = pool(oh.double().cpu(), kernel_size=2, stride=2, padding=0, ceil_mode=True)
    assert torch.equal(got.double().cpu(), ref64)


@pytest.mark.parametrize("shape,size", [((12, 10, 14), (6, 5, 7)), ((12, 9, 15), (4, 3, 5)), ((7, 13, 8), (10, 9, 11)), ((20, 18), (10, 9)), ((11, 13), (7, 5))],
                         ids=str)
def test_labels_soft_map_resize_vs_float64(ops, shape, size):
    """ratios 1/2, 1/3 and non-integer ones, volumes and slices, against float64 F.interpolate under the metric tests' rule"""
    B, C = 2, 6
    gen = torch.Generator().manual_seed(sum(shape))
    lab = L.make_labels(B, shape, C, torch.uint8, gen, True).to(DEV)
    got = ops.labels_soft_map(lab, C, size=size)
    mode = "trilinear" if len(shape) == 3 else "bilinear"
    ref64 = F.interpolate(L.one_hot(lab, C, torch.float64), size=size, mode=mode, align_corners=False)
    ref32 = F.interpolate(L.one_hot(lab, C, torch.float32), size=size, mode=mode, align_corners=False)
    assert got.shape == ref64.shape
    check_tensor(f"labels_resize {shape}->{size}", got, ref64, ref32, floor=FLOOR)
    assert bool((got[:, C - 1] == 0).all())
    if tuple(size) == tuple(shape):
        assert torch.equal(got, L.one_hot(lab, C, torch.float32))


def test_labels_soft_map_identity_size_is_the_one_hot_map(ops):
    gen = torch.Generator().manual_seed(1)
    lab = L.make_labels(1, (5, 6, 7), 4, torch.int32, gen, True).to(DEV)
    assert torch.equal(ops.labels_soft_map(lab, 4, size=(5, 6, 7)), L.one_hot(lab, 4, torch.float32))


# ================================================================================================ the range check
def test_check_raises_and_unchecked_stays_finite(ops):
    case = CASES[0]
    C = case[1]
    df, _, labels, target = _case(*case)
    bad = labels.clone()
    bad[0, 0, 2, 3, 4] = C
    with pytest.raises(IndexError):
        ops.label_dice_loss(df, bad, C, target)
    with pytest.raises(IndexError):
        ops.label_dice_loss(df, labels, C, bad)
    d = df.clone().requires_grad_(True)
    loss, dice = ops.label_dice_loss(d, bad, C, bad, check=False, return_dice=True)
    g, = torch.autograd.grad(loss, [d])
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dice).all()) and bool(torch.isfinite(g).all())
    ops.label_dice_loss(df, labels, C, target)          # in range: no exception


def test_prefetcher_carries_label_maps_unchanged(ops):
    from pulpo_amd.prefetch import DevicePrefetcher
    gen = torch.Generator().manual_seed(2)
    lab8, lab32 = L.make_labels(1, (6, 5, 4), 5, torch.uint8, gen, True), L.make_labels(1, (6, 5, 4), 5, torch.int32, gen, True)
    (x, a, b), = list(DevicePrefetcher([(torch.rand(1, 1, 6, 5, 4), lab8, lab32)], DEV))
    assert a.is_cuda and a.dtype == torch.uint8 and b.dtype == torch.int32 and x.dtype == torch.float32
    assert torch.equal(a.cpu(), lab8) and torch.equal(b.cpu(), lab32)


# ================================================================================================ the training step
STEP = dict(Tl=3, L=2, n0=2, size=[16, 16, 16], C=3, B=1)


@pytest.fixture(scope="module")
def step_inputs():
    """weights, images, noise and label maps of the step tests, and the oracle's step on one_hot(labels) per df_resolution (computed once)"""
    gen = torch.Generator().manual_seed(21)
    size, C, B = STEP["size"], STEP["C"], STEP["B"]
    x, y = torch.rand(B, 1, *size, generator=gen), torch.rand(B, 1, *size, generator=gen)
    eps = {l: torch.randn(B, 3, *[s // 2 ** (l + 1) for s in size], generator=gen) for l in range(STEP["L"])}
    blocks = torch.randint(0, C, (B, 1, 4, 4, 4), generator=gen)
    seg_x = blocks.repeat_interleave(4, 2).repeat_interleave(4, 3).repeat_interleave(4, 4).to(torch.uint8)
    seg_y = torch.roll(seg_x, shifts=(1, -1), dims=(3, 4)).contiguous()
    out = {"x": x, "y": y, "eps": eps, "seg_x": seg_x, "seg_y": seg_y}
    for res in ("level_res", "full_res"):
        cfg = O.Cfg(STEP["Tl"], STEP["L"], size, n0=STEP["n0"], df_resolution=res)
        sd0 = O.init_state_dict(cfg, seed=4)
        sd = O.clone_sd(sd0, requires_grad=True)
        ox, oy = L.one_hot(seg_x, C, torch.float32), L.one_hot(seg_y, C, torch.float32)
        outs = O.forward(sd, cfg, x, y, eps, training=True)
        segs = O.transform_segmentation(sd, cfg, outs[6], ox)
        _, kl, _, reg, *_ = O.losses(outs, y, cfg)
        rec, rec_l = O.recon_ncc_dice(outs, y, segs, oy, cfg)
        total = kl + rec + reg
        params = {k: v for k, v in sd.items() if v.requires_grad}
        grads = torch.autograd.grad(total, list(params.values()), allow_unused=True)
        out[res] = {"sd": sd0, "total": float(total.detach()), "kl": float(kl.detach()), "rec": float(rec.detach()), "reg": float(reg.detach()),
                    "rec_l": {l: float(v.detach()) for l, v in rec_l.items()}, "grads": {k: g.detach() for k, g in zip(params, grads) if g is not None}}
    return out


def _step_model(api, inp, res, **kw):
    models, nb = api
    model = models.PULPo(STEP["Tl"], STEP["L"], 0.1, STEP["size"], feedback=FB, n0=STEP["n0"], df_resolution=res, recon_loss=["ncc", "dice"],
                         segs=True, **kw)
    model.load_state_dict({k: v.clone() for k, v in inp[res]["sd"].items()}, strict=True)
    model = model.cuda().train()
    for l in range(STEP["L"]):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(inp["eps"][l].cuda())
    return model


@pytest.mark.parametrize("res", ["level_res", "full_res"])
def test_step_with_label_maps_matches_the_oracle_on_one_hot(api, step_inputs, res):
    """T3 / L2 at 16^3 (lk_offset 1: level 0's unpooled map beside the pooled chain), recon_loss ncc + dice, num_classes 3: total loss,
    per-level reconstruction terms and every parameter gradient against the oracle's step on one_hot(labels), with the tolerances of
    tests/test_gpu_step.py::test_dice_recon_with_segmentations_matches_reference_golden"""
    inp, ref = step_inputs, step_inputs[res]
    model = _step_model(api, inp, res, num_classes=STEP["C"])
    assert model.lk_offset == 1
    model.transform_segmentation = None                    # the label route must not touch it
    x, y, seg_x, seg_y = (inp[k].cuda() for k in ("x", "y", "seg_x", "seg_y"))
    outs, _, (total, kl, rec, reg), (_, rec_l, _) = model._forward_and_losses(x, y, seg_x, seg_y)
    for key, val in zip(("total", "kl", "rec", "reg"), (total, kl, rec, reg)):
        print(f"FIGURE step {res} {key}: {float(val.detach()):.7g} oracle {ref[key]:.7g}")
        np.testing.assert_allclose(float(val.detach()), ref[key], rtol=1e-4)
    for l, v in rec_l.items():
        np.testing.assert_allclose(float(v.detach()), ref["rec_l"][l], rtol=1e-4, atol=1e-6)
    total.backward()
    n = 0
    for k, p in model.named_parameters():
        if k not in ref["grads"]:
            continue
        g = ref["grads"][k].numpy()
        if k.endswith("_op.0.bias") and "velocity_field._op.2" not in k:
            wref = np.abs(ref["grads"][k[:-4] + "weight"].numpy()).max()
            assert np.abs(p.grad.cpu().numpy()).max() <= 1e-3 * max(wref, 1e-3), k
            continue
        assert rel_l2(p.grad, g) < 2e-2, (k, rel_l2(p.grad, g))
        n += 1
    assert n > 40
    # int64 maps (torch's default integer) take the same route
    total64 = model._forward_and_losses(x, y, seg_x.long(), seg_y.long())[2][0]
    assert torch.equal(total64, total.detach())


@pytest.mark.parametrize("res", ["level_res", "full_res"])
def test_one_hot_batch_still_takes_transform_segmentation(api, step_inputs, res):
    """float (B, C, ...) maps: the route of before, bit for bit - transform_segmentation is called, label_dice_terms is not, and the loss
    is HierarchicalReconstructionLoss on its output"""
    inp = step_inputs
    model = _step_model(api, inp, res, num_classes=STEP["C"])
    x, y = inp["x"].cuda(), inp["y"].cuda()
    ox, oy = L.one_hot(inp["seg_x"], STEP["C"], torch.float32).cuda(), L.one_hot(inp["seg_y"], STEP["C"], torch.float32).cuda()
    calls = []
    inner = model.transform_segmentation
    model.transform_segmentation = lambda dfs, seg: calls.append(1) or inner(dfs, seg)
    model.label_dice_terms = None
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    outs, _, (total, kl, rec, reg), (_, rec_l, _) = model._forward_and_losses(x, y, ox, oy)
    assert len(calls) == 1
    model.load_state_dict(state)
    outs2 = model.autoencoder(x, model.downpath(x, y, _needed=model._needed_levels))
    rec2, rec_l2 = model.hierarchical_recon_loss(outs2[7], y, inner(outs2[6], ox), oy, gamma=model.hparams.gamma, dice_factor=model.hparams.dice_factor)
    assert torch.equal(rec2, rec)
    for l in rec_l:
        assert torch.equal(rec_l2[l], rec_l[l])


def test_label_maps_without_num_classes_raise(api, step_inputs):
    inp = step_inputs
    model = _step_model(api, inp, "level_res")
    with pytest.raises(ValueError, match="num_classes"):
        model._forward_and_losses(inp["x"].cuda(), inp["y"].cuda(), inp["seg_x"].cuda(), inp["seg_y"].cuda())


# ================================================================================================ descent
def test_adam_on_the_field_raises_the_dice(ops):
    """20 Adam steps on a zero field with label_dice_loss alone, 4^3 label blocks on 16^3 against the same map shifted by one voxel: the
    mean Dice of warp_labels_soft_dice rises (a gradient of the right size with the wrong sign or axis order would not do that)"""
    C = 64
    idx = torch.arange(16) // 4
    lab = (idx.view(16, 1, 1) * 16 + idx.view(1, 16, 1) * 4 + idx.view(1, 1, 16)).view(1, 1, 16, 16, 16).to(torch.uint8).to(DEV)
    tgt = torch.roll(lab, shifts=1, dims=4).contiguous()
    df = torch.zeros(1, 3, 16, 16, 16, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([df], lr=0.05)
    before = float(ops.warp_labels_soft_dice(df.detach(), lab, C, tgt)[1])
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ops.label_dice_loss(df, lab, C, tgt, check=False)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    after = float(ops.warp_labels_soft_dice(df.detach(), lab, C, tgt)[1])
    print(f"FIGURE descent: mean Dice {before:.4f} -> {after:.4f}, loss {losses[0]:.2f} -> {losses[-1]:.2f}")
    assert after > before and losses[-1] < losses[0]


# ================================================================================================ the step as a HIP graph
def test_graphed_step_with_label_maps_equals_the_eager_step(api):
    """dp.DataParallelStepper(graph=True) captures the label route (no host read on it) and replays it on two alternating label batches:
    the losses of six steps equal the eager stepper's"""
    models, nb = api
    from pulpo_amd import dp
    size, Tl, Lv, n0, C = [32, 32, 32], 3, 2, 8, 4
    gen = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(2):
        x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
        seg_x = L.make_labels(1, size, C + 2, torch.uint8, gen, False).cuda()
        seg_y = torch.roll(seg_x, shifts=1, dims=3).contiguous()
        batches.append((x, y, seg_x, seg_y) + (torch.empty((0,), device="cuda"),) * 4)
    eps = [torch.randn(1, 3, *[s_ // 2 ** (l + 1) for s_ in size], generator=gen).cuda() for l in range(Lv)]

    def run(graph):
        torch.manual_seed(0)
        model = models.PULPo(Tl, Lv, 0.1, size, feedback=FB, n0=n0, recon_loss=["ncc", "dice"], segs=True, num_classes=C).cuda().train()
        for l in range(Lv):
            model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l])
        st = dp.DataParallelStepper(model, graph=graph)
        losses = [float(st.step(batches[i % 2])) for i in range(6)]
        assert (st._graph is not None) == graph
        return losses

    eager, graphed = run(False), run(True)
    np.testing.assert_allclose(graphed, eager, rtol=1e-4)
    assert abs(eager[0] - eager[1]) > 1e-6 * abs(eager[0])
