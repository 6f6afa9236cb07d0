"""GPU tests of the label-map warp (pulpo_warp_labels and its ops / uncertainty layers): warp3d on a one-hot map without the one-hot map,
its arg-max, per-class Dice and per-class Monte-Carlo moments, against the one-hot route through the existing operators and the CPU
oracle; mc_uncertainty's segmentation / landmark extras against the reference's stacked-sample procedure (evaluate.py:222-274,
1500-1576) on the same latent noise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FB = list(O.FEEDBACK_DEFAULT)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    import src.models as models
    import src.network_blocks as nb
    from pulpo_amd._lib import lib
    lib.load()
    return models, nb


def one_hot(lab, C):
    """(B, 1, ...) labels -> (B, C, ...) fp32 one-hot"""
    oh = F.one_hot(lab[:, 0].long(), C)
    return oh.permute(0, oh.dim() - 1, *range(1, oh.dim() - 1)).float().contiguous()


def rand_labels(shape, C, dtype, gen):
    return torch.randint(0, C, shape, generator=gen).to(dtype).cuda()


def rand_field(B, grid, scale, gen):
    """a displacement field large enough to leave the volume (border clamp) in places"""
    nd = len(grid)
    return (scale * torch.randn(B, nd, *grid, generator=gen)).cuda()


# (batch, field grid, label-map size): cube, ragged, coarse grid on a finer map, 2-D (depth-1) form
SHAPES = [(1, (16, 16, 16), (16, 16, 16)), (1, (17, 23, 12), (17, 23, 12)), (1, (8, 8, 8), (16, 16, 16)), (1, (24, 20), (24, 20)),
          (2, (16, 16, 16), (16, 16, 16))]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("C", [2, 5, 36])
def test_warp_labels_equals_warp3d_of_the_one_hot_map(api, C, dtype):
    from pulpo_amd import ops
    gen = torch.Generator().manual_seed(C)
    for B, grid, img in SHAPES:
        lab = rand_labels((B, 1) + img, C, dtype, gen)
        df = rand_field(B, grid, 6.0, gen)
        oh = one_hot(lab, C)
        ref = ops.warp3d(df, oh)
        got = ops.warp_labels(df, lab, C, onehot=True)
        assert got.shape == ref.shape and got.dtype == torch.float32
        err = float((got - ref).abs().max())
        assert err <= 1e-6, (grid, img, err)
        if len(grid) == 3:
            cpu = O.warp(df.cpu(), oh.cpu())
            err = float((got.cpu() - cpu).abs().max())
            assert err <= 1e-5, (grid, img, "oracle", err)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
def test_warp_labels_argmax(api, dtype):
    from pulpo_amd import ops
    gen = torch.Generator().manual_seed(11)
    for C in (2, 5, 36):
        for B, grid, img in SHAPES:
            lab = rand_labels((B, 1) + img, C, dtype, gen)
            df = rand_field(B, grid, 3.0, gen)
            oh = ops.warp3d(df, one_hot(lab, C))
            oh2, am = ops.warp_labels(df, lab, C, onehot=True, argmax=True)
            assert am.dtype == dtype and tuple(am.shape) == (B, 1) + grid
            assert bool((oh2 == ops.warp_labels(df, lab, C, onehot=True)).all())
            top = oh.topk(2, dim=1).values if C > 1 else None
            sure = (top[:, 0] - top[:, 1]) > 1e-6
            ref = oh.argmax(dim=1)
            assert bool((am[:, 0].long() == ref)[sure].all()), (C, grid)
    # exact ties: every grid point samples halfway between a column of class 2 and a column of class 1 -> class 1, the lower one
    # (2-D form, a 2 x 2 grid on a 4 x 4 map: x + dx = 0.5 -> column coordinate 1.5, y + dy = 0.375 -> row coordinate 1.0)
    df = torch.zeros(1, 2, 2, 2)
    df[0, 0, 0, :], df[0, 0, 1, :] = 0.375, -0.625
    df[0, 1, :, 0], df[0, 1, :, 1] = 0.5, -0.5
    lab = torch.tensor([0, 2, 1, 0]).repeat(4, 1)[None, None].to(dtype).cuda()
    p, am = ops.warp_labels(df.cuda(), lab, 3, onehot=True, argmax=True)
    assert bool((p[0, 1] == 0.5).all()) and bool((p[0, 2] == 0.5).all())
    assert bool((am == 1).all())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
def test_warp_labels_dice_per_class(api, dtype):
    from pulpo_amd import ops
    gen = torch.Generator().manual_seed(3)
    for C in (2, 5, 36):
        for B, grid, img in SHAPES:
            lab = rand_labels((B, 1) + img, C, dtype, gen)
            tgt = rand_labels((B, 1) + grid, C, dtype, gen)
            df = rand_field(B, grid, 2.0, gen)
            oh, toh = ops.warp3d(df, one_hot(lab, C)), one_hot(tgt, C)
            dice = ops.warp_labels(df, lab, C, target=tgt)
            assert tuple(dice.shape) == (B, C)
            ref = torch.tensor([[float(ops.dsc(oh[b:b + 1, c:c + 1], toh[b:b + 1, c:c + 1])) for c in range(C)] for b in range(B)])
            err = float((dice.cpu() - ref).abs().max())
            assert err <= 1e-6, (C, grid, err)
            again = ops.warp_labels(df, lab, C, target=tgt)
            assert torch.equal(dice, again)                    # deterministic reduction: bit-identical
            _, _, d3 = ops.warp_labels(df, lab, C, target=tgt, onehot=True, argmax=True)
            assert torch.equal(dice, d3)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
def test_label_moments_equal_streaming_moments_of_the_one_hot_warp(api, dtype):
    from pulpo_amd import ops
    gen = torch.Generator().manual_seed(7)
    for C in (2, 5, 36):
        for B, grid, img in SHAPES:
            lab = rand_labels((B, 1) + img, C, dtype, gen)
            tgt = rand_labels((B, 1) + grid, C, dtype, gen)
            oh = one_hot(lab, C)
            lm, sm = ops.LabelMoments(C), ops.StreamingMoments()
            for s in range(5):
                df = rand_field(B, grid, 2.0, gen)
                d = lm.update(df, lab, target=tgt if s % 2 else None)
                sm.update(ops.warp3d(df, oh))
                if s % 2:
                    assert torch.equal(d, ops.warp_labels(df, lab, C, target=tgt))
                else:
                    assert d is None
            assert lm.count == sm.count == 5 and lm.mean().shape == sm.mean().shape
            err_m = float((lm.mean() - sm.mean()).abs().max())
            err_s = float((lm.std_map() - sm.std_map()).abs().max())
            assert err_m <= 1e-6 and err_s <= 1e-6, (C, grid, err_m, err_s)


def test_label_errors_and_conversions(api):
    from pulpo_amd import ops
    from pulpo_amd._lib import PulpoHipError
    gen = torch.Generator().manual_seed(1)
    C = 5
    df = rand_field(1, (8, 8, 8), 1.0, gen)
    for dtype in (torch.uint8, torch.int32):
        lab = rand_labels((1, 1, 8, 8, 8), C, dtype, gen)
        bad = lab.clone()
        bad[0, 0, 7, 7, 7] = C                                  # anywhere in the map, gathered or not
        with pytest.raises(IndexError):
            ops.warp_labels(df, bad, C, onehot=True)
        with pytest.raises(IndexError):
            ops.warp_labels(df, lab, C, target=bad)
        with pytest.raises(IndexError):
            ops.LabelMoments(C).update(df, bad)
        with pytest.raises(PulpoHipError):
            ops.warp_labels(df.cpu(), lab.cpu(), C, onehot=True)
        with pytest.raises(PulpoHipError):
            ops.warp_labels(df, lab.cpu(), C, onehot=True)
        with pytest.raises(PulpoHipError):
            ops.labels_from_onehot(one_hot(lab, C).cpu())
        # one_hot -> labels round trip, both label dtypes, 3-D and 2-D
        for shape in ((2, 1, 9, 7, 5), (1, 1, 6, 10)):
            for c in (2, 5, 36):
                l0 = rand_labels(shape, c, dtype, gen)
                back = ops.labels_from_onehot(one_hot(l0, c), dtype=dtype)
                assert back.dtype == dtype and torch.equal(back, l0)
        assert ops.labels_from_onehot(one_hot(lab, C)).dtype == torch.uint8
    # ties in a soft map go to the lowest class
    soft = torch.full((1, 4, 2, 2, 2), 0.25).cuda()
    assert bool((ops.labels_from_onehot(soft) == 0).all())
    soft[:, 2] = 0.5
    soft[:, 3] = 0.5
    assert bool((ops.labels_from_onehot(soft) == 2).all())


def _ncc_numpy(a, v):
    """Evaluate.ncc (evaluate.py:334-353), zero-normed, in float64"""
    a, v = np.asarray(a, dtype=np.float64).flatten(), np.asarray(v, dtype=np.float64).flatten()
    eps = 1e-15
    a = (a - np.mean(a)) / (np.std(a) * len(a) + eps)
    v = (v - np.mean(v)) / (np.std(v) + eps)
    return np.correlate(a, v)[0]


def test_map_ncc_matches_evaluate_ncc(api):
    from pulpo_amd import ops
    gen = torch.Generator().manual_seed(2)
    for shape in ((16, 16, 16), (33, 17, 9), (96, 96, 96)):
        a = torch.rand(shape, generator=gen)
        b = 0.3 * a + torch.rand(shape, generator=gen)
        got = ops.map_ncc(a.cuda(), b.cuda())
        assert got.dtype == torch.float64 and got.dim() == 0
        ref = _ncc_numpy(a.numpy(), b.numpy())
        assert abs(float(got) - ref) <= 1e-9 * max(1.0, abs(ref)), (shape, float(got), ref)
        assert torch.equal(got, ops.map_ncc(a.cuda(), b.cuda()))


# ------------------------------------------------------------------------------------------------ mc_uncertainty with extras
def build_from_golden(models, nb, g, key="sd0."):
    Tl, L, n0, B, *size = [int(v) for v in g["cfg"]]
    model = models.PULPo(Tl, L, 0.1, size, feedback=FB, n0=n0)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith(key):
            sd[k[len(key):]] = T(v.copy())
    model.load_state_dict(sd, strict=True)
    return model.cuda(), (Tl, L, n0, B, size)


class Replay:
    """a latent sampler that replays a recorded noise sequence"""

    def __init__(self, seq):
        self.seq, self.i = seq, 0

    def __call__(self, mu, sigma):
        e = self.seq[self.i % len(self.seq)]
        self.i += 1
        return mu + sigma * e


def _lms_var_np(lms):
    return np.mean(np.var(lms, axis=0, ddof=1), axis=-1)


def test_mc_uncertainty_extras_match_stacked_samples(api, golden):
    models, nb = api
    from pulpo_amd import ops
    from pulpo_amd.uncertainty import mc_uncertainty, uncertainty_scores
    g = golden("step_T3L2_n4_16")
    model, (Tl, L, n0, B, size) = build_from_golden(models, nb, g)
    model.eval()
    x, y = T(g["x"])[:1].cuda(), T(g["y"])[:1].cuda()
    N, C = 4, 5
    gen = torch.Generator().manual_seed(5)
    noise = {l: [torch.randn(1, 3, *[s // 2 ** (l + Tl - L) for s in size], generator=gen).cuda() for _ in range(N)] for l in range(L)}
    seg_x = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    seg_y = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    lm_x = torch.stack([torch.randint(0, s, (6,), generator=gen) for s in size], dim=-1)[None].float().cuda()
    lm_y = (lm_x + torch.randn(lm_x.shape, generator=gen).cuda()).clamp(0, min(size) - 1)

    def set_samplers():
        for l in range(L):
            model.autoencoder.encoders[l].sampler = Replay(noise[l])

    set_samplers()
    plain = mc_uncertainty(model, x, y, N)
    set_samplers()
    res = mc_uncertainty(model, x, y, N, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, num_classes=C)
    for key, d in plain.items():                                    # the extras change nothing that was there
        for l, v in d.items():
            assert torch.equal(res[key][l], v), (key, l)
    set_samplers()
    res_oh = mc_uncertainty(model, x, y, N, seg_x=one_hot(seg_x, C), seg_y=one_hot(seg_y, C), lm_x=lm_x)
    for key in ("dice", "dice_samples"):
        assert torch.equal(res_oh[key], res[key]), key
    for l in range(L):
        assert torch.equal(res_oh["seg_std"][l], res["seg_std"][l])

    # the reference's procedure with stacked samples, on the same noise
    set_samplers()
    ohx, ohy = one_hot(seg_x, C), one_hot(seg_y, C)
    outs, fins = [], {l: [] for l in range(L)}
    with torch.no_grad():
        for _ in range(N):
            o, ind = model.predict(x, y, N=1)
            _, fin = model.combine_dfs(ind)
            outs.append(o[0][0])
            for l in range(L):
                fins[l].append(fin[l])
    for l in range(L):
        stack = torch.stack([ops.warp3d(f, ohx)[0] for f in fins[l]]).cpu()
        ref = O.mc_std_map(stack)
        assert tuple(res["seg_std"][l].shape) == tuple(ref.shape)
        err = float((res["seg_std"][l].cpu() - ref).abs().max())
        assert err <= 1e-5 * max(1.0, float(ref.abs().max())), ("seg_std", l, err)
        ws = ops.warp3d(res["final_dfs"][l], ohx)
        assert tuple(res["warped_seg"][l].shape) == (1, C) + tuple(res["final_dfs"][l].shape[2:])
        assert float((res["warped_seg"][l] - ws).abs().max()) <= 1e-6
        top = ws.topk(2, dim=1).values
        sure = (top[:, 0] - top[:, 1]) > 1e-6
        assert bool((res["warped_labels"][l][:, 0].long() == ws.argmax(dim=1))[sure].all())
    ref_ds = torch.tensor([[float(ops.dsc(ops.warp3d(f, ohx)[:, c:c + 1], ohy[:, c:c + 1])) for c in range(C)] for f in fins[0]])
    assert tuple(res["dice_samples"].shape) == (N, C)
    assert float((res["dice_samples"].cpu() - ref_ds).abs().max()) <= 1e-6
    ws0 = ops.warp3d(res["final_dfs"][0], ohx)
    ref_d = torch.tensor([float(ops.dsc(ws0[:, c:c + 1], ohy[:, c:c + 1])) for c in range(C)])
    assert float((res["dice"].cpu() - ref_d).abs().max()) <= 1e-6
    ref_lms = torch.cat([ops.warp_landmarks(lm_x, f) for f in fins[0]])
    assert tuple(res["lm_samples"].shape) == (N, 6, 3)
    assert float((res["lm_samples"] - ref_lms).abs().max()) <= 1e-5 * max(1.0, float(ref_lms.abs().max()))
    assert torch.equal(res["lm_hat"], ops.warp_landmarks(lm_x, res["final_dfs"][0]))
    mse = torch.mean((torch.stack(outs) - y[0]) ** 2, dim=0)[0].cpu()
    err = float((res["output_mse"].cpu() - mse).abs().max())
    assert err <= 1e-5 * float(mse.abs().max()), err

    # Evaluate.uncertainty's scalars, restated in numpy from the stacked samples
    sc = uncertainty_scores(res, lm_y=lm_y)
    var = (O.mc_std_map(torch.stack(outs).cpu()) ** 2).numpy()
    lms = ref_lms.cpu().numpy().astype(np.float64)
    lv = _lms_var_np(lms)
    err_lm = np.mean((res["lm_hat"].cpu().numpy().astype(np.float64) - lm_y.cpu().numpy()) ** 2, axis=-1).flatten()
    en = (err_lm - err_lm.mean()) / (np.std(err_lm, ddof=1) * len(err_lm))
    vn = (lv - lv.mean()) / np.std(lv, ddof=1)
    ref_sc = {"Var": var.mean(), "NCC": _ncc_numpy(var, mse.numpy()), "LM_VAR": lv.mean(), "LM_NCC": np.correlate(en, vn)[0],
              "Dice": ref_d.double().mean().item(), "Dice_std": ref_ds.double().std(dim=0).mean().item()}
    assert set(sc) == set(ref_sc)
    for k, v in ref_sc.items():
        assert abs(sc[k] - v) <= 1e-4 * max(abs(v), 1e-6), (k, sc[k], v)
    assert "LM_NCC" not in uncertainty_scores(res)


def test_mc_uncertainty_memory_does_not_grow_with_samples(api):
    models, _ = api
    from pulpo_amd.uncertainty import mc_uncertainty
    size, C = [96, 96, 96], 36
    torch.manual_seed(0)
    model = models.PULPo(3, 2, 0.1, size, feedback=FB, n0=8).cuda().eval()
    gen = torch.Generator().manual_seed(9)
    x, y = torch.rand(1, 1, *size, generator=gen).cuda(), torch.rand(1, 1, *size, generator=gen).cuda()
    seg_x = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    seg_y = torch.randint(0, C, (1, 1, *size), generator=gen).to(torch.uint8).cuda()
    lm_x = torch.randint(0, 96, (1, 10, 3), generator=gen).float().cuda()

    def peak(n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        res = mc_uncertainty(model, x, y, n, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, num_classes=C)
        torch.cuda.synchronize()
        del res
        return torch.cuda.max_memory_allocated()

    peak(2)                                          # (first-call caches: weight packs, workspaces)
    p2, p6 = peak(2), peak(6)
    assert p6 <= 1.05 * p2, (p2, p6)


def test_config5_shape_mc_uncertainty_with_segmentations(api):
    """BASELINE config 5 shape: 192 x 224 x 160, T6/L5, n0 = 32, bf16 conv operands, 8 samples, 36 classes (OASIS-style label count)"""
    models, _ = api
    from pulpo_amd import ops, synthetic
    from pulpo_amd.uncertainty import mc_uncertainty, uncertainty_scores
    size, C, N = [192, 224, 160], 36, 8
    torch.manual_seed(0)
    model = models.PULPo(6, 5, 0.1, size, feedback=FB, n0=32).cuda().eval()
    x, y = synthetic.oasis_like_pair(size, 1, 7, "cuda")
    gen = torch.Generator().manual_seed(4)

    def blocky():
        coarse = torch.randint(0, C, (1, 1) + tuple(s // 16 for s in size), generator=gen)
        return coarse.repeat_interleave(16, 2).repeat_interleave(16, 3).repeat_interleave(16, 4).to(torch.uint8).cuda()

    seg_x, seg_y = blocky(), blocky()
    lm_x = torch.stack([torch.randint(0, s, (12,), generator=gen) for s in size], dim=-1)[None].float().cuda()
    ops.set_conv_precision("bf16", activations="bf16")
    try:
        res = mc_uncertainty(model, x, y, N, seg_x=seg_x, seg_y=seg_y, lm_x=lm_x, num_classes=C)
    finally:
        ops.set_conv_precision("fp32")
    for l in range(5):
        assert bool(torch.isfinite(res["seg_std"][l]).all()) and float(res["seg_std"][l].min()) >= 0.0
        assert bool(torch.isfinite(res["warped_seg"][l]).all())
        assert res["warped_seg"][l].shape[1] == C
    assert tuple(res["dice_samples"].shape) == (N, C) and tuple(res["lm_samples"].shape) == (N, 12, 3)
    for key in ("dice", "dice_samples", "output_mse", "lm_samples", "lm_hat"):
        assert bool(torch.isfinite(res[key]).all()), key
    assert float(res["dice"].min()) >= 0.0 and float(res["dice"].max()) <= 1.0
    assert float(res["dice_samples"].min()) >= 0.0 and float(res["dice_samples"].max()) <= 1.0
    sc = uncertainty_scores(res, lm_y=lm_x)
    assert all(np.isfinite(v) for v in sc.values()), sc
