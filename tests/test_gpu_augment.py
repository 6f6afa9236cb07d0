"""Training augmentation on the MI355X against the float64 definitions of tests/augment_ref.py: the B-spline field, the fused
kernel's three routes (trilinear image with intensity, trilinear mask, nearest labels), the device Philox generator, the Augmenter on a batch
and a training step through the loader.

Shapes: (12,14,16) at s = 4, B = 2, C in {1, 2} - the smallest grid where a lattice cell, a partial last cell and the fill region all occur;
(40,36,44) at s = 8, B = 2 - several tiles (4 x 4 x 64 voxels) and lattice sub-tiles, a row that is no multiple of the tile, a batch stride;
(96,100,104) at s = 16 - 1200 tiles, float64 reference on the device; (20,24) at s = 4 - the 2-D form.  W = 14 (the "odd" case) has rows that
are no multiple of the vector width: the scalar stores.
Transforms: rotations within 10 degrees, scales within 10 %, shifts of a few voxels (part of every output samples outside the volume, which each
case asserts), lattice entries N(0, 1.5^2) voxels.
Bounds: max(4 x the error of the same reference run in fp32 on the CPU against float64, 1e-6 max|ref|) (metrics_ref.bound); `check` also asserts
that the bound rejects a 1e-3 max|ref| error.  Trilinear zero-fill sampling is continuous in the position: no voxel is left out.  Labels must be
EQUAL, except voxels whose float64 position lies within 1e-4 of a rounding boundary (a half-integer; the volume's edges at -0.5 and S - 0.5 are
among them), at most 1 % of the voxels (expected: 3 axes x 2e-4)."""
import functools
import math

import pytest
import torch

import augment_ref as A
import metrics_ref as M
from launch_log import LaunchLog
from test_gpu_affine import check
from test_host_augment import KAT

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops
    from pulpo_amd._lib import lib
    lib.load()
    return ops


# name: (grid, spacing, B, seed)
CASES = {
    "small": ((12, 14, 16), 4, 2, 11),
    "odd": ((9, 11, 14), 3, 1, 12),
    "larger": ((40, 36, 44), 8, 2, 13),
    "slice": ((1, 20, 24), 4, 2, 14),
}
LARGE = ((96, 100, 104), 16, 1, 15)


def make_transform(size, s, B, seed):
    """(theta (B,3,4), phi (B,3,G...)) as fp32 tensors: rotations within 10 degrees, scales within 10 %, shifts within 3 voxels; phi N(0, 1.5^2)"""
    from pulpo_amd.augment import Augmenter
    two_d = size[0] == 1
    aug = Augmenter(size[1:] if two_d else size, seed=seed, rotate_deg=10.0, scale=0.1, translate_vox=3.0, elastic_spacing=s, elastic_std_vox=1.5)
    m = aug.draw(B)["x"]
    theta, phi = m["theta"], m["phi"]
    return (A.lift_theta(theta), A.lift_phi(phi)) if two_d else (theta, phi)


@functools.lru_cache(maxsize=None)
def case_inputs(name: str, C: int = 1):
    size, s, B, seed = CASES[name]
    theta, phi = make_transform(size, s, B, seed)
    g = torch.Generator().manual_seed(seed + 100)
    img = torch.rand(B, C, *size, generator=g)
    mask = (torch.rand(B, 1, *size, generator=g) > 0.4).float()
    lab = torch.randint(0, 6, (B, 1, *size), generator=g, dtype=torch.uint8)
    p64 = A.positions(size, theta, phi, s, F64)
    hi = torch.tensor([n - 1 for n in size], dtype=F64).view(1, 3, 1, 1, 1)
    outside = ((p64 < 0) | (p64 > hi)).any(dim=1).double().mean()
    assert 0.02 < float(outside) < 0.9, f"case {name}: {float(outside):.3f} of the output samples outside the volume"
    return size, s, theta, phi, img, mask, lab, p64


def dev_args(name, theta, phi, *srcs):
    """the operator's arguments on the device: the slice case goes through the 2-D interface"""
    two_d = CASES.get(name, LARGE)[0][0] == 1
    th = None if theta is None else (theta[:, 1:, 1:] if two_d else theta).contiguous().to(DEV)
    ph = None if phi is None else (phi[:, 1:, 0] if two_d else phi).contiguous().to(DEV)
    return th, ph, [None if t is None else (t[:, :, 0] if two_d else t).contiguous().to(DEV) for t in srcs]


def lifted(name, t):
    return t.unsqueeze(2) if CASES[name][0][0] == 1 else t


def bound_of(fn, *args32):
    """(float64 reference, tolerance): fn run in float64 and in fp32 on the same fp32-valued inputs"""
    ref64, ref32 = fn(F64), fn(torch.float32)
    return ref64, M.bound(ref32, ref64, 1e-6)


# ================================================================================================ bspline_field
@pytest.mark.parametrize("with_theta", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_bspline_field_vs_float64(ops, name, with_theta):
    size, s, theta, phi, *_ = case_inputs(name)
    th = theta if with_theta else None
    ref, tol = bound_of(lambda dt: A.displacement(size, th, phi, s, dt))
    t_dev, p_dev, _ = dev_args(name, th, phi)
    got = ops.bspline_field(p_dev, size[1:] if size[0] == 1 else size, s, theta=t_dev)
    if size[0] == 1:
        assert tuple(got.shape) == (phi.shape[0], 2, *size[1:])
        got = torch.cat([torch.zeros_like(got[:, :1]), got], dim=1).unsqueeze(2)
    check(f"bspline_field {name} theta={with_theta}", got, ref, tol)


def test_bspline_field_large_on_device(ops):
    size, s, B, seed = LARGE
    theta, phi = make_transform(size, s, B, seed)
    th, ph = theta.to(DEV), phi.to(DEV)
    for t in (None, th):
        ref64 = A.displacement(size, t, ph, s, F64)
        ref32 = A.displacement(size, t, ph, s, torch.float32)
        check(f"bspline_field large theta={t is not None}", ops.bspline_field(ph, size, s, theta=t), ref64, M.bound(ref32, ref64, 1e-6))


# ================================================================================================ augment: images and masks
def intensity_configs(B, nd, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = 0.8 + 0.5 * torch.rand(B, generator=g)
    gain, offset = 0.9 + 0.2 * torch.rand(B, generator=g), 0.1 * (torch.rand(B, generator=g) - 0.5)
    bias = 0.3 * torch.randn(B, *([3] * nd), generator=g)
    sigma = torch.ones(B)
    return {
        "off": None,
        "gamma": {"gamma": gamma},
        "bias": {"bias": bias},
        "gain": {"gain": gain, "offset": offset},
        "noise": {"sigma": sigma, "seed": 987654321012345},
        "all": {"gamma": gamma, "bias": bias, "gain": gain, "offset": offset, "sigma": 0.05 * sigma, "seed": (1 << 40) + 17, "clip": True},
    }


def _dev_cfg(cfg, two_d):
    if cfg is None:
        return None
    out = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in cfg.items()}
    return out


def _ref_cfg(cfg, two_d):
    if cfg is None or "bias" not in cfg or not two_d:
        return cfg
    return dict(cfg, bias=cfg["bias"].unsqueeze(1))


@pytest.mark.parametrize("which", ["off", "gamma", "bias", "gain", "noise", "all"])
@pytest.mark.parametrize("name, C", [("small", 1), ("small", 2), ("odd", 1), ("larger", 1), ("slice", 2)])
def test_augment_image_and_mask_vs_float64(ops, name, C, which):
    size, s, theta, phi, img, mask, lab, p64 = case_inputs(name, C)
    two_d = size[0] == 1
    cfg = intensity_configs(img.shape[0], 2 if two_d else 3, 5)[which]
    rcfg = _ref_cfg(cfg, two_d)

    def ref(dt):
        return A.augment(img, mask, None, theta=theta, phi=phi, spacing=s, intensity_cfg=rcfg, dtype=dt)[:2]

    (ri64, rm64), (ri32, rm32) = ref(F64), ref(torch.float32)
    th, ph, (i_dev, m_dev) = dev_args(name, theta, phi, img, mask)
    gi, gm = ops.augment(i_dev, m_dev, theta=th, phi=ph, spacing=s, intensity=_dev_cfg(cfg, two_d))
    check(f"augment img {name} C={C} {which}", lifted(name, gi), ri64, M.bound(ri32, ri64, 1e-6))
    check(f"augment mask {name} C={C} {which}", lifted(name, gm), rm64, M.bound(rm32, rm64, 1e-6))


def test_augment_large_on_device(ops):
    """1200 tiles (the kernels have no grid cap and no trip loop: one tile per workgroup); image and labels against the float64 reference run on the device"""
    size, s, B, seed = LARGE
    theta, phi = make_transform(size, s, B, seed)
    th, ph = theta.to(DEV), phi.to(DEV)
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 1, *size, generator=g).to(DEV)
    lab = torch.randint(0, 200, (B, 1, *size), generator=g, dtype=torch.uint8).to(DEV)
    cfg = {"gamma": torch.tensor([1.2]), "sigma": torch.tensor([0.05]), "seed": 77, "clip": True}
    ref64, _, rl = A.augment(img, None, lab, theta=th, phi=ph, spacing=s, intensity_cfg=cfg, fill_label=3, dtype=F64)
    ref32 = A.augment(img, None, None, theta=th, phi=ph, spacing=s, intensity_cfg=cfg, dtype=torch.float32)[0]
    gi, gl = ops.augment(img, None, lab, theta=th, phi=ph, spacing=s, intensity=_dev_cfg(cfg, False), fill_label=3)
    check("augment img large", gi, ref64, M.bound(ref32, ref64, 1e-6))
    keep = A.rounding_margin(A.positions(size, th, ph, s, F64), size) >= 1e-4
    assert float((~keep).double().mean()) <= 0.01
    assert gl.dtype == torch.uint8 and bool((gl[:, 0][keep] == rl[:, 0][keep]).all())


# ================================================================================================ augment: labels
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("name", list(CASES))
def test_augment_labels_exact(ops, name, dtype):
    size, s, theta, phi, img, mask, lab, p64 = case_inputs(name)
    lab = lab.to(dtype) * (1 if dtype == torch.uint8 else 70000)             # (int32 values no uint8 could hold)
    ref = A.sample_nearest(lab, p64, fill_label=9)
    keep = A.rounding_margin(p64, size) >= 1e-4
    left_out = float((~keep).double().mean())
    print(f"LEFT OUT {name} {left_out:.2e}")
    assert left_out <= 0.01
    th, ph, (l_dev,) = dev_args(name, theta, phi, lab)
    got, = ops.augment(labels=l_dev, theta=th, phi=ph, spacing=s, fill_label=9)
    got = lifted(name, got).cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    assert bool((got[:, 0][keep] == ref[:, 0][keep]).all()), int((got[:, 0][keep] != ref[:, 0][keep]).sum())
    assert bool((ref == 9).any()) and bool((got != got.flatten()[0]).any())


# ================================================================================================ one launch, exactness
@pytest.mark.parametrize("name", ["small", "odd", "slice"])
def test_one_launch_serves_all_three(ops, name):
    size, s, theta, phi, img, mask, lab, _ = case_inputs(name)
    cfg = _dev_cfg(intensity_configs(img.shape[0], 2 if size[0] == 1 else 3, 5)["all"], size[0] == 1)
    th, ph, (i, m, l) = dev_args(name, theta, phi, img, mask, lab)
    kw = dict(theta=th, phi=ph, spacing=s)
    with LaunchLog() as log:
        gi, gm, gl = ops.augment(i, m, l, intensity=cfg, **kw)
    assert [line.split()[0] for line in log.lines] == ["pulpo_augment_apply"], log.lines
    assert torch.equal(gi, ops.augment(i, intensity=cfg, **kw)[0])
    assert torch.equal(gm, ops.augment(None, m, **kw)[0])
    assert torch.equal(gl, ops.augment(None, None, l, **kw)[0])
    assert torch.equal(gi, ops.augment(i, m, l, intensity=cfg, **kw)[0])          # and the same bits on a second call


@pytest.mark.parametrize("name", ["small", "odd", "slice"])
def test_identity_and_flip_are_exact(ops, name):
    size, s, _, _, img, mask, lab, _ = case_inputs(name)
    two_d = size[0] == 1
    B = img.shape[0]
    img = torch.randn(img.shape, generator=torch.Generator().manual_seed(1)) * 100                     # (any fp32 values, negative ones too)
    _, _, (i, m, l) = dev_args(name, None, None, img, mask, lab)
    l32 = l.to(torch.int32) * 70000
    eye = (torch.eye(2, 3) if two_d else torch.eye(3, 4)).expand(B, -1, -1).contiguous().to(DEV)
    zero_phi = torch.zeros(B, 2 if two_d else 3, *[A.lattice_size(n, s) for n in (size[1:] if two_d else size)], device=DEV)
    for kw in ({}, {"theta": eye}, {"theta": eye, "phi": zero_phi, "spacing": s}):
        gi, gm, gl = ops.augment(i, m, l, **kw)
        assert torch.equal(gi, i) and torch.equal(gm, m) and torch.equal(gl, l), kw.keys()
    assert torch.equal(ops.augment(labels=l32)[0], l32)
    flip = eye.clone()
    flip[:, 0, 0] = -1                                                       # mirrors the first spatial axis (H of a slice, D of a volume)
    gi, gm, gl = ops.augment(i, m, l, theta=flip)
    assert torch.equal(gi, i.flip(2)) and torch.equal(gm, m.flip(2)) and torch.equal(gl, l.flip(2))
    assert torch.equal(ops.augment(labels=l32, theta=flip)[0], l32.flip(2))
    flip_w = eye.clone()
    flip_w[:, -1, -2] = -1                                                   # and the last one, along the vector stores
    gi, gl = ops.augment(i, None, l, theta=flip_w)
    assert torch.equal(gi, i.flip(-1)) and torch.equal(gl, l.flip(-1))


@pytest.mark.parametrize("name", ["small", "larger", "slice"])
def test_fused_kernel_and_field_share_coordinates(ops, name):
    """ops.augment(phi, theta) against the reference sampler applied, in float64, to ops.bspline_field's materialised displacement"""
    size, s, theta, phi, img, mask, lab, p64 = case_inputs(name)
    th, ph, (i_dev,) = dev_args(name, theta, phi, img)
    field = ops.bspline_field(ph, size[1:] if size[0] == 1 else size, s, theta=th)
    if size[0] == 1:
        field = torch.cat([torch.zeros_like(field[:, :1]), field], dim=1).unsqueeze(2)
    p_dev = A.grid(size, F64).unsqueeze(0) + field.double().cpu()
    ref64 = A.sample_linear(img, p_dev)
    ref32 = A.sample_linear(img, A.positions(size, theta, phi, s, torch.float32))
    tol = M.bound(ref32, A.sample_linear(img, p64), 1e-6)
    check(f"augment vs field {name}", lifted(name, ops.augment(i_dev, theta=th, phi=ph, spacing=s)[0]), ref64, tol)


# ================================================================================================ device Philox
def _words(t):
    return [int(v) & 0xFFFFFFFF for v in t.cpu().tolist()]


def test_device_philox_known_answers_and_random_counters(ops):
    for counter, key, words in KAT:
        got = ops.philox4x32(torch.tensor([counter], dtype=torch.int64, device=DEV), torch.tensor(key, dtype=torch.int64, device=DEV))
        assert got.dtype == torch.int32 and _words(got[0]) == list(words)
    g = torch.Generator().manual_seed(0)
    c = torch.randint(0, 2 ** 32, (1000, 4), generator=g, dtype=torch.int64)
    key = (0x12345678, 0x9abcdef0)
    got = ops.philox4x32(c.to(DEV), key).cpu().to(torch.int64) & 0xFFFFFFFF
    want = torch.tensor([A.philox4x32(tuple(row), key) for row in c.tolist()], dtype=torch.int64)
    assert torch.equal(got, want)


def test_noise_is_reproducible_and_standard_normal(ops):
    shape = (2, 1, 12, 14, 16)
    zero = torch.zeros(shape, device=DEV)
    cfg = {"sigma": 1.0, "seed": 20240607}
    a, b = ops.augment(zero, intensity=cfg)[0], ops.augment(zero, intensity=cfg)[0]
    assert torch.equal(a, b)
    assert not torch.equal(a, ops.augment(zero, intensity=dict(cfg, seed=20240608))[0])
    n = a.numel()
    assert n == 5376
    mean, var = float(a.double().mean()), float(a.double().var())
    print(f"NOISE mean {mean:.4f} var {var:.4f}")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / (n - 1))
    ref64, ref32 = A.noise(cfg["seed"], n, F64).view(shape), A.noise(cfg["seed"], n, torch.float32).view(shape)
    check("noise", a, ref64, M.bound(ref32, ref64, 1e-6))
    # the same element gets the same value whatever the batch it arrives in: a pure function of (seed, index)
    assert torch.equal(ops.augment(zero[:1], intensity=cfg)[0], a[:1])


# ================================================================================================ Augmenter and loader
def _batch(B=2, size=(12, 14, 16), seed=3, landmarks=False):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand(B, 1, *size, generator=g), torch.rand(B, 1, *size, generator=g)
    seg_x = torch.randint(0, 4, (B, 1, *size), generator=g, dtype=torch.uint8)
    seg_y = torch.randint(0, 4, (B, 1, *size), generator=g, dtype=torch.uint8)
    mask1 = (torch.rand(B, 1, *size, generator=g) > 0.3).float()
    mask2 = (torch.rand(B, 1, *size, generator=g) > 0.3).to(torch.uint8)
    lm = torch.rand(B, 5, 3, generator=g) * torch.tensor([s - 1.0 for s in size]) if landmarks else torch.empty((0,))
    return tuple(t.to(DEV) for t in (x, y, seg_x, seg_y, lm, lm.clone(), mask1, mask2))


AUG = dict(rotate_deg=10.0, scale=0.1, translate_vox=2.0, flip_axes=(2,), elastic_spacing=4, elastic_std_vox=1.5, gamma=0.3, gain=0.1, offset=0.05,
           noise_std=0.05, bias_std=0.2)


def test_augmenter_on_a_batch(ops):
    from pulpo_amd.augment import Augmenter
    batch = _batch()
    aug = Augmenter((12, 14, 16), seed=21, **AUG)
    out = aug(batch)
    assert len(out) == 8
    for a, b in zip(out, batch):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    assert out[4] is batch[4] and out[5] is batch[5]                          # empty placeholders pass through
    assert not torch.equal(out[0], batch[0]) and not torch.equal(out[2], batch[2])
    params = aug.last_params
    # seg_x and mask1 follow x's map, seg_y and mask2 follow y's: the same parameters through apply() give the call's tensors bit for bit
    gx, gm, gs = aug.apply(params["x"], batch[0], batch[6], batch[2])
    assert torch.equal(gx, out[0]) and torch.equal(gm, out[6]) and torch.equal(gs, out[2])
    gy, gs2 = aug.apply(params["y"], batch[1], None, batch[3])
    assert torch.equal(gy, out[1]) and torch.equal(gs2, out[3])
    assert torch.equal(aug.apply(params["y"], batch[1], None, batch[7])[1], out[7])
    # with intensity off, the call's x is the spatial warp of x through the returned parameters
    spatial = Augmenter((12, 14, 16), seed=21, **{k: v for k, v in AUG.items() if k not in ("gamma", "gain", "offset", "noise_std", "bias_std")})
    out_s = spatial(batch)
    assert torch.equal(aug.apply(spatial.last_params["x"], batch[0], intensity=False)[0], out_s[0])
    assert torch.equal(spatial.last_params["x"]["theta"], params["x"]["theta"]) and torch.equal(out_s[2], out[2])
    # against the float64 definition, and label values stay within the input's set (0 is also the fill label)
    p64 = A.positions((12, 14, 16), params["x"]["theta"], params["x"]["phi"], 4, F64)
    keep = A.rounding_margin(p64, (12, 14, 16)) >= 1e-4
    assert bool((out[2].cpu()[:, 0][keep] == A.sample_nearest(batch[2].cpu(), p64)[:, 0][keep]).all())
    assert set(out[2].unique().tolist()) <= set(batch[2].unique().tolist()) | {0}
    assert set(out[7].unique().tolist()) <= {0, 1}
    # two augmenters with one seed agree bit for bit; another seed does not
    again = Augmenter((12, 14, 16), seed=21, **AUG)(batch)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert not torch.equal(Augmenter((12, 14, 16), seed=22, **AUG)(batch)[0], out[0])


def test_augmenter_identity_and_one_hot_route(ops):
    from pulpo_amd.augment import Augmenter
    batch = _batch()
    out = Augmenter((12, 14, 16), seed=1)(batch)
    assert all(torch.equal(a, b) for a, b in zip(out, batch))
    onehot = torch.nn.functional.one_hot(batch[2][:, 0].long(), 4).permute(0, 4, 1, 2, 3).float().contiguous()
    aug = Augmenter((12, 14, 16), seed=2, rotate_deg=10.0, translate_vox=2.0, gamma=0.3, shared_spatial=True)
    out = aug((batch[0], batch[1], onehot, onehot, batch[4], batch[5], batch[6], batch[7]))
    assert out[2].shape == onehot.shape and out[2].dtype == torch.float32
    assert torch.equal(out[2], out[3])                                        # one map for both sides; no intensity on the one-hot maps
    th = aug.last_params["x"]["theta"]
    ref64, ref32 = (A.sample_linear(onehot.cpu(), A.positions((12, 14, 16), th, dtype=dt)) for dt in (F64, torch.float32))
    check("one-hot through the augmenter", out[2], ref64, M.bound(ref32, ref64, 1e-6))


def test_augmenter_carries_landmarks_through_an_affine(ops):
    from pulpo_amd.augment import Augmenter
    batch = _batch(landmarks=True)
    aug = Augmenter((12, 14, 16), seed=5, rotate_deg=10.0, scale=0.1, translate_vox=2.0, flip_axes=(0,))
    out = aug(batch)
    c = torch.tensor([5.5, 6.5, 7.5], dtype=F64)
    for side, k in (("x", 4), ("y", 5)):
        th = aug.last_params[side]["theta"].double()
        P = batch[k].cpu().double()
        want = c + torch.einsum("bij,bnj->bni", torch.linalg.inv(th[:, :, :3]), P - c - th[:, :, 3].unsqueeze(1))
        assert out[k].shape == batch[k].shape and out[k].dtype == batch[k].dtype
        # fp32 landmarks of magnitude below 32: half an ulp is 2e-6
        assert float((out[k].cpu().double() - want).abs().max()) <= 4e-6
        # and the augmented image shows the point there: the map sends the new position back to the old one
        back = c + torch.einsum("bij,bnj->bni", th[:, :, :3], want - c) + th[:, :, 3].unsqueeze(1)
        assert float((back - P).abs().max()) < 1e-9
    with pytest.raises(ValueError, match="landmarks"):
        Augmenter((12, 14, 16), seed=5, elastic_spacing=4, elastic_std_vox=1.0)(batch)


def test_training_step_through_the_loader(ops):
    import src.models as models
    from oracle import pulpo_oracle as O
    from pulpo_amd.augment import AugmentedLoader, Augmenter
    size, C = (32, 32, 32), 4
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(1, 1, *size, generator=g), torch.rand(1, 1, *size, generator=g)
    seg = torch.randint(0, C, (1, 1, *size), generator=g, dtype=torch.uint8)
    mask = torch.ones(1, 1, *size)
    empty = torch.empty((0,))
    batch = tuple(t.to(DEV) for t in (x, y, seg, seg.roll(1, 3).contiguous(), empty, empty, mask, mask.clone()))
    aug = Augmenter(size, seed=9, rotate_deg=10.0, scale=0.1, translate_vox=2.0, elastic_spacing=8, elastic_std_vox=1.5, gamma=0.3, noise_std=0.03,
                    bias_std=0.2)
    loader = AugmentedLoader([batch, batch], aug)
    assert len(loader) == 2
    torch.manual_seed(0)
    model = models.PULPo(3, 2, 0.1, list(size), feedback=list(O.FEEDBACK_DEFAULT), n0=8, recon_loss=["ncc", "dice"], segs=True, mask=True,
                         num_classes=C).to(DEV).train()
    seen = []
    for b in loader:
        assert b[2].dtype == torch.uint8 and b[6].dtype == torch.float32 and float(b[6].min()) < 1.0      # the mask's fill region arrived
        model.zero_grad(set_to_none=True)
        loss = model.training_step(b, 0)
        loss.backward()
        assert bool(torch.isfinite(loss))
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g_).all()) for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)
        seen.append(b[0])
    assert not torch.equal(seen[0], seen[1])                                  # every pass draws anew
