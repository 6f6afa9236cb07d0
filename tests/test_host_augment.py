"""Training augmentation, the parts that need no GPU: the float64 definitions of tests/augment_ref.py hold the published
Philox vectors and the B-spline's defining properties, the reference sampler is grid_sample(align_corners=True, padding_mode="zeros"), the C
prototypes are declared and exported, Augmenter.draw is reproducible and stays inside its ranges, and every refusal is raised before a GPU is
needed."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import augment_ref as A

# Random123's known answers for Philox4x32-10 (kat_vectors): counter, key, words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ================================================================================================ Philox
@pytest.mark.parametrize("counter, key, words", KAT)
def test_philox_known_answers(counter, key, words):
    assert tuple(A.philox4x32(counter, key)) == words


def test_philox_array_form_matches_the_integer_form():
    import numpy as np
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    got = A.philox4x32(tuple(c), (np.uint64(0xa4093822), np.uint64(0x299f31d0)))
    for j in range(50):
        assert tuple(int(w[j]) for w in got) == tuple(A.philox4x32(tuple(int(v) for v in c[:, j]), (0xa4093822, 0x299f31d0)))


def test_noise_is_a_function_of_seed_and_index():
    n = A.noise(1234, 4096)
    assert torch.equal(n[:1001], A.noise(1234, 1001))               # independent of how many elements are asked for
    assert not torch.equal(n, A.noise(1235, 4096))
    assert abs(float(n.mean())) < 5 / math.sqrt(4096) and abs(float(n.var()) - 1) < 5 * math.sqrt(2 / 4096)


# ================================================================================================ B-spline
def test_bspline_partition_of_unity():
    size, s = (9, 10, 13), 4
    G = tuple(A.lattice_size(S, s) for S in size)
    phi = torch.tensor([0.75, -1.5, 2.25], dtype=torch.float64).view(1, 3, 1, 1, 1).expand(1, 3, *G).contiguous()
    e = A.bspline_field(phi, size, s)
    assert float((e - phi[:, :, :1, :1, :1]).abs().max()) <= 1e-12


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_bspline_reproduces_a_linear_field(s):
    """phi_j = a s (j - 1) along z gives e = a z to 1e-12 in float64: the lattice's offset is pinned"""
    size, a = (17, 6, 5), 0.37
    G = tuple(A.lattice_size(S, s) for S in size)
    phi = torch.zeros(1, 3, *G, dtype=torch.float64)
    phi[0, 0] = (a * s * (torch.arange(G[0], dtype=torch.float64) - 1)).view(-1, 1, 1)
    e = A.bspline_field(phi, size, s)
    want = (a * torch.arange(size[0], dtype=torch.float64)).view(-1, 1, 1).expand(size)
    assert float((e[0, 0] - want).abs().max()) <= 1e-12
    assert float(e[0, 1:].abs().max()) == 0


def test_bspline_is_c2_across_a_knot():
    """second differences of step h left and right of a knot agree (a C1-only curve would show a jump of the order of the lattice values)"""
    u = torch.tensor([1.0], dtype=torch.float64)
    z = torch.zeros(1, dtype=torch.float64)
    phi = torch.tensor([0.3, -1.1, 0.8, 1.9, -0.4], dtype=torch.float64)

    def curve(t):                         # cell 0 on [0, 1), cell 1 on [1, 2)
        i = int(t)
        return sum(float(b) * float(phi[i + l]) for l, b in enumerate(A.bspline_basis(torch.tensor(t - i, dtype=torch.float64))))

    h = 1e-3
    left = (curve(1 - 2 * h) - 2 * curve(1 - h) + curve(1.0)) / h ** 2
    right = (curve(1.0) - 2 * curve(1 + h) + curve(1 + 2 * h)) / h ** 2
    assert abs(left - right) < 20 * h                    # the third derivative is bounded by a few lattice values: O(h) apart, no jump
    end = [float(b) for b in A.bspline_basis(u)]          # value continuity: B(1) of a cell is B(0) of the next, shifted
    start = [float(b) for b in A.bspline_basis(z)]
    assert end[0] == 0 and start[3] == 0 and max(abs(end[l + 1] - start[l]) for l in range(3)) < 1e-15


# ================================================================================================ sampler
def _positions(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    p = A.grid(size, torch.float64).unsqueeze(0) + 2.5 * torch.randn(B, 3, *size, generator=g, dtype=torch.float64)
    return p


def test_sampler_is_grid_sample_3d():
    size, B, C = (6, 7, 9), 2, 2
    src = torch.randn(B, C, *size, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    p = _positions(B, size, 2)
    norm = torch.stack([2 * p[:, 2] / (size[2] - 1) - 1, 2 * p[:, 1] / (size[1] - 1) - 1, 2 * p[:, 0] / (size[0] - 1) - 1], dim=-1)
    want = F.grid_sample(src, norm, mode="bilinear", padding_mode="zeros", align_corners=True)
    got = A.sample_linear(src, p)
    assert float((got - want).abs().max()) < 1e-12
    assert float((got == 0).double().mean()) > 0.01           # some samples lie outside the volume


def test_sampler_is_grid_sample_2d():
    size, B, C = (1, 8, 11), 2, 3
    src = torch.randn(B, C, *size, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    p = _positions(B, size, 4)
    p[:, 0] = 0
    norm = torch.stack([2 * p[:, 2, 0] / (size[2] - 1) - 1, 2 * p[:, 1, 0] / (size[1] - 1) - 1], dim=-1)
    want = F.grid_sample(src[:, :, 0], norm, mode="bilinear", padding_mode="zeros", align_corners=True)
    assert float((A.sample_linear(src, p)[:, :, 0] - want).abs().max()) < 1e-12


def test_identity_and_fill():
    size = (4, 5, 6)
    src = torch.randn(1, 1, *size, dtype=torch.float64)
    lab = torch.randint(0, 5, (1, 1, *size), dtype=torch.uint8)
    p = A.positions(size)
    assert torch.equal(A.sample_linear(src, p), src) and torch.equal(A.sample_nearest(lab, p), lab)
    far = p + 100
    assert bool((A.sample_linear(src, far, fill=0.5) == 0.5).all()) and bool((A.sample_nearest(lab, far, fill_label=7) == 7).all())


# ================================================================================================ library
def test_prototypes_are_declared_and_exported():
    from pulpo_amd._lib import LIB_PATH, header_abi_version, parse_header
    protos = parse_header()
    for name, nargs in (("pulpo_augment_apply", 29), ("pulpo_bspline_field", 12), ("pulpo_philox4x32", 5)):
        assert name in protos, name
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))
    assert header_abi_version() == 8
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("pulpo_augment_apply", "pulpo_bspline_field", "pulpo_philox4x32"):
        assert hasattr(dll, name), f"{LIB_PATH} does not export {name}"


# ================================================================================================ Augmenter.draw
FULL = dict(rotate_deg=10.0, scale=0.1, shear=0.05, translate_vox=(2.0, 3.0, 4.0), flip_axes=(0, 2), elastic_spacing=4, elastic_std_vox=1.5,
            gamma=0.3, gain=0.2, offset=0.1, noise_std=0.05, bias_std=0.3, bias_nodes=3)


def _aug(size=(12, 14, 16), seed=0, **kw):
    from pulpo_amd.augment import Augmenter
    return Augmenter(size, seed=seed, **kw)


def _flat(params):
    out = []
    for side in ("x", "y"):
        m = params[side]
        out += [m["theta"]] + ([m["phi"]] if m["phi"] is not None else []) + [v for v in m["intensity"].values() if torch.is_tensor(v)]
    return out


def test_draw_is_reproducible():
    a, b, c = (_aug(seed=s, **FULL).draw(3) for s in (5, 5, 6))
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))
    assert not torch.equal(a["x"]["theta"], c["x"]["theta"]) and not torch.equal(a["x"]["phi"], c["x"]["phi"])
    assert not torch.equal(a["x"]["theta"], a["y"]["theta"])                 # two maps per pair


def test_draw_respects_every_range():
    B = 64
    p = _aug(seed=1, **FULL).draw(B)
    for side in ("x", "y"):
        m = p[side]
        theta, it = m["theta"].double(), m["intensity"]
        assert theta.shape == (B, 3, 4) and theta.dtype == torch.float64 and m["theta"].dtype == torch.float32
        for a, t in enumerate(FULL["translate_vox"]):
            assert float(theta[:, a, 3].abs().max()) <= t
        sv = torch.linalg.svdvals(theta[:, :, :3])
        # singular values of R Sh diag(s) F lie within the scale range widened by the shear: Sh = I + N, |N| <= 0.05 sqrt(3) (three entries
        # of at most 0.05), |Sh| <= 1 + |N| and |Sh^-1| <= 1 / (1 - |N|)
        slack = 1 / (1 - 0.05 * math.sqrt(3))
        assert float(sv.max()) <= 1.1 * slack and float(sv.min()) >= 0.9 / slack
        assert m["spacing"] == 4 and m["phi"].shape == (B, 3, 6, 7, 7)
        assert abs(float(m["phi"].std()) - 1.5) < 0.05
        assert float(it["gamma"].log().abs().max()) <= 0.3 + 1e-6
        assert float((it["gain"] - 1).abs().max()) <= 0.2 + 1e-6 and float(it["offset"].abs().max()) <= 0.1 + 1e-6
        assert float(it["sigma"].min()) >= 0 and float(it["sigma"].max()) <= 0.05 + 1e-6
        assert it["bias"].shape == (B, 3, 3, 3) and it["seed"].dtype == torch.int64 and it["clip"] is True
    dets = torch.linalg.det(p["x"]["theta"][:, :, :3].double())
    assert bool((dets < 0).any()) and bool((dets > 0).any())                  # an even and an odd number of flips both occur
    # rotation alone: the angle about each axis stays within its range
    r = _aug(seed=2, rotate_deg=(10.0, 0.0, 0.0)).draw(B)["x"]["theta"].double()
    ang = torch.atan2(r[:, 2, 1], r[:, 1, 1]) * 180 / math.pi
    assert float(ang.abs().max()) <= 10.0 + 1e-4 and float(ang.abs().max()) > 5.0
    assert float((r[:, 0, :3] - torch.tensor([1.0, 0, 0], dtype=torch.float64)).abs().max()) < 1e-7


def test_zero_ranges_give_the_identity():
    p = _aug(seed=3).draw(2)
    eye = torch.eye(3, 4).expand(2, 3, 4)
    for side in ("x", "y"):
        assert torch.equal(p[side]["theta"], eye) and p[side]["phi"] is None and p[side]["spacing"] is None and p[side]["intensity"] == {}
    p2 = _aug(size=(20, 24), seed=3).draw(2)
    assert torch.equal(p2["x"]["theta"], torch.eye(2, 3).expand(2, 2, 3))


def test_rigid_draw_is_a_rotation():
    theta = _aug(seed=4, rotate_deg=25.0, scale=0.3, shear=0.2, translate_vox=3.0, rigid=True).draw(16)["x"]["theta"].double()
    M = theta[:, :, :3]
    assert float((M @ M.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float((torch.linalg.det(M) - 1).abs().max()) <= 1e-6
    assert float((M - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.05


def test_shared_spatial_draws_one_map():
    p = _aug(seed=5, shared_spatial=True, **FULL).draw(2)
    assert torch.equal(p["x"]["theta"], p["y"]["theta"]) and torch.equal(p["x"]["phi"], p["y"]["phi"])
    assert not torch.equal(p["x"]["intensity"]["gamma"], p["y"]["intensity"]["gamma"])


def test_to_device_keeps_the_values():
    from pulpo_amd.augment import Augmenter
    p = _aug(seed=6, shared_spatial=True, **FULL).draw(2)
    q = Augmenter.to_device(p, "cpu")
    assert all(torch.equal(u, v) for u, v in zip(_flat(p), _flat(q)))
    assert q["x"]["theta"].data_ptr() == q["y"]["theta"].data_ptr()           # the shared map is staged once


# ================================================================================================ refusals (CPU tensors: nothing is launched)
def _src(B=2, size=(6, 7, 8)):
    return torch.zeros(B, 1, *size), torch.zeros(B, 1, *size), torch.zeros(B, 1, *size, dtype=torch.uint8)


def _phi(B=2, size=(6, 7, 8), s=2):
    return torch.zeros(B, 3, *[A.lattice_size(S, s) for S in size])


def test_operator_refusals():
    from pulpo_amd import ops
    img, mask, lab = _src()
    eye = torch.eye(3, 4).expand(2, 3, 4).contiguous()
    cases = {
        "no source": lambda: ops.augment(),
        "batch size": lambda: ops.augment(img, mask[:1], lab),
        "grid": lambda: ops.augment(img, mask[:, :, :5], None),
        "theta batch": lambda: ops.augment(img, theta=eye[:1]),
        "phi batch": lambda: ops.augment(img, phi=_phi(1), spacing=2),
        "lattice extents": lambda: ops.augment(img, phi=_phi()[:, :, :-1], spacing=2),
        "lattice for another spacing": lambda: ops.augment(img, phi=_phi(s=2), spacing=3),
        "spacing 1": lambda: ops.augment(img, phi=torch.zeros(2, 3, 8, 9, 10), spacing=1),
        "no spacing": lambda: ops.augment(img, phi=_phi()),
        "float labels": lambda: ops.augment(img, None, lab.float()),
        "int64 labels": lambda: ops.augment(img, None, lab.long()),
        "grad": lambda: ops.augment(img.clone().requires_grad_(True)),
        "mask grad": lambda: ops.augment(img, mask.clone().requires_grad_(True)),
        "2-D theta, 3-D image": lambda: ops.augment(img, theta=torch.eye(2, 3).expand(2, 2, 3)),
        "3-D theta, 2-D image": lambda: ops.augment(img[:, :, 0], theta=eye),
        "2-D mask, 3-D image": lambda: ops.augment(img, mask[:, :, 0]),
        "2-D phi, 3-D image": lambda: ops.augment(img, phi=torch.zeros(2, 2, 6, 7), spacing=2),
        "unknown intensity key": lambda: ops.augment(img, intensity={"contrast": 1.0}),
        "sigma without seed": lambda: ops.augment(img, intensity={"sigma": 0.1}),
        "intensity without image": lambda: ops.augment(None, mask, intensity={"gamma": 1.2}),
        "field: spacing": lambda: ops.bspline_field(_phi(), (6, 7, 8), 1),
        "field: extents": lambda: ops.bspline_field(_phi(), (6, 7, 10), 2),
        "field: theta": lambda: ops.bspline_field(_phi(), (6, 7, 8), 2, theta=torch.eye(2, 3).expand(2, 2, 3)),
        "philox: counters": lambda: ops.philox4x32(torch.zeros(3, 3, dtype=torch.int32), [0, 0]),
    }
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: not refused")


def test_augmenter_refuses_landmarks_under_an_elastic_map():
    aug = _aug(seed=0, elastic_spacing=4, elastic_std_vox=1.0)
    x = torch.zeros(1, 1, 12, 14, 16)
    empty = torch.empty((0,))
    lm = torch.zeros(1, 5, 3)
    with pytest.raises(ValueError, match="landmarks"):
        aug((x, x, empty, empty, lm, lm, empty, empty))
    with pytest.raises(ValueError):
        _aug(elastic_std_vox=1.0)                                             # an elastic part needs a spacing
    with pytest.raises(ValueError):
        _aug(size=(12, 14, 16))((x[:, :, :10], x, empty, empty, empty, empty, empty, empty))


def test_landmark_transport_inverts_the_affine():
    """CPU, float64: a point P of the input shows in the output at the v with p(v) = P"""
    aug = _aug(seed=7, rotate_deg=10.0, scale=0.1, translate_vox=2.0)
    theta = aug.draw(2)["x"]["theta"]
    lm = torch.rand(2, 6, 3, dtype=torch.float64) * 10
    v = aug.transport_landmarks(lm, theta)
    c = torch.tensor([5.5, 6.5, 7.5], dtype=torch.float64)
    th = theta.double()
    back = c + torch.einsum("bij,bnj->bni", th[:, :, :3], v - c) + th[:, :, 3].unsqueeze(1)
    assert float((back - lm).abs().max()) < 1e-10
