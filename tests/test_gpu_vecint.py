"""The VecInt (scaling-and-squaring) kernels against float64, element by element and step by step (references and field generators in
tests/pyramid_ref.py, pinned to the oracle on the CPU by tests/test_oracle_golden.py).

  forward    pulpo_vecint_fwd into a NaN-filled `work`: every stored field work[k] against the float64 chain, on both sides of the
             2048-voxel switch between the one-launch LDS kernel and the step-by-step kernels, nsteps 0 / 1 / 2 / 7, a depth-1 grid;
             pulpo_vecint_pair_fwd (both directions) at the same cases.
  one step   pulpo_vecint_bwd / pulpo_vecint_bwd_det with nsteps = 1 and work = [w, step(w)] run exactly one backward squaring step on a
             field of the test's choosing: twice the result is g + gd + gi.  The field's size selects the kernel: the plain scatter
             (warp_bwd_kernel<true>: an axis below 8), the LDS-tiled scatter with a one-voxel rim (vecint_bwd_tile_kernel<1>) and with a
             two-voxel rim (<2>: from 64^3 voxels on); the deterministic call runs warp_bwd_fx_kernel<true> at every size.
  chain      the nsteps-step call equals the same entry point applied nsteps times with nsteps = 1 - bit for bit in deterministic mode.
  autograd   ops.vecint forward and gradient, both modes, against the float64 oracle.

Bounds follow test_warp_vs_float64 (tests/test_gpu_pyramid_ops.py): max(1e-5 max(1, max|ref|), twice the spread of torch's own fp32
evaluation of the same expression on the same data).  The displacement-role gradient gd jumps where a sample coordinate crosses a cell
boundary or a clamp: voxels whose float64 coordinate lies within 1e-4 voxel of one (`bnd`) are allowed, on top, the largest change of the
float64 gd under a nudge of the displacement by +-2e-4 voxel along each axis.  The image-role scatter gi is continuous there and gets no
allowance.  Every comparison must reject the reference with one element moved by 1e-3 of its maximum."""
import ctypes

import pytest
import torch

import pyramid_ref as R
import test_gpu_pyramid_ops as P          # check() and the "faces" field of the warp tests
from oracle import pulpo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
check, amax = P.check, P.amax


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


def _lib():
    from pulpo_amd._lib import lib
    return lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the entry points, through the C ABI
def run_fwd(v, nsteps):
    """pulpo_vecint_fwd into a NaN-filled work: (nsteps + 1, B, 3, D, H, W)"""
    B, _, D, H, W = v.shape
    work = torch.full((nsteps + 1, B, 3, D, H, W), NAN, device=DEV)
    _lib().call("pulpo_vecint_fwd", _ptr(v), _ptr(work), B, D, H, W, nsteps, _stream())
    return work


def run_pair(v, nsteps):
    """pulpo_vecint_pair_fwd into NaN-filled outputs with a NaN-filled scratch: (fwd, inv, scratch floats asked for)"""
    B, _, D, H, W = v.shape
    nscr = int(_lib().query("pulpo_vecint_pair_scratch_floats", B, D, H, W, nsteps))
    scratch = torch.full((nscr,), NAN, device=DEV) if nscr else None
    fwd, inv = torch.full_like(v, NAN), torch.full_like(v, NAN)
    _lib().call("pulpo_vecint_pair_fwd", _ptr(v), _ptr(fwd), _ptr(inv), _ptr(scratch), B, D, H, W, nsteps, _stream())
    return fwd, inv, nscr


def scratch_size(det, B, size, nsteps) -> int:
    """bytes of workspace (deterministic) or floats of scratch (atomic) the library asks for"""
    return int(_lib().query("pulpo_vecint_bwd_det_ws_bytes" if det else "pulpo_vecint_bwd_tmp_floats", B, *size, nsteps))


def run_bwd(det, work, g, nsteps, scratch=None):
    """pulpo_vecint_bwd_det / pulpo_vecint_bwd on work (nsteps + 1 fields) into a NaN-filled gin.  scratch None: a fresh one with every
    byte 0xFF (NaN as floats, -1 as the fixed-point accumulators), or nothing when the query returns 0.  Returns (gin, scratch)"""
    assert work.is_contiguous() and g.is_contiguous() and work.shape[0] == nsteps + 1
    B, _, D, H, W = g.shape
    n = scratch_size(det, B, (D, H, W), nsteps)
    if scratch is None and n:
        scratch = torch.full((n if det else 4 * n,), 0xFF, device=DEV, dtype=torch.uint8)
    gin = torch.full_like(g, NAN)
    _lib().call("pulpo_vecint_bwd_det" if det else "pulpo_vecint_bwd", _ptr(work), _ptr(g), _ptr(gin), _ptr(scratch), B, D, H, W, nsteps, _stream())
    return gin, scratch


def kernel_of(size) -> str:
    """the backward squaring step's kernel in pulpo_vecint_bwd (warp.hip: vecint_bwd_tiled, and the R = 2 rule for the last step)"""
    D, H, W = size
    if min(size) < 8:
        return "plain"
    return "tile2" if D * H * W >= 64 ** 3 else "tile1"


# ================================================================================================ forward: every stored field
# (B, size, nsteps, peak displacement of the smooth field).  2048 voxels is the last size of the one-launch LDS kernels, 8x16x17 the first
# of the step-by-step ones; 2025 voxels is no multiple of the 1024 threads; nsteps = 1 and 0; a depth-1 grid; 66x63x65 is odd on every axis
# and more than one trip of the capped grid
FWD_CASES = [(2, (8, 16, 16), 7, 12.0), (2, (8, 16, 17), 7, 12.0), (1, (9, 15, 15), 7, 6.0), (2, (10, 10, 10), 1, 3.0), (1, (20, 20, 20), 7, 8.0),
             (1, (12, 14, 10), 0, 5.0), (1, (1, 24, 20), 7, 9.0), (1, (66, 63, 65), 2, 4.0)]


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("B,size,nsteps,amp", FWD_CASES)
def test_forward_every_stored_field_vs_float64(ops, B, size, nsteps, amp, kind):
    """work[k] for every k (NaN on entry: every buffer must be written) and both outputs of the pair kernel.  The forward is continuous in
    the field, so no element is exempt.  Smooth fields with peak displacements of 3 - 12 voxels (samples clamped at every face of the last
    step) and white noise of amplitude 3"""
    if kind == "noise":
        amp = 3.0
    v = R.vecint_field(kind, B, size, amp=amp, seed=size[2] + nsteps).to(DEV)
    V = size[0] * size[1] * size[2]
    name = f"vecint fwd {B}/{size}/n{nsteps}/{kind}"
    if kind == "smooth":
        assert 3.0 <= amp <= 12.0 and abs(amax(v) - amp) < 1e-4
    work = run_fwd(v, nsteps)
    fwd, inv, nscr = run_pair(v, nsteps)
    assert nscr == (0 if V <= 2048 or nsteps == 0 else 2 * v.numel()), (name, nscr)
    for sign, pair_out in ((1.0, fwd), (-1.0, inv)):
        ref = R.vecint_chain_ref(sign * v.double(), nsteps)
        r32 = R.vecint_chain_ref(sign * v, nsteps)
        if nsteps > 0:
            assert R.vecint_clamped_at_every_face(ref[nsteps - 1]), name
        tols = [max(1e-5 * max(1.0, amax(r)), 2 * R.ratio(s, r, 1.0)) for r, s in zip(ref, r32)]
        print(f"RATIO {name} sign {sign:+.0f} spread32 of the last field {R.ratio(r32[-1], ref[-1], 1.0):.3g} tol {tols[-1]:.3g}")
        if sign > 0:
            for k in range(nsteps + 1):
                check(f"{name} work[{k}]", work[k], ref[k], tols[k])
        check(f"{name} pair {'fwd' if sign > 0 else 'inv'}", pair_out, ref[-1], tols[-1])
    if nsteps == 0:
        assert torch.equal(work[0], v) and torch.equal(fwd, v) and torch.equal(inv, -v)


# ================================================================================================ one backward squaring step
def step_field(kind, B, size, seed):
    """the field w of one squaring step, on the device.  smooth_small: below one voxel, everything stays in the tile's box and the lane
    merges fire almost everywhere; smooth_large: 0 to 4 voxels within a tile, in-box lanes and memory-atomic fallback lanes side by side in
    one wave; bands: neighbouring lanes sample the same cell, adjacent cells and cells two apart; faces: samples clamped at all six faces
    and slabs exactly on the border indices (the warp tests' field); noise: almost no merges; zero: every lane of a row merges"""
    if kind == "faces":
        w = P._warp_field(gen(seed), B, size, size, 3.0, "faces")
        if size[0] == 1:
            w[:, 0] = 0
        return w.contiguous()
    amp = {"smooth_small": 0.9, "smooth_large": 4.0, "noise": 3.0}.get(kind, 0.0)
    src = "smooth" if kind == "smooth_small" else kind
    return R.vecint_field(src, B, size, amp=amp, seed=seed).to(DEV)


class StepRef:
    """float64 reference of one backward squaring step for (w, g), the fp32 torch evaluation's spread, the boundary set and the bound"""

    def __init__(self, w, g, with_spread=True):
        w64, g64 = w.double(), g.double()
        self.gd, self.gi = R.vecint_step_grads_ref(w64, g64)
        self.ref = g64 + self.gd + self.gi
        self.bnd = R.vecint_near_cell_boundary(w64)
        self.share = float(self.bnd[:, 0].float().mean())
        off = ~self.bnd
        nudge = torch.zeros_like(self.ref)
        for a, S, _ in R.vecint_coords(w64):          # one axis at a time, 2e-4 voxel of the sample coordinate to either side
            for sgn in (1.0, -1.0):
                d = w64.clone()
                d[:, a] += sgn * 2e-4 * (S - 1) / S
                nudge = torch.maximum(nudge, (R.vecint_step_grads_ref(w64, g64, disp=d)[0] - self.gd).abs())
        self.spread = 0.0
        if with_spread:
            gd32, gi32 = R.vecint_step_grads_ref(w, g)
            self.r32 = g + gd32 + gi32
            self.spread = float((self.r32.double() - self.ref).abs()[off].max())
        self.floor = 1e-5 * max(1.0, amax(self.ref))
        self.tol = max(self.floor, 2 * self.spread)
        self.tol_t = torch.where(self.bnd, self.tol + nudge, torch.full_like(nudge, self.tol))
        self.last_inner = int(torch.nonzero(off.reshape(-1)).reshape(-1)[-1])
        self.off = off


def step_work(w, nan_next=False):
    """work = [w, step(w)]: the float64 step rounded to fp32 - or NaN: the backward pass reads work[0] only"""
    nxt = torch.full_like(w, NAN) if nan_next else R.vecint_step_ref(w.double()).float()
    return torch.stack([w, nxt]).contiguous()


def check_step(name, w, g, sr, nan_next=False, power=True):
    """2 * gin of a one-step call, atomic and deterministic, against sr.ref"""
    B, size = w.shape[0], tuple(w.shape[2:])
    n, tiled = w.numel(), kernel_of(size) != "plain"
    assert scratch_size(False, B, size, 1) == (n if tiled else 2 * n), (name, kernel_of(size))          # the library's own choice of kernel
    work = step_work(w, nan_next)
    out = {}
    for det in (False, True):
        gin, _ = run_bwd(det, work, g, 1)
        out[det] = 2 * gin
        kern = "fx" if det else kernel_of(size)
        print(f"RATIO {name} {kern} off bnd {R.ratio(out[det][sr.off], sr.ref[sr.off], sr.tol):.3g}")
        check(f"{name} {kern}", out[det], sr.ref, sr.tol_t, power=sr.last_inner if power else None)
    return out


# size -> (B, kernel of the atomic call).  One axis below 8 and the depth-1 grid: the plain scatter; 8^3 is one tile column of two full
# tiles; 9x17x15 and 12x26x29 have partial tiles on all three axes; 64^3 is the first size of the two-voxel rim, 66x63x65 (270 270 >= 64^3)
# has partial tiles on all axes
STEP_SIZES = {(6, 7, 5): (2, "plain"), (7, 16, 16): (2, "plain"), (1, 24, 20): (2, "plain"), (8, 8, 8): (2, "tile1"), (9, 17, 15): (2, "tile1"),
              (24, 20, 28): (2, "tile1"), (12, 26, 29): (2, "tile1"), (64, 64, 64): (1, "tile2"), (66, 63, 65): (1, "tile2")}
STEP_CASES = [((6, 7, 5), "smooth_small"), ((6, 7, 5), "noise"), ((7, 16, 16), "smooth_large"), ((1, 24, 20), "smooth_large"), ((1, 24, 20), "noise"),
              ((8, 8, 8), "smooth_small"), ((8, 8, 8), "zero"), ((8, 8, 8), "noise"),
              ((9, 17, 15), "smooth_small"), ((9, 17, 15), "smooth_large"), ((9, 17, 15), "bands"), ((9, 17, 15), "faces"), ((9, 17, 15), "noise"),
              ((24, 20, 28), "smooth_small"), ((24, 20, 28), "smooth_large"), ((24, 20, 28), "bands"), ((24, 20, 28), "faces"), ((24, 20, 28), "noise"),
              ((24, 20, 28), "zero"), ((12, 26, 29), "bands"), ((12, 26, 29), "smooth_large"),
              ((64, 64, 64), "zero"), ((64, 64, 64), "smooth_small"), ((64, 64, 64), "faces"), ((64, 64, 64), "bands"),
              ((66, 63, 65), "smooth_small"), ((66, 63, 65), "smooth_large"), ((66, 63, 65), "bands"), ((66, 63, 65), "noise"), ((66, 63, 65), "faces")]


def test_step_cases_cover_every_kernel_and_field():
    """each field kind runs through the one-voxel-rim and the two-voxel-rim tile kernel at least once, and the sizes select what they say"""
    for size, (_, kern) in STEP_SIZES.items():
        assert kernel_of(size) == kern, size
    for kind in ("smooth_small", "smooth_large", "bands", "faces", "noise", "zero"):
        assert {"tile1", "tile2"} <= {STEP_SIZES[s][1] for s, k in STEP_CASES if k == kind}, kind
    assert {s for s, _ in STEP_CASES} == set(STEP_SIZES)


@pytest.mark.parametrize("size,kind", STEP_CASES)
def test_backward_step_vs_float64(ops, size, kind):
    """one backward squaring step with a random upstream gradient through the kernel the size selects and through the fixed-point kernel.
    The band fields run with work[1] = NaN: the backward pass reads work[0] only"""
    B = STEP_SIZES[size][0]
    seed = size[0] * 100 + size[2] + len(kind)
    w = step_field(kind, B, size, seed)
    g = torch.randn(B, 3, *size, device=DEV, generator=gen(seed + 1))
    sr = StepRef(w, g)
    name = f"vecint step {B}/{size}/{kind}"
    print(f"RATIO {name} spread32 off bnd {sr.spread:.3g} / floor {sr.floor:.3g} = {sr.spread / sr.floor:.3g}; bnd share {sr.share:.3g}; "
          f"fp32 torch itself, all voxels {R.ratio(sr.r32, sr.ref, sr.tol_t):.3g}")
    if kind == "faces":          # slabs are put exactly on the border indices and on interior integers, on purpose (as in test_warp_vs_float64)
        assert sr.share > 0 and R.vecint_clamped_at_every_face(w.double())
    else:
        assert sr.share < 0.01, (name, sr.share)
    if kind == "bands":
        assert sr.share == 0
    if kind == "smooth_small":
        assert amax(w) < 1.0
    if kind == "smooth_large":          # within single tiles the displacement spans most of 0 .. 4 voxels
        assert float((w[..., :8].amax(-1) - w[..., :8].amin(-1)).max()) > 2.0
    check_step(name, w, g, sr, nan_next=kind == "bands")


def _delta_voxels(size):
    D, H, W = size
    return {"first": (0, 0, 0), "last": (D - 1, H - 1, W - 1), "lane7": (D // 2, H // 2, 7)}     # x = 7: the right neighbour belongs to another workgroup


@pytest.mark.parametrize("kind", ["smooth_small", "smooth_large"])
@pytest.mark.parametrize("size", [(24, 20, 28), (66, 63, 65)])
def test_backward_step_delta_gradients(ops, size, kind):
    """an upstream gradient with one non-zero element: the float64 result has at most 27 non-zero elements (8 corners, the displacement
    gradient's three channels, the identity path).  Each must be in its place, and everything else exactly 0 on the device"""
    B = STEP_SIZES[size][0]
    w = step_field(kind, B, size, 11 + size[0])
    w64 = w.double()
    bnd = R.vecint_near_cell_boundary(w64)
    for tag, (z, y, x) in _delta_voxels(size).items():
        assert not bool(bnd[B - 1, 0, z, y, x]), (tag, "the delta voxel's own sample lies on a cell boundary")
        g = torch.zeros(B, 3, *size, device=DEV)
        g[B - 1, 1, z, y, x] = 1.7
        sr = StepRef(w, g, with_spread=False)
        nz = sr.ref != 0
        assert 1 <= int(nz.sum()) <= 27
        out = check_step(f"vecint step delta {B}/{size}/{kind}/{tag}", w, g, sr, power=False)
        for det, got in out.items():
            assert int(((got != 0) & ~nz).sum()) == 0, (tag, det, "a contribution landed outside the float64 result's support")
            # power, at the smallest corner contribution: dropping it is rejected
            cells = [(c, val) for c, val in R.vecint_corner_contributions(w64, g.double(), B - 1, 1, z, y, x) if val != 0]
            (iz, iy, ix), val = min(cells, key=lambda t: abs(t[1]))
            bad = sr.ref.clone()
            bad[B - 1, 1, iz, iy, ix] -= val
            if abs(val) > sr.floor:
                assert R.ratio(got, bad, sr.tol_t) > 1.0, (tag, det, val)


@pytest.mark.parametrize("size", [(6, 7, 5), (24, 20, 28), (66, 63, 65)])
def test_backward_step_zero_gradient_is_exactly_zero(ops, size):
    B = STEP_SIZES[size][0]
    w = step_field("smooth_large", B, size, 5)
    g = torch.zeros(B, 3, *size, device=DEV)
    work = step_work(w)
    for det in (False, True):
        gin, _ = run_bwd(det, work, g, 1)
        assert int(torch.count_nonzero(gin)) == 0 and bool(torch.isfinite(gin).all()), (size, det)


def test_elementwise_bound_rejects_what_rel_l2_accepts(ops):
    """power, once, on the data of test_vecint_backward_lds_tiled_scatter_vs_oracle's first case (24x20x28, white noise of amplitude 1 as v,
    the step at k = 6: w = work[6]).  The element-wise bound rejects the reference with one element moved by 1e-3 of its maximum, and the
    reference with the smallest non-zero corner contribution of one voxel removed from the image-role gradient (float64, subtracted at its
    cell).  The relative-L2 rule of the older tests, rel_l2 < max(1e-4, 3 rel_l2(fp32, float64)), accepts the second one"""
    size, B = (24, 20, 28), 2
    g0 = torch.Generator().manual_seed(int(1.0 * 10) + size[0])
    v = torch.randn(2, 3, *size, generator=g0) * 1.0
    g = torch.randn(2, 3, *size, generator=g0).to(DEV)
    w = R.vecint_chain_ref(v.to(DEV), 7)[6].contiguous()
    sr = StepRef(w, g)
    out = check_step("vecint power 2/(24, 20, 28)/k6", w, g, sr)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    old_bound = max(1e-4, 3.0 * rel(sr.r32, sr.ref))
    z, y, x = 13, 11, 15
    assert not bool(sr.bnd[1, 0, z, y, x])
    cells = [(c, val) for c, val in R.vecint_corner_contributions(w.double(), g.double(), 1, 2, z, y, x) if val != 0]
    (iz, iy, ix), val = min(cells, key=lambda t: abs(t[1]))
    dropped = sr.ref.clone()
    dropped[1, 2, iz, iy, ix] -= val
    moved = R.perturbed(sr.ref, sr.last_inner)
    r_moved, r_drop = R.ratio(moved, sr.ref, sr.tol_t), R.ratio(dropped, sr.ref, sr.tol_t)
    print(f"POWER one element moved by 1e-3 max|ref|: element-wise ratio {r_moved:.3g} (rejected), rel_l2 {rel(moved, sr.ref):.3g} against the old bound {old_bound:.3g}")
    print(f"POWER smallest corner contribution of voxel (1, 2, {z}, {y}, {x}) dropped ({val:.3g} at cell ({iz}, {iy}, {ix}); max|ref| {amax(sr.ref):.3g}): "
          f"element-wise ratio {r_drop:.3g} (rejected), rel_l2 {rel(dropped, sr.ref):.3g} against the old bound {old_bound:.3g} (accepted)")
    assert r_moved > 1.0 and r_drop > 1.0
    assert rel(dropped, sr.ref) < old_bound
    for got in out.values():          # and the kernels' results are told apart from both
        assert R.ratio(got, dropped, sr.tol_t) > 1.0 and R.ratio(got, moved, sr.tol_t) > 1.0


# ================================================================================================ the chain is the composition of its steps
def compose(det, work, g, nsteps):
    """the entry point applied nsteps times with nsteps = 1: g_k = 2 bwd([work[k], work[k + 1]], g_{k+1}), then 2^-nsteps g_0"""
    gk = g
    for k in range(nsteps - 1, -1, -1):
        gk = 2 * run_bwd(det, work[k:k + 2], gk, 1)[0]
    return gk * (1.0 / 2 ** nsteps)


# (24, 20, 28): R = 1 throughout; (66, 63, 65): R = 2 on the chain's last step only, R = 1 below it - the single-step calls take R = 2 every
# time, so this also compares the two rims on the same inputs; (6, 7, 5): the plain scatter with its ping-pong scratch
@pytest.mark.parametrize("nsteps", [0, 2, 7])
@pytest.mark.parametrize("kind", ["smooth_large", "noise"])
@pytest.mark.parametrize("B,size", [(2, (24, 20, 28)), (1, (66, 63, 65)), (2, (6, 7, 5))])
def test_chain_is_the_composition_of_its_steps(ops, B, size, kind, nsteps):
    """deterministic mode: torch.equal (integer sums commute, each step's fixed-point unit comes from the same maximum, every scale is a
    power of two).  The atomic chain and the atomic composition differ from it only by the order of fp32 additions: 1e-5 max|g| per
    element.  Every call runs twice on one scratch buffer: all bytes 0xFF before the first call, reused as left for the second"""
    v = R.vecint_field(kind, B, size, amp=4.0 if kind == "smooth_large" else 3.0, seed=nsteps + size[0]).to(DEV)
    g = torch.randn(B, 3, *size, device=DEV, generator=gen(7 * nsteps + size[1]))
    work = run_fwd(v, nsteps)
    name = f"vecint chain {B}/{size}/{kind}/n{nsteps}"
    res = {}
    for det in (True, False):
        first, scratch = run_bwd(det, work, g, nsteps)
        second, _ = run_bwd(det, work, g, nsteps, scratch=scratch)
        assert (scratch is None) == (nsteps == 0) and (scratch_size(det, B, size, nsteps) == 0) == (nsteps == 0)
        res[det] = (first, second, compose(det, work, g, nsteps))
    d1, d2, dc = res[True]
    assert bool(torch.isfinite(d1).all())
    assert torch.equal(d1, d2), f"{name}: the deterministic call depends on what its workspace held"
    assert torch.equal(d1, dc), f"{name}: the deterministic chain is not the composition of its steps ({int((d1 != dc).sum())} elements differ)"
    if nsteps == 0:
        assert torch.equal(d1, g) and all(torch.equal(t, g) for t in res[False])
    bound = 1e-5 * amax(d1)
    for tag, t in zip(("chain", "chain on its used scratch", "composition"), res[False]):
        check(f"{name} atomic {tag} vs deterministic", t, d1.double(), bound)


# ================================================================================================ ops.vecint end to end
@pytest.mark.parametrize("B,size", [(2, (24, 20, 28)), (1, (66, 63, 65))])
def test_ops_vecint_autograd_vs_float64(ops, B, size):
    """the Python side (planar, scratch sizing, DETERMINISTIC dispatch): forward and gradient of ops.vecint(v, 7) in both modes against the
    float64 oracle per element.  Exempt are the elements where torch's fp32 evaluation itself leaves 1e-5 max|ref| (a sample that took the
    other cell in one of the seven steps): at most 1e-4 of them"""
    v = R.vecint_field("smooth", B, size, amp=3.0, seed=1).to(DEV)
    up = torch.randn(B, 3, *size, device=DEV, generator=gen(size[0]))

    def oracle(x, u):
        x = x.clone().requires_grad_(True)
        o = O.vecint(x, 7)
        return o.detach(), torch.autograd.grad((o * u).sum(), [x])[0]

    refs, r32s = oracle(v.double(), up.double()), oracle(v, up)
    name = f"vecint autograd {B}/{size}"
    bounds = []
    for what, ref, r32 in zip(("out", "grad"), refs, r32s):
        exempt = (r32.double() - ref).abs() > 1e-5 * amax(ref)
        share = float(exempt.float().mean())
        spread = float((r32.double() - ref).abs()[~exempt].max())
        tol = max(1e-5 * max(1.0, amax(ref)), 2 * spread)
        print(f"RATIO {name} {what} exempt share {share:.3g} ({int(exempt.sum())} of {exempt.numel()}) spread32 {spread:.3g} tol {tol:.3g}")
        assert share <= 1e-4, (name, what, share)
        bounds.append((torch.where(exempt, torch.full_like(ref, float("inf")), torch.full_like(ref, tol)),
                       int(torch.nonzero(~exempt.reshape(-1)).reshape(-1)[-1])))
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            vg = v.clone().requires_grad_(True)
            out = ops.vecint(vg, 7)
            gv, = torch.autograd.grad((out * up).sum(), [vg])
        finally:
            ops.set_deterministic(P.det_default())
        for what, got, ref, (tol_t, last) in zip(("out", "grad"), (out, gv), refs, bounds):
            check(f"{name} det={det} {what}", got, ref, tol_t, power=last)
