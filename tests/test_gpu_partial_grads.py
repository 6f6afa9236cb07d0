"""Frozen parameters and accumulated gradients: the backward code branches on which leaves ask for a gradient (`needs`, the .grad slots of a
direct pass, the deferred finishing jobs) and on whether a .grad already holds something, and every other test lets all leaves ask and starts
from zeroed gradients.  Here every branch is taken and held to float64 (tests/partial_ref.py: plain torch ops in double on the GPU for the
operators, oracle/pulpo_oracle.py for the training step).

Section 1 - operators under every requires_grad subset, under plain autograd and inside ops.backward_pass(direct=True).  Per subset:
  (a) every requested gradient is within the stated fp32 bounds of float64: 2e-6 relative L2 for a bare convolution's result and data gradient,
      1e-5 for its weight and bias gradient, 1e-3 through a whole ConvUnit or head, and 1e-4 of the unit's largest gradient element for a conv
      bias in front of a training-mode BatchNorm (true gradient zero);
  (b) plain autograd leaves `.grad is None` on a leaf that did not ask;
  (c) direct pass: every attached .grad starts as g0 (normal variates on the rms of the float64 gradient) and must end as g0 + ref - judged on
      grad - g0 with the bound of (a).  Power: the same comparison on `grad` instead of `grad - g0` is asserted to FAIL for every leaf of every
      subset (an overwrite, a double add or a missed flush is an error of that size): the smallest such ratio over a test's leaves, subsets
      and passes is printed as POWER - measured 231 to 501 bounds through a ConvUnit or head (|g0| / |ref| = 1 in relative L2 against 1e-3;
      two passes: 0.5 against 1e-3, which is where the smallest sit), 4.0e4 and 5.0e4 for the bare convolution (against 1e-5);
  (d) a frozen leaf that still carries a .grad tensor (frozen after the optimizer was built) holds 7.0 before and, bit for bit, after;
  (e) two direct passes without refilling give g0 + 2 ref;
  (f) with ops.set_deterministic(True) two runs of (c) are bit-equal (and within the bounds).
Sections 2 and 3 - the training step (PULPo(3, 2), 32^3, n0 = 8) with frozen parts and with gradients accumulated over two batches, through plain
autograd, the stepper's pieces and the LightningModule hooks; their docstrings say what is asserted.

Every test prints `RATIO <case> <worst error / bound>`; profiles/partial_grads_gpu_tests.txt keeps one run's figures."""
import functools
import os

import numpy as np
import pytest
import torch

import partial_ref as P
import pyramid_ref as R
from oracle import pulpo_oracle as O
from test_gpu_pyramid_convunit import family

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last_3d
B_UNIT, B_CONV, B_CONV_WB, B_ZERO = 1e-3, 2e-6, 1e-5, 1e-4       # module docstring (a)


def det_default() -> bool:
    return os.environ.get("PULPO_DETERMINISTIC", "0") == "1"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from pulpo_amd import ops as _ops
    from pulpo_amd._lib import lib
    lib.load()
    return _ops


@pytest.fixture(scope="module", autouse=True)
def leave_no_cached_blocks():
    """the references are computed once per module; its end hands their blocks back to the driver (later tests count allocated memory)"""
    yield
    for cached in (unit_case, unit_ref, seq_case, head_case, conv_case, step_refs, gpu_flips):
        cached.cache_clear()
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ================================================================================================ 1. operators: the machinery
class Case:
    """one operator on fixed data.  names: the leaves in argument order; t: their fp32 values; forward(lv) -> the scalar loss of leaves lv;
    ref: float64 gradient per leaf; bound: relative-L2 bound per leaf; zero: {leaf: scale} for gradients whose true value is zero, judged by
    max |g| <= 1e-4 scale; always: leaves that ask in every subset"""

    def __init__(self, tag, names, t, forward, ref, bound, zero=None, always=()):
        self.tag, self.names, self.t, self.forward, self.ref = tag, tuple(names), t, forward, ref
        self.bound = bound if isinstance(bound, dict) else {n: bound for n in names}
        self.zero, self.always = dict(zero or {}), frozenset(always)
        self.g0 = P.prefill_like({n: ref[n] for n in names}, t, self.zero, _gen(len(tag) + 77))


class Watch:
    """route bookkeeping around one run: begin() before the forward pass, end(req, direct, passes) after the last backward"""

    def begin(self):
        pass

    def end(self, req, direct, passes):
        pass


def run(ops, case, req, direct, passes=1, watch=None):
    """forward + backward `passes` times on fresh leaves; direct: inside ops.backward_pass(True) with g0 attached to the leaves that ask and
    7.0 to those that do not"""
    lv = {n: case.t[n].detach().clone().requires_grad_(n in req) for n in case.names}
    if direct:
        for n in case.names:
            lv[n].grad = case.g0[n].clone() if n in req else torch.full_like(lv[n], P.FROZEN_FILL)
    if watch is not None:
        watch.begin()
    for _ in range(passes):
        loss = case.forward(lv)
        if direct:
            with ops.backward_pass(True):
                loss.backward()
            assert ops._PASS is ops._DEFAULT_PASS and not ops._PASS.jobs and not ops._PASS.keep
        else:
            loss.backward()
    if watch is not None:
        watch.end(req, direct, passes)
    return lv


def judge(case, tag, lv, req, direct, passes=1):
    """(a) - (e) for one run -> (worst error / bound, smallest ratio of the same comparison without subtracting g0)"""
    worst, power = 0.0, float("inf")
    for n in case.names:
        g = lv[n].grad
        if n not in req:
            if direct:
                assert g is not None and bool((g == P.FROZEN_FILL).all()), f"{tag}: the .grad of frozen leaf {n} was written"          # (d)
            else:
                assert g is None, f"{tag}: leaf {n} did not ask for a gradient and has one"                                          # (b)
            continue
        assert g is not None, f"{tag}: no gradient for {n}"
        d = g - case.g0[n] if direct else g
        if n in case.zero:
            tol = B_ZERO * case.zero[n]
            r = float(d.abs().max()) / tol if bool(torch.isfinite(d).all()) else float("inf")
            p = float(g.abs().max()) / tol
        else:
            want = case.ref[n] * passes
            r, p = P.rel_l2(d, want) / case.bound[n], P.rel_l2(g, want) / case.bound[n]
        assert r <= 1.0, f"{tag}: gradient of {n}: error / bound = {r:.3g}"
        worst = max(worst, r)
        if direct:
            assert p > 1.0, f"{tag}: {n}: the comparison without `- g0` passes ({p:.3g}): g0 gives it no power"
            power = min(power, p)
    return worst, power


def exercise(ops, case, subsets, watch=None):
    """every subset through plain autograd, one direct pass, two direct passes and two deterministic direct passes"""
    worst, power = 0.0, float("inf")
    for req in subsets:
        req = frozenset(req) | case.always
        sid = P.sid(case.names, req)

        def one(kind, direct, passes=1):
            nonlocal worst, power
            lv = run(ops, case, req, direct, passes, watch)
            w, p = judge(case, f"{case.tag} [{sid}] {kind}", lv, req, direct, passes)
            worst, power = max(worst, w), min(power, p)
            return lv

        one("plain", False)
        one("direct", True)
        one("direct x2", True, passes=2)
        ops.set_deterministic(True)
        try:
            a, b = one("deterministic", True), one("deterministic", True)
        finally:
            ops.set_deterministic(det_default())
        for n in req:
            assert torch.equal(a[n].grad, b[n].grad), f"{case.tag} [{sid}]: deterministic runs differ in the gradient of {n}"          # (f)
    print(f"RATIO {case.tag} {worst:.3g}")
    print(f"POWER {case.tag} {power:.3g}")
    assert worst <= 1.0 and power > 1.0


def _amax(ref, names) -> float:
    return max(float(ref[n].abs().max()) for n in names)


# ================================================================================================ 1a. ConvUnit
UNIT = ("x", "weight", "bias", "gamma", "beta")
UNIT_EXTRA = [("x", "bias"), ("weight", "gamma"), ("x", "gamma", "beta")]
# route -> (B, Cin, Cout, size): the smallest shape of each kernel route (asserted in _assert_unit_route)
UNIT_ROUTES = {
    "direct": (2, 32, 32, (12, 12, 12)), "wino2": (2, 32, 32, (24, 24, 24)), "wino3": (2, 96, 96, (24, 24, 24)), "wino3g": (1, 128, 128, (10, 10, 10)),
    "narrow16": (1, 16, 96, (12, 16, 16)), "input24": (2, 2, 32, (24, 24, 24)), "input64": (1, 2, 32, (64, 64, 64)),
}


def _assert_unit_route(ops, route, B, Cin, Cout, size):
    q = ops.lib.query
    w = torch.zeros(Cout, Cin, 3, 3, 3, device=DEV)
    pack = lambda dgrad: ops._pack_weight_now(w, dgrad, (B, *size), register=False)._pulpo_algo
    fams = (family(B, size, Cin, Cout), family(B, size, Cout, Cin), q("pulpo_conv3d_k3_wgrad_algo", B, *size, Cin, Cout, int(Cin % 4 == 0)))
    packs = (pack(False), pack(True))
    if route == "direct":
        assert fams == ("ds", "ds", 3) and packs == ("direct", "direct"), (fams, packs)
    elif route == "wino2":
        assert fams == ("yp", "yp", 3) and packs == ("wino2", "wino2"), (fams, packs)
    elif route == "wino3":
        assert fams == ("z", "z", 3) and packs == ("wino3", "wino3"), (fams, packs)
    elif route == "wino3g":
        assert q("pulpo_conv3d_k3_wino3g_ok", B, *size, Cin, Cout) == 1 and packs == ("wino3g", "wino3g") and fams[2] == 3, (fams, packs)
    elif route == "narrow16":
        assert q("pulpo_conv3d_k3_narrow16", 1, Cin, Cout) == 1 and fams[2] == 3 and packs == ("direct", "wino2"), (fams, packs)
    else:
        assert Cin <= 2 and fams[2] == 0 and packs == ("direct", "wino2"), (fams, packs)
        if route == "input64":                   # whole 4x8x8 tiles: the persistent small-channel kernel's sizes (tests/test_gpu_ops.py)
            assert all(s % 8 == 0 for s in size) and size[0] >= 64


@functools.lru_cache(maxsize=None)
def unit_case(B, Cin, Cout, size):
    g = _gen(1000 * B + 10 * Cin + Cout + size[0] + size[2])
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ru = lambda *s: torch.rand(*s, device=DEV, generator=g)
    x = rn(B, Cin, *size)
    if Cin > 4:                                  # (the <= 4-channel input layers take their image planar, as the step passes it)
        x = x.contiguous(memory_format=CL)
    return dict(x=x, weight=rn(Cout, Cin, 3, 3, 3) / (27 * Cin) ** 0.5, bias=0.1 * rn(Cout), gamma=0.75 + 0.5 * ru(Cout), beta=0.1 * rn(Cout),
                rm=0.1 * rn(Cout), rv=0.75 + 0.5 * ru(Cout), up=rn(B, Cout, *size).contiguous(memory_format=CL))


@functools.lru_cache(maxsize=None)
def unit_ref(B, Cin, Cout, size, training):
    t = unit_case(B, Cin, Cout, size)
    lv = P.double_leaves(t, UNIT)
    z = P.conv_unit_ref(*[lv[n] for n in UNIT], t["rm"].double(), t["rv"].double(), training)
    ref = P.grads_of((z * t["up"].double()).sum(), lv)
    return z.detach(), ref


class InputLayerWatch(Watch):
    """the input layer's BatchNorm backward runs inside its weight gradient (ops._input_layer_param_grads) exactly when the layer has at most two
    input channels, nobody asks for dx, somebody asks for dw, and the mode is not deterministic (ops._bwd_bn_apply)"""

    def __init__(self, ops, monkeypatch, Cin):
        self.ops, self.Cin, self.calls = ops, Cin, 0
        inner = ops._input_layer_param_grads

        def counted(*a, **k):
            self.calls += 1
            return inner(*a, **k)

        monkeypatch.setattr(ops, "_input_layer_param_grads", counted)

    def begin(self):
        self.calls = 0

    def end(self, req, direct, passes):
        fused = self.Cin <= 2 and "x" not in req and "weight" in req and not self.ops.DETERMINISTIC and self.ops.FUSE_INPUT_WGRAD
        assert self.calls == (passes if fused else 0), (P.sid(UNIT, req), direct, self.calls, fused)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("route", list(UNIT_ROUTES))
def test_conv_unit_under_requires_grad_subsets(ops, monkeypatch, route, training):
    """ops.conv_bn_lrelu(x, weight, bias, gamma, beta) on the smallest shape of every kernel route, training mode and eval mode with gradients
    enabled (the use_means = 0 form of pulpo_bn_bwd_finalize: a frozen-statistics BatchNorm inside a training step).  All 31 non-empty subsets on
    the direct-kernel shape; elsewhere "one frozen", "one only", {x, bias}, {weight, gamma} and {x, gamma, beta}.  In eval mode the conv bias
    has an ordinary gradient (1e-3); in training mode it is the zero-gradient case."""
    B, Cin, Cout, size = UNIT_ROUTES[route]
    _assert_unit_route(ops, route, B, Cin, Cout, size)
    t = unit_case(B, Cin, Cout, size)
    zref, ref = unit_ref(B, Cin, Cout, size, training)
    seen = {}

    def forward(lv):
        rm, rv = t["rm"].clone(), t["rv"].clone()
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        z = ops.conv_bn_lrelu(lv["x"], lv["weight"], lv["bias"], lv["gamma"], lv["beta"], rm, rv, training=training,
                              num_batches_tracked=nbt if training else None)
        seen["z"] = z.detach()
        return (z * t["up"]).sum()

    case = Case(f"unit {route} {'train' if training else 'eval'}", UNIT, t, forward, ref, B_UNIT,
                zero={"bias": _amax(ref, UNIT)} if training else None)
    subsets = P.all_subsets(UNIT) if route == "direct" else P.edge_subsets(UNIT, UNIT_EXTRA)
    assert len(subsets) == (31 if route == "direct" else 14)
    exercise(ops, case, subsets, InputLayerWatch(ops, monkeypatch, Cin))
    assert P.rel_l2(seen["z"], zref) <= B_UNIT


# ================================================================================================ 1b. blocked dy / blocked z: a two-unit ConvSequence
SEQ = ("x", "w0", "b0", "g0", "be0", "w1", "b1", "g1", "be1")
SEQ_KEYS = {"w0": "_op.0._op.0.weight", "b0": "_op.0._op.0.bias", "g0": "_op.0._op.1.weight", "be0": "_op.0._op.1.bias",
            "w1": "_op.1._op.0.weight", "b1": "_op.1._op.0.bias", "g1": "_op.1._op.1.weight", "be1": "_op.1._op.1.bias"}
SEQ_SHAPE = (1, 32, (64, 64, 64))
_ALL = frozenset(SEQ)
SEQ_SUBSETS = [_ALL, _ALL - {"w1"}, _ALL - {"x"}, _ALL - {"x", "w1"}, _ALL - {"w1", "b1"}, _ALL - {"w0"}, frozenset({"x"}), frozenset({"w1"}),
               frozenset({"x", "g1", "be1"})]


@functools.lru_cache(maxsize=None)
def seq_case():
    B, C, size = SEQ_SHAPE
    g = _gen(6464)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ru = lambda *s: torch.rand(*s, device=DEV, generator=g)
    t = dict(x=rn(B, C, *size).contiguous(memory_format=CL), up=rn(B, C, *size).contiguous(memory_format=CL))
    for u in "01":
        t.update({"w" + u: rn(C, C, 3, 3, 3) / (27 * C) ** 0.5, "b" + u: 0.1 * rn(C), "g" + u: 0.75 + 0.5 * ru(C), "be" + u: 0.1 * rn(C)})
    lv = P.double_leaves(t, SEQ)
    h = lv["x"]
    for u in "01":
        h = P.conv_unit_ref(h, lv["w" + u], lv["b" + u], lv["g" + u], lv["be" + u], None, None, True)
    return t, P.grads_of((h * t["up"].double()).sum(), lv)


class BlockedWatch(Watch):
    """ops.BLOCKED_DY_HITS / BLOCKED_Z_HITS against what the predicates say for 32 -> 32 -> 32 at 64^3 (F(2x2x2,3x3x3) forward, data and weight
    gradient).  A unit writes a blocked dy when its input asks for a gradient (ops._blocked_dy_ok: need_dx; with need_dw the weight gradient's
    checks on top, which this shape passes; without need_dw its own branch): the second unit when anything upstream of it asks, the first when
    x asks.  The first unit's output travels blocked when ops.BLOCKED_Z is on and the SECOND unit's weight asks (ops.blocked_z_wanted)."""

    def __init__(self, ops):
        self.ops = ops

    def begin(self):
        self.dy0, self.z0 = self.ops.BLOCKED_DY_HITS, self.ops.BLOCKED_Z_HITS

    def end(self, req, direct, passes):
        upstream = bool(req & {"x", "w0", "b0", "g0", "be0"})
        dy = (int("x" in req) + int(upstream)) * passes
        z = int(self.ops.BLOCKED_Z and "w1" in req) * passes
        got = (self.ops.BLOCKED_DY_HITS - self.dy0, self.ops.BLOCKED_Z_HITS - self.z0)
        assert got == (dy, z), (P.sid(SEQ, req), direct, got, (dy, z))


@pytest.mark.parametrize("blocked_z", [False, True], ids=["cl-z", "blocked-z"])
def test_conv_sequence_blocked_gradients_with_the_second_weight_frozen(ops, blocked_z):
    """a two-unit ConvSequence 32 -> 32 -> 32 at 64^3 in training mode, the second unit's weight frozen and trainable in turn (and x, and the
    first unit's weight): `_blocked_dy_ok`'s branch for need_dx without need_dw, and `blocked_z_wanted`'s question to the NEXT unit's weight"""
    import src.network_blocks as nb
    B, C, size = SEQ_SHAPE
    q = ops.lib.query
    assert family(B, size, C, C) == "z" and q("pulpo_conv3d_k3_wgrad_algo", B, *size, C, C, 1) == 3
    assert ops.BLOCKED_DY and size[0] * size[1] * size[2] >= max(ops.BLOCKED_DY_MIN_VOXELS, ops.BLOCKED_Z_MIN_VOXELS)
    t, ref = seq_case()
    seq = nb.ConvSequence(list(size), C, C, 2).to(DEV).train()
    buffers = {k: v.detach().clone() for k, v in seq.named_buffers()}

    def forward(lv):
        state = {SEQ_KEYS[n]: lv[n] for n in SEQ_KEYS}
        state.update({k: v.clone() for k, v in buffers.items()})
        z = torch.func.functional_call(seq, state, (lv["x"],))
        assert z.dim() == 5
        return (z * t["up"]).sum()

    zero = {"b0": _amax(ref, ("w0", "g0", "be0")), "b1": _amax(ref, ("w1", "g1", "be1"))}
    case = Case(f"sequence 32-32-32 @64^3 {'blocked z' if blocked_z else 'channels-last z'}", SEQ, t, forward, ref, B_UNIT, zero=zero)
    saved = ops.BLOCKED_Z
    ops.BLOCKED_Z = blocked_z
    try:
        exercise(ops, case, SEQ_SUBSETS, BlockedWatch(ops))
    finally:
        ops.BLOCKED_Z = saved


# ================================================================================================ 1c. bare convolution
CONV = ("x", "weight", "bias")


@functools.lru_cache(maxsize=None)
def conv_case(B, Cin, Cout, size):
    g = _gen(31 * Cin + size[0])
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    t = dict(x=rn(B, Cin, *size).contiguous(memory_format=CL), weight=rn(Cout, Cin, 3, 3, 3) / (27 * Cin) ** 0.5, bias=rn(Cout),
             up=rn(B, Cout, *size).contiguous(memory_format=CL))
    lv = P.double_leaves(t, CONV)
    out = R.conv3_ref(lv["x"], lv["weight"], lv["bias"])
    return t, out.detach(), P.grads_of((out * t["up"].double()).sum(), lv)


@pytest.mark.parametrize("B,Cin,Cout,size,fam", [(2, 32, 32, (12, 12, 12), "ds"), (2, 96, 96, (24, 24, 24), "z")], ids=["direct", "wino3"])
def test_conv3d_k3_under_requires_grad_subsets(ops, B, Cin, Cout, size, fam):
    """ops.conv3d_k3(x, weight, bias): all 7 subsets; result and dx 2e-6, dw and db 1e-5"""
    assert family(B, size, Cin, Cout) == fam and family(B, size, Cout, Cin) == fam
    t, out_ref, ref = conv_case(B, Cin, Cout, size)
    seen = {}

    def forward(lv):
        out = ops.conv3d_k3(lv["x"], lv["weight"], lv["bias"])
        seen["out"] = out.detach()
        return (out * t["up"]).sum()

    case = Case(f"conv3d_k3 {Cin}to{Cout} @{size[0]}^3", CONV, t, forward, ref, {"x": B_CONV, "weight": B_CONV_WB, "bias": B_CONV_WB})
    exercise(ops, case, P.all_subsets(CONV))
    r = P.rel_l2(seen["out"], out_ref) / B_CONV
    print(f"RATIO {case.tag} result {r:.3g}")
    assert r <= 1.0


# ================================================================================================ 1d. heads
HEAD6 = ("h", "w_mu", "b_mu", "w_sigma", "b_sigma")
HEAD3 = ("h", "w", "b")
HEAD_SHAPE = (2, 32, (9, 10, 11))
UNIT_P = ("weight", "bias", "gamma", "beta")


@functools.lru_cache(maxsize=None)
def head_case(kind):
    """kind: "mu_sigma", "to3" (the head on an activation h), "unit_mu_sigma", "unit_to3" (ConvUnit 32 -> 32 + head in one node, h = the unit's x)"""
    B, C, size = HEAD_SHAPE
    g = _gen(910 + len(kind))
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ru = lambda *s: torch.rand(*s, device=DEV, generator=g)
    six = kind.endswith("mu_sigma")
    names = HEAD6 if six else HEAD3
    t = dict(h=rn(B, C, *size).contiguous(memory_format=CL), eps=rn(B, 3, *size), ups=[rn(B, 3, *size) for _ in range(3 if six else 1)])
    for n in names[1:]:
        t[n] = rn(3, C, 1, 1, 1) / C ** 0.5 if n.startswith("w") else rn(3)
    fused = kind.startswith("unit")
    if fused:
        t.update(weight=rn(C, C, 3, 3, 3) / (27 * C) ** 0.5, bias=0.1 * rn(C), gamma=0.75 + 0.5 * ru(C), beta=0.1 * rn(C))
        names = names + UNIT_P
    lv = P.double_leaves(t, names)
    a = P.conv_unit_ref(lv["h"], lv["weight"], lv["bias"], lv["gamma"], lv["beta"], None, None, True) if fused else lv["h"]
    if six:
        outs = R.mu_sigma_ref(a, lv["w_mu"], lv["b_mu"], lv["w_sigma"], lv["b_sigma"], t["eps"].double())
    else:
        outs = (R.conv1x1_ref(a, lv["w"], lv["b"]),)
    loss = sum((o * u.double()).sum() for o, u in zip(outs, t["ups"]))
    return names, t, P.grads_of(loss, lv)


class HeadWatch(Watch):
    """a head's parameter gradients take the deferred path (partial rows in a persistent buffer, summed by flush_param_grads) only inside a
    direct pass in which the weight AND bias of EVERY part of the head ask and carry a .grad (ops._heads_part_rows): "w_mu frozen, w_sigma
    trainable" and "weight trainable, bias frozen" leave it"""

    def __init__(self, ops, monkeypatch, params):
        self.params, self.deferred, self.calls = params, 0, 0
        inner = ops._heads_part_rows

        def counted(*a, **k):
            part, slots = inner(*a, **k)
            self.calls += 1
            self.deferred += int(slots is not None)
            return part, slots

        monkeypatch.setattr(ops, "_heads_part_rows", counted)

    def begin(self):
        self.deferred = self.calls = 0

    def end(self, req, direct, passes):
        want = passes if (direct and all(p in req for p in self.params)) else 0
        assert self.calls == passes and self.deferred == want, (sorted(req), direct, self.calls, self.deferred, want)


@pytest.mark.parametrize("kind", ["mu_sigma", "to3", "unit_mu_sigma", "unit_to3"])
def test_heads_under_requires_grad_subsets(ops, monkeypatch, kind):
    """ops.mu_sigma_sample / ops.conv1x1_to3 on an activation and ops.conv_bn_lrelu_mu_sigma / ops.conv_bn_lrelu_to3 (the last ConvUnit and its
    head in one node) at C = 32, 9x10x11, B = 2: every subset of (h or x, head weights and biases) - the fused nodes with the unit's own
    parameters asking throughout, and once more with nothing else asking"""
    B, C, size = HEAD_SHAPE
    names, t, ref = head_case(kind)
    six, fused = kind.endswith("mu_sigma"), kind.startswith("unit")
    hits = {"n": 0}

    def forward(lv):
        if fused:
            rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            unit_args = (lv["weight"], lv["bias"], lv["gamma"], lv["beta"], rm, rv, torch.zeros((), dtype=torch.long, device=DEV))
            assert ops.head_bn_ok(lv["h"], True)
            h0 = ops.HEAD_BN_HITS
            if six:
                outs = ops.conv_bn_lrelu_mu_sigma(lv["h"], unit_args, 0.1, 1e-5, lv["w_mu"], lv["b_mu"], lv["w_sigma"], lv["b_sigma"], t["eps"])
            else:
                outs = (ops.conv_bn_lrelu_to3(lv["h"], unit_args, 0.1, 1e-5, lv["w"], lv["b"]),)
            hits["n"] += ops.HEAD_BN_HITS - h0
        elif six:
            outs = ops.mu_sigma_sample(lv["h"], lv["w_mu"], lv["b_mu"], lv["w_sigma"], lv["b_sigma"], t["eps"])
        else:
            outs = (ops.conv1x1_to3(lv["h"], lv["w"], lv["b"]),)
        return sum((o * u).sum() for o, u in zip(outs, t["ups"]))

    case = Case(f"head {kind}", names, t, forward, ref, B_UNIT, zero={"bias": _amax(ref, UNIT_P)} if fused else None,
                always=UNIT_P if fused else ())
    head_names = HEAD6 if six else HEAD3
    subsets = P.all_subsets(head_names) + ([frozenset()] if fused else [])
    assert len(subsets) == (31 if six else 7) + int(fused)
    exercise(ops, case, subsets, HeadWatch(ops, monkeypatch, head_names[1:]))
    assert not fused or hits["n"] > 0



# ================================================================================================ 2. the training step with frozen parts
FB = list(O.FEEDBACK_DEFAULT)
STEP_SEED = 2                                    # (see step_refs)
STEP_LR = 1e-4                                   # the model's default, as in test_step_vs_oracle_at_baseline_width (see assert_moved_like_adam)
GRAD_TIGHT, GRAD_FLIPPED, FLIP_CAP = 2e-4, 5e-3, 1e-5          # test_step_vs_oracle_at_baseline_width's rule
INPUT_WEIGHT = "downpath.down_blocks.0._op.0._op.0.weight"


@pytest.fixture(scope="module")
def api(ops):
    import src.models as models
    import src.network_blocks as nb
    return models, nb


@functools.lru_cache(maxsize=None)
def step_refs():
    """PULPo(3, 2) at 32^3, n0 = 8 (the smallest size that runs every node of the step), weights O.init_state_dict(seed 2), two batches and
    one set of noise from generator seed 102.  Float64 oracle steps on the CPU, once per module: b0 then b1 on ONE state dict (the BatchNorm
    running statistics move twice), all in training mode ("train") and with O.down_path(training=False) in front of the training-mode autoencoder
    ("eval": a frozen encoder under .eval()).  The b0 runs serve every frozen pattern - the gradient of a trainable parameter does not depend on
    which others are frozen -, both serve the accumulation tests.
    The seed was chosen on the CPU: the fp32 oracle on its own has 0 LeakyReLU slope flips of 1 433 600 activations against each of the four
    float64 runs for seeds 2, 3 and 4 (seed 1: one flip in the first), so the flip cap (1e-5 of the activations: 14) leaves the GPU its room."""
    cfg = O.Cfg(3, 2, [32, 32, 32], n0=8)
    sd = O.init_state_dict(cfg, seed=STEP_SEED)
    gen = torch.Generator().manual_seed(100 + STEP_SEED)
    batches = [(torch.rand(1, 1, 32, 32, 32, generator=gen), torch.rand(1, 1, 32, 32, 32, generator=gen)) for _ in range(2)]
    eps = {0: torch.randn(1, 3, 16, 16, 16, generator=gen), 1: torch.randn(1, 3, 8, 8, 8, generator=gen)}
    eps64 = {l: e.double() for l, e in eps.items()}
    runs = {}
    for mode, down_training in (("train", True), ("eval", False)):
        sd64 = O.clone_sd(P.as_double(sd), requires_grad=True)
        steps = []
        for x, y in batches:
            units = {}
            ls, grads, _ = P.oracle_step(sd64, cfg, x.double(), y.double(), eps64, down_training, units)
            steps.append(([float(v) for v in ls[:4]], grads, units))
        runs[mode] = (steps, {k: v.detach().clone() for k, v in sd64.items() if "running_" in k})
    return sd, batches, eps, runs


def make_model(api, lr=STEP_LR):
    models, nb = api
    sd, _, eps, _ = step_refs()
    model = models.PULPo(3, 2, 0.1, [32, 32, 32], feedback=FB, n0=8, lr=lr)
    assert set(model.state_dict()) == set(sd)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.cuda().train()
    for l in range(2):
        model.autoencoder.encoders[l].sampler = nb.FixedNoiseSampler(eps[l].cuda())
    return model


def gpu_batch(i):
    x, y = step_refs()[1][i]
    empty = torch.empty((0,), device=DEV)
    return (x.cuda(), y.cuda(), empty, empty, empty, empty, empty, empty)


def _is_gamma(k, p):
    return k.endswith("_op.1.weight") and p.dim() == 1


def _is_beta(k, p):
    return k.endswith("_op.1.bias") and p.dim() == 1


def _is_head(k, p):
    return "mu_sigma." in k or "velocity_field._op.2." in k


# pattern -> (forward mode of the oracle run, frozen?(name, parameter))
PATTERNS = {
    "i-downpath": ("train", lambda k, p: k.startswith("downpath.")),
    "ii-downpath-eval": ("eval", lambda k, p: k.startswith("downpath.")),
    "iii-batchnorm": ("train", lambda k, p: _is_gamma(k, p) or _is_beta(k, p)),
    "iv-gamma": ("train", _is_gamma),
    "v-biases": ("train", lambda k, p: k.endswith(".bias") and not _is_beta(k, p)),
    "vi-input-weight": ("train", lambda k, p: k == INPUT_WEIGHT),
    "vii-heads-only": ("train", lambda k, p: not _is_head(k, p)),
    "viii-k3-weights": ("train", lambda k, p: p.dim() == 5 and p.shape[-1] == 3),
}


def freeze(model, pattern):
    """-> names of the frozen parameters; "ii" also puts the DownPath in eval mode"""
    _, frozen = PATTERNS[pattern]
    names = set()
    for k, p in model.named_parameters():
        if frozen(k, p):
            p.requires_grad_(False)
            names.add(k)
    if pattern.startswith("ii-"):
        model.downpath.eval()
    assert names and len(names) < len(list(model.parameters())), pattern
    return names


@functools.lru_cache(maxsize=None)
def gpu_flips(mode, batch):
    """LeakyReLU slope flips of the GPU's forward pass against the float64 run, counted on a pass of its own with a forward hook on every
    ConvUnit (hooks make every unit write its activation: the head and pooling fusions step aside, the convolution and BatchNorm coefficient
    kernels in front of the LeakyReLU are the same) -> (flips, activations)"""
    import src.models as models
    import src.network_blocks as nb
    from test_gpu_step import _record_unit
    model = make_model((models, nb))
    model._needed_levels = None
    if mode == "eval":
        model.downpath.eval()
    got = {}
    for name, mod in model.named_modules():
        if isinstance(mod, nb.ConvUnit):
            mod.register_forward_hook(lambda m, i, o, name=name: _record_unit(got, name, o))
    b = gpu_batch(batch)
    model._forward_and_losses(b[0], b[1])
    ref = step_refs()[3][mode][0][batch][2]
    assert set(got) == set(ref)
    flips, n = P.count_flips(got, ref)
    print(f"FLIPS {mode} batch {batch}: {flips} of {n}")
    assert flips <= FLIP_CAP * n, (flips, n)
    return flips, n


def grads_of(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def hold_to_float64(tag, got, want, frozen, flips):
    """every trainable parameter's gradient against the float64 one(s) (`want`: name -> gradient, None for a parameter the loss does not reach):
    2e-4 relative L2 with no slope flip, 5e-3 otherwise; frozen parameters have no gradient -> (worst error / bound, parameters checked)"""
    bound = GRAD_TIGHT if flips == 0 else GRAD_FLIPPED
    worst, checked = 0.0, 0
    for k, g in got.items():
        if k in frozen:
            assert g is None, f"{tag}: frozen parameter {k} has a gradient"
            continue
        if want.get(k) is None:
            assert g is None or float(g.abs().max()) == 0.0, (tag, k)
            continue
        assert g is not None, (tag, k)
        if P.bn_bias(k):
            continue                             # (zero-mean gradient in front of a BatchNorm: noise on both sides, as in test_step_vs_oracle_at_baseline_width)
        r = P.rel_l2(g, want[k]) / bound
        assert r <= 1.0, f"{tag}: gradient of {k}: error / bound = {r:.3g} ({flips} flips)"
        worst, checked = max(worst, r), checked + 1
    assert checked >= 10, (tag, checked)
    return worst, checked


def same_as_plain(tag, got, plain, bound=1e-5):
    """a route's gradients against plain autograd's on the same weights (float-atomic order is all that differs) -> worst error / bound"""
    worst = 0.0
    for k, gp in plain.items():
        g = got[k]
        if gp is None:
            assert g is None or float(g.abs().max()) == 0.0, (tag, k)
            continue
        if float(gp.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, (tag, k)
            continue
        if P.bn_bias(k):                         # (rounding noise on both sides: on the scale of its unit's largest gradient element)
            unit = [v for j, v in plain.items() if j.startswith(k[:-len("_op.0.bias")]) and j != k and v is not None]
            wmax = max([float(v.abs().max()) for v in unit] + [1e-6])
            assert float((g - gp).abs().max()) <= 1e-4 * wmax, (tag, k)
            continue
        r = P.rel_l2(g, gp) / bound
        assert r <= 1.0, f"{tag}: gradient of {k} against plain autograd: error / bound = {r:.3g}"
        worst = max(worst, r)
    return worst


def hook_backward(model, opt, batch, i, zero=True):
    """the closure of pytorch_lightning 1.8's automatic optimization up to the update, over the model's own hooks (HookOrderTrainer's order)"""
    model.on_train_batch_start(batch, i)
    loss = model.training_step(batch, i)
    if zero:
        model.on_before_zero_grad(opt)
        model.optimizer_zero_grad(0, i, opt, 0)
    model.on_before_backward(loss)
    model.backward(loss, opt, 0)
    model.on_after_backward()
    return loss.detach()


def hook_update(model, opt, batch, i):
    model.on_before_optimizer_step(opt, 0)
    model.optimizer_step(0, i, opt, 0, lambda: None)
    model.on_train_batch_end({}, batch, i)


def assert_moved_like_adam(tag, model, start, frozen, want, reached=()):
    """after three steps: frozen parameters bit-unchanged, the others where plain autograd + torch.optim.Adam put them (atol 2e-4).
    Adam's first steps move an element by about lr each whatever its gradient's size, so at the default lr = 1e-4 a parameter that was skipped,
    or stepped twice, ends 3e-4 from where it belongs: outside 2e-4 - asserted for every parameter the loss reaches (`reached`).  (A larger lr
    buys no power: two routes whose gradients agree to 1e-5 still take opposite +-lr moves on the elements whose gradient is rounding noise,
    the next step's gradients then differ by 1e-3, and the distance between the routes grows with lr - 4e-4 at lr = 1e-3, measured.)"""
    for k, p in model.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach(), start[k]), f"{tag}: frozen parameter {k} moved"
        elif not P.bn_bias(k):                   # (Adam normalises pure rounding noise on these: not comparable element-wise)
            np.testing.assert_allclose(p.detach().cpu().numpy(), want[k].cpu().numpy(), atol=2e-4, rtol=0, err_msg=f"{tag} {k}")
            if k in reached:
                assert float((p.detach() - start[k]).abs().max()) > 2e-4, f"{tag}: {k} has not moved by more than the comparison's tolerance"


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_training_step_with_frozen_parts(api, pattern, monkeypatch):
    """One frozen pattern through plain autograd, the stepper's pieces (weight gradients in line and on the side stream) and the LightningModule
    hooks, every stepper and optimizer built AFTER freezing.  Losses against the float64 oracle at rtol 1e-4; every trainable gradient against
    float64 by the flip rule (at least 10 parameters); frozen parameters have `.grad is None`; the stepper and hook routes agree with plain
    autograd at 1e-5; after three steps frozen parameters are bit-unchanged and the others sit where plain autograd + torch.optim.Adam over the
    trainable subset puts them (atol 2e-4)."""
    from pulpo_amd import dp
    mode = PATTERNS[pattern][0]
    _, _, _, runs = step_refs()
    ls64, g64, _ = runs[mode][0][0]
    flips, _ = gpu_flips(mode, 0)
    batch = gpu_batch(0)
    worst = {}

    # ---- plain autograd + torch.optim.Adam over the trainable subset
    model = make_model(api)
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    frozen = freeze(model, pattern)
    _, _, lossv, _ = model._forward_and_losses(batch[0], batch[1])
    np.testing.assert_allclose([float(v) for v in lossv], ls64, rtol=1e-4)
    lossv[0].backward()
    plain = grads_of(model)
    worst["plain"], checked = hold_to_float64(f"{pattern} plain", plain, g64, frozen, flips)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=STEP_LR)
    for _ in range(3):
        opt.zero_grad()
        model.training_step(batch, 0).backward()
        opt.step()
    adam = {k: p.detach().clone() for k, p in model.named_parameters()}
    reached = {k for k, g in plain.items() if g is not None and float(g.abs().max()) > 0.0}
    assert_moved_like_adam(f"{pattern} plain", model, start, frozen, adam, reached)      # (frozen parameters unchanged, the others moved)

    # ---- the stepper's pieces
    for side in ("auto", "1"):
        monkeypatch.setenv("PULPO_WGRAD_SIDE_STREAM", side)
        model = make_model(api)
        frozen_s = freeze(model, pattern)
        stepper = dp.DataParallelStepper(model)
        assert frozen_s == frozen and stepper.wgrad_on_side_stream() == (side == "1")
        assert {id(p) for p in stepper.arena.params} == {id(p) for p in model.parameters() if p.requires_grad}
        stepper.zero_grad()
        loss = model.training_step(batch, 0)
        np.testing.assert_allclose(float(loss), ls64[0], rtol=1e-4)
        stepper.backward(loss)
        got = grads_of(model)
        tag = f"{pattern} stepper side={side}"
        worst[f"stepper-{side}"], _ = hold_to_float64(tag, got, g64, frozen, flips)
        worst[f"stepper-{side} vs plain"] = same_as_plain(tag, got, plain)
        for _ in range(3):
            stepper.step(batch)
        assert_moved_like_adam(tag, model, start, frozen, adam, reached)
    monkeypatch.setenv("PULPO_WGRAD_SIDE_STREAM", "auto")

    # ---- the LightningModule hooks in pytorch_lightning 1.8's order
    model = make_model(api)
    assert freeze(model, pattern) == frozen
    opt = model.configure_optimizers()
    assert isinstance(opt, dp.ArenaAdam) and len(opt.param_groups[0]["params"]) == len(list(model.parameters())) - len(frozen)
    loss = hook_backward(model, opt, batch, 0)
    np.testing.assert_allclose(float(loss), ls64[0], rtol=1e-4)
    got = grads_of(model)
    worst["hooks"], _ = hold_to_float64(f"{pattern} hooks", got, g64, frozen, flips)
    worst["hooks vs plain"] = same_as_plain(f"{pattern} hooks", got, plain)
    for i in range(3):
        hook_backward(model, opt, batch, i)
        hook_update(model, opt, batch, i)
    assert_moved_like_adam(f"{pattern} hooks", model, start, frozen, adam, reached)
    for k, v in worst.items():
        print(f"RATIO step {pattern} {k} {v:.3g}")
    print(f"RATIO step {pattern} ({checked} parameters, {flips} flips) {max(worst.values()):.3g}")


@pytest.mark.parametrize("pattern", ["i-downpath", "vii-heads-only"])
def test_graphed_step_with_frozen_parts_equals_the_eager_step(api, pattern):
    """DataParallelStepper(graph=True) over a partly frozen model, six steps against the eager stepper: test_graphed_step_equals_the_eager_step's
    assertions, and frozen parameters bit-unchanged on both"""
    from pulpo_amd import dp
    batches = [gpu_batch(0), gpu_batch(1)]

    def run(graph):
        model = make_model(api)
        start = {k: p.detach().clone() for k, p in model.named_parameters()}
        frozen = freeze(model, pattern)
        st = dp.DataParallelStepper(model, graph=graph)
        losses = [float(st.step(batches[i % 2])) for i in range(6)]
        assert (st._graph is not None) == graph
        for k, p in model.named_parameters():
            if k in frozen:
                assert torch.equal(p.detach(), start[k]) and p.grad is None, k
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    eager, sd_e = run(False)
    graphed, sd_g = run(True)
    np.testing.assert_allclose(graphed, eager, rtol=1e-4)
    assert abs(eager[0] - eager[1]) > 1e-6 * abs(eager[0])
    worst = 0.0
    for k, v in sd_e.items():
        if P.bn_bias(k):
            assert float((sd_g[k] - v).abs().max()) <= 6 * 2e-4, k       # (Adam moves rounding noise by +-lr per step)
        elif k.endswith("running_mean"):
            assert float((sd_g[k] - v).abs().max()) <= 2e-3 * max(1.0, float(v.abs().max())), k
        elif v.is_floating_point():
            r = float((sd_g[k] - v).abs().max()) / (1e-4 * max(1.0, float(v.abs().max())))
            assert r <= 1.0, (k, r)
            worst = max(worst, r)
        else:
            assert torch.equal(sd_g[k], v), k
    print(f"RATIO graphed step {pattern} {worst:.3g}")


def test_stepper_built_before_freezing_refuses_to_update(api):
    """A stepper's arena and Adam moments cover the parameters that were trainable when it was built.  Freezing one afterwards must not move it
    through stale moments: the update raises a ValueError that says to rebuild, nothing has moved, and a stepper built after freezing steps."""
    from pulpo_amd import dp
    batch = gpu_batch(0)
    model = make_model(api)
    stepper = dp.DataParallelStepper(model)
    stepper.step(batch)                          # (the moments of every parameter are non-zero now)
    p = dict(model.named_parameters())[INPUT_WEIGHT]
    p.requires_grad_(False)
    before = {k: q.detach().clone() for k, q in model.named_parameters()}
    with pytest.raises(ValueError, match="[Rr]ebuild"):
        stepper.step(batch)
    for k, q in model.named_parameters():
        assert torch.equal(q.detach(), before[k]), k
    opt = model.configure_optimizers()           # the Lightning route builds its engine the same way
    p.requires_grad_(True)
    model.downpath.requires_grad_(False)
    with pytest.raises(ValueError, match="[Rr]ebuild"):
        hook_backward(model, opt, batch, 0)
        hook_update(model, opt, batch, 0)
    for k, q in model.named_parameters():
        assert torch.equal(q.detach(), before[k]), k


# ================================================================================================ 3. accumulated gradients
def _accum_want(mode):
    steps, stats = step_refs()[3][mode]
    g0, g1 = steps[0][1], steps[1][1]
    return {k: (None if g0[k] is None else g0[k] + g1[k]) for k in g0}, stats


def _assert_running_stats(tag, model, stats):
    for k, v in model.named_buffers():
        if "running_" in k:
            np.testing.assert_allclose(v.detach().cpu().numpy(), stats[k].float().numpy(), atol=1e-6, rtol=1e-5, err_msg=f"{tag} {k}")


def _accumulate(api, route, pattern=None):
    """two batches' gradients accumulated without an update in between -> (model, gradients, frozen names)"""
    from pulpo_amd import dp
    model = make_model(api)
    frozen = freeze(model, pattern) if pattern else set()
    b0, b1 = gpu_batch(0), gpu_batch(1)
    if route == "plain":
        model.training_step(b0, 0).backward()
        model.training_step(b1, 1).backward()
    elif route == "stepper":
        stepper = dp.DataParallelStepper(model)
        stepper.zero_grad()
        stepper.backward(model.training_step(b0, 0))
        stepper.backward(model.training_step(b1, 1))
    else:
        # accumulate_grad_batches = 2 in pytorch_lightning 1.8: batch 0 runs training_step, optimizer_zero_grad, backward; batch 1 training_step,
        # backward - and only then optimizer_step (the gradients are read before it)
        opt = model.configure_optimizers()
        hook_backward(model, opt, b0, 0, zero=True)
        hook_backward(model, opt, b1, 1, zero=False)
    torch.cuda.synchronize()
    return model, grads_of(model), frozen


def test_accumulated_gradients_of_two_batches(api, ops):
    """backward twice between two zero_grad calls (how a B = 1 model gets an effective batch of two): every route's gradients are the sum of the
    two float64 gradients by the flip rule, the BatchNorm running statistics are the oracle's after two forward passes (atol 1e-6), the stepper
    and hook routes equal plain autograd's accumulation at 1e-5, and in deterministic mode the stepper sequence is bit-identical run to run"""
    want, stats = _accum_want("train")
    flips = gpu_flips("train", 0)[0] + gpu_flips("train", 1)[0]
    res, worst = {}, {}
    for route in ("plain", "stepper", "hooks"):
        model, res[route], _ = _accumulate(api, route)
        worst[route], checked = hold_to_float64(f"accumulate {route}", res[route], want, set(), flips)
        _assert_running_stats(f"accumulate {route}", model, stats)
    for route in ("stepper", "hooks"):
        worst[f"{route} vs plain"] = same_as_plain(f"accumulate {route}", res[route], res["plain"])
    ops.set_deterministic(True)
    try:
        a, b = _accumulate(api, "stepper")[1], _accumulate(api, "stepper")[1]
    finally:
        ops.set_deterministic(det_default())
    worst["deterministic"], _ = hold_to_float64("accumulate deterministic", a, want, set(), flips)
    for k, g in a.items():
        assert torch.equal(g, b[k]), f"deterministic accumulation differs run to run in {k}"
    # power: one batch's gradient alone (an overwrite instead of an add) is far outside the bound
    single = step_refs()[3]["train"][0][1][1]
    power = min(P.rel_l2(res["stepper"][k], single[k]) for k in single if single[k] is not None and not P.bn_bias(k)) / GRAD_FLIPPED
    for k, v in worst.items():
        print(f"RATIO accumulate {k} {v:.3g}")
    print(f"POWER accumulate (second batch's gradient alone, {checked} parameters) {power:.3g}")
    assert power > 1.0


def test_accumulation_composes_with_a_frozen_eval_mode_downpath(api):
    """pattern (ii) - DownPath frozen and in eval mode - under accumulation: the trainable gradients are the sum of the two float64 gradients of
    the eval-mode oracle runs, frozen parameters have none, the DownPath's running statistics stay where they were and the autoencoder's move twice"""
    want, stats = _accum_want("eval")
    flips = gpu_flips("eval", 0)[0] + gpu_flips("eval", 1)[0]
    worst = {}
    res = {}
    for route in ("plain", "stepper", "hooks"):
        model, res[route], frozen = _accumulate(api, route, "ii-downpath-eval")
        worst[route], _ = hold_to_float64(f"accumulate+frozen {route}", res[route], want, frozen, flips)
        _assert_running_stats(f"accumulate+frozen {route}", model, stats)
    worst["stepper vs plain"] = same_as_plain("accumulate+frozen stepper", res["stepper"], res["plain"])
    sd = step_refs()[0]
    assert all(torch.equal(stats[k].float(), sd[k]) for k in stats if k.startswith("downpath."))
    assert any(not torch.equal(stats[k].float(), sd[k]) for k in stats if k.startswith("autoencoder."))
    for k, v in worst.items():
        print(f"RATIO accumulate+frozen {k} {v:.3g}")
