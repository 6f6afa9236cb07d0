"""CPU-side tests of ops.backward_pass: the one place the state of a backward pass (ops._BackwardPass) is installed and torn down.  No
library and no GPU: without a side stream and without pending jobs the exit launches nothing."""
import pytest
import torch

from pulpo_amd import ops
from pulpo_amd._lib import PulpoHipError


class _Window:
    """stand-in for ops.CoarseWindow: records the calls backward_pass makes"""

    def __init__(self):
        self.calls, self.held = [], []

    def begin(self):
        self.calls.append("begin")

    def join(self):
        self.calls.append("join" if not self.held else "join with jobs held")      # (the real one launches what is held)


def _default_installed_and_empty():
    d = ops._PASS
    return (d is ops._DEFAULT_PASS and (d.direct, d.side, d.window) == (False, None, None) and not d.jobs and not d.keep and not d.bn_parts)


def test_entering_and_leaving_installs_and_reinstalls_the_default():
    assert _default_installed_and_empty()
    ops._DEFAULT_PASS.bn_parts[1] = "left by a plain-autograd backward whose producer never ran"
    with ops.backward_pass(True) as bp:
        assert ops._PASS is bp and bp is not ops._DEFAULT_PASS and isinstance(bp, ops._BackwardPass)
        assert (bp.direct, bp.side, bp.window) == (True, None, None) and bp.jobs == [] and bp.keep == [] and bp.bn_parts == {}
        assert not ops._DEFAULT_PASS.bn_parts              # cleared on entry
        assert not hasattr(bp, "__dict__")                 # __slots__: no seventh field appears by assignment
    assert _default_installed_and_empty() and bp.direct is False
    with ops.backward_pass(False) as bp2:                  # a second pass is a fresh object
        assert bp2 is not bp and bp2.direct is False
    assert _default_installed_and_empty()


def test_nesting_raises_and_leaves_the_outer_pass_installed():
    with ops.backward_pass(True) as outer:
        with pytest.raises(PulpoHipError):
            with ops.backward_pass(True):
                pass
        assert ops._PASS is outer and outer.direct is True
    assert _default_installed_and_empty()


def test_an_exception_propagates_and_leaves_the_default_pass_empty():
    class Boom(Exception):
        pass

    m = torch.nn.Linear(2, 2)
    m.weight._pulpo_wgrad_scratch = torch.zeros(4)
    buf = torch.zeros(3)
    with pytest.raises(Boom):
        with ops.backward_pass(True, None, None, m) as bp:
            bp.jobs.append((1, 2, 0, 3, 4, 5))             # (were they still pending at the exit, flush_param_grads() would reach for the library)
            bp.keep.append(buf)
            bp.bn_parts[7] = (buf,)
            raise Boom()
    assert _default_installed_and_empty()
    assert not bp.jobs and not bp.keep and not bp.bn_parts and bp.direct is False
    assert not hasattr(m.weight, "_pulpo_wgrad_scratch")   # the given module's persistent scratch goes with the interrupted pass


def test_window_sees_begin_join_begin_on_a_normal_exit():
    w = _Window()
    with ops.backward_pass(True, None, w) as bp:
        assert w.calls == ["begin"] and bp.window is w
    assert w.calls == ["begin", "join", "begin"] and _default_installed_and_empty()


def test_window_held_is_emptied_on_an_exception():
    w = _Window()
    with pytest.raises(RuntimeError):
        with ops.backward_pass(True, None, w):
            w.held.append("a weight gradient held back for the window")
            raise RuntimeError("interrupted")
    assert w.held == [] and w.calls == ["begin", "join", "begin"] and _default_installed_and_empty()
