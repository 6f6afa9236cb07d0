"""What pulpo_amd/ops.py hands the kernels in a ConvUnit training step, held launch by launch: every scenario of tests/launch_log.py replayed and
compared, line for line, with the log recorded before the ConvUnit autograd node was split into stages (tests/golden/convunit_launches.txt,
scripts/record_launch_log.py).  Same entry points, same arguments, same streams, same order."""
import difflib

import pytest
import torch

import launch_log as LL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_log():
    return LL.read_golden()


@pytest.mark.parametrize("name", list(LL.SCENARIOS))
def test_convunit_launches_are_the_recorded_ones(golden_log, name):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    size, n0, want = golden_log[name]
    assert not LL.missing_entries(name, want), f"the fixture of scenario {name} no longer covers {LL.missing_entries(name, want)}"
    got = LL.run_scenario(name, size, n0)
    if got != want:
        diff = list(difflib.unified_diff(want, got, "recorded", "now", lineterm="", n=1))
        pytest.fail(f"scenario {name}: {len(got)} launches against {len(want)} recorded\n" + "\n".join(diff[:60]), pytrace=False)
