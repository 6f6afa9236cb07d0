#!/usr/bin/env python
"""Record tests/golden/convunit_launches.txt: the `lib.call` log of the ConvUnit scenarios of tests/launch_log.py (plain autograd, blocked z, every
fused pass off, deterministic, bf16, the stepper's coarse window, inference).  Run it on the GPU at the commit whose launches are to be HELD -
before a restructuring of pulpo_amd/ops.py, not after - and commit the file; tests/test_gpu_launch_log.py replays the scenarios against it.

  python scripts/record_launch_log.py [--out FILE] [--digest]

--digest also prints the SHA-256 of scenario d's parameter gradients (deterministic mode: two builds of the same kernels must agree bit for bit).
A scenario whose log at 32^3 / n0 = 32 misses the entry points it exists to cover is recorded at 64^3 / n0 = 16 instead (its section says so)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import launch_log as LL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=LL.GOLDEN)
    ap.add_argument("--digest", action="store_true")
    args = ap.parse_args()
    text = ["## lib.call log of the ConvUnit scenarios (tests/launch_log.py), written by scripts/record_launch_log.py.  One line per launch: entry point,",
            "## arguments (pointers p / 0, ints, floats by repr), stream.  Sections: `# <scenario> <volume edge> <n0>`; T3 / L2, B = 1."]
    raised = []
    for name in LL.SCENARIOS:
        for size, n0 in ((32, 32), (64, 16)):
            lines = LL.run_scenario(name, size, n0)
            missing = LL.missing_entries(name, lines)
            if not missing:
                break
            print(f"scenario {name} at {size}^3 / n0 = {n0}: missing {missing}")
        else:
            raise SystemExit(f"scenario {name} does not reach its entry points at either size")
        print(f"scenario {name}: {len(lines)} launches at {size}^3 / n0 = {n0}")
        raised += [name] if size != 32 else []
        text += [f"# {name} {size} {n0}"] + lines
    text.insert(2, "## Recorded at 64^3 / n0 = 16 because 32^3 / n0 = 32 does not reach the entry points they exist to cover: " + (", ".join(raised) or "none") + ".")
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")
    if args.digest:
        size, n0, _ = LL.read_golden(args.out)["d"]
        print("scenario d gradient sha256", LL.run_scenario("d", size, n0, digest=True)[1])


if __name__ == "__main__":
    main()
