"""examples/quadruped_arm_stack_fall.py runs end to end (the push grid of quadruped_arm_stack_push.py with a trunk box and the knees as
body points and the touch mask as the reset mask): 2 robots at a short horizon, robot 1 pushed hard enough to fall, on the CPU test build
of the kernel bodies and on the HIP library.  The output names the touched robot; every state is finite at the end; the pushed robot is
back at its start pose after its reset; the unpushed robot equals the run without body points bit for bit."""
import os
import re

import numpy as np
import pytest

from test_example_push_stack import ENV, _run

SCALE = 100.0  # robot 1: 6000 N from the side and as much from above on a robot of 19 kg for 40 ms


def _check(emu, steps, start, length, tmp_path):
    trace, plain = str(tmp_path / "fall.npz"), str(tmp_path / "plain.npz")
    out = _run("quadruped_arm_stack_fall.py", [2, steps, start, length, SCALE], emu, dict(ENV, SMPC_EXAMPLE_TRACE=trace))
    print(out)
    _run("quadruped_arm_stack_fall.py", [2, steps, start, length, SCALE], emu, dict(ENV, SMPC_EXAMPLE_TRACE=plain, SMPC_EXAMPLE_NO_POINTS="1"))
    t, p = np.load(trace), np.load(plain)
    assert "12 body points each (on)" in out and "robot-seconds per second with the resets on" in out
    m = re.search(r"robot 1 \(push ([0-9.]+) N, mu ([0-9.]+)\) touched down: (\d+) resets", out)
    assert m and float(m.group(1)) == 60.0 * SCALE and int(m.group(3)) >= 1 and "robot 0 (push" not in out
    assert "every state finite at the end: True" in out and np.isfinite(t["X"]).all() and np.isfinite(t["states"]).all()
    assert t["states"].shape[:2] == (steps, 2) and t["touch"].shape == (steps, 2)
    assert not t["touch"][:, 0].any() and t["touch"][:, 1].any() and not p["touch"].any()
    k = int(np.flatnonzero(t["touch"][:, 1])[0])
    assert np.array_equal(t["states"][k, 1], t["X0"][1]) and not np.array_equal(t["states"][max(k - 1, 0), 1], t["X0"][1])  # (back at its start state)
    assert np.array_equal(t["states"][:, 0], p["states"][:, 0]) and np.array_equal(t["X"][0], p["X"][0])  # (the points never touched robot 0)


def test_quad_arm_fall_stack_on_the_cpu_build(built, tmp_path):
    _check(True, 8, 10, 40, tmp_path)


@pytest.mark.gpu
def test_quad_arm_fall_stack(built, tmp_path):
    _check(False, 8, 10, 40, tmp_path)
