"""examples/quadruped_arm_stack_resident.py runs end to end (centroidal MPC + CentroidalID + BatchedRobotSim on the 19-joint quad_arm, one
shared stream, states and torques resident): 2 robots at a short horizon, on the CPU test build of the kernel bodies and on the HIP
library.  The example itself asserts finite states and torques inside the limits (a failed assertion fails `_run`)."""
import re

import pytest

from test_examples import _run

SCRIPT = "quadruped_arm_stack_resident.py"


def _check(out, steps):
    print(out)
    assert "controller of 19 joints: 36 variables, 88 rows per QP; simulator: 2 robots, 12 contact rows each" in out
    assert "2 robots, %.2f s of walking" % (steps * 0.01) in out and re.search(r"robots that stay up: \d of 2", out) and "robot-seconds per second" in out
    m = re.search(r"max \|tau\| ([0-9.]+) N m", out)
    assert m and 0.0 < float(m.group(1)) <= 45.43 + 1e-6


def test_quad_arm_resident_stack_on_the_cpu_build(built):
    _check(_run(SCRIPT, [2, 2], True, {"SMPC_EXAMPLE_HORIZON": "12"}), 2)


@pytest.mark.gpu
def test_quad_arm_resident_stack(built):
    _check(_run(SCRIPT, [2, 5], False, {"SMPC_EXAMPLE_HORIZON": "12"}), 5)
