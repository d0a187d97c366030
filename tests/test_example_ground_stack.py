"""examples/quadruped_arm_stack_ground.py runs end to end standing (centroidal MPC + CentroidalID + BatchedRobotSim.stepGroundDevice on the
19-joint quad_arm, one shared stream, the contact plan to the controller only): 2 robots at a short horizon, on the CPU test build of the
kernel bodies and on the HIP library.  Standing must work: both robots up, every foot detected on the ground where the plan has it, no
penetration beyond 1 mm.  The example itself asserts finite states and torques inside the limits (a failed assertion fails `_run`)."""
import re

import pytest

from test_examples import _run

SCRIPT = "quadruped_arm_stack_ground.py"


def _check(out, steps):
    print(out)
    assert "simulator: 2 robots on the plane z = " in out and "4 contact points each" in out and "mode: stand" in out
    assert "2 robots, %.2f s of standing" % (steps * 0.01) in out and "robots that stay up: 2 of 2" in out and "robot-seconds per second" in out
    pen = re.search(r"largest penetration: ([0-9.e+-]+) m", out)
    assert pen and float(pen.group(1)) <= 1e-3
    mis = re.search(r"contacts differ on ([0-9.]+) % of the sampled control ticks", out)
    assert mis and float(mis.group(1)) == 0.0
    m = re.search(r"max \|tau\| ([0-9.]+) N m", out)
    assert m and 0.0 < float(m.group(1)) <= 45.43 + 1e-6


def test_quad_arm_ground_stack_standing_on_the_cpu_build(built):
    _check(_run(SCRIPT, [2, 3, "stand"], True, {"SMPC_EXAMPLE_HORIZON": "12"}), 3)


@pytest.mark.gpu
def test_quad_arm_ground_stack_standing(built):
    _check(_run(SCRIPT, [2, 10, "stand"], False, {"SMPC_EXAMPLE_HORIZON": "12"}), 10)
