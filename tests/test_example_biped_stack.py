"""examples/biped_legs_stack_resident.py runs end to end (centroidal MPC with 6-D feet + CentroidalID with flat feet + BatchedRobotSim with 6-D
contacts on the 13-joint biped_legs, one shared stream, states and torques resident): 4 robots, 1 s of simulated walking at a short horizon,
on the CPU test build of the kernel bodies and on the HIP library.  Every robot stays up (base height within 5 cm of the reference height),
the torques stay inside their limits and the QP residual is finite."""
import re

import pytest

from test_examples import _run

SCRIPT = "biped_legs_stack_resident.py"


def _check(out):
    print(out)
    assert "controller of 13 joints: 42 variables, 106 rows per QP; simulator: 4 robots, 12 contact rows each" in out
    assert "4 bipeds, 1.00 s of walking" in out and "robots that stay up: 4 of 4" in out
    m = re.search(r"base height ([0-9.]+) \.\. ([0-9.]+) m \(reference ([0-9.]+)\); largest \|tau\| / limit ([0-9.]+); QP residual (\S+)", out)
    assert m, out
    lo, hi, ref, over, resid = (float(v) for v in m.groups())
    assert abs(lo - ref) < 0.05 and abs(hi - ref) < 0.05
    assert 0.0 < over <= 1.0 + 1e-6
    assert resid == resid and resid < 1e300


def test_biped_legs_resident_stack_on_the_cpu_build(built):
    _check(_run(SCRIPT, [4, 100], True, {"SMPC_EXAMPLE_HORIZON": "20"}))


@pytest.mark.gpu
def test_biped_legs_resident_stack(built):
    _check(_run(SCRIPT, [4, 100], False, {"SMPC_EXAMPLE_HORIZON": "20"}))
