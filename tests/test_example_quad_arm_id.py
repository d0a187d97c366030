"""examples/quadruped_arm_centroidal_id_batched.py runs end to end (centroidal MPC + CentroidalID on the 19-joint quad_arm, targets handed
over on the device, robots advanced with the QP's own accelerations): two MPC steps at a short horizon on the CPU test build of the kernel
bodies, the example's own walk (1 s: double support, then most of the first swing of a diagonal foot pair) on the HIP library."""
import pytest

from test_examples import _run

SCRIPT = "quadruped_arm_centroidal_id_batched.py"


def test_quad_arm_centroidal_id_stack_on_the_cpu_build(built):
    out = _run(SCRIPT, [2, 2], True, {"SMPC_EXAMPLE_HORIZON": "12"})
    print(out)
    assert "controller of 19 joints: 36 variables, 88 rows per QP" in out and "robots that stay up: 2 of 2" in out


@pytest.mark.gpu
def test_quad_arm_centroidal_id_stack(built):
    out = _run(SCRIPT, [4, 100], False)
    print(out)
    assert "4 robots, 1.00 s of walking" in out and "robots that stay up: 4 of 4" in out
