"""GPU tier of test_centroidal_any_robot.py: the same cases on the shipped HIP library (frontend_rt_body of smpc_frontend_rt.h as a gfx950
kernel, one code object for the 13-, 19-, 23- and 32-joint tables).  Closed loop at the device bar of the centroidal tests (1e-4)."""
import pytest

import test_centroidal_any_robot as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", T.ROBOTS)
def test_frontend_against_oracle(built, name):
    T.frontend_vs_oracle(name, None, B=8)


@pytest.mark.parametrize("name", ["go2_like", "talos_like"])
def test_runtime_frontend_against_templated_frontends(built, name):
    T.rt_vs_templated(name, None, B=8)


@pytest.mark.parametrize("name", ["quad_arm", "tree32"])
def test_closed_loop_against_oracle(built, name):
    worst = T.closed_loop(name, None, 3, 1e-4)
    print("%s: worst relative xs error over 6 steps %.3e" % (name, worst))


def test_instances_are_independent(built):
    T.independence("quad_arm", None)  # (wavefront per instance: block indices past 64)
