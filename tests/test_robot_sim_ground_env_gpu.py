"""GPU tier of tests/test_robot_sim_ground_env.py: the same cases on the HIP library (sim_ground_env_rt_body<12> / <24> on the device),
states and torques in torch tensors."""
import ctypes as C

import pytest

import test_robot_sim_ground_env as E
from test_robot_sim_any_robot_gpu import Dev

pytestmark = pytest.mark.gpu


def dev_poke(ptr, index, value):
    """Write one double of device memory (a blocking copy; the caller has joined the handle's stream)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    v = C.c_double(value)
    assert hip.hipMemcpy(C.c_void_p(ptr + 8 * index), C.byref(v), 8, 1) == 0  # hipMemcpyHostToDevice
    assert hip.hipDeviceSynchronize() == 0


@pytest.mark.parametrize("where", ["base", "foot"])
@pytest.mark.parametrize("name,P,seed", E.CASES)
def test_one_solve_against_the_checker(built, name, P, seed, where):
    E.solve_against_checker(name, P, seed, where, None)


@pytest.mark.parametrize("name,P", [(c[0], c[1]) for c in E.CASES])
def test_uniform_environment_equals_the_flat_kernel(built, name, P):
    E.uniform_environment(name, P, None, Dev)


@pytest.mark.parametrize("name,P", [("go2_like", 1), ("biped_legs", 4)])
def test_a_slope_is_a_rotated_world(built, name, P):
    E.slope_is_rotated_world(name, P, None)


@pytest.mark.parametrize("name", ["quad_arm", "biped_legs"])
def test_push_power_and_angular_momentum(built, name):
    E.push_power(name, None)


def test_friction_decides(built):
    E.friction_decides(None, Dev)


@pytest.mark.parametrize("name,P", [("quad_arm", 1), ("biped_legs", 4)])
def test_batch_hygiene(built, name, P):
    E.batch_hygiene(name, P, None, Dev, dev_poke)


def test_admission_and_errors(built):
    E.admission(None, Dev)
