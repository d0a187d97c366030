"""GPU tier of tests/test_robot_sim_ground.py: the same cases on the HIP library (sim_ground_rt_body<12> / <24> on the device), states and
torques in torch tensors."""
import pytest

import test_robot_sim_ground as G
from test_robot_sim_any_robot_gpu import Dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,P,seed", G.CASES)
def test_one_solve_against_the_reference(built, name, P, seed):
    G.solve_against_reference(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", G.CASES)
def test_physics_of_the_outputs(built, name, P, seed):
    G.physics(name, P, seed, None)


def test_difference_from_the_bilateral_simulator(built):
    G.difference_from_bilateral(None)


@pytest.mark.parametrize("name,P", [("quad_arm", 1), ("biped_legs", 4)])
def test_steps_against_the_host_loop(built, name, P):
    G.stepping(name, P, None, Dev)


@pytest.mark.parametrize("name,P", [("quad_arm", 1), ("biped_legs", 4)])
def test_blocks_are_independent(built, name, P):
    G.independence(name, P, None, Dev)


def test_resident_stack_standing_on_quad_arm(built):
    G.resident_stack(None, Dev)


def test_admission_and_errors(built):
    G.admission(None, Dev)
