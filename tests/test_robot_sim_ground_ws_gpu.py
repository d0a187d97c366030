"""GPU tier of tests/test_robot_sim_ground_ws.py: the same cases on the HIP library (sim_ground_ws_rt_body<12> / <24> on the device),
states, torques and reset masks in torch tensors."""
import pytest

import test_robot_sim_ground_ws as W
from test_robot_sim_any_robot_gpu import Dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,P,seed", W.CASES)
def test_inert_settings_bit_for_bit(built, name, P, seed):
    W.inert_settings(name, P, seed, None, Dev)


@pytest.mark.parametrize("name,P,seed", W.CASES)
def test_parity_with_the_checker(built, name, P, seed):
    W.parity(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", W.CASES)
def test_parity_when_the_sweep_bound_is_reached(built, name, P, seed):
    W.sweep_bound(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", W.CASES)
def test_non_finite_start_entries(built, name, P, seed):
    W.non_finite_start(name, P, seed, None)


def test_fixed_point(built):
    W.fixed_point(None)


@pytest.mark.parametrize("start", W.STARTS)
@pytest.mark.parametrize("name,P", [("biped_legs", 4), ("go2_like", 1)])
def test_warm_start_across_steps(built, name, P, start):
    W.warm_across_steps(name, P, start, None, Dev)


def test_warm_start_at_fixed_sweeps(built):
    W.warm_fixed_sweeps(None, Dev)


@pytest.mark.parametrize("name,P", [("go2_like", 1), ("biped_legs", 4)])
def test_resets(built, name, P):
    W.resets(name, P, None, Dev)


@pytest.mark.parametrize("name,P", [("go2_like", 1), ("biped_legs", 4)])
def test_batch_hygiene(built, name, P):
    W.batch_hygiene(name, P, None, Dev)


def test_admission_and_errors(built):
    W.admission(None, Dev)
