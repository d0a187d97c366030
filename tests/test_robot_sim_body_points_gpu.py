"""GPU tier of tests/test_robot_sim_body_points.py: the same cases on the HIP library (sim_ground_points_rt_body<32> and
sim_ground_points_terrain_rt_body<32> on the device), states, torques and the handle-owned read-outs in device memory."""
import pytest

import test_robot_sim_body_points as BPT
from test_robot_sim_joint_model_gpu import DevR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rough", BPT.GROUNDS)
@pytest.mark.parametrize("name,P,seed", BPT.CASES)
def test_parity_with_the_checker(built, name, P, seed, rough):
    BPT.parity(name, P, BPT.ROUGH_SEED.get(name, seed) if rough else seed, rough, None)


@pytest.mark.parametrize("name,P,seed", BPT.CASES)
def test_points_outside_the_band_change_no_bit(built, name, P, seed):
    BPT.inert_points(name, P, seed, None, DevR)


@pytest.mark.parametrize("rough", BPT.GROUNDS)
def test_a_body_point_is_a_foot_point(built, rough):
    BPT.body_point_is_a_foot_point(None, rough)


def test_admission_and_errors(built):
    BPT.admission(None, DevR)


@pytest.mark.parametrize("rough", BPT.GROUNDS)
def test_a_fallen_robot_lies_on_its_trunk(built, rough):
    BPT.fallen_robot_lies_on_its_trunk(None, DevR, rough)


def test_the_touch_mask_is_the_reset_mask(built):
    BPT.mask_is_the_reset_mask(None, DevR)


@pytest.mark.parametrize("name,P,seed", BPT.CASES)
def test_batch_hygiene(built, name, P, seed):
    BPT.batch_hygiene(name, P, seed, None, DevR, False)
