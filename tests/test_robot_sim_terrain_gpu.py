"""GPU tier of tests/test_robot_sim_terrain.py: the same cases on the HIP library (sim_ground_terrain_rt_body<24> / <32> on the device),
states, torques and the handle-owned terrain in device memory."""
import pytest

import test_robot_sim_terrain as TT
from test_robot_sim_joint_model_gpu import DevR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,P,seed", TT.CASES)
def test_parity_with_the_checker(built, name, P, seed):
    TT.parity(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", TT.CASES)
def test_a_flat_tile_is_the_plane_bit_for_bit(built, name, P, seed):
    TT.flat_tile_is_the_plane(name, P, seed, None, DevR)


@pytest.mark.parametrize("name,P,seed", TT.CASES)
def test_a_sampled_plane_is_the_plane(built, name, P, seed):
    TT.sampled_plane_is_the_plane(name, P, seed, None)


def test_the_scale_reads_the_weight_on_rough_ground(built):
    TT.scale_reads_the_weight(None, DevR)


@pytest.mark.parametrize("name,P,seed", TT.CASES)
def test_batch_hygiene(built, name, P, seed):
    TT.batch_hygiene(name, P, seed, None, DevR, False)


def test_admission_and_errors(built):
    TT.admission(None, DevR)
