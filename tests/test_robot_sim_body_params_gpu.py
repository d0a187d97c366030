"""GPU tier of tests/test_robot_sim_body_params.py: the same cases on the HIP library (sim_ground_body_rt_body<24> / <32> on the device),
states, torques and the handle-owned body parameters in device memory."""
import pytest

import test_robot_sim_body_params as B
from test_robot_sim_joint_model_gpu import DevR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,P,seed", B.CASES)
def test_parity_with_the_checker(built, name, P, seed):
    B.parity(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", B.CASES)
def test_equal_bits_with_a_modified_table(built, name, P, seed):
    B.equal_bits_with_a_modified_table(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", B.CASES)
def test_nominal_rows_are_inert(built, name, P, seed):
    B.nominal_rows_are_inert(name, P, seed, None, DevR)


@pytest.mark.parametrize("name,P,seed", B.CASES)
def test_batch_hygiene(built, name, P, seed):
    B.batch_hygiene(name, P, seed, None, DevR)


def test_the_scale_reads_the_payload(built):
    B.scale_reads_the_payload(None, DevR)


def test_admission_and_errors(built):
    B.admission(None, DevR)
