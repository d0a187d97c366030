"""GPU tier of tests/test_robot_sim_joint_model.py: the same cases on the HIP library (sim_ground_joint_rt_body<24> / <32> on the device),
states and torques in torch tensors."""
import pytest

import test_robot_sim_joint_model as J
from test_robot_sim_any_robot_gpu import Dev

pytestmark = pytest.mark.gpu


class _Raw:
    """A handle-owned device buffer of doubles by address, for torch.as_tensor."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f8", data=(int(ptr), False), version=2)


class DevR(Dev):
    @staticmethod
    def read(ptr, shape):
        import torch

        torch.cuda.synchronize()
        return torch.as_tensor(_Raw(ptr, shape), device="cuda").cpu().numpy().copy()


@pytest.mark.parametrize("name,P,seed", J.CASES)
def test_parity_with_the_checker(built, name, P, seed):
    J.parity(name, P, seed, None)


@pytest.mark.parametrize("name,P,seed", J.CASES)
def test_inert_model_bit_for_bit(built, name, P, seed):
    J.inert_model(name, P, seed, None, DevR)


@pytest.mark.parametrize("name,P,seed", J.CASES)
def test_clipping(built, name, P, seed):
    J.clipping(name, P, seed, None, DevR)


def test_a_stop_holds(built):
    J.stop_holds(None, DevR)


def test_damping_and_armature_across_steps(built):
    J.damping_across_steps(None, DevR)


@pytest.mark.parametrize("name,P,seed", J.CASES)
def test_batch_hygiene(built, name, P, seed):
    J.batch_hygiene(name, P, seed, None, DevR)


def test_admission_and_errors(built):
    J.admission(None, DevR)
