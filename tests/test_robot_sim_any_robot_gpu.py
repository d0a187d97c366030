"""GPU tier of tests/test_robot_sim_any_robot.py: the same cases on the HIP library (sim_rt_body on the device), states and torques in
torch tensors."""
import numpy as np
import pytest

import test_robot_sim_any_robot as T

pytestmark = pytest.mark.gpu


class Dev:
    def __init__(self, a):
        import torch

        self.t = torch.from_numpy(np.array(a, order="C", copy=True)).cuda()
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()


@pytest.mark.parametrize("name,fs", T.CASES)
def test_forward_dynamics_against_oracle(built, name, fs):
    T.fd_against_oracle(name, fs, None)


def test_against_templated_kernel(built):
    T.against_templated(None)


@pytest.mark.parametrize("name,fs", [("quad_arm", 3), ("tree32", 6)])
def test_step_against_host_loop(built, name, fs):
    T.step_against_host_loop(name, fs, None, Dev)


def test_per_robot_masks(built):
    T.per_robot_masks(None, Dev)


@pytest.mark.parametrize("name,fs", [("quad_arm", 3), ("tree32", 6)])
def test_blocks_are_independent(built, name, fs):
    T.independence(name, fs, None, Dev)


def test_resident_stack_on_quad_arm(built):
    T.resident_stack(None, Dev)


def test_admission(built):
    T.admission(None, Dev)
