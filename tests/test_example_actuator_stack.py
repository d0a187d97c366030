"""examples/quadruped_arm_stack_actuators.py runs end to end (the resident ground stack of quadruped_arm_stack_ground.py, standing, with an
effort-limit scale and a joint damping per robot and the joint-limit stops on): 8 robots, one per cell of the grid, for 0.3 s at a short
horizon, on the CPU test build of the kernel bodies and on the HIP library.  The robots of the inert cell (tau_max = inf, damping 0) must
reproduce the standing run of quadruped_arm_stack_ground.py at 8 robots bit for bit: that example is run with one line appended that saves
its final states (the loop is a deterministic map of the state, so equal final states after the same number of steps mean equal
trajectories).  The stops are on for every robot, so this holds only while no joint of those robots gets a stop row: that none did is
asserted first.  The largest applied torque of every joint over all ticks respects that joint's tau_max, and no joint ends beyond a limit by more than the gate of the stop test
(tests/test_robot_sim_joint_model.py, case 4: ten times the checker's largest penetration of a held stop)."""
import os

import numpy as np
import pytest

import test_example_push_stack as P
import test_robot_sim_joint_model as J

B, STEPS = 8, 30


def _check(emu, tmp_path):
    trace, ref = str(tmp_path / "actuators.npz"), str(tmp_path / "ground.npy")
    out = P._run("quadruped_arm_stack_actuators.py", [B, STEPS], emu, dict(P.ENV, SMPC_EXAMPLE_TRACE=trace))
    print(out)
    P._run("quadruped_arm_stack_ground.py", [B, STEPS, "stand"], emu, P.ENV, "\nnp.save(%r, X)\n" % ref)
    t, Xg = np.load(trace), np.load(ref)
    assert "simulator: %d robots on the plane z = " % B in out and "robots that stay up:" in out
    for i in range(B):
        assert "robot %d (tau_max scale" % i in out
    assert out.count("peak demanded torque") == B and out.count("largest stop force") == B
    inert = np.isinf(t["scale"]) & (t["damping"] == 0.0)
    assert inert.sum() >= 1 and (~inert).sum() >= 6
    assert (t["stop_rows_max"][inert] == 0).all()  # (no joint of the inert robots came within the activation distance of a limit)
    assert np.isfinite(t["X"][inert]).all() and np.array_equal(t["X"][inert], Xg[inert])
    assert (t["peak_applied"] <= t["peak_demanded"]).all() and (t["peak_demanded"] > 0.0).all()
    # |tau_applied| <= tau_max, joint by joint, on every tick (the example keeps the largest |tau_applied| of every joint over all ticks)
    assert t["peak_applied_joint"].shape == t["tau_max"].shape == (B, len(t["q_lo"]))
    assert (t["peak_applied_joint"] <= t["tau_max"]).all()
    limited = np.isfinite(t["scale"])
    assert np.isfinite(t["tau_max"][limited]).all() and np.isinf(t["tau_max"][~limited]).all()
    assert (t["peak_applied_joint"] == t["tau_max"])[t["scale"] == t["scale"].min()].any()  # (a joint of the weakest actuators sits on its limit)
    assert (t["peak_applied"] < t["peak_demanded"]).any()  # (the weakest actuators are in their limits)
    _, pen = J.knee_loop()
    gate = 10.0 * pen[50:].max()
    q = t["X"][:, 7 : 7 + len(t["q_lo"])]
    ok = np.isfinite(q).all(axis=1)
    beyond = np.maximum(t["q_lo"][None, :] - q[ok], q[ok] - t["q_hi"][None, :]).max()
    print("largest excursion beyond a joint limit at the end %.3e rad (gate %.3e rad); robots up %d of %d" % (max(beyond, 0.0), gate, int(t["up"].sum()), B))
    assert ok.all() and beyond <= gate


def test_quad_arm_actuator_stack_on_the_cpu_build(built, tmp_path):
    _check(True, tmp_path)


@pytest.mark.gpu
def test_quad_arm_actuator_stack(built, tmp_path):
    _check(False, tmp_path)
