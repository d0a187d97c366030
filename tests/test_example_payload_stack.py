"""examples/quadruped_arm_stack_payload.py runs end to end (the resident ground stack of quadruped_arm_stack_actuators.py, standing, the
controllers on the nominal table, every simulated robot with its own payload in the gripper and its own base mass): 2 robots, the smallest
batch that has an unloaded robot (payload 0, base scale 1) and a loaded one (1 kg in the gripper), for 0.6 s at a short horizon, on the CPU
test build of the kernel bodies and on the HIP library.  The unloaded robot must reproduce the same robot of the run without body parameters
bit for bit (the example's `nominal` argument; the loop is a deterministic map of the state, so equal final states after the same number of
steps mean equal trajectories).  The loaded robot's mean normal force over the last third of the run exceeds the unloaded one's by the
payload's weight, within the gate of the scale test (tests/test_robot_sim_body_params.py, case 5: ten times the checker's largest relative
deviation of a quasi-static robot's normal force from its weight, of the loaded robot's weight).  The controller plans for the nominal mass,
so the loaded robot sinks while the posture feedback catches up: over the last 0.2 s of 0.6 s its feet carry 7.1 N more than the unloaded
robot's against 9.8 N of extra weight, gate 6.5 N (at 0.3 s the difference is 4.1 N; by 1.0 s the force has reached the weight and the base
has sunk past the example's 8 cm threshold)."""
import numpy as np
import pytest

import test_example_push_stack as P
import test_robot_sim_body_params as BP

B, STEPS = 2, 60
GRAVITY = 9.81


def _check(emu, tmp_path):
    trace, ref = str(tmp_path / "payload.npz"), str(tmp_path / "nominal.npz")
    out = P._run("quadruped_arm_stack_payload.py", [B, STEPS], emu, dict(P.ENV, SMPC_EXAMPLE_TRACE=trace))
    print(out)
    P._run("quadruped_arm_stack_payload.py", [B, STEPS, "nominal"], emu, dict(P.ENV, SMPC_EXAMPLE_TRACE=ref))
    t, n = np.load(trace), np.load(ref)
    assert "simulator: %d robots on the plane z = " % B in out and "robots that stay up:" in out
    for i in range(B):
        assert "robot %d (payload" % i in out
    assert out.count("mean normal force") == B
    unloaded = (t["payload"] == 0.0) & (t["base_scale"] == 1.0)
    assert unloaded.sum() >= 1 and (~unloaded).sum() >= 1 and unloaded[0]
    # the unloaded robot carries the table's rows, and its trajectory is that of the run without body parameters
    assert abs(t["true_mass"][0] - float(t["nominal_mass"])) < 1e-12 * float(t["nominal_mass"]) and (t["true_mass"][~unloaded] > t["true_mass"][0]).all()
    assert np.isfinite(t["X"]).all() and np.array_equal(t["X"][unloaded], n["X"][unloaded])
    assert np.array_equal(t["mean_normal"][unloaded], n["mean_normal"][unloaded])
    assert not np.array_equal(t["X"][~unloaded], n["X"][~unloaded])
    assert t["up"][unloaded].all()
    # the scale: loaded minus unloaded = the extra weight
    ref_sum, mass = BP.scale_loop()
    dev_ref = float((np.abs(ref_sum - mass * BP.GRAVITY * BP.SCALE_LAST) / (mass * BP.GRAVITY * BP.SCALE_LAST)).max())
    f0 = float(t["mean_normal"][0])
    for i in np.flatnonzero(~unloaded):
        extra = (t["true_mass"][i] - t["true_mass"][0]) * GRAVITY
        gate = 10.0 * dev_ref * t["true_mass"][i] * GRAVITY
        got = float(t["mean_normal"][i]) - f0
        print("robot %d: mean normal force above the unloaded robot's %.3f N, extra weight %.3f N, gate %.3f N" % (i, got, extra, gate))
        assert extra > 0.0 and abs(got - extra) <= gate, (got, extra, gate)


def test_quad_arm_payload_stack_on_the_cpu_build(built, tmp_path):
    _check(True, tmp_path)


@pytest.mark.gpu
def test_quad_arm_payload_stack(built, tmp_path):
    _check(False, tmp_path)
