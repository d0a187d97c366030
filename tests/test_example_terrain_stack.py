"""examples/quadruped_arm_stack_terrain.py runs end to end (the resident ground stack of quadruped_arm_stack_payload.py, walking, the
controllers on flat ground, every simulated robot on its own height-field tile): 2 robots, the smallest batch that has a robot on the tile
of amplitude 0 and one on a rough tile (amplitude 1 cm), for 0.6 s at a short horizon, on the CPU test build of the kernel bodies and on
the HIP library.  The robot on amplitude 0 must reproduce the same robot of the run without a terrain bit for bit (the example's `flat`
argument; the loop is a deterministic map of the state, so equal final states after the same number of steps mean equal trajectories).  The
robot on the rough tile has finite states, and the normals recorded under its feet are not all e_z."""
import numpy as np
import pytest

import test_example_push_stack as P

B, STEPS = 2, 60


def _check(emu, tmp_path):
    trace, ref = str(tmp_path / "terrain.npz"), str(tmp_path / "flat.npz")
    out = P._run("quadruped_arm_stack_terrain.py", [B, STEPS], emu, dict(P.ENV, SMPC_EXAMPLE_TRACE=trace))
    print(out)
    P._run("quadruped_arm_stack_terrain.py", [B, STEPS, "flat"], emu, dict(P.ENV, SMPC_EXAMPLE_TRACE=ref))
    t, f = np.load(trace), np.load(ref)
    assert "simulator: %d robots on " % B in out and "robots that stay up:" in out
    for i in range(B):
        assert "robot %d (amplitude" % i in out
    assert out.count("along x") == B
    flat = t["amplitude"] == 0.0
    assert flat.sum() >= 1 and (~flat).sum() >= 1 and flat[0]
    # the robot on amplitude 0 stands on a tile that is the plane, and its trajectory is that of the run without a terrain
    assert (t["heights"][0] == t["heights"][0, 0, 0]).all() and np.ptp(t["heights"][1]) > 0.005
    assert np.isfinite(t["X"]).all() and np.array_equal(t["X"][flat], f["X"][flat])
    assert (t["tilt"][flat] == 0.0).all()
    # the robot on the rough tile went elsewhere, and the normals under its feet were tilted
    assert not np.array_equal(t["X"][~flat], f["X"][~flat])
    assert (t["tilt"][~flat] > 1e-3).all()


def test_quad_arm_terrain_stack_on_the_cpu_build(built, tmp_path):
    _check(True, tmp_path)


@pytest.mark.gpu
def test_quad_arm_terrain_stack(built, tmp_path):
    _check(False, tmp_path)
