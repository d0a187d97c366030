"""examples/quadruped_arm_stack_push.py runs end to end (the resident ground stack of quadruped_arm_stack_ground.py, standing, with a
friction coefficient and a lateral push per robot): 2 robots at a short horizon and a short, early push, on the CPU test build of the kernel
bodies and on the HIP library.  Robot 0 (no push, the default mu) must reproduce the standing run of quadruped_arm_stack_ground.py at 2
robots: that example is run with one line appended that saves its final states, and robot 0's whole final state (the base pose with it)
must agree to 1e-8 relative, the resident-stack bar -- the loop is a deterministic map of the state, so equal final states after the same
number of steps mean equal trajectories.  Robot 1 (pushed) must be displaced along the push at the end of the push by more than robot 0,
with a penetration of at most 1 mm.  Whether pushed robots stay up is printed, not gated."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mpc_setup as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"SMPC_EXAMPLE_HORIZON": "12"}


def _run(script, args, emu, env_extra, suffix=""):
    """tests/test_examples.py's _run with source text appended to the example."""
    src = open(os.path.join(ROOT, "examples", script)).read()
    if emu:
        assert "LIB = None" in src
        src = src.replace("LIB = None", "LIB = __import__('mpc_setup').emu_lib()")
    code = "import sys; sys.path.insert(0, %r); sys.argv = ['x'] + %r; __file__ = %r\n" % (
        os.path.join(ROOT, "tests"), [str(a) for a in args], os.path.join(ROOT, "examples", script)) + src + suffix
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env_extra), cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _check(emu, steps, start, length, tmp_path):
    trace, ref = str(tmp_path / "push.npz"), str(tmp_path / "ground.npy")
    out = _run("quadruped_arm_stack_push.py", [2, steps, start, length], emu, dict(ENV, SMPC_EXAMPLE_TRACE=trace))
    print(out)
    _run("quadruped_arm_stack_ground.py", [2, steps, "stand"], emu, ENV, "\nnp.save(%r, X)\n" % ref)
    t, Xg = np.load(trace), np.load(ref)
    assert "simulator: 2 robots on the plane z = " in out and "robot-seconds per second" in out and "robots that stay up:" in out
    assert t["base"].shape == (steps + 1, 2, 3) and int(t["push_end"]) == (start + length) // 10 <= steps
    err = S.rel_err(Xg[0], t["X"][0])
    print("robot 0 against quadruped_arm_stack_ground.py after %d MPC periods: %.2e" % (steps, err))
    assert np.isfinite(t["X"]).all() and err < 1e-8, err
    k = int(t["push_end"])
    dy = t["base"][k, :, 1] - t["base"][0, :, 1]
    print("base displacement along the push at the end of the push: robot 0 %+.3e m, robot 1 %+.3e m" % (dy[0], dy[1]))
    assert dy[1] > dy[0] and dy[1] > 1e-5
    pens = [float(m) for m in re.findall(r"largest penetration ([0-9.e+-]+) m", out)]
    assert len(pens) == 2 and max(pens) <= 1e-3, pens
    m = re.search(r"robot 1 \(push ([0-9.]+) N, mu ([0-9.]+)\)", out)
    assert m and float(m.group(1)) > 0.0 and "robot 0 (push 0 N, mu 0.8)" in out


def test_quad_arm_push_stack_on_the_cpu_build(built, tmp_path):
    _check(True, 3, 10, 10, tmp_path)


@pytest.mark.gpu
def test_quad_arm_push_stack(built, tmp_path):
    _check(False, 8, 20, 50, tmp_path)
