"""examples/biped_legs_stack_ground.py runs end to end (the resident flat-foot stack of biped_legs_stack_resident.py, standing, on the
unilateral ground with four corner points per sole, once with a cold and once with a warm-started contact solve): 2 robots at a short
horizon, on the CPU test build of the kernel bodies and on the HIP library.  Asserted: the run is finite (the example asserts it), the
penetration stays within 1 mm in both runs, the warm run's mean sweeps_used is not above the cold run's, and both robots stay up in both
runs (the emulated run shows it at these lengths)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"SMPC_EXAMPLE_HORIZON": "12"}


def _run(script, args, emu):
    """tests/test_examples.py's _run."""
    src = open(os.path.join(ROOT, "examples", script)).read()
    if emu:
        assert "LIB = None" in src
        src = src.replace("LIB = None", "LIB = __import__('mpc_setup').emu_lib()")
    code = "import sys; sys.path.insert(0, %r); sys.argv = ['x'] + %r; __file__ = %r\n" % (
        os.path.join(ROOT, "tests"), [str(a) for a in args], os.path.join(ROOT, "examples", script)) + src
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **ENV), cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _check(emu, steps):
    out = _run("biped_legs_stack_ground.py", [2, steps], emu)
    print(out)
    assert "simulator: 2 robots on the plane z = " in out and "8 contact points each" in out
    stats = {}
    for name in ("cold", "warm"):
        up = re.search(r"%s: robots that stay up: (\d+) of 2" % name, out)
        pen = re.search(r"%s: largest penetration ([0-9.e+-]+) m" % name, out)
        sw = re.search(r"%s: sweeps_used mean ([0-9.]+), largest (\d+) \(of 60\); largest residual ([0-9.e+-]+) m/s" % name, out)
        assert up and pen and sw and ("%s: " % name) in out and "robot-seconds per second" in out
        stats[name] = dict(up=int(up.group(1)), pen=float(pen.group(1)), mean=float(sw.group(1)), largest=int(sw.group(2)), res=float(sw.group(3)))
    for name, s in stats.items():
        assert s["pen"] <= 1e-3, (name, s)
        assert 1 <= s["largest"] <= 60 and s["mean"] >= 1.0, (name, s)
        assert s["up"] == 2, (name, s)
    assert stats["warm"]["mean"] <= stats["cold"]["mean"], stats


def test_biped_ground_stack_on_the_cpu_build(built):
    _check(True, 3)


@pytest.mark.gpu
def test_biped_ground_stack(built):
    _check(False, 8)
