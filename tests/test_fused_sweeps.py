"""Both kinodynamics sweeps as one staggered persistent launch (sweeps_kino_body) against the two-launch form.

The fused launch runs the SAME per-instance device functions (riccati_kino_inst, forward_kino_inst) in another order, so everything a
caller can read must be bit-identical: np.array_equal, on the sequential-lane build and on the GPU.  Shapes: the smallest grids at
which a slot's walk can go wrong (smpc_sweep_order.h; the walks themselves are checked by tests/cpp/sweep_order_check.cpp):

    slots  B   walks per slot
      2    3   BFBF / BF
      2    4   BFBF / BBFF
      2    7   BFBFBFBF / BBFF BF
      3    7   uneven lists: BFBFBF / BBFF / BFBF
      1    3   one slot walks everything

Go2 kinodynamics, H = 30, max_iters = 3 (the speculative schedule), three control steps from random states.
"""
import os
import subprocess

import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, ITERS, STEPS = 30, 3, 3
CASES = [(2, 3), (2, 4), (2, 7), (3, 7), (1, 3)]  # (SMPC_SWEEP_SLOTS, B)
NAMES = ["xs", "us", "vs", "lams", "K0", "info", "Ks"]
SWITCHES = ("SMPC_FUSED_SWEEPS", "SMPC_SWEEP_SLOTS", "SMPC_STREAMS", "SMPC_PHASE_PROFILE")


def _run(lib, B, env, monkeypatch):
    """Outputs after every control step and the calls per kernel slot of a handle created under `env`."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gm, rb, _, _ = S.make_product(B, ITERS, lib=lib, horizon=H)  # (the switches are read at handle creation)
    for k in env:
        monkeypatch.delenv(k)
    ctor = gm.kernel_times()
    gm.generateCycleHorizon(O.trot_cycle())
    gm.switchToWalk(np.array([0.1, 0, 0, 0, 0, 0.0]))
    outs = []
    for k in range(STEPS):
        gm.iterate(S.random_states(rb, B, seed=k, scale=0.5))
        outs.append([np.array(getattr(gm, n)) for n in NAMES])
    return outs, ctor, gm.kernel_times()


_two_launch = {}  # (library, B) -> the two-launch form's run, computed once and shared by the cases of that B


def _reference(key, lib, B, monkeypatch):
    if (key, B) not in _two_launch:
        _two_launch[(key, B)] = _run(lib, B, {"SMPC_FUSED_SWEEPS": "0"}, monkeypatch)
    return _two_launch[(key, B)]


def _case(key, lib, slots, B, monkeypatch):
    ref, ref_ctor, ref_kt = _reference(key, lib, B, monkeypatch)
    got, ctor, kt = _run(lib, B, {"SMPC_FUSED_SWEEPS": "1", "SMPC_SWEEP_SLOTS": str(slots)}, monkeypatch)
    for k in range(STEPS):
        for n, a, b in zip(NAMES, got[k], ref[k]):
            assert np.isfinite(b).all(), (n, k)
            assert np.array_equal(a, b), "%s differs after control step %d: max |diff| = %g" % (n, k, np.abs(a - b).max())
    # the two-launch form: one forward launch per backward launch.  The fused form: the same number of launches in the backward
    # sweep's slot, and forward launches only where the launch was not fused -- the cold solve of the constructor
    assert ref_kt["riccati"][1] == ref_kt["forward"][1] > ref_ctor["riccati"][1]
    assert {n: v[1] for n, v in ctor.items()} == {n: v[1] for n, v in ref_ctor.items()}
    assert kt["riccati"][1] == ref_kt["riccati"][1]
    assert kt["forward"][1] == ctor["forward"][1]
    for n in ("deriv", "trial", "select", "apply", "tree", "tree_ls", "recede"):
        assert kt[n][1] == ref_kt[n][1], n


def _default_small_batch(lib, monkeypatch):
    """A default handle whose batch does not exceed the resident slots runs the two launches (every grid has at least 16 slots)."""
    _, _, kt = _run(lib, 2, {}, monkeypatch)
    assert kt["riccati"][1] == kt["forward"][1] > 0


def test_sweep_orders_host(tmp_path):
    exe = str(tmp_path / "sweep_order_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "simple-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sweep_order_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sweep order check: OK" in out.stdout


@pytest.mark.parametrize("slots,B", CASES)
def test_fused_sweeps_bit_identical_emu(built, slots, B, monkeypatch):
    _case("emu", S.emu_lib(), slots, B, monkeypatch)


def test_default_small_batch_two_launches_emu(built, monkeypatch):
    _default_small_batch(S.emu_lib(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("slots,B", CASES)
def test_fused_sweeps_bit_identical_gpu(built, slots, B, monkeypatch):
    _case("gpu", None, slots, B, monkeypatch)


@pytest.mark.gpu
def test_default_small_batch_two_launches_gpu(built, monkeypatch):
    _default_small_batch(None, monkeypatch)
