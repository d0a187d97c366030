"""Characterisation of the host driver the kinodynamics and the dense (full-dynamics / 6-D kinodynamics) engines share
(smpc_stage_engine.h): for one handle of each family, the launch schedule (calls per kernel slot of smpc_get_kernel_times_n after the
constructor and after a few control steps, cold-solve iteration count), the checkpoint (size, bit-identical resume) and what each
handle kind answers to the debug getters it refuses.  The constants were recorded before the two engines were put on one driver:
a host refactor must reproduce them exactly."""
import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O

SLOTS = ["recede", "deriv", "riccati", "forward", "trial", "select", "apply", "tree", "tree_ls"]
B, H, STEPS = 2, 30, 3
# (max_iters, early exit): one sequential iteration | the speculative schedule | the sequential schedule with the convergence test
SCHEDULES = [(1, False), (3, False), (3, True)]

KINO_EXT = dict(settings_override={"force_cone": True, "land_cstr": True, "mu": 0.3}, mpc_override={"terminal_constraint": True})
FAMILIES = {
    "go2_kino": (S.make_product, {}, "kino", O.trot_cycle, S.random_states),
    "go2_kino_ext": (S.make_product, KINO_EXT, "kino", O.trot_cycle, S.random_states),
    "go2_full": (S.make_full_product, {}, "full", O.trot_cycle, S.random_states),
    "talos_full": (S.make_talos_product, {}, "full", O.walk_cycle, S.talos_random_states),
    "talos_kino6d": (S.make_talos_kino_product, {}, "full", O.walk_cycle, S.talos_random_states),
}

# per family: cold-solve iterations, calls per slot after the constructor, calls per slot after STEPS control steps (constructor
# included) for each entry of SCHEDULES, bytes of the checkpoint
RECORDED = {
    "go2_kino": dict(cold_iters=4, ctor=[0, 4, 4, 4, 4, 21, 4, 4, 4], state_size=126717,
                     steps=[[3, 7, 7, 7, 7, 36, 7, 7, 7], [3, 13, 13, 13, 7, 99, 13, 13, 7], [3, 13, 13, 13, 13, 66, 13, 13, 13]]),
    "go2_kino_ext": dict(cold_iters=4, ctor=[0, 4, 4, 8, 4, 16, 4, 0, 0], state_size=132717,
                         steps=[[3, 7, 7, 14, 7, 28, 7, 0, 0], [3, 13, 13, 26, 7, 79, 13, 0, 0], [3, 13, 13, 26, 13, 52, 13, 0, 0]]),
    "go2_full": dict(cold_iters=7, ctor=[0, 7, 7, 7, 7, 42, 7, 0, 0], state_size=126509,
                     steps=[[3, 10, 10, 10, 10, 60, 10, 0, 0], [3, 16, 16, 16, 10, 123, 16, 0, 0], [3, 16, 16, 16, 16, 96, 16, 0, 0]]),
    "talos_full": dict(cold_iters=4, ctor=[0, 4, 4, 4, 4, 24, 4, 0, 0], state_size=291529,
                       steps=[[3, 7, 7, 7, 7, 42, 7, 0, 0], [3, 13, 13, 13, 7, 105, 13, 0, 0], [3, 13, 13, 13, 13, 78, 13, 0, 0]]),
    "talos_kino6d": dict(cold_iters=4, ctor=[0, 4, 4, 4, 4, 24, 4, 0, 0], state_size=331465,
                         steps=[[3, 7, 7, 7, 7, 42, 7, 0, 0], [3, 13, 13, 13, 7, 105, 13, 0, 0], [3, 13, 13, 13, 13, 78, 13, 0, 0]]),
}

# what a handle kind answers (return code, text) to: debug_lq with a bad index, debug_terminal with a bad instance, phase_cycles
# with the timers off, get_contact_forces (a dense handle has them: None)
ERRORS = {
    "kino": [
        (-1, "Stage index exceeds stage vector size"),
        (-1, "instance index out of range"),
        (-1, "phase timers are off (set SMPC_PHASE_PROFILE=1 before smpc_create)"),
        (-1, "smpc_get_contact_forces needs a full-dynamics handle (the other problems carry the forces in us)"),
    ],
    "full": [
        (-2, "Stage index exceeds stage vector size"),
        (-2, "instance index out of range"),
        (-2, "phase timers are off (set SMPC_PHASE_PROFILE=1 before smpc_create_fulldynamics)"),
        None,
    ],
}


def _calls(gm):
    kt = gm.kernel_times()
    return [kt[n][1] for n in SLOTS]


def _outputs(gm):
    return [gm.xs, gm.us, gm.vs, gm.lams, gm.info]


def _measure(family, lib):
    make, kw, kind, cycle, states = FAMILIES[family]
    rec = {"steps": []}
    for max_iters, early in SCHEDULES:
        gm, rb, _, _ = make(B, max_iters, lib=lib, horizon=H, **kw)
        if early:
            gm.setEarlyExitOnTol(True)
        rec["cold_iters"] = len(gm.cold_trace())
        rec["ctor"] = _calls(gm)
        gm.generateCycleHorizon(cycle())
        gm.switchToWalk(np.array([0.1, 0, 0, 0, 0, 0.0]))
        Xs = [states(rb, B, seed=s, scale=0.5) for s in range(STEPS + 2)]
        for k in range(STEPS):
            gm.iterate(Xs[k])
        rec["steps"].append(_calls(gm))
        blob = gm.save_state()
        rec["state_size"] = len(blob)
        ref = []
        for k in range(STEPS, STEPS + 2):
            gm.iterate(Xs[k])
            ref.append(_outputs(gm))
        gm.load_state(blob)
        for k in range(STEPS, STEPS + 2):
            gm.iterate(Xs[k])
            for a, b in zip(_outputs(gm), ref[k - STEPS]):
                assert np.array_equal(a, b)
    # the debug getters this handle kind refuses (gm: the last handle)
    L, h = gm._lib.L, gm._h
    out = np.zeros(max(int(L.smpc_lq_size(h)), gm.ndx * gm.ndx, gm.B * gm.H * gm.nf * 6, 64))
    q = np.zeros(gm.ndx)
    got = []
    for call in (lambda: L.smpc_debug_get_lq(h, 0, H, out), lambda: L.smpc_debug_get_terminal(h, B, out, q), lambda: L.smpc_debug_get_phase_cycles(h, out)):
        got.append((call(), L.smpc_last_error().decode()))
    rc = L.smpc_get_contact_forces(h, out)
    got.append((rc, L.smpc_last_error().decode()) if rc != 0 else None)
    rec["errors"] = got
    return rec, kind


def _case(family, lib, monkeypatch):
    monkeypatch.delenv("SMPC_PHASE_PROFILE", raising=False)
    rec, kind = _measure(family, lib)
    print("measured %s: %r" % (family, rec))
    want = RECORDED[family]
    assert rec["cold_iters"] == want["cold_iters"]
    assert rec["ctor"] == want["ctor"]
    assert rec["steps"] == want["steps"]
    assert rec["state_size"] == want["state_size"]
    assert rec["errors"] == ERRORS[kind]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_engine_schedule_emu(built, family, monkeypatch):
    _case(family, S.emu_lib(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_engine_schedule_gpu(built, family, monkeypatch):
    _case(family, None, monkeypatch)
