"""Each Riccati sweep (riccati_kino_body, riccati_dense_body<...>, forward_kino_body, forward_full_body, and the centroidal ones: cent_bwd_body /
cent_fwd_body of the point-foot pipeline, riccati_dense_body<Cent6Dims> / cent6_forward_body of 6-D feet) against CPU solves of its own knots
(tests/sweep_check.py): step and gains of ALL stages, per stage and per quantity, at gates of 10 x the measured disagreement of the two CPU
references.  The same bodies run on the emulated kernel bodies (CPU tier) and on the device (-m gpu).  Also here: the single-writer invariant of
the dense cone rows behind O_cdirty, and the rows of [A B] the forward sweep rebuilds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O
import sweep_check as SC

SHORT = dict(horizon=20, cycle=O.walk_cycle(5, 20), mpc_override=dict(T_fly=20, T_contact=5))
TALOS_TIGHT = dict(mu=0.3, Lfoot=0.05, Wfoot=0.04)
TALOS_TURN = (0.2, 0.1, 0, 0, 0, 0.2)
KINO6_TIGHT = dict(mu=0.1, Lfoot=0.01, Wfoot=0.01)
KINO6_TURN = (0.3, 0.2, 0, 0, 0, 0.3)
WALK = np.array([0.2, 0, 0, 0, 0, 0.0])


def _go2_kino(lib, B=2, iters=1, horizon=50, cycle=None, **kw):
    gm, rb, _, _ = S.make_product(B, max_iters=iters, lib=lib, horizon=horizon, **kw)
    gm.generateCycleHorizon(O.trot_cycle() if cycle is None else cycle)
    gm.switchToWalk(WALK)
    return gm, rb


def _steps(gm, X, n):
    for _ in range(n):
        gm.iterate(X)
        X = gm.xs[:, 1, :].copy()
    return X


# ---- scenarios: generators of (label, gm) at every control step that is checked ----
def _kino_record(lib, iters):
    """Settings of record, short trot (4 double / 8 single), checked at control steps 3, 6, 14.  The cycle enters at the far end of the horizon:
    a take-off is inside the horizon from control step 5 on, a touch-down from step 13 on; stage 0 itself stays in full contact until step 54
    (tests/test_knots.py::_kino_record asserts the contact masks; as _cent_record below spells out)."""
    gm, rb = _go2_kino(lib, 2, iters, cycle=O.trot_cycle(T_ds=4, T_ss=8), mpc_override=dict(T_fly=8, T_contact=4))
    X = S.random_states(rb, 2)
    done = 0
    for at in (3, 6, 14):
        X = _steps(gm, X, at - done)
        done = at
        yield " step %d" % at, gm


def _kino_horizon(lib, horizon):
    gm, rb = _go2_kino(lib, 2, 2, horizon=horizon)
    _steps(gm, S.random_states(rb, 2), 3)
    yield "", gm


def _kino_dense_w(lib):
    rb = O.Robot("go2_like")
    s0 = O.go2_kino_settings(rb)
    rng = np.random.default_rng(5)

    def couple(w, eps):
        w = np.array(w, float)
        d = np.sqrt(np.abs(np.diag(w)))
        m = rng.standard_normal(w.shape)
        return w + eps * np.outer(d, d) * (m + m.T) / 2

    gm, rb = _go2_kino(lib, 2, 2, settings_override=dict(w_x=couple(s0["w_x"], 0.05), w_u=couple(s0["w_u"], 0.05)))
    _steps(gm, S.random_states(rb, 2), 3)
    yield "", gm


def _kino_tight(lib):
    q = O.Robot("go2_like").q_ref[7:]
    gm, rb = _go2_kino(lib, 2, 1, settings_override=dict(qmin=q - 0.02, qmax=q + 0.02))
    _steps(gm, S.random_states(rb, 2, scale=0.5), 3)
    nbox, _ = SC.active_rows(gm)
    assert nbox >= 20, ("the scenario must hold active joint-box rows", nbox)
    yield "", gm


def _kino_backtrack(lib):
    gm, rb = _go2_kino(lib, 4, 2)
    X = S.random_states(rb, 4, seed=3, scale=4.0)
    seen = 0
    for step in range(3):
        X = _steps(gm, X, 1)
        seen += int((gm.info[:, 2] < 1.0).sum())
        yield " step %d" % step, gm
    assert seen > 0, "at least one checked instance must have taken alpha < 1"


def _full_go2_record(lib):
    gm, rb, _, _ = S.make_full_product(2, max_iters=2, lib=lib)
    gm.generateCycleHorizon(O.trot_cycle())
    gm.switchToWalk(WALK)
    _steps(gm, S.random_states(rb, 2), 2)
    yield "", gm


def _full_go2_cone(lib):
    gm, rb, _, _ = S.make_full_product(2, max_iters=2, lib=lib, horizon=20, settings_override={"force_cone": True, "mu": 0.6})
    gm.generateCycleHorizon(O.trot_cycle())
    gm.switchToWalk(np.array([0.3, 0.1, 0, 0, 0, 0.2]))
    _steps(gm, S.random_states(rb, 2), 4)
    _, nden = SC.active_rows(gm)
    assert nden >= 50, ("the scenario must hold active friction-cone rows", nden)
    yield "", gm


def _talos(lib, tight, horizon=20):
    kw = dict(SHORT) if horizon == 20 else dict(horizon=horizon, cycle=O.walk_cycle(), mpc_override=None)
    cyc = kw.pop("cycle")
    gm, rb, _, _ = S.make_talos_product(2, max_iters=2, lib=lib, settings_override=TALOS_TIGHT if tight else None, **kw)
    gm.generateCycleHorizon(cyc)
    gm.switchToWalk(np.array(TALOS_TURN if tight else (0.1, 0, 0, 0, 0, 0), float))
    _steps(gm, S.talos_random_states(rb, 2, scale=0.7), 6 if tight else 3)
    if tight:
        _, nden = SC.active_rows(gm)
        assert nden >= 20, ("the scenario must hold active wrench-cone rows", nden)
    yield "", gm


def _talos_kino(lib):
    kw = dict(SHORT)
    cyc = kw.pop("cycle")
    gm, rb, _, _ = S.make_talos_kino_product(2, max_iters=2, lib=lib, settings_override=KINO6_TIGHT, **kw)
    assert gm.ocp_handler.settings["force_cone"]
    gm.generateCycleHorizon(cyc)
    gm.switchToWalk(np.array(KINO6_TURN, float))
    _steps(gm, S.talos_random_states(rb, 2, scale=1.0), 3)
    _, nden = SC.active_rows(gm)
    assert nden >= 8, ("the scenario must hold active wrench-cone rows", nden)
    yield "", gm


# ---- centroidal scenarios.  Generators of (label, gm, om): om is the oracle run on the same measured states when `paired` (the knot parity
#      of tests/test_centroidal_knots.py), else None.  The measured multibody state drifts as a simulator would report it. ----
CENT_HARD = dict(settings_override=dict(mu=0.1), walk=(0.8, 0.5, 0, 0, 0, 0.5))  # (HARD of tests/test_centroidal_mpc.py)
CENT_HARD_SEED = 20240529
TWO_PARTS_INSTS = (0, 63, 64, 127)


def _go2_cent(lib, B, iters, horizon=50, cycle=None, walk=WALK, paired=False, env=None, **kw):
    """env: switches of the engine (SMPC_CENT_PARTS; SMPC_CENT_FUSED of a cross-check build), which it reads when the handle is created."""
    names = ("SMPC_CENT_FUSED", "SMPC_CENT_LS", "SMPC_CENT_PARTS")
    old = {k: os.environ.pop(k, None) for k in names}
    try:
        os.environ.update(env or {})
        gm, rb, _, _ = S.make_cent_product(B, iters, lib, horizon, **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    om = S.make_cent_oracle(B, iters, horizon, **kw)[0] if paired else None
    for m in (gm, om):
        if m is not None:
            m.generateCycleHorizon(O.trot_cycle() if cycle is None else cycle)
            m.switchToWalk(np.array(walk, float))
    if om is not None:
        om.keep_knots()
    return gm, om, rb


def _cent_steps(gm, om, rb, X, n):
    nv = rb.nv
    for _ in range(n):
        gm.iterate(X)
        if om is not None:
            om.iterate(X)
        X = np.stack([rb.integrate(x, np.r_[np.zeros(nv), 0.02, 0.01, np.zeros(nv - 2)]) for x in X])
    return X


def _cent_record(lib, iters, paired=False):
    """Settings of record, H = 50, short trot (4 double / 8 single).  Checked at control steps 3, 6, 14 (ring head 3, 6, 14; the contact changes
    of the cycle are inside the horizon) and at 56 and 64: the cycle enters at the far end of the horizon, so stage 0 has its take-off at
    control step 54 and its touch-down at 62 (ring head 5 and 13: the ring has wrapped)."""
    gm, om, rb = _go2_cent(lib, 2, iters, cycle=O.trot_cycle(T_ds=4, T_ss=8), mpc_override=dict(T_fly=8, T_contact=4), paired=paired)
    X = S.random_states(rb, 2)
    done = 0
    masks = []
    for at in (3, 6, 14, 56, 64):
        X = _cent_steps(gm, om, rb, X, at - done)
        done = at
        masks.append(sum(gm.ocp_handler.getContactState(0)))
        yield " step %d" % at, gm, om
    assert masks == [4, 4, 4, 2, 4], ("stage 0 must have passed a take-off and a touch-down", masks)


def _cent_cones(lib, paired=False):
    """Active friction-cone rows and backtracking: the [Z z] rows of cent_bwd_body, the `any` branch of cent_fwd_body, both pivot panels."""
    kw = dict(CENT_HARD)
    gm, om, rb = _go2_cent(lib, 2, 2, walk=kw.pop("walk"), paired=paired, **kw)
    X = S.random_states(rb, 2, seed=CENT_HARD_SEED, scale=2.0)
    nact, lo, hi, mixed, back = 0, 0, 0, False, False
    for step in range(4):
        X = _cent_steps(gm, om, rb, X, 1)
        for b in range(2):
            kn = SC.knots(gm, b)
            act = np.stack([g["act"] for g in kn])
            anys = np.array([g["any"] for g in kn])
            assert np.array_equal(anys != 0.0, act.any(1)), "the record's flag must say whether a cone row of the stage is active"
            nact += int(act.sum())
            lo += int(act[:, :4].sum())
            hi += int(act[:, 4:].sum())
            mixed = mixed or (anys.any() and not anys.all())
        back = back or bool((gm.info[:, 2] < 1.0).any())
        yield " step %d" % step, gm, om
    assert nact >= 10, ("the scenario must hold active cone rows", nact)
    assert lo > 0 and hi > 0, ("active rows in both pivot panels (rows 0..3 -> nu_a, 4..7 -> nu_b)", lo, hi)
    assert mixed, "one instance must hold stages with and without an active cone row"
    assert back, "at least one instance must have taken alpha < 1"


def _cent_horizon(lib, horizon, paired=False):
    gm, om, rb = _go2_cent(lib, 2, 2, horizon=horizon, paired=paired)
    _cent_steps(gm, om, rb, S.random_states(rb, 2), 3)
    yield "", gm, om


def _cent_dense_w(lib, paired=False):
    """The dense weights and CoM reference of test_centroidal_mpc.py::test_emu_dense_weights_and_com_reference."""
    rng = np.random.default_rng(4)

    def spd(n, s):
        a = rng.normal(size=(n, n))
        return s * (a @ a.T / n + np.eye(n))

    ov = dict(w_u=spd(12, 1e-3), w_com=spd(3, 10.0), w_linear_mom=spd(3, 1.0), w_angular_mom=spd(3, 5.0), w_linear_acc=spd(3, 0.01),
              w_angular_acc=spd(3, 0.01))
    gm, om, rb = _go2_cent(lib, 2, 2, settings_override=ov, paired=paired)
    xr = np.r_[0.02, -0.01, 0.31, np.zeros(6)]
    gm.x_reference = xr
    if om is not None:
        om.set_x_reference(xr)
    _cent_steps(gm, om, rb, S.random_states(rb, 2), 4)
    yield "", gm, om


def _cent_two_parts(lib):
    """B = 128 as two parts of 64 on two streams (record and ring addressing across inst0).  The engine splits by itself from B = 1024 on;
    at this batch SMPC_CENT_PARTS = 2 asks for it (read when the handle is created)."""
    gm, om, rb = _go2_cent(lib, 128, 1, env={"SMPC_CENT_PARTS": "2"})
    _cent_steps(gm, om, rb, S.random_states(rb, 128), 3)
    yield "", gm, om


def _talos_cent(lib, tight, horizon=20, paired=False):
    kw = dict(SHORT) if horizon == 20 else dict(horizon=horizon, cycle=O.walk_cycle(), mpc_override=None)
    walk = TALOS_TURN if tight else (0.1, 0, 0, 0, 0, 0)
    ov = TALOS_TIGHT if tight else None
    if paired:
        om, gm, rb = S.make_talos_cent_pair(2, max_iters=2, lib=lib, walk=walk, settings_override=ov, **kw)
        om.keep_knots()
    else:
        cyc = kw.pop("cycle")
        om = None
        gm, rb, _, _ = S.make_talos_cent_product(2, max_iters=2, lib=lib, settings_override=ov, **kw)
        gm.generateCycleHorizon(cyc)
        gm.switchToWalk(np.array(walk, float))
    _cent_steps(gm, om, rb, S.talos_random_states(rb, 2, scale=0.7), 6 if tight else 3)
    if tight:
        _, nden = SC.active_rows(gm)
        assert nden >= 20, ("the scenario must hold active wrench-cone rows", nden)
    yield "", gm, om


CENT_SCENARIOS = {
    "cent_record_k1": lambda lib, **kw: _cent_record(lib, 1, **kw),
    "cent_record_k3": lambda lib, **kw: _cent_record(lib, 3, **kw),
    "cent_cones_backtrack": _cent_cones,
    "cent_h2": lambda lib, **kw: _cent_horizon(lib, 2, **kw),
    "cent_h63": lambda lib, **kw: _cent_horizon(lib, 63, **kw),  # the last horizon of the polynomial line search (H + 1 <= 64)
    "cent_h65": lambda lib, **kw: _cent_horizon(lib, 65, **kw),  # the first whose pre-pass needs more than one lane per stage slot
    "cent_dense_w": _cent_dense_w,
    "cent_two_parts": _cent_two_parts,
    "talos_cent_walk": lambda lib, **kw: _talos_cent(lib, False, **kw),
    "talos_cent_tight": lambda lib, **kw: _talos_cent(lib, True, **kw),
    "talos_cent_h100": lambda lib, **kw: _talos_cent(lib, False, 100, **kw),  # the device only
}
CENT_INSTS = {"cent_two_parts": TWO_PARTS_INSTS}


def _unpaired(gen):
    return lambda lib: ((label, gm) for label, gm, _ in gen(lib))


SCENARIOS = {
    "kino_record_k1": lambda lib: _kino_record(lib, 1),
    "kino_record_k3": lambda lib: _kino_record(lib, 3),
    "kino_h3": lambda lib: _kino_horizon(lib, 3),
    "kino_h65": lambda lib: _kino_horizon(lib, 65),
    "kino_dense_w": _kino_dense_w,
    "kino_tight_limits": _kino_tight,
    "kino_backtrack": _kino_backtrack,
    "full_go2_record": _full_go2_record,
    "full_go2_cone": _full_go2_cone,
    "talos_walk": lambda lib: _talos(lib, False),
    "talos_tight": lambda lib: _talos(lib, True),
    "talos_kino_cone": _talos_kino,
    "talos_walk_h100": lambda lib: _talos(lib, False, 100),  # the device only
}
SCENARIOS.update({k: _unpaired(v) for k, v in CENT_SCENARIOS.items()})
CPU_SCENARIOS = [k for k in SCENARIOS if k not in ("talos_walk_h100", "talos_cent_h100")]


def _body(name, lib, scenario=None):
    """Runs a scenario and checks it at every yielded control step; returns the device step (dxs, dus) of the last one."""
    for label, gm in SCENARIOS[name](lib):
        res = SC.check(gm, scenario or name, insts=CENT_INSTS.get(name), label=label)
        if SC.is_cent(gm):
            steps = gm.debug_steps()
            continue
        if SC.kind_of(gm) != "kino":
            SC.check_rebuilt_rows(gm, scenario or name, res, label)
        if SC.kind_of(gm) == "kino6":
            SC.check_vel_fold(gm, scenario or name)
        steps = gm.debug_steps()
    return steps


@pytest.mark.parametrize("name", CPU_SCENARIOS)
def test_emulated_sweeps_solve_their_knots(built, name):
    _body(name, S.emu_lib())


def test_emulated_dense_sweep_of_kinodynamics_solves_its_knots(built, tmp_path):
    """riccati_dense_body / the model-independent forward sweep on the Go2 kinodynamics knots (SMPC_RICCATI=dense, read when the handle is
    created: a child process, as test_dense_and_structured_riccati_agree does)."""
    code = (
        "import sys; sys.path.insert(0, %r); import numpy as np, mpc_setup as S, test_sweeps as T\n"
        "dxs, dus = T._body('kino_record_k1', S.emu_lib(), 'kino_record_k1_dense')\n"
        "np.savez(sys.argv[1], dxs=dxs, dus=dus)\n" % os.path.dirname(os.path.abspath(__file__))
    )
    path = str(tmp_path / "dense_steps.npz")
    subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, SMPC_RICCATI="dense"))
    # the switch must have selected another sweep: the structured sweep of this process, on the same scenario, gives a step that differs in
    # its rounding (and only in its rounding) from the child's
    env = os.environ.pop("SMPC_RICCATI", None)
    try:
        dxs, dus = _body("kino_record_k1", S.emu_lib())
    finally:
        if env is not None:
            os.environ["SMPC_RICCATI"] = env
    out = np.load(path)
    assert not (np.array_equal(out["dxs"], dxs) and np.array_equal(out["dus"], dus)), "SMPC_RICCATI=dense did not select the dense sweep"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_hip_sweeps_solve_their_knots(built, name):
    _body(name, None)


def test_checker_raises_on_one_perturbed_entry(built):
    """Self-test of SC.check on cent_record_k1 (emulated bodies; the checker itself is CPU code): the outputs as they are pass; a copy with ONE
    entry moved by 100 x its gate, relative to that stage's block, must raise -- a gain entry at a middle stage, a dvs entry in a stage with an
    active cone row, a dus entry at stage H - 1."""
    name = "cent_record_k1"
    gates = dict(zip(("dxs", "dus", "Ks", "dvs", "dlams"), SC.gate(name)))
    found = None
    for label, gm in SCENARIOS[name](S.emu_lib()):
        acts = [(b, t) for b in range(gm.B) for t, g in enumerate(SC.knots(gm, b)) if g["act"].any()]
        if acts and found is None:
            found = label
            out = SC.device_outputs(gm)
            res = SC.check(gm, name, label=label, outputs={k: v.copy() for k, v in out.items()})
            H = gm.H
            b, t = acts[0]
            row = int(np.flatnonzero(SC.knots(gm, b)[t]["act"])[0])
            for key, idx in (("Ks", (1, H // 2, 5, 4)), ("dvs", (b, t, row)), ("dus", (0, H - 1, 7))):
                pert = {k: v.copy() for k, v in out.items()}
                block = np.abs(out[key][idx[:2]]).max()
                assert block > 0.0
                pert[key][idx] += 100.0 * gates[key] * block
                with pytest.raises(AssertionError) as err:
                    SC.check(gm, name, label=label + " perturbed " + key, outputs=pert, solved=res)
                assert err.value.args[0][3] == key and err.value.args[0][4] == "stage %d" % idx[1], err.value.args
    assert found is not None, "cent_record_k1 must hold a stage with an active cone row at one of its checked steps"


# ---- the dense cone rows of the knot behind O_cdirty ----
def _cdirty_invariant(om, gm, rb, steps, X, oracle_rows, next_state=None):
    """At every control step and every (inst, t): cdirty == 1 exactly when Cd | Dd hold a nonzero entry; both are exactly zero when no dense row
    is active; active rows equal the oracle's (the gate of test_emulated_kernels_talos_stage_knots at iterate 5: 1e-6, floored at 1).  Returns
    how many (inst, t) positions went active -> inactive -> active."""
    B, H = gm.B, gm.H
    hist = np.zeros((steps, B, H), bool)
    for step in range(steps):
        gm.iterate(X)
        if om is not None:
            om.iterate(X)
        X = om.xs[:, 1, :].copy() if next_state is None else next_state(step + 1)
        for b in range(B):
            for t in range(H):
                kg = gm.debug_lq(b, t)
                ncd = kg["Cd"].shape[0]
                nvel = kg["Cv"].shape[0] if "Cv" in kg else 0
                act = kg["act"][gm.nc - nvel - ncd:gm.nc - nvel]
                nz = bool(np.any(kg["Cd"] != 0.0) or np.any(kg["Dd"] != 0.0))
                assert kg["cdirty"] in (0.0, 1.0) and (kg["cdirty"] == 1.0) == nz, (step, b, t, float(kg["cdirty"]), nz)
                if not act.any():
                    assert not nz, (step, b, t, "stale dense cone rows")
                assert np.all(kg["Cd"][act == 0.0] == 0.0) and np.all(kg["Dd"][act == 0.0] == 0.0), (step, b, t)
                hist[step, b, t] = act.any()
                if act.any() and oracle_rows is not None:
                    assert S.rel_err(oracle_rows(om.knot(b, t)), kg["Cd"]) < 1e-6, (step, b, t)
    # a position (b, t) of the knot array: active at some step, inactive later, active again later
    n_flip = 0
    for b in range(B):
        for t in range(H):
            h = hist[:, b, t]
            on = np.flatnonzero(h)
            if len(on) >= 2 and not h[on[0]:on[-1] + 1].all():
                n_flip += 1
    return n_flip, int(hist.sum())


def _cdirty_talos_full(lib, steps):
    om, gm, rb = S.make_talos_pair(2, max_iters=2, lib=lib, walk=TALOS_TURN, settings_override=TALOS_TIGHT, **SHORT)
    om.keep_knots()
    nb = 2 * gm.nu
    n_flip, n_act = _cdirty_invariant(om, gm, rb, steps, S.talos_random_states(rb, 2, scale=0.7), lambda ko: ko["C"][nb:])
    print("O_cdirty, Talos full dynamics: %d active (step, inst, t) positions, %d positions went active -> inactive -> active" % (n_act, n_flip))
    assert n_act > 0 and n_flip > 0, "the run must drive a knot position active -> inactive -> active"


def _cdirty_talos_kino(lib, steps):
    """The kinodynamics variant's cone rows are constant rows of Dd (Cd = 0).  "Active rows equal the oracle's" is not checked here: the parity of Dd (which rows are present, against
    the activity flags) stays with test_talos_kinodynamics.py::test_emulated_kernels_stage_knots; this test holds the flag, the zero block and
    the active -> inactive -> active transition."""
    kw = dict(SHORT)
    cyc = kw.pop("cycle")
    gm, rb, _, _ = S.make_talos_kino_product(2, max_iters=2, lib=lib, settings_override=KINO6_TIGHT, **kw)
    gm.generateCycleHorizon(cyc)
    gm.switchToWalk(np.array(KINO6_TURN, float))
    # (closed on its own plan the cone rows wake up in the first steps and stay asleep afterwards: measured states that alternate between
    #  far from and close to the reference posture make them come and go)
    state = lambda step: S.talos_random_states(rb, 2, seed=step, scale=1.0 if step % 2 == 0 else 0.1)
    n_flip, n_act = _cdirty_invariant(None, gm, rb, steps, state(0), None, state)
    print("O_cdirty, Talos kinodynamics: %d active (step, inst, t) positions, %d positions went active -> inactive -> active" % (n_act, n_flip))
    assert n_act > 0 and n_flip > 0, "the run must drive a knot position active -> inactive -> active"


CDIRTY_STEPS = 14


def test_emulated_cone_block_flag_single_writer_talos_full(built):
    _cdirty_talos_full(S.emu_lib(), CDIRTY_STEPS)


def test_emulated_cone_block_flag_single_writer_talos_kino(built):
    _cdirty_talos_kino(S.emu_lib(), CDIRTY_STEPS)


@pytest.mark.gpu
def test_hip_cone_block_flag_single_writer_talos_full(built):
    _cdirty_talos_full(None, CDIRTY_STEPS)


@pytest.mark.gpu
def test_hip_cone_block_flag_single_writer_talos_kino(built):
    _cdirty_talos_kino(None, CDIRTY_STEPS)
