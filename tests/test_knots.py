"""The LQ knots of the kinodynamics and full-dynamics engines (deriv_body, lane_tree_body -> deriv2_body, fdyn_deriv_body and its KIN = 1
instantiation) against the oracle's knots at an IDENTICAL evaluation point (tests/knot_check.py): every stage, every field, per block, and the
terminal node, at gates of 10 x the measured disagreement of the oracle with its reframed twin.  The same bodies run on the emulated kernel
bodies (CPU tier) and on the device (-m gpu).  Also here: the CPU test of the oracle entries the sync needs (set_iterate, terminal_knot) and
the checker's self-test."""
import os

import numpy as np
import pytest

import knot_check as KC
import mpc_setup as S
import oracle_lib as O
import test_sweeps as T

LANE_SWITCHES = ("SMPC_LANE_EVAL", "SMPC_LANE_DERIV", "SMPC_LANE_STREAM")
B65_INSTS = (0, 63, 64)


def _walk(ms, cycle, walk):
    for m in ms:
        if m is not None:
            m.generateCycleHorizon(cycle)
            m.switchToWalk(np.array(walk, float))
            if isinstance(m, O.OracleMPC):
                m.keep_knots()


def _with_env(env, make):
    """The engine reads its switches when the handle is created: set them for `make()` alone and restore."""
    old = {k: os.environ.pop(k, None) for k in LANE_SWITCHES}
    try:
        os.environ.update(env or {})
        return make()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _go2_kino(lib, twin, B=2, horizon=50, cycle=None, env=None, **kw):
    gm, rb, _, _ = _with_env(env, lambda: S.make_product(B, 1, lib, horizon, **kw))
    om = S.make_oracle(B, 1, horizon, **kw)[0]
    om2 = S.make_oracle(B, 1, horizon, robot="go2_like_rf", **kw)[0] if twin else None
    _walk((gm, om, om2), O.trot_cycle() if cycle is None else cycle, T.WALK)
    return gm, om, om2, rb


def _go2_full(lib, twin, B=2, horizon=50, cycle=None, walk=T.WALK, **kw):
    gm, rb, _, _ = S.make_full_product(B, 1, lib, horizon, **kw)
    om = S.make_full_oracle(B, 1, horizon, walk=None, **kw)[0]
    om2 = S.make_full_oracle(B, 1, horizon, walk=None, robot="go2_like_rf", **kw)[0] if twin else None
    _walk((gm, om, om2), O.trot_cycle() if cycle is None else cycle, walk)
    return gm, om, om2, rb


def _talos_oracle(kino, robot, horizon, settings_override, mpc_override):
    rb = S._oracle_robot(robot, "talos_like")
    s = (O.talos_kino_settings if kino else O.talos_full_settings)(rb)
    s.update(settings_override or {})
    ms = O.talos_mpc_settings(rb, max_iters=1)
    ms["T"] = horizon
    ms.update(mpc_override or {})
    return O.OracleMPC(O.Kino(rb, s), ms, 2) if kino else O.OracleFullMPC(O.Full(rb, s), ms, 2)


def _talos(lib, twin, kino, walk, settings_override=None):
    kw = dict(T.SHORT)
    cyc = kw.pop("cycle")
    make = S.make_talos_kino_product if kino else S.make_talos_product
    gm, rb, _, _ = make(2, max_iters=1, lib=lib, settings_override=settings_override, **kw)
    om = _talos_oracle(kino, None, kw["horizon"], settings_override, kw["mpc_override"])
    om2 = _talos_oracle(kino, "talos_like_rf", kw["horizon"], settings_override, kw["mpc_override"]) if twin else None
    _walk((gm, om, om2), cyc, walk)
    return gm, om, om2, rb


def _run(gm, om, om2, X, checked):
    """Synced control steps (every step is synced: the oracles follow the product's closed loop); yields at the checked ones."""
    oms = [m for m in (om, om2) if m is not None]
    for step in range(1, max(checked) + 1):
        X = KC.synced_step(gm, oms, X)
        if step in checked:
            yield (" step %d" % step) if len(checked) > 1 else "", gm, om, om2


# ---- scenarios: generators of (label, gm, om, om2) at the checked control steps; om2 is the oracle on the reframed twin (floors) or None ----
def _kino_record(lib, twin=False, env=None):
    """Settings of record, H = 50, short trot (4 double / 8 single), checked at the control steps 3, 6 and 14.  The cycle enters at the far end
    of the horizon, so at these steps a take-off (stage 46 at step 6, 38 at step 14) and a touch-down (stage 46 at step 14) are among the
    checked stages, while stage 0 itself stays in full contact until control step 54 (as test_sweeps.py::_cent_record spells out)."""
    gm, om, om2, rb = _go2_kino(lib, twin, cycle=O.trot_cycle(T_ds=4, T_ss=8), mpc_override=dict(T_fly=8, T_contact=4), env=env)
    masks = set()
    for out in _run(gm, om, om2, S.random_states(rb, 2), (3, 6, 14)):
        masks |= {tuple(gm.ocp_handler.getContactState(t)) for t in range(gm.H)}
        yield out
    assert len(masks) >= 2, ("swing stages must be among the checked stages", masks)


def _kino_horizon(lib, horizon, twin=False):
    gm, om, om2, rb = _go2_kino(lib, twin, horizon=horizon)
    yield from _run(gm, om, om2, S.random_states(rb, 2), (3,))


def _kino_dense_w(lib, twin=False):
    rb = O.Robot("go2_like")
    s0 = O.go2_kino_settings(rb)
    rng = np.random.default_rng(5)

    def couple(w, eps):
        w = np.array(w, float)
        d = np.sqrt(np.abs(np.diag(w)))
        m = rng.standard_normal(w.shape)
        return w + eps * np.outer(d, d) * (m + m.T) / 2

    gm, om, om2, rb = _go2_kino(lib, twin, settings_override=dict(w_x=couple(s0["w_x"], 0.05), w_u=couple(s0["w_u"], 0.05)))
    yield from _run(gm, om, om2, S.random_states(rb, 2), (3,))


def _kino_tight(lib, twin=False):
    q = O.Robot("go2_like").q_ref[7:]
    gm, om, om2, rb = _go2_kino(lib, twin, settings_override=dict(qmin=q - 0.02, qmax=q + 0.02))
    for out in _run(gm, om, om2, S.random_states(rb, 2, scale=0.5), (3,)):
        n = KC.active_rows(gm)
        assert n["joint box"] >= 20, ("the scenario must hold active joint-box rows", n)
        yield out


def _kino_b65(lib, twin=False):
    """B = 65: smpc_kino_lane.h runs one lane per problem, 64 consecutive instances per wavefront -- instance 64 is a lone lane in a second
    wavefront, instance 63 the last lane of the first."""
    gm, om, om2, rb = _go2_kino(lib, twin, B=65, horizon=10)
    yield from _run(gm, om, om2, S.random_states(rb, 65), (3,))


def _full_go2_record(lib, twin=False):
    gm, om, om2, rb = _go2_full(lib, twin)
    for out in _run(gm, om, om2, S.random_states(rb, 2), (12,)):
        masks = {tuple(gm.ocp_handler.getContactState(t)) for t in range(gm.H)}
        assert len(masks) >= 2, "swing stages must be inside the horizon"
        yield out


def _full_go2_cone(lib, twin=False):
    gm, om, om2, rb = _go2_full(lib, twin, horizon=20, walk=(0.3, 0.1, 0, 0, 0, 0.2), settings_override={"force_cone": True, "mu": 0.6})
    for out in _run(gm, om, om2, S.random_states(rb, 2), (4,)):
        n = KC.active_rows(gm)
        assert n["cone"] >= 50, ("the scenario must hold active friction-cone rows", n)
        yield out


def _full_go2_land(lib, twin=False):
    """land_cstr with the settings of test_fulldyn_land_cstr.py: a landing stage is inside the horizon at the checked step."""
    gm, om, om2, rb = _go2_full(lib, twin, horizon=20, cycle=O.trot_cycle(2, 6), settings_override={"land_cstr": True},
                                mpc_override={"T_fly": 6, "T_contact": 2})
    for out in _run(gm, om, om2, S.random_states(rb, 2), (12,)):
        n = KC.active_rows(gm)
        assert n["land"] >= 8, ("the scenario must hold active land rows (4 per landing foot, two feet land together)", n)
        yield out


def _full_go2_wide_cone(lib, twin=False):
    """mu = 3 (test_fulldyn_friction_cone.py::test_emulated_kernels_wide_cones): cone rows present, none active along the trajectory."""
    gm, om, om2, rb = _go2_full(lib, twin, horizon=20, settings_override={"force_cone": True, "mu": 3.0})
    yield from _run(gm, om, om2, S.random_states(rb, 2), (5,))


def _talos_full(lib, tight, twin=False):
    gm, om, om2, rb = _talos(lib, twin, False, T.TALOS_TURN if tight else (0.1, 0, 0, 0, 0, 0), T.TALOS_TIGHT if tight else None)
    for out in _run(gm, om, om2, S.talos_random_states(rb, 2, scale=0.7), (6 if tight else 3,)):
        if tight:
            n = KC.active_rows(gm)
            assert n["cone"] >= 20, ("the scenario must hold active wrench-cone rows", n)
        yield out


def _talos_kino(lib, cone, twin=False):
    gm, om, om2, rb = _talos(lib, twin, True, T.KINO6_TURN, dict(T.KINO6_TIGHT, force_cone=cone))
    assert bool(gm.ocp_handler.settings["force_cone"]) == cone
    for out in _run(gm, om, om2, S.talos_random_states(rb, 2, scale=1.0), (3,)):
        if cone:
            n = KC.active_rows(gm)
            assert n["cone"] >= 8, ("the scenario must hold active wrench-cone rows", n)
        yield out


SCENARIOS = {
    "kino_record": _kino_record,
    "kino_h3": lambda lib, **kw: _kino_horizon(lib, 3, **kw),
    "kino_h65": lambda lib, **kw: _kino_horizon(lib, 65, **kw),
    "kino_dense_w": _kino_dense_w,
    "kino_tight_limits": _kino_tight,
    "kino_b65": _kino_b65,
    # the record scenario on the one-kernel derivative pass (deriv_body), and with the line search on the one-kernel path too
    "kino_one_kernel_deriv": lambda lib, **kw: _kino_record(lib, env={"SMPC_LANE_DERIV": "0"}, **kw),
    "kino_one_kernel_eval": lambda lib, **kw: _kino_record(lib, env={"SMPC_LANE_EVAL": "0"}, **kw),
    "full_go2_record": _full_go2_record,
    "full_go2_cone": _full_go2_cone,
    "full_go2_land": _full_go2_land,
    "full_go2_wide_cone": _full_go2_wide_cone,
    "talos_walk": lambda lib, **kw: _talos_full(lib, False, **kw),
    "talos_tight": lambda lib, **kw: _talos_full(lib, True, **kw),
    "talos_kino_cone": lambda lib, **kw: _talos_kino(lib, True, **kw),
    "talos_kino_nocone": lambda lib, **kw: _talos_kino(lib, False, **kw),
}
INSTS = {"kino_b65": B65_INSTS}
XCHECK = ("kino_one_kernel_deriv", "kino_one_kernel_eval")  # (on the device the one-kernel path of a cone-free problem lives in the cross-check build)


def _body(name, lib):
    n = 0
    for label, gm, om, _ in SCENARIOS[name](lib):
        KC.check(gm, om, name, insts=INSTS.get(name), label=label)
        n += 1
    assert n > 0


def measure_floors(name):
    """Row of KC.FLOORS for a scenario (emulated bodies; the largest of the checked control steps)."""
    row = None
    for label, gm, om, om2 in SCENARIOS[name](S.emu_lib(), twin=True):
        r = KC.floors(gm, om, om2, INSTS.get(name))
        row = r if row is None else tuple(max(a, b) for a, b in zip(row, r))
    print('    "%s": (%s),' % (name, ", ".join("%.1e" % v for v in row)))
    return row


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_emulated_knots_match_oracle_per_block(built, name):
    _body(name, S.emu_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_hip_knots_match_oracle_per_block(built, name):
    _body(name, S.xcheck_lib() if name in XCHECK else None)


# ---- the oracle entries of the sync ----
def _oracle_state(om):
    return [a.copy() for a in (om.xs, om.us, om.vs, om.lams, om.info, om.K0)]


@pytest.mark.parametrize("kind", ["kino", "full"])
def test_oracle_set_iterate_of_own_iterate_changes_nothing(kind):
    """set_iterate(the oracle's own iterate) must leave the next iterate bit-identical to a run without it; set_iterate of another iterate
    must be what the next iterate starts from."""
    def pair():
        if kind == "kino":
            a, rb, _ = S.make_oracle(2, 1, 10)
        else:
            a, rb = S.make_full_oracle(2, 1, 10, walk=None)
        _walk((a,), O.trot_cycle(2, 6), T.WALK)
        return a, rb

    (a, rb), (b, _) = pair(), pair()
    X = S.random_states(rb, 2)
    for step in range(3):
        b.set_iterate(b.xs, b.us, b.vs, b.lams)
        a.iterate(X)
        b.iterate(X)
        for u, v in zip(_oracle_state(a), _oracle_state(b)):
            assert np.array_equal(u, v), step
        for t in (0, 9):
            ka, kb = a.knot(1, t), b.knot(1, t)
            assert all(np.array_equal(ka[k], kb[k]) for k in ka)
        X = a.xs[:, 1, :].copy()
    # another iterate: the knots of the next iteration are evaluated there (A of stage t at xs[t + 1], us[t + 1] of what was set)
    xs, us = a.xs.copy(), a.us.copy()
    xs[:, 3, 7] += 1e-3
    b.set_iterate(xs, us, a.vs, a.lams)
    assert np.array_equal(b.xs, xs) and np.array_equal(b.us, us) and np.array_equal(b.vs, a.vs) and np.array_equal(b.lams, a.lams)
    a.iterate(X)
    b.iterate(X)
    assert np.array_equal(a.knot(0, 5)["A"], b.knot(0, 5)["A"]) and not np.array_equal(a.knot(0, 2)["A"], b.knot(0, 2)["A"])


def test_oracle_terminal_knot_is_the_terminal_node():
    """terminal_knot against QN = LxxN + preg I, qN = lxN - lam_H recomputed in numpy: kinodynamics from orc_kino_term's pieces (oracle_lib
    Kino.term); full dynamics (no export of the terminal derivatives) by central differences of Full.term."""
    om, rb, K = S.make_oracle(2, 1, 10)
    _walk((om,), O.trot_cycle(2, 6), T.WALK)
    X = S.random_states(rb, 2)
    for _ in range(3):
        xs0 = om.xs
        om.iterate(X)
        X = om.xs[:, 1, :].copy()
    for b in range(2):
        QN, qN, preg = om.terminal_knot(b)
        assert preg == 1e-9
        # the iterate the iteration was evaluated at: the receded one (stage H repeats stage H; the trailing multiplier is zeroed)
        _, lx, Lxx = K.term(rb.x_ref, xs0[b, -1])
        assert np.array_equal(QN, Lxx + preg * np.eye(K.ndx))
        assert np.array_equal(qN, lx)  # (qN = lxN - lam_H, and the recede has zeroed lam_H)
    # with a multiplier at the terminal node: set one
    lams = om.lams
    lams[:, -2:] = np.random.default_rng(1).normal(size=lams[:, -2:].shape)
    om.set_iterate(om.xs, om.us, om.vs, lams)
    xsH = om.xs[:, -1]
    om.iterate(X)
    for b in range(2):
        QN, qN, preg = om.terminal_knot(b)
        _, lx, Lxx = K.term(rb.x_ref, xsH[b])
        assert np.array_equal(QN, Lxx + preg * np.eye(K.ndx)) and np.array_equal(qN, lx)  # (the recede zeroes lam_H)
    of, rb = S.make_full_oracle(1, 1, 6, walk=None)
    _walk((of,), O.trot_cycle(2, 6), T.WALK)
    of.iterate(S.random_states(rb, 1))
    xH = of.xs[0, -1]
    of.iterate(of.xs[:, 1, :].copy())
    QN, qN, preg = of.terminal_knot(0)
    F, eps = of.kino, 1e-6
    g = np.zeros(F.ndx)
    for i in range(F.ndx):
        e = np.zeros(F.ndx)
        e[i] = eps
        g[i] = (F.term(rb.x_ref, rb.integrate(xH, e)) - F.term(rb.x_ref, rb.integrate(xH, -e))) / (2 * eps)
    assert np.abs(qN - g).max() < 1e-6 * max(1.0, np.abs(g).max())  # (central differences of a quadratic cost: rounding over eps)
    assert np.abs(QN - QN.T).max() < 1e-14 * np.abs(QN).max() and np.all(np.linalg.eigvalsh((QN + QN.T) / 2) > 0) and preg == 1e-9


# ---- the checker's self-test ----
@pytest.mark.parametrize("name", ["kino_record", "talos_tight"])
def test_checker_raises_on_one_perturbed_entry(built, name):
    """KC.check on the emulated bodies: the outputs as they are pass; a copy with ONE entry moved by 100 x its gate, relative to its own block,
    must raise and name the field, the stage and the block -- an entry of the base-angular columns of A at a middle stage, an entry of an active
    row of [C D], an entry of qN."""
    gates = KC.gate(name)
    label, gm, om, _ = list(SCENARIOS[name](S.emu_lib()))[-1]
    out = KC.device_outputs(gm)
    KC.check(gm, om, name, label=label, outputs=out)
    H, part = gm.H, KC.blocks(gm)
    x = dict(part["x"])
    # an active row of [C D]: the first stage of instance 0 that holds one in a dense family
    fld = "D" if name == "talos_tight" else "C"
    fam = "cone" if name == "talos_tight" else "frame vel"
    cols = dict(part["u"] if fld == "D" else part["x"])
    found = None
    for t in range(H):
        for rn, ri in part["c"]:
            act = np.flatnonzero(out[(0, t)]["act"][ri])
            if rn.startswith(fam) and len(act) and found is None:
                row = ri[act[0]]
                cn = max(cols, key=lambda c: np.abs(out[(0, t)][fld][row, cols[c]]).max())
                found = (t, rn, row, cn, int(cols[cn][np.abs(out[(0, t)][fld][row, cols[cn]]).argmax()]))
    assert found is not None
    t, rn, row, cn, col = found
    # qN: the block that is largest against the terms it is a difference of (KC.term_gaps)
    oQ, oq, _ = om.terminal_knot(0)
    qb = max(x, key=lambda n: np.abs(oq[x[n]]).max() / max(np.abs(oQ[x[n]]).max(), 1e-300))
    # the base-angular columns of A at a middle stage: the derivative block (not the identity's) that is largest there
    Am = out[(1, H // 2)]["A"]
    ar = max((n for n in x if n != "base ang"), key=lambda n: np.abs(Am[np.ix_(x[n], x["base ang"])]).max())
    cases = [("A", (1, H // 2), (int(x[ar][1]), int(x["base ang"][1])), ar + " x base ang"), (fld, (0, t), (row, col), rn + " x " + cn),
             ("qN", (0, "N"), (int(x[qb][np.abs(oq[x[qb]]).argmax()]),), qb)]
    for key, at, idx, blk in cases:
        pert = dict(out)
        if key == "qN":
            QN, qN = out[at]
            qN = qN.copy()
            block = np.abs(qN[x[blk]]).max()
            assert block > 0.0
            qN[idx] += 100.0 * gates[key] * block
            pert[at] = (QN, qN)
        else:
            kg = dict(out[at])
            kg[key] = kg[key].copy()
            rn_, cn_ = blk.split(" x ")
            rows = dict(part["c"] if key in ("C", "D") else part["x"])[rn_]
            block = np.abs(kg[key][np.ix_(rows, (cols if key == fld else x)[cn_])]).max()
            assert block > 0.0, (key, blk)
            kg[key][idx] += 100.0 * gates[key] * block
            pert[at] = kg
        with pytest.raises(AssertionError) as err:
            KC.check(gm, om, name, label=label + " perturbed " + key, outputs=pert)
        first = err.value.args[0]
        stage = "terminal node" if at[1] == "N" else "stage %d" % at[1]
        assert first[2:6] == ("instance %d" % at[0], key, stage, blk), (first, key, at, blk)
