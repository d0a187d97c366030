"""The constant tile column of the kinodynamics knot (Dims::CT_J, smpc_model.h): the joint-acceleration columns of S (zeros) and of R (the
weights w_u) live once per handle, the current diagonal of that block of R (w + preg of the derivation) and the 0 / 1 selectors of the joint-box
rows of C as two contiguous runs of the knot.  The knot getter puts them back where the documented row-major form has them; the sweeps read
them from their new places.  Go2 kinodynamics, B = 3, H = 4, with a diagonal and with a full SPD w_u; the emulated kernel bodies (CPU tier) and
the device (-m gpu) run the same bodies.

Bars: the oracle's knot as test_stage_knots_match_oracle; the closed loop as test_closed_loop_parity of either tier; structured against dense
sweep as test_dense_and_structured_riccati_agree; the own-knot sweep check by the rule of sweep_check.py (10 x the mutual gap of its two CPU
references on the very knots of the run, 1e-11 where that gap is below 1e-12) -- the scenarios here (H = 4) have no row in its table, so the
floor is measured in the run (neither reference is the code under test)."""
import os

import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O
import sweep_check as SC

B, H = 3, 4
NA, UC = 12, 12  # joints ; first joint-acceleration column of u = [forces(12) | accelerations(12)]
LIMIT_JOINT = 4
HARD = 1  # the instance whose full step is rejected in iteration 1 of the second control step of `_hard_case`


def _w_u(full):
    rb = O.Robot("go2_like")
    w = np.array(O.go2_kino_settings(rb)["w_u"], float)
    if not full:
        return w
    rng = np.random.default_rng(5)
    d = np.sqrt(np.abs(np.diag(w)))
    m = rng.standard_normal(w.shape)
    w = w + 0.05 * np.outer(d, d) * (m + m.T) / 2
    assert np.linalg.eigvalsh(w).min() > 0.0 and np.count_nonzero(w[:, UC:]) == w[:, UC:].size
    return w


def _states(rb):
    """Ordinary samples; instance 0 starts beyond the upper limit of one joint (its box row is active)."""
    X = S.random_states(rb, B)
    X[0, 7 + LIMIT_JOINT] = rb.q_hi[LIMIT_JOINT] + 0.05
    return X


def _step(om, gm, g1, X):
    """One control step of oracle and product.  The twin g1 (one iteration per step) first resumes from the product's state and runs the same
    step: what its line search leaves is what iteration 1 of the product leaves -- alpha of iteration 1, and the regularisation the knots of
    the product's last derivative pass are made with.  Returns (alpha of iteration 1, that regularisation)."""
    g1.load_state(gm.save_state())
    g1.iterate(X)
    i1 = g1.info
    om.iterate(X)
    gm.iterate(X)
    return i1[:, 2].copy(), i1[:, 7].copy()


def _pair(lib, full, iters):
    return S.make_pair(B, max_iters=iters, lib=lib, horizon=H, settings_override=dict(w_u=_w_u(full), kinematics_limits=True))


_cache = {}


def _case(lib, full):
    """(oracle, product, robot, X, preg of the last derivation, alpha of iteration 1) after one control step of two iterations; shared by the
    tests of a tier and never changed by them."""
    key = (lib is None, full)
    if key not in _cache:
        om, gm, rb = _pair(lib, full, 2)
        om.keep_knots()
        _, g1, _ = _pair(lib, full, 1)
        X = _states(rb)
        alpha1, preg = _step(om, gm, g1, X)
        _cache[key] = (om, gm, rb, X, preg, alpha1)
    return _cache[key]


def _diag_is_weight_plus_preg(gm, w, preg):
    for b in range(B):
        for t in range(H):
            assert np.array_equal(np.diag(gm.debug_lq(b, t)["R"])[UC:], np.diag(w)[UC:] + preg[b]), (b, t, preg[b])


def getter_contents(lib, full):
    om, gm, rb, X, preg, alpha1 = _case(lib, full)
    w = _w_u(full)
    off = ~np.eye(NA, dtype=bool)
    nact = 0
    for b in range(B):
        for t in range(H):
            kg = gm.debug_lq(b, t)
            assert np.all(kg["S"][:, UC:] == 0.0), (b, t)
            assert np.array_equal(kg["R"][UC:, UC:][off], w[UC:, UC:][off]), (b, t)
            assert np.array_equal(kg["R"][:UC, UC:], w[:UC, UC:]) and np.array_equal(kg["R"][UC:, :UC], w[UC:, :UC]), (b, t)
            assert np.array_equal(np.diag(kg["R"])[UC:], np.diag(w)[UC:] + preg[b]), (b, t, preg[b])
            box = kg["C"][:NA]
            sel = np.diag(box[:, 6:6 + NA]).copy()
            assert np.all((sel == 0.0) | (sel == 1.0)), (b, t)
            assert np.array_equal(box, np.pad(np.diag(sel), ((0, 0), (6, box.shape[1] - 6 - NA)))), (b, t)
            ko = om.knot(b, t)
            assert np.array_equal(sel, np.diag(ko["C"][:NA, 6:6 + NA])), (b, t, "active box rows differ from the oracle's")
            nact += int(sel.sum())
            for k in ("A", "B", "Q", "S", "R", "C", "f", "d"):
                assert S.rel_err(ko[k], kg[k]) < 1e-8, (b, t, k)
            for k in ("q", "r"):
                assert S.rel_err(ko[k], kg[k]) < 1e-6, (b, t, k)
    assert gm.debug_lq(0, 1)["C"][LIMIT_JOINT, 6 + LIMIT_JOINT] == 1.0, "the instance at its joint limit must hold an active box row"
    assert nact >= 1


def preg_timing(lib, full, tol_x, tol_u, tol_k):
    """Two control steps from measured states far from the plan (8 sigma): in iteration 1 of the second one instance HARD rejects the full
    step, its neighbours accept it.  Its regularisation is put back, the line search backtracks, its knots are derived again -- the sweep of
    iteration 2 must see the diagonal of that derivation, whatever the scalar holds by then.
    (By the solver's rule every line search that finds a step divides the regularisation by 3, the rejected instance's as its neighbours':
    after this scenario all three hold the same value -- printed.  Only a line search that fails on all ten candidates multiplies it by 10.)"""
    om, gm, rb = _pair(lib, full, 2)
    _, g1, _ = _pair(lib, full, 1)
    w = _w_u(full)
    for seed in (0, 1):
        X = S.random_states(rb, B, seed=seed, scale=8.0)
        alpha1, preg = _step(om, gm, g1, X)
        print("alpha of iteration 1:", alpha1, " of iteration 2:", gm.info[:, 2], " preg of the last derivation:", preg, " after the step:", gm.info[:, 7])
        _diag_is_weight_plus_preg(gm, w, preg)
        assert S.rel_err(om.xs, gm.xs) < tol_x and S.rel_err(om.us, gm.us) < tol_u and S.rel_err(om.K0, gm.K0) < tol_k, seed
        assert S.alphas_agree(om, gm), (om.info[:, 2], gm.info[:, 2])
    keep = [i for i in range(B) if i != HARD]
    assert alpha1[HARD] < 1.0 and np.all(alpha1[keep] == 1.0), ("instance %d alone must reject the full step of iteration 1" % HARD, alpha1)


def own_knot_sweep(lib, full):
    om, gm, rb, X, preg, alpha1 = _case(lib, full)
    dxs, dus = gm.debug_steps()
    Ks = gm.Ks
    # the floor of a scenario is the largest stage of its largest instance (sweep_check.floors), the gains at every stage
    floor = SC.floors(gm, k_stages=list(range(H)))
    gates = [1e-11 if f < 1e-12 else 10.0 * f for f in floor]
    for b in range(B):
        rx, ru, _, _, rK = O.riccati(*SC.lq_inputs(gm, b))
        gaps = [SC.stage_gaps(dxs[b], rx).max(), SC.stage_gaps(dus[b], ru).max(), SC.stage_gaps(Ks[b], rK).max()]
        print("own-knot sweep check, instance %d: dxs dus Ks %.2e %.2e %.2e | gates %.1e %.1e %.1e" % (b, *gaps, *gates))
        for name, gap, lim in zip(("dxs", "dus", "Ks"), gaps, gates):
            assert gap < lim, (b, name, gap, lim)


def structured_vs_dense(lib, dense_lib, full, tol_x, tol_k):
    """The same control step with the model-independent dense sweep (SMPC_RICCATI=dense of the cross-check build, read when the handle is
    created): every reader of the dense path goes through the accessors of the knot."""
    om, gm, rb, X, preg, alpha1 = _case(lib, full)
    old = os.environ.get("SMPC_RICCATI")
    os.environ["SMPC_RICCATI"] = "dense"
    try:
        _, gd, _ = _pair(dense_lib, full, 2)
    finally:
        if old is None:
            del os.environ["SMPC_RICCATI"]
        else:
            os.environ["SMPC_RICCATI"] = old
    gd.iterate(X)
    assert not (np.array_equal(gd.xs, gm.xs) and np.array_equal(gd.K0, gm.K0)), "SMPC_RICCATI=dense did not select the dense sweep"
    assert S.rel_err(gd.xs, gm.xs) < tol_x and S.rel_err(gd.K0, gm.K0) < tol_k


def checkpoint_and_reset(lib, full):
    def fresh():
        g, rb, _, _ = S.make_product(B, 2, lib=lib, horizon=H, settings_override=dict(w_u=_w_u(full)))
        g.generateCycleHorizon(O.trot_cycle())
        g.switchToWalk(np.array([0.2, 0, 0, 0, 0, 0.0]))
        return g, rb

    ref, rb = fresh()
    X = [_states(rb)] + [S.random_states(rb, B, seed=s) for s in (11, 12)]
    out = []
    for x in X:
        ref.iterate(x)
        out.append((ref.xs.copy(), ref.us.copy(), ref.K0.copy()))

    def same(g, k, rows=slice(None)):
        return all(np.array_equal(a[rows], b_[rows]) for a, b_ in zip((g.xs, g.us, g.K0), out[k]))

    # checkpoint after a step, roll the same handle back after another one ; a handle that never iterated resumes from the checkpoint
    a, _ = fresh()
    a.iterate(X[0])
    blob = a.save_state()
    a.iterate(X[1])
    a.load_state(blob)
    a.iterate(X[1])
    assert same(a, 1)
    c, _ = fresh()
    c.load_state(blob)
    c.iterate(X[1])
    assert same(c, 1)
    c.iterate(X[2])
    assert same(c, 2)
    # reset of one instance: the others continue as on a handle that was never reset ; the reset one as on a handle reset as a whole
    a.resetInstances([HARD])
    a.iterate(X[2])
    keep = [i for i in range(B) if i != HARD]
    assert same(a, 2, keep)
    d, _ = fresh()
    d.iterate(X[0])
    d.iterate(X[1])
    d.resetInstances(list(range(B)))
    d.iterate(X[2])
    assert all(np.array_equal(p[HARD], q[HARD]) for p, q in zip((a.xs, a.us, a.K0), (d.xs, d.us, d.K0)))
    kg = a.debug_lq(HARD, 1)
    assert np.all(kg["S"][:, UC:] == 0.0) and np.all(np.isfinite(kg["R"]))


VARIANTS = pytest.mark.parametrize("full", [False, True], ids=["diag_w_u", "full_w_u"])


@VARIANTS
def test_emulated_getter_contents(built, full):
    getter_contents(S.emu_lib(), full)


@VARIANTS
def test_emulated_preg_timing(built, full):
    preg_timing(S.emu_lib(), full, 1e-7, 1e-7, 1e-6)


@VARIANTS
def test_emulated_own_knot_sweep(built, full):
    own_knot_sweep(S.emu_lib(), full)
    structured_vs_dense(S.emu_lib(), S.emu_lib(), full, 1e-7, 1e-6)


@VARIANTS
def test_emulated_checkpoint_and_reset(built, full):
    checkpoint_and_reset(S.emu_lib(), full)


@pytest.mark.gpu
@VARIANTS
def test_hip_getter_contents(built, full):
    getter_contents(None, full)


@pytest.mark.gpu
@VARIANTS
def test_hip_preg_timing(built, full):
    preg_timing(None, full, 1e-4, 1e-3, 1e-4)


@pytest.mark.gpu
@VARIANTS
def test_hip_own_knot_sweep(built, full):
    own_knot_sweep(None, full)
    structured_vs_dense(None, S.xcheck_lib(), full, 1e-7, 1e-6)


@pytest.mark.gpu
@VARIANTS
def test_hip_checkpoint_and_reset(built, full):
    checkpoint_and_reset(None, full)
