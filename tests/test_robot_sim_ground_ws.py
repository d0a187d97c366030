"""The warm-started ground contact solve with a stopping rule (simple_mpc.BatchedRobotSim.setGroundSolver / resetGroundWarmStart /
lastGroundSweeps / lastGroundResiduals / groundSolveDynamics, simple-mpc_amd/csrc/smpc_sim_ground_ws_rt.h: sim_ground_ws_rt_body<12> and
<24>) against the numpy checker tests/ground_ws_ref.py (the written model of DESIGN 3.25 on top of tests/ground_env_ref.py), against the
kernels of the fixed-sweep ground bit for bit, and against itself across resets and batch sizes.

CPU tier: the kernel body compiled with the sequential-lane test backend (tests/emu); tests/test_robot_sim_ground_ws_gpu.py runs the same
cases on the HIP library.  Bars: 1e-9 relative with max(1, |.|_inf) as the scale on v+, a, lambda (world and contact frame) and the gaps of
one solve; sweeps_used equal exactly (the inputs are chosen on the checker so that no rho lies within 1e-3 relative of tol); the residual
within 1e-9 max(1, |lambda|_inf) max_r dt G_rr absolute (it is a difference of nearly equal numbers); 1e-8 relative on the state for 40
steps (that of the 20-step test of DESIGN 3.23); np.array_equal where the model promises equal bits."""
import ctypes as C

import numpy as np
import pytest

import ground_env_ref as ER
import ground_ws_ref as WR
import mpc_setup as S
import robot_tables as RT
import simple_mpc
import test_id_any_robot as T
import test_robot_sim_any_robot as SIM
import test_robot_sim_ground as G
import test_robot_sim_ground_env as E
from simple_mpc._capi import GroundSolverSettingsC

HostArray = SIM.HostArray
_INVALID = -1  # SMPC_ERR_INVALID (include/smpc.h)
DT = G.DT
MU = G.MU
OUT = ("v_next", "a", "lam", "gap", "contact")
# (robot, points per foot, seed): the built shape (the 12-row instantiation); 32 joints (the bound of every array); soles of four corners (8
# points: the 24-row instantiation).  The seeds are chosen on the checker alone, so that the conditions of parity() hold.
CASES = [("go2_like", 1, 0), ("tree32p", 1, 0), ("biped_legs", 4, 0)]
TOL, MIN_SWEEPS, SWEEPS = 1e-6, 2, 60


def flat_plane(gz):
    return np.array([0.0, 0.0, 1.0, gz])


# ---------------------------------------------------------------------------------------------------------------------- 1
def inert_settings(name, P, seed, lib, alloc, steps=20):
    """Case 1: with warm_start = 0 and tol = 0 the new kernel gives the bits of the existing ones: one solve on 24 states with their own
    environment, then 20 steps on a handle with the inert settings against a handle without them, with and without an environment."""
    tab, rb, sim, gz = G.make(name, P, lib, 3)
    X, tau = G.ground_states(name, 24, seed)
    planes, mu, push = E.environment(name, X, seed)
    j = E.push_joint(tab, "foot")
    env = sim.groundEnvDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j)
    ws = sim.groundSolveDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, lam0=None, warm_start=False, tol=0.0)
    for k in OUT:
        assert np.array_equal(env[k], ws[k]), k
    assert env["contact"].any() and (ws["sweeps"] == 30).all() and ws["sweeps"].dtype == np.int32
    B = 3
    X0, tq = G.drop_states(rb, B, 71)
    for with_env in (False, True):
        pair = []
        for solver in (True, False):
            _, _, h, _ = G.make(name, P, lib, B)
            if with_env:
                h.setGroundEnv(planes=planes[:B], mu=mu[:B])
                h.setPush(push[:B], joint=j)
            if solver:
                h.setGroundSolver(warm_start=False, tol=0.0, min_sweeps=0)
            pair.append(h)
        new, old = pair
        Xn, Xo, td = alloc(X0), alloc(X0), alloc(tq)
        landed = np.zeros(B, np.uint32)
        for k in range(steps):
            new.stepGroundDevice(Xn.ptr, td.ptr, DT)
            old.stepGroundDevice(Xo.ptr, td.ptr, DT)
            new.wait()
            old.wait()
            assert np.array_equal(Xn.get(), Xo.get()), (with_env, k)
            assert np.array_equal(new.lastGroundForces(), old.lastGroundForces()) and np.array_equal(new.lastContacts(), old.lastContacts()), (with_env, k)
            assert np.array_equal(new.lastAccelerations(), old.lastAccelerations()), (with_env, k)
            assert (new.lastGroundSweeps() == 30).all()
            landed |= new.lastContacts()
        assert (landed != 0).all() and np.abs(Xn.get() - X0).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------------- 2
_cache = {}


def parity_inputs(name, P, seed, n=24):
    """States, torques, environment, start vectors and the checker's answers of one case: computed once, shared by both tiers, never
    modified.  lam0 by i % 3: zeros; the checker's cold 30-sweep lambda scaled entrywise by 1 + 0.05 N(0, 1); N(0, 20^2)."""
    key = ("parity", name, P, seed, n)
    if key not in _cache:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        X, tau = G.ground_states(name, n, seed)
        planes, mu, push = E.environment(name, X, seed)
        j = E.push_joint(tab, "foot")
        rng = np.random.default_rng(2000 + seed)
        nr = 3 * P * tab.nfeet
        lam0 = np.zeros((n, nr))
        for i in range(n):
            if i % 3 == 1:
                cold = ER.solve(rb, tab, X[i], tau[i], DT, planes[i], mu[i], push[i], j, points=G.points(P))["lam_c"]
                lam0[i] = cold * (1.0 + 0.05 * rng.normal(size=nr))
            elif i % 3 == 2:
                lam0[i] = rng.normal(size=nr) * 20.0
        ref = [WR.solve(rb, tab, X[i], tau[i], DT, planes[i], mu[i], push[i], j, points=G.points(P), sweeps=SWEEPS, lam0=lam0[i], tol=TOL, min_sweeps=MIN_SWEEPS)
               for i in range(n)]
        _cache[key] = (X, tau, planes, mu, push, j, lam0, ref)
    return _cache[key]


def parity(name, P, seed, lib):
    """Case 2: groundSolveDynamics with tol = 1e-6, min_sweeps = 2, sweeps = 60 on 24 states against the checker."""
    X, tau, planes, mu, push, j, lam0, ref = parity_inputs(name, P, seed)
    used = np.array([r["sweeps"] for r in ref])
    print("%s P %d: checker: sweeps used %s" % (name, P, used.tolist()))
    # conditions on the inputs, on the checker alone
    assert all(WR.decided(r["rhos"], TOL, MIN_SWEEPS) for r in ref)
    assert (used < SWEEPS).sum() >= 3, used
    # (point feet converge: over seeds 0 .. 7 of the generator no solve of go2_like or tree32p needs more than 18 sweeps at this tol, from any
    # of the three start vectors, so "at least 3 solves run all 60 sweeps" can be asked of the four-corner soles only; sweep_bound() below
    # takes every case through "tol > 0 and the bound reached" on a ground of 5 sweeps)
    assert P == 1 or (used == SWEEPS).sum() >= 3, used
    assert used.max() > MIN_SWEEPS and len(set(used.tolist())) >= 4, used
    assert (lam0[2::3][:, 2::3] < 0.0).any()
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    out = sim.groundSolveDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, lam0=lam0, tol=TOL, min_sweeps=MIN_SWEEPS)
    worst = dict(v_next=0.0, a=0.0, lam=0.0, lam_contact=0.0, gap=0.0)
    worst_res = 0.0
    for i, r in enumerate(ref):
        for k in worst:
            worst[k] = max(worst[k], G._rel(out[k][i], r["lam_c" if k == "lam_contact" else k]))
        bar = 1e-9 * max(1.0, np.abs(r["lam_c"]).max()) * r["dtG"].max()
        worst_res = max(worst_res, abs(out["residual"][i] - r["residual"]) / bar)
    print("%s P %d: v+ %.2e  a %.2e  lambda %.2e  lambda (contact frame) %.2e  gap %.2e; residual %.2e of its bar; sweeps that differ %d"
          % (name, P, worst["v_next"], worst["a"], worst["lam"], worst["lam_contact"], worst["gap"], worst_res, int((out["sweeps"] != used).sum())))
    assert np.array_equal(out["sweeps"], used)
    assert max(worst.values()) < 1e-9, worst
    assert worst_res <= 1.0, worst_res
    return worst


def sweep_bound(name, P, seed, lib, sweeps=5):
    """Case 2, the path "tol > 0 and the sweep bound reached", which point feet never take at 60 sweeps: the same 24 states, environment and
    start vectors on a ground of 5 sweeps, tol = 1e-6, min_sweeps = 2, against the checker."""
    X, tau, planes, mu, push, j, lam0, _ = parity_inputs(name, P, seed)
    key = ("bound", name, P, seed, sweeps)
    if key not in _cache:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        _cache[key] = [WR.solve(rb, tab, X[i], tau[i], DT, planes[i], mu[i], push[i], j, points=G.points(P), sweeps=sweeps, lam0=lam0[i], tol=TOL,
                                min_sweeps=MIN_SWEEPS) for i in range(len(X))]
    ref = _cache[key]
    used = np.array([r["sweeps"] for r in ref])
    assert all(WR.decided(r["rhos"], TOL, MIN_SWEEPS) for r in ref)
    assert (used == sweeps).sum() >= 3 and (used < sweeps).sum() >= 3, used
    assert sum(r["residual"] > TOL for r in ref) >= 3  # (stopped by the bound, not by the rule)
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=sweeps)
    out = sim.groundSolveDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, lam0=lam0, tol=TOL, min_sweeps=MIN_SWEEPS)
    worst, worst_res = 0.0, 0.0
    for i, r in enumerate(ref):
        for k in ("v_next", "a", "lam", "lam_contact", "gap"):
            worst = max(worst, G._rel(out[k][i], r["lam_c" if k == "lam_contact" else k]))
        worst_res = max(worst_res, abs(out["residual"][i] - r["residual"]) / (1e-9 * max(1.0, np.abs(r["lam_c"]).max()) * r["dtG"].max()))
    print("%s P %d, %d sweeps at most: checker: sweeps used %s; outputs %.2e, residual %.2e of its bar" % (name, P, sweeps, used.tolist(), worst, worst_res))
    assert np.array_equal(out["sweeps"], used)
    assert worst < 1e-9 and worst_res <= 1.0, (worst, worst_res)


# ---------------------------------------------------------------------------------------------------------------------- 3
def non_finite_start(name, P, seed, lib):
    """Case 3: NaN and +-inf in robot 1's lam0 read as zeros, bitwise; robots 0 and 2 are unchanged."""
    X, tau, planes, mu, push, j, _, _ = parity_inputs(name, P, seed)
    rows = [3, 4, 5]  # (states with contact)
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    nr = 3 * P * tab.nfeet
    rng = np.random.default_rng(7)
    lam0 = np.abs(rng.normal(size=(3, nr))) * 10.0
    bad, zeroed = lam0.copy(), lam0.copy()
    for col, v in ((0, np.nan), (2, np.inf), (4, -np.inf), (nr - 1, np.nan)):
        bad[1, col] = v
        zeroed[1, col] = 0.0
    kw = dict(planes=planes[rows], mu=mu[rows], push=push[rows], joint=j, tol=TOL, min_sweeps=MIN_SWEEPS)
    a = sim.groundSolveDynamics(X[rows], tau[rows], DT, lam0=bad, **kw)
    b = sim.groundSolveDynamics(X[rows], tau[rows], DT, lam0=zeroed, **kw)
    c = sim.groundSolveDynamics(X[rows], tau[rows], DT, lam0=lam0, **kw)
    for k in OUT + ("lam_contact", "sweeps", "residual"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][[0, 2]], c[k][[0, 2]]), k
    assert np.isfinite(a["lam"]).all() and a["contact"].any()


# ---------------------------------------------------------------------------------------------------------------------- 4
def fixed_point(lib):
    """Case 4: go2_like at rest on the plane, started from the checker's cold lambda after 2000 sweeps: one sweep, lambda unchanged."""
    name = "go2_like"
    key = ("fixed", name)
    tab = T.table(name)
    rb = RT.oracle_robot(tab)
    gz = G.ground_height(rb)
    x, tau = rb.x_ref.copy(), np.zeros(rb.nv - 6)
    if key not in _cache:
        cold = WR.solve(rb, tab, x, tau, DT, flat_plane(gz), MU, sweeps=2000)
        warm = WR.solve(rb, tab, x, tau, DT, flat_plane(gz), MU, sweeps=SWEEPS, lam0=cold["lam_c"], tol=1e-9, min_sweeps=1)
        _cache[key] = (cold, warm)
    cold, warm = _cache[key]
    print("go2_like at rest: checker: rho after 2000 cold sweeps %.2e; restarted there: sweeps %d, rho %.2e" % (cold["residual"], warm["sweeps"], warm["residual"]))
    assert warm["sweeps"] == 1 and warm["residual"] < 1e-9 * (1 - 1e-3)  # (the checker decides first)
    _, _, sim, _ = G.make(name, 1, lib, 1, sweeps=SWEEPS)
    out = sim.groundSolveDynamics(x[None], tau[None], DT, lam0=cold["lam_c"][None], tol=1e-9, min_sweeps=1)
    print("go2_like at rest: kernel: sweeps %d, rho %.2e, lambda against the start %.2e" % (out["sweeps"][0], out["residual"][0], G._rel(out["lam_contact"][0], cold["lam_c"])))
    assert out["sweeps"][0] == 1 and out["residual"][0] <= 1e-9
    assert G._rel(out["lam_contact"][0], cold["lam_c"]) < 1e-9 and (out["lam_contact"][0, 2::3] > 1.0).all()


# ---------------------------------------------------------------------------------------------------------------------- 5
STARTS = ("rest", "drop")


def start_state(rb, start):
    """The reference state at rest on the plane, or 1 cm above it at -0.3 m/s."""
    x = rb.x_ref.copy()
    if start == "drop":
        x[2] += 0.01
        x[rb.nq : rb.nq + 3] = G.GR._quat_to_R(x[3:7]).T @ np.array([0.0, 0.0, -0.3])
    return x


def host_loop(name, P, start, warm_start, tol, sweeps, steps=40):
    """The checker's loop on the host: states, sweeps per step, whether each step's count is decided, normal-velocity infeasibility per step.
    Computed once, shared by both tiers."""
    key = ("loop", name, P, start, warm_start, tol, sweeps, steps)
    if key not in _cache:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        gz = G.ground_height(rb)
        x, tau = start_state(rb, start), np.zeros(rb.nv - 6)
        w = np.zeros(3 * P * tab.nfeet)
        used, decided, infeas, rs = [], [], [], []
        for _ in range(steps):
            x, w, r = WR.step(rb, tab, x, tau, DT, flat_plane(gz), MU, w, warm_start, points=G.points(P), sweeps=sweeps, tol=tol, min_sweeps=1)
            used.append(r["sweeps"])
            decided.append(tol == 0.0 or WR.decided(r["rhos"], tol, 1))
            infeas.append(G._residuals(r["J"], r["gapterm"], r["v_next"], r["lam_c"])[0])
            rs.append(dict(J=r["J"], gapterm=r["gapterm"]))
        _cache[key] = (x, np.array(used), np.array(decided), np.array(infeas), rs)
    return _cache[key]


def device_loop(name, P, start, lib, alloc, warm_start, tol, sweeps, steps=40, B=3):
    tab, rb, sim, gz = G.make(name, P, lib, B, sweeps=sweeps)
    sim.setGroundSolver(warm_start=warm_start, tol=tol, min_sweeps=1)
    Xd, td = alloc(np.tile(start_state(rb, start), (B, 1))), alloc(np.zeros((B, rb.nv - 6)))
    used, V, lam = [], [], []
    for _ in range(steps):
        sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
        sim.wait()
        sw = sim.lastGroundSweeps()
        assert (sw == sw[0]).all()  # (replicas)
        used.append(int(sw[0]))
        V.append(Xd.get()[0, rb.nq :])
        lam.append(sim.lastGroundForces()[0])
    X = Xd.get()
    assert np.array_equal(X[0], X[1]) and np.array_equal(X[0], X[2])
    return X[0], np.array(used), V, lam


def warm_across_steps(name, P, start, lib, alloc):
    """Case 5 (a): 40 warm-started steps with tol = 1e-6, sweeps = 400 against the checker's host loop; fewer sweeps than the cold start."""
    xh, used_h, decided, _, _ = host_loop(name, P, start, True, 1e-6, 400)
    assert (~decided).sum() <= 2, decided
    x, used, _, _ = device_loop(name, P, start, lib, alloc, True, 1e-6, 400)
    _, cold, _, _ = device_loop(name, P, start, lib, alloc, False, 1e-6, 400)
    err = S.rel_err(xh[None], x[None])
    print("%s P %d %s: 40 steps vs the host loop %.2e; sweeps warm %d (checker %d), cold %d; steps left out %d"
          % (name, P, start, err, used.sum(), used_h.sum(), cold.sum(), (~decided).sum()))
    assert err < 1e-8, err
    assert np.array_equal(used[decided], used_h[decided]), (used, used_h)
    assert used.sum() < cold.sum()
    if name == "biped_legs" and start == "rest":
        assert 2 * used.sum() <= cold.sum(), (used.sum(), cold.sum())


def warm_fixed_sweeps(lib, alloc):
    """Case 5 (b): biped_legs at rest, 30 fixed sweeps: the warm start leaves at most a tenth of the cold start's normal-velocity
    infeasibility over steps 10 .. 39 on the checker, and the kernel stays within 10 x the checker's value (the gate of DESIGN 3.23)."""
    name, P = "biped_legs", 4
    _, _, _, cold_h, _ = host_loop(name, P, "rest", False, 0.0, 30)
    _, used_h, _, warm_h, rs = host_loop(name, P, "rest", True, 0.0, 30)
    ref_cold, ref_warm = cold_h[10:].max(), warm_h[10:].max()
    _, used, V, lam = device_loop(name, P, "rest", lib, alloc, True, 0.0, 30)
    got = max(G._residuals(rs[k]["J"], rs[k]["gapterm"], V[k], lam[k])[0] for k in range(10, 40))
    print("biped_legs P 4 at rest, 30 sweeps: infeasibility from step 10 on: checker cold %.2e, warm %.2e; kernel warm %.2e" % (ref_cold, ref_warm, got))
    assert (used == 30).all() and (used_h == 30).all()
    assert ref_warm <= 0.1 * ref_cold
    assert got <= 10.0 * ref_warm


# ---------------------------------------------------------------------------------------------------------------------- 6
def _warm_handle(name, P, lib, alloc, X0, tq, steps):
    tab, rb, sim, gz = G.make(name, P, lib, len(X0), sweeps=SWEEPS)
    sim.setGroundSolver(warm_start=True, tol=TOL, min_sweeps=1)
    Xd, td = alloc(X0), alloc(tq)
    for _ in range(steps):
        sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
    sim.wait()
    return sim, Xd, td, gz


def _one_step(sim, X, td, alloc):
    Xd = alloc(X)
    sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
    sim.wait()
    return dict(X=Xd.get(), lam=sim.lastGroundForces(), a=sim.lastAccelerations(), sweeps=sim.lastGroundSweeps(), con=sim.lastContacts())


def resets(name, P, lib, alloc):
    """Case 6: resetGroundWarmStart (host list and device mask), setGround and setGroundSolver called again, and a NaN state that heals."""
    tab = T.table(name)
    rb = RT.oracle_robot(tab)
    X0, tq = G.drop_states(rb, 3, 71)

    def warmed():
        sim, Xd, td, gz = _warm_handle(name, P, lib, alloc, X0, tq, 10)
        return sim, Xd.get(), td, gz

    keep, X10, td, gz = warmed()
    plain = _one_step(keep, X10, td, alloc)  # the eleventh step without any reset
    cold_handle, _, _, _ = _warm_handle(name, P, lib, alloc, X0, tq, 0)
    cold = _one_step(cold_handle, X10, td, alloc)  # the same states on a zero warm buffer
    assert plain["con"].all() and not np.array_equal(plain["lam"][1], cold["lam"][1])  # (the warm start matters at these states)
    assert plain["sweeps"].sum() < cold["sweeps"].sum()
    F = ("lam", "a", "sweeps", "X")
    for how in ("list", "mask"):
        sim, X, td, _ = warmed()
        assert np.array_equal(X, X10)
        if how == "list":
            sim.resetGroundWarmStart([1])
        else:
            m = alloc(np.array([0, 1, 0], np.uint8))
            sim.resetGroundWarmStartDevice(m.ptr)
        got = _one_step(sim, X, td, alloc)
        for k in F:
            assert np.array_equal(got[k][1], cold[k][1]), (how, k)
            assert np.array_equal(got[k][[0, 2]], plain[k][[0, 2]]), (how, k)
    # every robot: n = 0
    sim, X, td, _ = warmed()
    sim.resetGroundWarmStart()
    got = _one_step(sim, X, td, alloc)
    for k in F:
        assert np.array_equal(got[k], cold[k]), k
    # setGroundSolver again zeroes the buffer
    sim, X, td, _ = warmed()
    sim.setGroundSolver(warm_start=True, tol=TOL, min_sweeps=1)
    assert (sim.lastGroundSweeps() == 0).all()
    got = _one_step(sim, X, td, alloc)
    for k in F:
        assert np.array_equal(got[k], cold[k]), k
    # setGround again drops the solver settings: the next step is a fresh handle's (30 fixed sweeps from zero on sim_ground_rt_body)
    sim, X, td, gz = warmed()
    sim.setGround(ground_z=gz, points=G.points(P))
    _, _, fresh, _ = G.make(name, P, lib, 3)
    got, want = _one_step(sim, X, td, alloc), _one_step(fresh, X, td, alloc)
    for k in ("lam", "a", "X", "con"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["sweeps"] == 0).all()  # (the read-outs belong to the solver settings, which are gone)
    # a NaN state in robot 1 for one step, then the finite state written back: a cold start without any reset call
    sim, X, td, _ = warmed()
    Xn = X.copy()
    Xn[1, 9] = np.nan
    spoiled = _one_step(sim, Xn, td, alloc)
    assert not np.isfinite(spoiled["X"][1]).all() and np.isfinite(spoiled["X"][[0, 2]]).all()
    healed = _one_step(sim, X, td, alloc)
    assert np.isfinite(healed["X"]).all()
    for k in F:
        assert np.array_equal(healed[k][1], cold[k][1]), k


# ---------------------------------------------------------------------------------------------------------------------- 7
def batch_hygiene(name, P, lib, alloc, steps=5):
    """Case 7: B = 65 against handles of B = 64 and B = 1, bitwise, over 5 warm steps from states whose sweep counts differ between
    neighbouring robots."""
    X, tau = G.ground_states(name, 65, 81)
    out = []
    for B, rows in ((65, slice(0, 65)), (64, slice(0, 64)), (1, slice(64, 65))):
        sim, Xd, td, _ = _warm_handle(name, P, lib, alloc, X[rows], tau[rows], 0)
        sw, res = [], []
        for _ in range(steps):
            sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
            sw.append(sim.lastGroundSweeps())  # (joins the stream)
            res.append(sim.lastGroundResiduals())
        out.append((Xd.get(), sim.lastAccelerations(), sim.lastGroundForces(), sim.lastContacts(), np.array(sw).T, np.array(res).T))
    for a, b, c in zip(*out):
        assert np.array_equal(a[:64], b) and np.array_equal(a[64:], c)
    sw = out[0][4].T  # [step][robot]
    differ = (np.diff(sw, axis=1) != 0).sum(axis=1)
    print("%s P %d: neighbouring robots whose sweeps differ, per step: %s; sweeps at the first step %s" % (name, P, differ.tolist(), sw[0].tolist()))
    assert np.isfinite(out[0][0]).all() and differ[0] >= 16 and differ.min() >= 6 and len(set(sw[0].tolist())) >= 4


# ---------------------------------------------------------------------------------------------------------------------- 8
def admission(lib, alloc):
    """Case 8: refusals through the C ABI, each with the field named and the previous settings left in force."""
    lib = lib or simple_mpc.default_lib()
    L = lib.L
    name, B = "go2_like", 3
    tab, rb, sim = SIM.make(name, 3, lib, B)
    X, tau = G.ground_states(name, B, 5)
    X[:, 2] -= 0.005  # (the feet touch)

    def err():
        return L.smpc_last_error().decode()

    def settings(w, tol, m):
        s = GroundSolverSettingsC()
        s.warm_start, s.tol, s.min_sweeps = w, tol, m
        return s

    def set_solver(w, tol, m):
        return L.smpc_robot_sim_set_ground_solver(sim._h, C.byref(settings(w, tol, m)))

    def ints(*v):
        return np.array(v, np.int32).ctypes.data_as(C.c_void_p)

    sw, res, p3 = np.zeros(B, np.int32), np.zeros(B), [C.c_void_p() for _ in range(3)]
    mask = alloc(np.zeros(B, np.uint8))
    # every entry before setGround
    before_ground = [
        lambda: set_solver(1, 1e-6, 0),
        lambda: L.smpc_robot_sim_reset_ground_warm_start(sim._h, None, 0),
        lambda: L.smpc_robot_sim_reset_ground_warm_start_device(sim._h, C.c_void_p(mask.ptr)),
        lambda: L.smpc_robot_sim_get_ground_solver_last(sim._h, C.byref(p3[0]), C.byref(p3[1]), C.byref(p3[2])),
        lambda: L.smpc_robot_sim_read_ground_solver_last(sim._h, sw.ctypes.data, res.ctypes.data),
    ]
    for call in before_ground:
        assert call() == _INVALID and "smpc_robot_sim_set_ground first" in err(), err()
    with pytest.raises(RuntimeError, match="set_ground"):
        sim.groundSolveDynamics(X, tau, DT)
    sim.setGround(ground_z=G.ground_height(rb), sweeps=40)
    # before the setter the read-outs answer without a warm buffer: null pointers, zeros, resets that succeed
    assert sim.groundSolverDevicePointers() == (0, 0, 0)
    assert (sim.lastGroundSweeps() == 0).all() and (sim.lastGroundResiduals() == 0.0).all()
    sim.resetGroundWarmStart([1])
    sim.resetGroundWarmStartDevice(mask.ptr)
    assert sim.groundSolverDevicePointers() == (0, 0, 0)
    sim.setGroundSolver(warm_start=True, tol=1e-6, min_sweeps=3)
    td = alloc(tau)
    for _ in range(3):  # (a warm buffer in force: refused calls must leave it as it is)
        Xd = alloc(X)
        sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
    sim.wait()
    ptrs = sim.groundSolverDevicePointers()
    assert all(ptrs)

    def one_step(h):
        Xd = alloc(X)
        h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        return Xd.get(), h.lastGroundForces(), h.lastGroundSweeps(), h.lastGroundResiduals()

    nan, inf = float("nan"), float("inf")
    refusals = [
        (lambda: set_solver(1, -1e-6, 0), ("tol = -1e-06", "negative")),
        (lambda: set_solver(1, nan, 0), ("tol", "finite")),
        (lambda: set_solver(0, inf, 0), ("tol", "finite")),
        (lambda: set_solver(1, 1e-6, -1), ("min_sweeps = -1",)),
        (lambda: set_solver(1, 1e-6, 41), ("min_sweeps = 41", "sweeps = 40")),
        (lambda: set_solver(2, 1e-6, 0), ("warm_start = 2",)),
        (lambda: L.smpc_robot_sim_reset_ground_warm_start(sim._h, ints(0, B, 1), 3), ("indices[1] = %d" % B,)),
        (lambda: L.smpc_robot_sim_reset_ground_warm_start(sim._h, ints(-1), 1), ("indices[0] = -1",)),
        (lambda: L.smpc_robot_sim_reset_ground_warm_start(sim._h, ints(0), -1), ("n = -1",)),
        (lambda: L.smpc_robot_sim_reset_ground_warm_start_device(sim._h, None), ("null argument",)),
        (lambda: L.smpc_robot_sim_ground_solve_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, C.byref(settings(0, -1.0, 0)), None, None, None, None, None, None,
                                                        None, None, None), ("tol = -1", "negative")),
        (lambda: L.smpc_robot_sim_ground_solve_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, C.byref(settings(0, 0.0, 41)), None, None, None, None, None, None,
                                                        None, None, None), ("min_sweeps = 41",)),
    ]
    # the reference: a twin handle brought to the same point that meets no refusal; after each refusal both take one step (a step moves
    # the warm buffer on, so "the same bits as before" are the twin's)
    _, _, twin = SIM.make(name, 3, lib, B)
    twin.setGround(ground_z=G.ground_height(rb), sweeps=40)
    twin.setGroundSolver(warm_start=True, tol=1e-6, min_sweeps=3)
    for _ in range(3):
        Xt = alloc(X)
        twin.stepGroundDevice(Xt.ptr, td.ptr, DT)
    twin.wait()
    for call, words in refusals:
        assert call() == _INVALID, words
        assert all(w in err() for w in words), (words, err())
        assert sim.groundSolverDevicePointers() == ptrs
        got, want = one_step(sim), one_step(twin)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), words
        assert (got[2] >= 3).all() and (got[2] < 40).any() and got[1].any()
    # the mirrors refuse shapes themselves; every output of the host-buffer solve may be NULL; min_sweeps = sweeps is admitted
    with pytest.raises(RuntimeError, match="lam0 \\[n, 3 points\\]"):
        sim.groundSolveDynamics(X, tau, DT, lam0=np.zeros((B, 5)))
    assert L.smpc_robot_sim_ground_solve_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, None, None, None, None, None, None, None, None, None, None) == 0
    assert set_solver(0, 0.0, 40) == 0, err()
    assert L.smpc_robot_sim_reset_ground_warm_start(sim._h, ints(2, 0, 2), 3) == 0, err()
    sim.wait()


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("name,P,seed", CASES)
def test_inert_settings_bit_for_bit(built, name, P, seed):
    inert_settings(name, P, seed, S.emu_lib(), HostArray)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_parity_with_the_checker(built, name, P, seed):
    parity(name, P, seed, S.emu_lib())


@pytest.mark.parametrize("name,P,seed", CASES)
def test_parity_when_the_sweep_bound_is_reached(built, name, P, seed):
    sweep_bound(name, P, seed, S.emu_lib())


@pytest.mark.parametrize("name,P,seed", CASES)
def test_non_finite_start_entries(built, name, P, seed):
    non_finite_start(name, P, seed, S.emu_lib())


def test_fixed_point(built):
    fixed_point(S.emu_lib())


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name,P", [("biped_legs", 4), ("go2_like", 1)])
def test_warm_start_across_steps(built, name, P, start):
    warm_across_steps(name, P, start, S.emu_lib(), HostArray)


def test_warm_start_at_fixed_sweeps(built):
    warm_fixed_sweeps(S.emu_lib(), HostArray)


@pytest.mark.parametrize("name,P", [("go2_like", 1), ("biped_legs", 4)])
def test_resets(built, name, P):
    resets(name, P, S.emu_lib(), HostArray)


@pytest.mark.parametrize("name,P", [("go2_like", 1), ("biped_legs", 4)])
def test_batch_hygiene(built, name, P):
    batch_hygiene(name, P, S.emu_lib(), HostArray)


def test_admission_and_errors(built):
    admission(S.emu_lib(), HostArray)
