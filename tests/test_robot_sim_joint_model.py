"""The simulator's joint model: effort limits, implicit joint damping, armature and joint-limit stops (simple_mpc.BatchedRobotSim.setJointModel
/ lastJointStops / lastAppliedTorques / jointModelDevicePointers / groundJointDynamics, simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h:
sim_ground_joint_rt_body<24> and <32>) against the numpy checker tests/ground_joint_ref.py (the written model of DESIGN 3.26 on top of
tests/ground_ws_ref.py), against the kernels without a joint model bit for bit, and against itself across batch sizes.

CPU tier: the kernel body compiled with the sequential-lane test backend (tests/emu); tests/test_robot_sim_joint_model_gpu.py runs the same
cases on the HIP library.  Bars (those of DESIGN 3.25): 1e-9 relative with max(1, |.|_inf) as the scale on v+, a, lambda (world and contact
frame) and lam_stop of one solve; the residual within 1e-9 max(1, |lambda|_inf) max_r dt G_rr absolute; tau_applied, stop_rows, dropped and
sweeps_used equal exactly (the inputs are chosen on the checker so that no decision is marginal); 1e-8 relative on the state after a loop
of steps; np.array_equal where the model promises equal bits."""
import ctypes as C

import numpy as np
import pytest

import ground_joint_ref as JR
import ground_ws_ref as WR
import mpc_setup as S
import robot_tables as RT
import simple_mpc
import test_id_any_robot as T
import test_robot_sim_any_robot as SIM
import test_robot_sim_ground as G
import test_robot_sim_ground_env as E
from simple_mpc._capi import JointModelSettingsC

HostArray = SIM.HostArray
_INVALID = -1  # SMPC_ERR_INVALID (include/smpc.h)
DT = G.DT
MU = G.MU
# (robot, points per foot, seed): 12 joints, one point per foot (<24>); 32 joints (the bound of every array, <24>); soles of four corners
# (24 contact rows: <32>)
CASES = [("go2_like", 1, 0), ("tree32p", 1, 0), ("biped_legs", 4, 0)]
TOL, MIN_SWEEPS, SWEEPS = 1e-6, 2, 60
ROWS_SEED = 3001
SHARED = ("v_next", "a", "lam", "gap", "contact", "lam_contact", "sweeps", "residual")
JOINT = ("tau_applied", "stop_rows", "lam_stop", "dropped")
_cache = {}


def limits(tab, na):
    return np.array(tab.q_lo[:na]), np.array(tab.q_hi[:na])


def parity_inputs(name, P, seed, n=24):
    """States, torques, environment, joint-model rows and the checker's answers of one case: computed once, shared by both tiers, never
    modified.  Every state has its own tau_max (5 .. 40 N m), damping (0 .. 0.5) and armature (0 .. 0.05) rows and its own limits (the
    robot table's, each widened by up to 0.05 rad: no joint sits midway between its limits).  The seed of these rows is chosen on the
    checker alone, so that the conditions of parity() hold.  Edits by i % 4: 0 as drawn; 1 two joints at q_lo - 0.02 and q_hi + 0.03 with
    velocity into the stop; 2 ten joints 0.03 rad inside a limit (two of them faster than 0.03 rad per step into it); 3 torques of
    5 tau_max."""
    key = ("parity", name, P, seed, n)
    if key not in _cache:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        nq, na = rb.nq, rb.nv - 6
        lo, hi = limits(tab, na)
        X, tau = G.ground_states(name, n, seed)
        planes, mu, push = E.environment(name, X, seed)
        j = E.push_joint(tab, "foot")
        rng = np.random.default_rng(ROWS_SEED + seed)
        tmax = rng.uniform(5.0, 40.0, (n, na))
        dmp = rng.uniform(0.0, 0.5, (n, na))
        arm = rng.uniform(0.0, 0.05, (n, na))
        qlo, qhi = lo - rng.uniform(0.0, 0.05, (n, na)), hi + rng.uniform(0.0, 0.05, (n, na))
        for i in range(n):
            lo, hi = qlo[i], qhi[i]
            if i % 4 == 1:
                ka, kb = i % na, (i + 5) % na
                X[i, 7 + ka], X[i, nq + 6 + ka] = lo[ka] - 0.02, -rng.uniform(0.5, 2.0)
                X[i, 7 + kb], X[i, nq + 6 + kb] = hi[kb] + 0.03, rng.uniform(0.5, 2.0)
            elif i % 4 == 2:
                ks = rng.permutation(na)[:10]
                for m, k in enumerate(ks):
                    lower = m % 2 == 0
                    X[i, 7 + k] = lo[k] + 0.03 if lower else hi[k] - 0.03
                    speed = 40.0 if m < 2 else rng.uniform(0.0, 2.0)
                    X[i, nq + 6 + k] = -speed if lower else speed
            elif i % 4 == 3:
                tau[i] = 5.0 * tmax[i] * np.where(rng.uniform(size=na) < 0.5, -1.0, 1.0)
        ref = [JR.solve(rb, tab, X[i], tau[i], DT, planes[i], mu[i], push[i], j, points=G.points(P), sweeps=SWEEPS, tol=TOL, min_sweeps=MIN_SWEEPS,
                        tau_max=tmax[i], damping=dmp[i], armature=arm[i], q_lo=qlo[i], q_hi=qhi[i], stops=1) for i in range(n)]
        _cache[key] = (X, tau, planes, mu, push, j, tmax, dmp, arm, qlo, qhi, ref)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------- 1
def parity(name, P, seed, lib):
    """Case 1: groundJointDynamics with stops on 24 states, each with its own plane, mu, push and joint-model rows, against the checker."""
    X, tau, planes, mu, push, j, tmax, dmp, arm, qlo, qhi, ref = parity_inputs(name, P, seed)
    # conditions on the inputs, on the checker alone
    margins = np.concatenate([r["margins"] for r in ref])
    loaded = [(r["stop_rows"][k], r["stop_gaps"][k]) for r in ref for k in range(JR.NJ) if r["lam_stop"][k] > 0.0]
    both = sum(1 for r in ref if r["contact"] != 0 and (r["lam_stop"] > 0.0).any())
    print("%s P %d: checker: loaded stop rows %d (lower %d, upper %d, penetrating %d); solves with dropped candidates %d; a stop and a foot loaded in %d; "
          "smallest margin %.2e; sweeps %s" % (name, P, len(loaded), sum(s > 0 for s, _ in loaded), sum(s < 0 for s, _ in loaded), sum(g < 0 for _, g in loaded),
                                               sum(r["dropped"] > 0 for r in ref), both, margins.min(), [r["sweeps"] for r in ref]))
    assert margins.min() >= 1e-9
    assert len(loaded) >= 10 and any(s > 0 for s, _ in loaded) and any(s < 0 for s, _ in loaded) and any(g < 0.0 for _, g in loaded)
    assert sum(r["dropped"] > 0 for r in ref) >= 6
    assert both >= 1
    assert all(WR.decided(r["rhos"], TOL, MIN_SWEEPS) for r in ref)
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    out = sim.groundJointDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, tol=TOL, min_sweeps=MIN_SWEEPS, tau_max=tmax, damping=dmp,
                                  armature=arm, q_lo=qlo, q_hi=qhi, stops=True)
    worst = dict(v_next=0.0, a=0.0, lam=0.0, lam_contact=0.0, lam_stop=0.0)
    worst_res = 0.0
    for i, r in enumerate(ref):
        for k in worst:
            worst[k] = max(worst[k], G._rel(out[k][i], r["lam_c" if k == "lam_contact" else k]))
        bar = 1e-9 * max(1.0, np.abs(r["lam_all"]).max()) * r["dtG"].max()
        worst_res = max(worst_res, abs(out["residual"][i] - r["residual"]) / bar)
    print("%s P %d: v+ %.2e  a %.2e  lambda %.2e  lambda (contact frame) %.2e  lam_stop %.2e; residual %.2e of its bar"
          % (name, P, worst["v_next"], worst["a"], worst["lam"], worst["lam_contact"], worst["lam_stop"], worst_res))
    assert np.array_equal(out["tau_applied"], np.array([r["tau_applied"] for r in ref]))
    assert np.array_equal(out["stop_rows"], np.array([r["stop_rows"] for r in ref])) and out["stop_rows"].dtype == np.int32
    assert np.array_equal(out["dropped"], np.array([r["dropped"] for r in ref]))
    assert np.array_equal(out["sweeps"], np.array([r["sweeps"] for r in ref]))
    assert max(worst.values()) < 1e-9, worst
    assert worst_res <= 1.0, worst_res


# ---------------------------------------------------------------------------------------------------------------------- 2
def inert_model(name, P, seed, lib, alloc, steps=20):
    """Case 2: with tau_max = inf, d = r_a = 0 and stops = 0 the new kernel gives the bits of the existing ones: one solve on 24 states,
    then 20 steps on a handle with the inert model against a handle without one, with and without an environment, cold and warm-started."""
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    X, tau, planes, mu, push, j = parity_inputs(name, P, seed)[:6]
    na = rb.nv - 6
    for kw in (dict(tol=0.0), dict(tol=TOL, min_sweeps=MIN_SWEEPS)):
        ws = sim.groundSolveDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, **kw)
        for model in (dict(stops=False), dict(tau_max=np.full(na, np.inf), damping=np.zeros(na), armature=np.zeros((len(X), na)), stops=False)):
            jm = sim.groundJointDynamics(X, tau, DT, planes=planes, mu=mu, push=push, joint=j, **kw, **model)
            for k in SHARED:
                assert np.array_equal(ws[k], jm[k]), (k, kw)
            assert np.array_equal(jm["tau_applied"], tau) and not jm["stop_rows"].any() and not jm["lam_stop"].any() and not jm["dropped"].any()
        assert ws["contact"].any()
    B = 3
    X0, tq = G.drop_states(rb, B, 71)
    for with_env in (False, True):
        for warm in (False, True):
            pair = []
            for model in (True, False):
                _, _, h, _ = G.make(name, P, lib, B)
                if with_env:
                    h.setGroundEnv(planes=planes[:B], mu=mu[:B])
                    h.setPush(push[:B], joint=j)
                if warm:
                    h.setGroundSolver(warm_start=True, tol=1e-6, min_sweeps=0)
                if model:
                    h.setJointModel(tau_max=np.full(na, np.inf), damping=np.zeros((B, na)), armature=np.zeros(na), stops=False)
                pair.append(h)
            new, old = pair
            Xn, Xo, td = alloc(X0), alloc(X0), alloc(tq)
            landed = np.zeros(B, np.uint32)
            for k in range(steps):
                new.stepGroundDevice(Xn.ptr, td.ptr, DT)
                old.stepGroundDevice(Xo.ptr, td.ptr, DT)
                new.wait()
                old.wait()
                where = (with_env, warm, k)
                assert np.array_equal(Xn.get(), Xo.get()), where
                assert np.array_equal(new.lastGroundForces(), old.lastGroundForces()) and np.array_equal(new.lastContacts(), old.lastContacts()), where
                assert np.array_equal(new.lastAccelerations(), old.lastAccelerations()), where
                assert np.array_equal(new.lastAppliedTorques(), tq), where
                if warm:
                    assert np.array_equal(new.lastGroundSweeps(), old.lastGroundSweeps()) and np.array_equal(new.lastGroundResiduals(), old.lastGroundResiduals())
                    wn, wo = new.groundSolverDevicePointers()[2], old.groundSolverDevicePointers()[2]
                    assert wn and wo and np.array_equal(alloc.read(wn, (B, 3 * P * tab.nfeet)), alloc.read(wo, (B, 3 * P * tab.nfeet))), where
                landed |= new.lastContacts()
            assert (landed != 0).all() and np.abs(Xn.get() - X0).max() > 1e-4
            assert not new.lastJointStops()["stop_rows"].any()


# ---------------------------------------------------------------------------------------------------------------------- 3
def clipping(name, P, seed, lib, alloc):
    """Case 3: a step with tau = 10 tmax sign equals the step with tau = tmax sign bit for bit; where tau_max = inf, tau_applied == tau."""
    X, tau, planes, mu, push, j, tmax, dmp, arm, qlo, qhi, _ = parity_inputs(name, P, seed)
    rows = [0, 5, 9]
    B, na = 3, tau.shape[1]
    sign = np.where(np.random.default_rng(5).uniform(size=(B, na)) < 0.5, -1.0, 1.0)
    tm = tmax[rows].copy()
    tm[:, ::4] = np.inf
    lim = np.where(np.isfinite(tm), tm, 7.0)
    big, small = 10.0 * lim * sign, np.where(np.isfinite(tm), lim, 10.0 * lim) * sign
    tab, rb, sim, gz = G.make(name, P, lib, B)
    kw = dict(planes=planes[rows], mu=mu[rows], push=push[rows], joint=j, tau_max=tm, damping=dmp[rows], armature=arm[rows], q_lo=qlo[rows], q_hi=qhi[rows], stops=True)
    a, b = sim.groundJointDynamics(X[rows], big, DT, **kw), sim.groundJointDynamics(X[rows], small, DT, **kw)
    for k in SHARED + JOINT:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["tau_applied"], small) and np.array_equal(a["tau_applied"][:, ::4], big[:, ::4])
    assert (np.abs(a["tau_applied"])[:, 1::4] < np.abs(big)[:, 1::4]).all()
    out = []
    for t in (big, small):
        _, _, h, _ = G.make(name, P, lib, B)
        h.setJointModel(tau_max=tm, damping=dmp[rows], armature=arm[rows], q_lo=qlo[rows], q_hi=qhi[rows])
        Xd, td = alloc(X[rows]), alloc(t)
        h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        out.append((Xd.get(), h.lastAppliedTorques(), h.lastAccelerations()))
    for u, v in zip(*out):
        assert np.array_equal(u, v)
    assert np.array_equal(out[0][1], small) and np.abs(out[0][0] - X[rows]).max() > 1e-6


# ---------------------------------------------------------------------------------------------------------------------- 4
KNEE, KNEE_TAU, FAR = 2, 10.0, 10.0


def knee_loop(steps=200):
    """The checker's host loop of case 4: go2_like falling freely (the ground 10 m below), a constant torque driving joint 2 into q_hi.
    (final state, q_knee - q_hi per step)."""
    key = ("knee", steps)
    if key not in _cache:
        tab = T.table("go2_like")
        rb = RT.oracle_robot(tab)
        na = rb.nv - 6
        gz = G.ground_height(rb) - FAR
        x, tau = rb.x_ref.copy(), np.zeros(na)
        tau[KNEE] = KNEE_TAU
        pen = []
        for _ in range(steps):
            x, _, r = JR.step(rb, tab, x, tau, DT, np.array([0.0, 0.0, 1.0, gz]), MU, stops=1)
            pen.append(x[7 + KNEE] - tab.q_hi[KNEE])
        _cache[key] = (x, np.array(pen))
    return _cache[key]


def stop_holds(lib, alloc, steps=200, B=3):
    """Case 4: the stop of a knee holds against a constant torque for 200 steps; without stops the joint runs through."""
    name = "go2_like"
    xh, pen_h = knee_loop(steps)
    ref_pen = pen_h[50:].max()
    print("go2_like knee at q_hi: checker: largest q - q_hi over steps 50 .. %d: %.3e rad (over all steps %.3e)" % (steps - 1, ref_pen, pen_h.max()))
    assert pen_h.max() > -1e-3  # (the joint has arrived at its stop)
    tab, rb, _ = SIM.make(name, 3, lib, B)
    na = rb.nv - 6
    tau = np.zeros((B, na))
    tau[:, KNEE] = KNEE_TAU
    res = {}
    for stops in (True, False):
        _, _, sim = SIM.make(name, 3, lib, B)
        sim.setGround(ground_z=G.ground_height(rb) - FAR)
        sim.setJointModel(stops=stops)
        Xd, td = alloc(np.tile(rb.x_ref, (B, 1))), alloc(tau)
        pen, loaded = [], 0
        for _ in range(steps):
            sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
            sim.wait()
            pen.append(Xd.get()[0, 7 + KNEE] - tab.q_hi[KNEE])
            if stops:
                st = sim.lastJointStops()
                loaded += int(((st["stop_rows"] == -(KNEE + 1)) & (st["lam_stop"] > 0.0)).any(axis=1).all())
        X = Xd.get()
        assert np.array_equal(X[0], X[1]) and np.array_equal(X[0], X[2])
        res[stops] = (X[0], np.array(pen), loaded)
    x, pen, loaded = res[True]
    err = S.rel_err(xh[None], x[None])
    print("go2_like knee at q_hi: kernel: %d steps vs the host loop %.2e; largest q - q_hi over steps 50 .. %d: %.3e rad; steps with the stop loaded %d; "
          "without stops the joint ends at q_hi %+.3f rad" % (steps, err, steps - 1, pen[50:].max(), loaded, res[False][1][-1]))
    assert err < 1e-8, err
    assert loaded >= 50
    assert pen[50:].max() <= 10.0 * ref_pen, (pen[50:].max(), ref_pen)
    assert res[False][1].max() > 0.5


# ---------------------------------------------------------------------------------------------------------------------- 5
def damping_inputs():
    tab = T.table("go2_like")
    rb = RT.oracle_robot(tab)
    na = rb.nv - 6
    X0, _ = G.drop_states(rb, 1, 71)
    x0 = X0[0].copy()
    x0[rb.nq + 6 :] = np.random.default_rng(9).normal(size=na) * 2.0
    return tab, rb, x0, np.linspace(0.05, 0.4, na), np.linspace(0.0, 0.03, na)


def damping_loop(steps=40):
    key = ("damping", steps)
    if key not in _cache:
        tab, rb, x, d, ra = damping_inputs()
        gz = G.ground_height(rb)
        for _ in range(steps):
            x, _, _ = JR.step(rb, tab, x, np.zeros(rb.nv - 6), DT, np.array([0.0, 0.0, 1.0, gz]), MU, damping=d, armature=ra, stops=1)
        _cache[key] = x
    return _cache[key]


def damping_across_steps(lib, alloc, steps=40, B=3):
    """Case 5: 40 steps at zero torque with damping and armature against the checker's host loop; damping takes kinetic energy out of the
    joints."""
    tab, rb, x0, d, ra = damping_inputs()
    xh = damping_loop(steps)
    end = {}
    for damped in (True, False):
        _, _, sim, _ = G.make("go2_like", 1, lib, B)
        sim.setJointModel(damping=d if damped else None, armature=np.tile(ra, (B, 1)))
        Xd, td = alloc(np.tile(x0, (B, 1))), alloc(np.zeros((B, rb.nv - 6)))
        for _ in range(steps):
            sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
        sim.wait()
        X = Xd.get()
        assert np.array_equal(X[0], X[1]) and np.array_equal(X[0], X[2])
        end[damped] = X[0]
    err = S.rel_err(xh[None], end[True][None])
    e = {k: 0.5 * float(v[rb.nq + 6 :] @ v[rb.nq + 6 :]) for k, v in end.items()}
    print("go2_like, %d steps with damping and armature vs the host loop %.2e; 1/2 |v_joint|^2 at the end: damped %.4f, undamped %.4f" % (steps, err, e[True], e[False]))
    assert err < 1e-8, err
    assert e[True] < e[False]


# ---------------------------------------------------------------------------------------------------------------------- 6
def batch_hygiene(name, P, seed, lib, alloc):
    """Case 6: each robot of a B = 3 solve and of a B = 3 step equals its B = 1 solve with its own rows; a NaN state stays in its robot."""
    X, tau, planes, mu, push, j, tmax, dmp, arm, qlo, qhi, _ = parity_inputs(name, P, seed)
    rows = [1, 2, 7]  # (stops loaded, candidates dropped, torques clipped)
    B = 3
    tab, rb, sim, gz = G.make(name, P, lib, B)
    kw = lambda r: dict(planes=planes[r], mu=mu[r], push=push[r], joint=j, tau_max=tmax[r], damping=dmp[r], armature=arm[r], q_lo=qlo[r], q_hi=qhi[r], stops=True)
    three = sim.groundJointDynamics(X[rows], tau[rows], DT, **kw(rows))
    assert three["stop_rows"][0].any() and three["dropped"][1] > 0 and (three["tau_applied"][2] != tau[rows][2]).any()
    _, _, one, _ = G.make(name, P, lib, 1)
    for i, r in enumerate(rows):
        single = one.groundJointDynamics(X[[r]], tau[[r]], DT, **kw([r]))
        for k in SHARED + JOINT:
            assert np.array_equal(three[k][i], single[k][0]), (k, i)
    bad = X[rows].copy()
    bad[1, 9] = np.nan
    nan = sim.groundJointDynamics(bad, tau[rows], DT, **kw(rows))
    for k in SHARED + JOINT:
        assert np.array_equal(nan[k][[0, 2]], three[k][[0, 2]]), k
    assert np.isnan(nan["v_next"][1]).any()
    # the handle's step with the same rows: the read-outs of the step are those of the solve
    sim.setGroundEnv(planes=planes[rows], mu=mu[rows])
    sim.setPush(push[rows], joint=j)
    sim.setJointModel(tau_max=tmax[rows], damping=dmp[rows], armature=arm[rows], q_lo=qlo[rows], q_hi=qhi[rows], stops=True)
    Xd, td = alloc(X[rows]), alloc(tau[rows])
    sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
    sim.wait()
    st = sim.lastJointStops()
    assert np.array_equal(sim.lastAccelerations(), three["a"]) and np.array_equal(sim.lastGroundForces(), three["lam"])
    assert np.array_equal(sim.lastAppliedTorques(), three["tau_applied"]) and np.array_equal(Xd.get()[:, rb.nq :], three["v_next"])
    for k in ("stop_rows", "lam_stop", "dropped"):
        assert np.array_equal(st[k], three[k]), k
    ptrs = sim.jointModelDevicePointers()
    assert all(ptrs) and np.array_equal(alloc.read(ptrs[0], (B, rb.nv - 6)), three["tau_applied"])


# ---------------------------------------------------------------------------------------------------------------------- 7
def admission(lib, alloc):
    """Case 7: every refusal, through the C ABI; a refused call keeps the previous model; setGround drops it; read-outs before the setter."""
    lib = lib or simple_mpc.default_lib()
    L = lib.L
    err = lambda: L.smpc_last_error().decode()
    name, B = "go2_like", 3
    tab, rb, sim = SIM.make(name, 3, lib, B)
    na = rb.nv - 6
    lo, hi = limits(tab, na)

    def model(per_robot=0, stops=1, activation=0.0, stop_erp=0.0, **arrays):
        m = JointModelSettingsC()
        keep = []
        for k, v in arrays.items():
            v = np.ascontiguousarray(np.array(v, dtype=np.float64))
            keep.append(v)
            setattr(m, k, v.ctypes.data)
        m.per_robot, m.stops, m.activation, m.stop_erp = per_robot, stops, activation, stop_erp
        return m, keep

    def set_model(**kw):
        m, keep = model(**kw)
        return L.smpc_robot_sim_set_joint_model(sim._h, C.byref(m))

    # no ground yet
    assert set_model() == _INVALID and "no ground" in err()
    with pytest.raises(RuntimeError, match="no ground"):
        sim.setJointModel()
    with pytest.raises(RuntimeError, match="no ground"):
        sim.lastAppliedTorques()
    far = G.ground_height(rb) - FAR  # (no foot reaches the plane: the knee meets nothing but its stop)
    sim.setGround(ground_z=far)
    # before the setter: zeros and null pointers
    assert sim.jointModelDevicePointers() == (0, 0, 0, 0)
    st = sim.lastJointStops()
    assert not sim.lastAppliedTorques().any() and not st["stop_rows"].any() and not st["lam_stop"].any() and not st["dropped"].any()
    X, tau = G.drop_states(rb, B, 71)
    X[:, 7 + KNEE] = hi[KNEE] + 0.01  # (a stop is loaded from the first step on)
    X[:, rb.nq + 6 + KNEE] = 1.0
    tau[:, KNEE] = 5.0
    tmax = np.full((B, na), 3.0)
    good = dict(tau_max=tmax, damping=np.full(na, 0.1), armature=np.full(na, 0.01), stops=True)
    sim.setJointModel(**good)
    ptrs = sim.jointModelDevicePointers()
    assert all(ptrs)
    td = alloc(tau)

    def one_step(h):
        Xd = alloc(X)
        h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        s = h.lastJointStops()
        return Xd.get(), h.lastAppliedTorques(), s["stop_rows"], s["lam_stop"]

    _, _, twin = SIM.make(name, 3, lib, B)
    twin.setGround(ground_z=far)
    twin.setJointModel(**good)
    nan, inf = float("nan"), float("inf")

    def arr(value, at=(1, 4), fill=1.0):
        a = np.full((B, na), fill)
        a[at] = value
        return a

    refusals = [
        (dict(per_robot=1, tau_max=arr(-1.0)), ("tau_max[1][4]", "negative")),
        (dict(per_robot=1, tau_max=arr(nan)), ("tau_max[1][4]", "NaN")),
        (dict(per_robot=1, damping=arr(-0.5)), ("damping[1][4]", "negative")),
        (dict(per_robot=1, damping=arr(inf)), ("damping[1][4]", "finite")),
        (dict(per_robot=1, damping=arr(nan)), ("damping[1][4]",)),
        (dict(armature=np.r_[np.zeros(5), -1e-3, np.zeros(na - 6)]), ("armature[0][5]", "negative")),
        (dict(armature=np.r_[np.zeros(5), inf, np.zeros(na - 6)]), ("armature[0][5]", "finite")),
        (dict(per_robot=1, q_lo=arr(2.0, fill=-1.0), q_hi=arr(1.0)), ("q_lo[1][4]", "exceeds")),
        (dict(q_lo=hi + 1.0), ("q_lo[0][0]", "exceeds")),  # (against the table's q_hi)
        (dict(per_robot=1, q_lo=arr(nan, fill=-1.0)), ("q_lo[1][4]", "NaN")),
        (dict(per_robot=1, q_hi=arr(nan)), ("q_hi[1][4]", "NaN")),
        (dict(activation=-0.1), ("activation = -0.1",)),
        (dict(activation=nan), ("activation",)),
        (dict(stop_erp=1.5), ("stop_erp = 1.5",)),
        (dict(stop_erp=-0.1), ("stop_erp = -0.1",)),
        (dict(stop_erp=nan), ("stop_erp",)),
        (dict(stops=2), ("stops = 2",)),
        (dict(stops=-1), ("stops = -1",)),
    ]
    for kw, words in refusals:
        assert set_model(**kw) == _INVALID, words
        assert all(w in err() for w in words), (words, err())
        assert sim.jointModelDevicePointers() == ptrs
        got, want = one_step(sim), one_step(twin)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), words
        assert (np.abs(got[1]) <= 3.0).all() and (got[2] == -(KNEE + 1)).any() and (got[3] > 0.0).any()
    # the host-buffer solve refuses the same values, and admits a null model and null outputs
    m, keep = model(per_robot=1, tau_max=arr(-1.0))
    none = [None] * 12
    assert L.smpc_robot_sim_ground_joint_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, None, None, C.byref(m), *none) == _INVALID
    assert "tau_max[1][4]" in err()
    assert L.smpc_robot_sim_ground_joint_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, None, None, None, *none) == 0, err()
    with pytest.raises(RuntimeError, match="tau_max \\[na\\]"):
        sim.setJointModel(tau_max=np.ones((B, na + 1)))
    # infinite limits and a zero effort limit are admitted
    sim.setJointModel(tau_max=np.zeros(na), q_lo=np.full(na, -inf), q_hi=np.full(na, inf))
    got = one_step(sim)
    assert not got[1].any() and not got[2].any()
    # setGround drops the model
    sim.setGround(ground_z=far)
    assert sim.jointModelDevicePointers() == (0, 0, 0, 0) and not sim.lastAppliedTorques().any()
    plain = SIM.make(name, 3, lib, B)[2]
    plain.setGround(ground_z=far)
    Xa, Xb = alloc(X), alloc(X)
    sim.stepGroundDevice(Xa.ptr, td.ptr, DT)
    plain.stepGroundDevice(Xb.ptr, td.ptr, DT)
    sim.wait()
    plain.wait()
    assert np.array_equal(Xa.get(), Xb.get())


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
class Host(HostArray):
    """HostArray, and a reader of handle-owned buffers by address."""

    @staticmethod
    def read(ptr, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array((C.c_double * n).from_address(ptr)).reshape(shape).copy()


@pytest.mark.parametrize("name,P,seed", CASES)
def test_parity_with_the_checker(built, name, P, seed):
    parity(name, P, seed, S.emu_lib())


@pytest.mark.parametrize("name,P,seed", CASES)
def test_inert_model_bit_for_bit(built, name, P, seed):
    inert_model(name, P, seed, S.emu_lib(), Host)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_clipping(built, name, P, seed):
    clipping(name, P, seed, S.emu_lib(), Host)


def test_a_stop_holds(built):
    stop_holds(S.emu_lib(), Host)


def test_damping_and_armature_across_steps(built):
    damping_across_steps(S.emu_lib(), Host)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_batch_hygiene(built, name, P, seed):
    batch_hygiene(name, P, seed, S.emu_lib(), Host)


def test_admission_and_errors(built):
    admission(S.emu_lib(), Host)
