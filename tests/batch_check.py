"""Batch independence of the MPC engines under heavy backtracking.  TEST INFRASTRUCTURE of tests/test_batch_independence.py.

A pool of N = 150 distinct measured states (two full waves and a partial one) is chosen ON THE ORACLE ALONE so that, at control step 0, more than
LS_SLOTS = 64 instances reject alpha = 1 in the first iteration (the list the speculative scheme restores, backtracks and re-derives) and more
than 64 in the final line search, while some instances accept it (the list is a proper subset of the batch).  The pool is then solved in
several arrangements -- in order, rotated, in chunks of 1 / 63 / 64 / 22 on handles of their own, padded into a batch of 342, and with the
environment switches that change the schedule -- and every output a caller can read must be the same bit for bit; the in-order arrangement is
also compared with the oracle at control step 0."""
import os
import time
import types

import numpy as np

import mpc_setup as S
import oracle_lib as O

N = 150  # 2 * 64 + 22
LS_SLOTS = 64  # smpc_stage_engine.h: instance slots of the list-mode launches
ROLL = 37  # no state keeps its lane or its wave
CHUNKS = (1, 63, 64, 22)
PAD_B, PAD_AT = N + 64 * 3, 100  # per = ceil(B / 64) of compact_body: 3 at B = 150, 6 at B = 342
SEED = 3
STEPS = 2
TOL = 1e-4  # the bar of every family's own parity tests (test_gpu_parity.py, test_fulldynamics_mpc.py, test_talos_*.py, test_centroidal_mpc.py)
# info[:, :12] are the solver's scalars (SC_PHI0 .. SC_LS_INDEX of smpc_model.h: what the oracle's info holds too); column 12 is SC_PREG_OLD, the
# slot in which the speculative scheme keeps the regularisation across a tentative full step -- the sequential scheme never writes it
INFO_SOLVER = 12
ENV_SWITCHES = ("SMPC_NO_SPECULATIVE_LS", "SMPC_STREAMS", "SMPC_FULL_PARTS", "SMPC_CENT_PARTS", "SMPC_CENT_FUSED", "SMPC_CENT_LS", "SMPC_RICCATI")

GO2_WALK = (0.2, 0, 0, 0, 0, 0.1)
TALOS_WALK = (0.1, 0, 0, 0, 0, 0.0)
# the short gait cycles of tests/test_sweeps.py (_kino_record; SHORT)
GO2_SHORT = dict(cycle=O.trot_cycle(T_ds=4, T_ss=8), mpc=dict(T_fly=8, T_contact=4))
TALOS_SHORT = dict(cycle=O.walk_cycle(5, 20), mpc=dict(T_fly=20, T_contact=5))
KINO_EXT = dict(settings_override={"force_cone": True, "land_cstr": True, "mu": 0.3}, mpc_override={"terminal_constraint": True})  # test_engine_schedule.py


def _talos_oracle(kind):
    def make(B, max_iters, horizon, settings_override=None, mpc_override=None):
        rb = O.Robot("talos_like")
        settings, model, mpc = {
            "full": (O.talos_full_settings, O.Full, O.OracleFullMPC),
            "kino": (O.talos_kino_settings, O.Kino, O.OracleMPC),
            "cent": (O.talos_centroidal_settings, O.Cent, O.OracleCentMPC),
        }[kind]
        s = settings(rb)
        s.update(settings_override or {})
        ms = O.talos_mpc_settings(rb, max_iters=max_iters)
        ms["T"] = horizon
        ms.update(mpc_override or {})
        return mpc(model(rb, s), ms, B), rb

    return make


def _go2_oracle(make):
    def wrapped(B, max_iters, horizon, **kw):
        r = make(B, max_iters, horizon, **kw)
        return r[0], r[1]

    return wrapped


def _go2_full_oracle(B, max_iters, horizon, **kw):
    return S.make_full_oracle(B, max_iters, horizon, walk=None, **kw)


# family -> product factory, oracle factory, overrides, gait, states; `scale`: the scatter of the pool ({horizon: scale}; how each was found: the
# docstrings of tests/test_batch_independence.py); `cent`: the measured state drifts (tests/test_centroidal_mpc.py) instead of following xs[1];
# `forces`: the handle answers getContactForces; `parts`: the environment switch that runs the batch as parts on streams of their own
FAMILIES = {
    "go2_kino": dict(product=S.make_product, oracle=_go2_oracle(S.make_oracle), kw={}, gait=GO2_SHORT, walk=GO2_WALK, states=S.random_states,
                     scale={20: 16.0}, cent=False, forces=False, parts="SMPC_STREAMS", sequential=True),
    "go2_kino_ext": dict(product=S.make_product, oracle=_go2_oracle(S.make_oracle), kw=KINO_EXT, gait=GO2_SHORT, walk=GO2_WALK, states=S.random_states,
                         scale={20: 1.0, 6: 1.0}, cent=False, forces=False, parts=None, sequential=False),
    "go2_full": dict(product=S.make_full_product, oracle=_go2_full_oracle, kw={}, gait=GO2_SHORT, walk=GO2_WALK, states=S.random_states,
                     scale={20: 3.0, 6: 6.0}, cent=False, forces=True, parts="SMPC_FULL_PARTS", sequential=False),
    "talos_full": dict(product=S.make_talos_product, oracle=_talos_oracle("full"), kw={}, gait=TALOS_SHORT, walk=TALOS_WALK, states=S.talos_random_states,
                       scale={20: 3.0, 6: 3.0}, cent=False, forces=True, parts="SMPC_FULL_PARTS", sequential=False),
    "talos_kino6d": dict(product=S.make_talos_kino_product, oracle=_talos_oracle("kino"), kw={}, gait=TALOS_SHORT, walk=TALOS_WALK,
                         states=S.talos_random_states, scale={20: 4.0, 6: 6.0}, cent=False, forces=True, parts="SMPC_FULL_PARTS", sequential=False),
    "go2_cent": dict(product=S.make_cent_product, oracle=_go2_oracle(S.make_cent_oracle), kw={}, gait=GO2_SHORT, walk=GO2_WALK, states=S.random_states,
                     scale={20: 2.0, 6: 2.0}, cent=True, forces=False, parts="SMPC_CENT_PARTS", sequential=True, subset=False),
    "talos_cent": dict(product=S.make_talos_cent_product, oracle=_talos_oracle("cent"), kw={}, gait=TALOS_SHORT, walk=TALOS_WALK,
                       states=S.talos_random_states, scale={20: 6.0, 6: 6.0}, cent=True, forces=False, parts=None, sequential=False),
}


def _overrides(fam):
    kw = {k: dict(v) for k, v in fam["kw"].items()}
    kw["mpc_override"] = dict(kw.get("mpc_override", {}), **fam["gait"]["mpc"])
    return kw


def make_oracle(family, B, max_iters, horizon):
    fam = FAMILIES[family]
    om, rb = fam["oracle"](B, max_iters, horizon, **_overrides(fam))
    om.generateCycleHorizon(fam["gait"]["cycle"])
    om.switchToWalk(np.array(fam["walk"], float))
    return om, rb


def make_handle(family, B, lib, horizon, env=None):
    """A handle of the family with max_iters = 3 (the speculative scheme) and retained state derivatives.  env: switches the engine reads when the
    handle is created (every such switch is cleared otherwise)."""
    fam = FAMILIES[family]
    old = {k: os.environ.pop(k, None) for k in ENV_SWITCHES}
    try:
        os.environ.update(env or {})
        gm = fam["product"](B, max_iters=3, lib=lib, horizon=horizon, **_overrides(fam))[0]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    gm.generateCycleHorizon(fam["gait"]["cycle"])
    gm.switchToWalk(np.array(fam["walk"], float))
    gm.setRetainStateDerivatives(True)
    return gm


def drift(rb, X):
    """The measured multibody state of the centroidal families moves as a simulator would report it (tests/test_centroidal_mpc.py::_run_pair)."""
    d = np.r_[np.zeros(rb.nv), 0.02, 0.01, np.zeros(rb.nv - 2)]
    return np.stack([rb.integrate(x, d) for x in X])


def backtracked(info):
    return int((info[:, 2] < 1.0).sum())


_pools = {}


def pool(family, horizon):
    """The pool of the family at this horizon and the oracle's control step 0 on it: dict(X, rb, oracle = outputs of the max_iters = 3 oracle,
    n1, n3).  The conditions on the pool are asserted here, on the oracle alone, before any kernel runs.  Computed once per session."""
    key = (family, horizon)
    if key in _pools:
        return _pools[key]
    fam = FAMILIES[family]
    t0 = time.time()
    out, counts = {}, {}
    for k in (1, 3):
        om, rb = make_oracle(family, N, k, horizon)
        X = fam["states"](rb, N, seed=SEED, scale=fam["scale"][horizon])
        for step in range(STEPS if k == 3 else 1):
            om.iterate(X)
            rec = dict(xs=om.xs, us=om.us, vs=om.vs, lams=om.lams, K0=om.K0, info=om.info)
            for name, v in rec.items():
                assert np.all(np.isfinite(v)), "%s: the oracle's %s is not finite (max_iters = %d, control step %d)" % (family, name, k, step)
            if step == 0:
                counts[k] = backtracked(rec["info"])
                out[k] = rec
            X = drift(rb, X) if fam["cent"] else rec["xs"][:, 1, :].copy()
    p = dict(X=fam["states"](rb, N, seed=SEED, scale=fam["scale"][horizon]), rb=rb, oracle=out[3], n1=counts[1], n3=counts[3])
    print("%s, H = %d, scale %g: the oracle backtracks %d of %d instances at control step 0 with max_iters = 1, %d with max_iters = 3 (%.1f s)"
          % (family, horizon, fam["scale"][horizon], p["n1"], N, p["n3"], time.time() - t0))
    _pools[key] = p
    return p


def check_pool(p, family):
    assert p["n3"] > LS_SLOTS, "%s: the final line search must backtrack more than %d instances: %d" % (family, LS_SLOTS, p["n3"])
    assert p["n1"] > LS_SLOTS, "%s: the first iteration must reject alpha = 1 for more than %d instances: %d" % (family, LS_SLOTS, p["n1"])
    if FAMILIES[family].get("subset", True):  # (go2_cent: the oracle backtracks every instance at every scale -- tests/test_batch_independence.py)
        assert p["n1"] <= N - 3, "%s: at least 3 instances must accept alpha = 1 in the first iteration: %d reject it" % (family, p["n1"])
        assert p["n3"] < N, "%s: the final line search must leave an instance out of the list: %d" % (family, p["n3"])


def outputs(gm, fam):
    """Everything a caller can read after a control step."""
    xd = gm.getStateDerivatives()
    rec = dict(xs=gm.xs, us=gm.us, vs=gm.vs, lams=gm.lams, K0=gm.K0, Ks=gm.Ks, info=gm.info, xdot0=gm.getStateDerivative(0),
               xdot1=gm.getStateDerivative(1), xdot_last=xd[:, gm.H - 1], poses=gm.getReferencePoses())
    if fam["forces"]:
        rec["forces"] = gm.getContactForces()
    return rec


def run(family, pieces, X0, rb, steps=STEPS):
    """pieces: [(handle, idx)], idx[i] = the pool index of the handle's instance i, or -1 for an instance that starts at the reference state.
    Every instance is fed its own xs[:, 1] (its own drifted state for the centroidal families).  Returns per control step the outputs in POOL
    order ({name: [N, ...]})."""
    fam = FAMILIES[family]
    recs = [dict() for _ in range(steps)]
    for gm, idx in pieces:
        idx = np.asarray(idx)
        own = idx >= 0
        X = np.where(own[:, None], X0[np.maximum(idx, 0)], rb.x_ref[None, :])
        for step in range(steps):
            gm.iterate(X)
            out = outputs(gm, fam)
            for name, v in out.items():
                if name not in recs[step]:
                    recs[step][name] = np.full((len(X0),) + v.shape[1:], np.nan)
                recs[step][name][idx[own]] = v[own]
            X = drift(rb, X) if fam["cent"] else out["xs"][:, 1, :].copy()
    return recs


def same_bits(a, b, what, info_cols=None):
    """info_cols: compare info[:, :info_cols] only (see INFO_SOLVER)."""
    for step, (ra, rb_) in enumerate(zip(a, b)):
        assert ra.keys() == rb_.keys()
        if info_cols is not None:
            ra, rb_ = dict(ra, info=ra["info"][:, :info_cols]), dict(rb_, info=rb_["info"][:, :info_cols])
        for name in ra:
            if not np.array_equal(ra[name], rb_[name]):
                bad = np.flatnonzero((ra[name] != rb_[name]).reshape(len(ra[name]), -1).any(1))
                raise AssertionError("%s: %s differs at control step %d for %d instances (pool indices %s ..), max |difference| %.3e"
                                     % (what, name, step, len(bad), bad[:8].tolist(), np.nanmax(np.abs(ra[name][bad] - rb_[name][bad]))))


def arrangements(family):
    """name -> pieces [(B, idx, env)]: the handles of the arrangement, the pool index of each of their instances (-1: padding), the environment
    switches set while they are created."""
    fam = FAMILIES[family]
    order = np.arange(N)
    start = np.cumsum((0,) + CHUNKS[:-1])
    padded = np.full(PAD_B, -1)
    padded[PAD_AT:PAD_AT + N] = order
    arr = {
        "A1 rotated": [(N, np.roll(order, ROLL), None)],
        "A2 chunked": [(n, order[s:s + n], None) for s, n in zip(start, CHUNKS)],
        "A3 padded": [(PAD_B, padded, None)],
    }
    if fam["parts"]:
        arr["A5 two parts"] = [(N, order, {fam["parts"]: "2"})]
    return arr


# Pools whose oracle is itself ill-conditioned for some instance: (family, horizon) -> {pool index: (xs, us)}, the disagreement of two oracle runs
# (max_iters = 3, control step 0), the second on the measured states times (1 + 1e-15), normalised as S.rel_err does over the pool.  Such an
# instance is gated at 10 x that figure (the convention of tests/sweep_check.py), every other one at TOL.  talos_full, H = 20, scale 3: instance
# 109 alone carries the oracle's disagreement -- xs 1.469e-4, us 2.046e-4 (with the states times (1 - 1e-15): 9.9e-5 / 1.4e-4; times
# 1 +- 1e-15 with random signs, seeds 0 and 1: 3.4e-5 / 5.2e-5 and 3.6e-4 / 4.9e-4); the next instances (27, 92, 90) disagree by 4.8e-6, 4.3e-6,
# 3.3e-6, the median instance by 2e-13.  Against the unperturbed oracle the emulated bodies are 9.94e-5 / 1.35e-4 away at instance 109, an
# MI355X 3.73e-4 / 5.13e-4: the device does not meet TOL there, hence the measured gate.  At H = 6 (CPU tier) every instance meets TOL.
SENSITIVE = {("talos_full", 20): {109: (1.469e-4, 2.046e-4)}}


def check_parity(family, horizon, p, rec0):
    """Control step 0 of the in-order arrangement against the oracle (max_iters = 3, all N instances): line-search decisions by the rule of
    test_centroidal_mpc.py::test_gpu_full_size_properties; xs and us of the instances with identical decisions at TOL, relative to the pool
    as S.rel_err is (SENSITIVE: the instances gated at 10 x the oracle's own disagreement instead)."""
    o = p["oracle"]
    og, gg = types.SimpleNamespace(info=o["info"]), types.SimpleNamespace(info=rec0["info"])
    same = o["info"][:, 2] == rec0["info"][:, 2]
    err = {k: np.abs(o[k] - rec0[k]).reshape(N, -1).max(1) / max(1.0, np.abs(o[k]).max()) for k in ("xs", "us")}
    gate = {k: np.full(N, TOL) for k in err}
    for i, (gx, gu) in SENSITIVE.get((family, horizon), {}).items():
        gate["xs"][i], gate["us"][i] = max(TOL, 10.0 * gx), max(TOL, 10.0 * gu)
        print("%s: instance %d, gated at 10 x the oracle's own disagreement (xs %.3e, us %.3e): xs %.3e, us %.3e"
              % (family, i, gate["xs"][i], gate["us"][i], err["xs"][i], err["us"][i]))
    at_tol = same & (gate["xs"] == TOL)
    print("%s: %d of %d line-search decisions differ from the oracle's; of the others, worst relative error at the bar of %g: xs %.3e, us %.3e"
          % (family, int((~same).sum()), N, TOL, err["xs"][at_tol].max(), err["us"][at_tol].max()))
    assert S.alphas_agree(og, gg), ("line-search step sizes differ", o["info"][~same, :4], rec0["info"][~same, :4])
    assert same.mean() >= 0.9, "line-search decisions differ for %d of %d instances" % (int((~same).sum()), N)
    for k in err:
        bad = np.flatnonzero(same & ~(err[k] < gate[k]))
        assert len(bad) == 0, "%s: %s of instances %s is %s from the oracle's (gates %s)" % (family, k, bad.tolist(), err[k][bad], gate[k][bad])
