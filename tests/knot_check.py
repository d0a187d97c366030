"""Knot-level checker: the LQ knots of a product handle (derivative pass: deriv_body, lane_tree_body -> deriv2_body, fdyn_deriv_body and its
KIN = 1 instantiation) against the oracle's knots of the SAME evaluation point, per stage, per field and per block.  TEST INFRASTRUCTURE.

The synced step.  `synced_step(gm, oms, X)` hands the product's iterate to the oracle (OracleMPC.set_iterate(gm.xs, gm.us, gm.vs, gm.lams)) and
then runs om.iterate(X) and gm.iterate(X), both with max_iters = 1.  Both sides recede the same iterate, insert the same measured state and
restart preg, so the knots of that one iteration are evaluated at the same point up to the recede, and what remains between them is the
rounding of the derivative pass (and of the recede: the last stage's copy, the zeroed trailing multipliers, the centres -- a difference there
shows in f, d, q, r of the stages it touches).  Without the sync both sides sit at their own iterates, 1e-10 and more apart after a few control
steps, and a knot gate measures the closed loop.

Partition (`blocks`).  Tangent state [base lin 3 | base ang 3 | joints na | base lin vel 3 | base ang vel 3 | joint vel na]; controls of the
kinodynamics engines [force / wrench of foot 0 | .. | foot nf-1 | joint part na], of full dynamics [torques na]; constraint rows by family, in
the oracle's row order (smpc_model.h, smpc_full_model.h, oracle/orc_kino.hpp, orc_fulldyn.hpp):
  * Go2 kinodynamics:   joint box na | frame velocity 3 per foot                      (D = 0: the oracle's D must be exactly zero)
  * full dynamics:      torque box na | joint box na | cone rows per foot (5 / 17) | land rows per foot (4 / 6)
  * Talos kinodynamics: joint box na | frame velocity 6 per foot | wrench cone 17 per foot (force_cone)
`device_knot` brings debug_lq into that layout: for the dense engines the box rows are rebuilt from the activity flags exactly as
sweep_check.lq_inputs does (torque box: unit rows of D; joint box: unit rows of C on dx[6 + i]), the dense rows are Cd | Dd, and for Talos
kinodynamics the device's rows [control box (absent) | joint box | cone | velocity] are permuted into the oracle's order and the frame-velocity
rows Cv take their place in C.

Per-block gaps (`knot_gaps`): max|a - b| / max|b| over the block, b the oracle's, NOT floored.  A block the oracle holds at exactly zero must be
exactly zero on the device: "holds" means exactly zero at EVERY stage of the instance (`held_at_zero`).  A block that is a ROUNDING RESIDUE in
the oracle -- at most 2^-40 = 9e-13 of the largest entry of the whole field at that stage: a structural zero the oracle forms as a cancelling
difference, 1e-17 in A next to its identity, 1e-33 in Q next to 1e5, exactly zero at one stage and 1e-33 at the next -- has no size of its own
to be relative to; it must be a residue on the device too and counts as gap 0 (`_gap`).  Without this rule the two oracles themselves differ by
O(1) .. 1e3 in such blocks and the measured floor of A, Q, S, C, QN would be meaningless; every block above 9e-13 of its field stays unfloored.  Fields: A, B, Q, S, R, C, D (block = row family x column block), f, d, q, r, lpd, vpd (block = the vector's
partition), QN, qN.  The activity pattern must be equal: the device's flags against the nonzero rows of the oracle's [C D].

  * lpd and vpd are what debug_lq returns beside the knot and what the line search consumes; their reference is formed from oracle quantities,
    lpd = lam_{t+1} + 2 f / mu and on active rows vpd = v_t + 2 d / mu, zero on inactive rows (oracle/orc_proxddp.hpp: 2 lam+ - lam, 2 v+ - v,
    with f = mu (lam+ - lam), d = mu (v+ - v)); lam, v are the synced iterate after the recede.
  * lx and lu are NOT compared: the oracle exports q = lx + A^T lam+ + Cx^T v - lam with ALL rows of Cx, but C only with its active rows,
    so lx cannot be taken out of q without the inactive rows of Cx (likewise lu).
  * Cancelling sums.  f, d, q, r, qN are differences of terms far larger than themselves near a solution; relative to their own size the
    rounding of the terms shows as 1e-9 .. O(1) (tests/test_centroidal_knots.py).  They are gated relative to the terms they are differences
    of, max|a - b| / max(max|b|, scale), with the scales of test_centroidal_knots.py::_scales restated for a state that is not its own tangent:
    f: max|x_{t+1}|; d: max(|D u_t|, |C_vel v_t|, |C_joints q_joints|) (the terms of the frame-velocity rows, cone rows and box rows);
    q: max(|lam_t|, |A^T lam_{t+1}|, |C^T v_t|); r: max(|B^T lam_{t+1}|, |D^T v_t|, |R u_t|); qN: max|lam_H| -- all from the oracle's knot
    and the synced iterate (lam_H is zero after the recede of a max_iters = 1 handle, so qN = lxN is in fact compared unfloored).  lpd and vpd carry f / mu and d / mu: the same scales divided by mu are added to theirs.  Every run prints the raw
    figure (relative to the vector's own size) beside the gated one.  Matrices stay unfloored.
  * Talos kinodynamics.  The stage kernel folds the frame-velocity rows, Q += Cv^T Cv / mu, q += Cv^T d_vel / mu.  The checker takes the
    fold out with the device's own Cv and compares the unfolded Q and q with the oracle's; Cv is compared with the oracle's velocity rows.
    Taking the fold out is a subtraction of terms of 1e8 |Cv|^2: the unfolded Q and q are cancelling sums of the checker's own making and are
    gated relative to the fold term of the block, max|a - b| / max(max|b|, max|Cv^T Cv / mu| of the block) (q: max|Cv^T d / mu|).  The fold
    identity itself -- the device's folded Q against the oracle's Q + Cv^T Cv / mu with the oracle's rows, relative to max|Q folded| -- is
    kept at the 1e-12 of test_talos_kinodynamics.py::test_emulated_kernels_stage_knots.

Gates are measured, not chosen.  FLOOR of a (scenario, field) is the largest per-stage, per-block gap between TWO ORACLES at the same synced
iterate: one on the built-in robot table, one on its reframed twin (tests/robot_tables.py::reframe with REFRAME_SEED: every joint frame turned
about its own axis; tests/test_reframed_robots.py establishes that the twin is the same robot up to rounding).  Neither is the code under
test.  GATE = 10 x FLOOR, 1e-11 where the floor is below 1e-12 (the rule of sweep_check.py).  `floors(...)` prints a row of the table; the
floors below were measured with it on the emulated bodies' iterates (CPU).  A device or emulated gap above 100 x its floor is a finding to
explain, not a number to widen.  The twin exists for every family checked here (go2_like_rf, talos_like_rf).

Not covered (stated so that nobody assumes otherwise):
  * the extra rows of the structured Go2 kinodynamics sweep under force_cone / land_cstr: they are not in debug_lq's C, and
    sweep_check.kind_of -- which this module uses -- refuses such handles;
  * handles with terminal_constraint = True: the product has no read-out of the terminal multiplier to sync;
  * iterates of max_iters > 1 (the five older knot tests keep those);
  * lx, lu (above).

%(observed)s

FLOORS / GATES (per scenario and field)
%(table)s
"""
import numpy as np

import sweep_check as SC

MATS = ("A", "B", "Q", "S", "R", "C", "D")
VECS = ("f", "d", "q", "r", "lpd", "vpd")
TERM = ("QN", "qN")
FIELDS = MATS + VECS + TERM
SCALED = ("f", "d", "q", "r", "lpd", "vpd", "qN")  # gated relative to the terms they are differences of (module docstring)

# scenario -> floor per field, in the order of FIELDS: the largest per-stage, per-block gap between the oracle and its reframed twin at the
# synced iterates of the scenario's checked control steps (emulated bodies).  `floors(...)` prints a row.
FLOORS = {
    "kino_record": (6.5e-15, 5.5e-15, 2.8e-14, 1.5e-15, 1.6e-15, 9.9e-16, 0.0e+00, 2.4e-16, 1.7e-15, 6.3e-14, 8.4e-16, 2.4e-16, 1.7e-15, 9.9e-15, 6.6e-15),
    "kino_h3": (2.6e-15, 3.1e-15, 9.6e-15, 9.3e-16, 7.7e-16, 5.6e-16, 0.0e+00, 2.3e-16, 5.2e-16, 9.1e-15, 5.5e-16, 2.3e-16, 5.2e-16, 9.6e-15, 5.7e-16),
    "kino_h65": (6.3e-15, 4.6e-15, 3.5e-14, 1.3e-15, 1.2e-15, 9.7e-16, 0.0e+00, 2.6e-16, 1.3e-15, 7.4e-14, 6.1e-16, 2.6e-16, 1.3e-15, 1.4e-14, 2.5e-15),
    "kino_dense_w": (5.6e-15, 4.7e-15, 6.6e-15, 1.2e-15, 1.2e-15, 9.1e-16, 0.0e+00, 2.1e-16, 1.2e-15, 9.1e-14, 7.3e-16, 2.1e-16, 1.2e-15, 1.1e-14, 3.5e-15),
    "kino_tight_limits": (1.0e-14, 4.9e-15, 1.7e-14, 1.1e-15, 1.2e-15, 9.5e-16, 0.0e+00, 6.0e-16, 1.7e-16, 3.0e-14, 2.2e-15, 6.0e-16, 1.7e-16, 3.3e-15, 4.4e-16),
    "kino_b65": (4.3e-15, 4.5e-15, 2.7e-14, 1.1e-15, 1.0e-15, 1.2e-15, 0.0e+00, 2.6e-16, 9.6e-16, 3.5e-14, 6.0e-16, 2.6e-16, 9.6e-16, 2.7e-14, 1.2e-15),
    "kino_one_kernel_deriv": (7.5e-15, 5.4e-15, 2.5e-14, 1.4e-15, 1.3e-15, 8.9e-16, 0.0e+00, 2.6e-16, 1.4e-15, 1.5e-13, 8.7e-16, 2.6e-16, 1.4e-15, 1.9e-14, 5.6e-15),
    "kino_one_kernel_eval": (7.5e-15, 5.4e-15, 2.5e-14, 1.4e-15, 1.3e-15, 8.9e-16, 0.0e+00, 2.6e-16, 1.4e-15, 1.5e-13, 8.7e-16, 2.6e-16, 1.4e-15, 1.9e-14, 5.6e-15),
    "full_go2_record": (2.9e-14, 2.1e-14, 9.0e-15, 9.2e-15, 2.3e-15, 0.0e+00, 0.0e+00, 5.6e-15, 0.0e+00, 2.1e-15, 6.2e-12, 5.6e-15, 0.0e+00, 1.2e-15, 3.0e-16),
    "full_go2_cone": (2.3e-14, 1.9e-14, 8.2e-15, 2.6e-14, 2.7e-15, 1.1e-14, 1.6e-15, 6.1e-15, 1.1e-15, 2.5e-14, 1.1e-13, 6.1e-15, 1.1e-15, 4.0e-15, 3.1e-15),
    "full_go2_land": (2.1e-14, 1.9e-14, 9.0e-15, 1.0e-14, 2.3e-15, 4.5e-16, 0.0e+00, 4.9e-15, 1.2e-16, 4.1e-15, 4.8e-13, 4.9e-15, 1.2e-16, 2.0e-15, 5.4e-16),
    "full_go2_wide_cone": (3.3e-14, 2.6e-14, 8.4e-15, 9.9e-15, 2.5e-15, 0.0e+00, 0.0e+00, 5.7e-15, 0.0e+00, 5.1e-15, 2.4e-13, 5.7e-15, 0.0e+00, 1.7e-15, 3.5e-16),
    "talos_walk": (8.8e-14, 8.3e-14, 1.0e-14, 1.7e-14, 4.6e-15, 0.0e+00, 0.0e+00, 7.2e-15, 0.0e+00, 4.6e-14, 4.4e-15, 7.2e-15, 0.0e+00, 3.2e-15, 2.7e-14),
    "talos_tight": (8.2e-14, 8.0e-14, 1.1e-14, 1.3e-14, 3.9e-15, 4.2e-14, 4.2e-15, 8.3e-15, 2.9e-15, 4.1e-15, 6.6e-15, 8.3e-15, 2.9e-15, 2.2e-15, 5.1e-14),
    "talos_kino_cone": (2.3e-14, 1.6e-15, 1.1e-14, 1.3e-15, 8.3e-16, 1.4e-15, 0.0e+00, 6.8e-17, 6.3e-15, 1.0e-13, 2.2e-15, 6.8e-17, 6.3e-15, 9.9e-15, 1.3e-15),
    "talos_kino_nocone": (2.0e-14, 2.4e-15, 6.8e-15, 9.6e-16, 5.6e-16, 1.4e-15, 0.0e+00, 3.3e-16, 2.8e-15, 9.0e-15, 8.7e-15, 3.0e-16, 2.8e-15, 6.6e-15, 2.5e-15),
}

OBSERVED = """Observed, as multiples of the floor of the (scenario, field), the smallest and the largest over all fields and scenarios of a family (absolute gaps
in brackets; every gate but one is the 1e-11 minimum, the floors being 1e-17 .. 2e-13; r of full_go2_record: floor 6.2e-12, gate 6.2e-11):
  emulated bodies: Go2 kinodynamics 0.17 - 3.1 (<= 1.3e-13), Go2 full dynamics 0.44 - 4.3 (<= 7.8e-12, r of full_go2_record), Talos full dynamics
                   0.26 - 12 (<= 4.0e-13; the 12 is r of talos_tight, 7.9e-14 against a floor of 6.6e-15), Talos kinodynamics 0.36 - 6.3 (<= 5.8e-14)
  MI355X (-m gpu): Go2 kinodynamics 0.06 - 3.7 (<= 1.8e-13), Go2 full dynamics 0.33 - 2.6 (<= 9.6e-12, r of full_go2_record), Talos full dynamics
                   0.19 - 8.8 (<= 5.1e-13; r of talos_tight 5.8e-14), Talos kinodynamics 0.30 - 3.2 (<= 3.5e-14); fold identity 5e-16 .. 7e-16
No (scenario, field) lies above 100 x its floor on either tier.  Relative to their OWN size (printed, not gated) the cancelling sums show
f 1e-10 .. 1e-6, d 1e-13 .. 1e-9, q 1e-12 .. 3e-9, r 1e-12 .. 2e-9, lpd 1e-10 .. 2e-7, vpd 1e-13 .. 1e-9 on both tiers."""


def gate(scenario):
    """Gates of a scenario per field: 10 x its measured floor, 1e-11 where the floor is below 1e-12."""
    return {k: (1e-11 if f < 1e-12 else 10.0 * f) for k, f in zip(FIELDS, FLOORS[scenario])}


def _table():
    head = "  %-22s %s" % ("", " ".join("%7s" % k for k in FIELDS))
    rows = [head]
    for k, v in FLOORS.items():
        rows.append("  %-22s %s" % (k, " ".join("%7.1e" % x for x in v)))
    return "\n".join(rows)


# ---- partitions ----
def _dims(gm):
    kind = SC.kind_of(gm)
    assert kind in ("kino", "full", "kino6"), kind
    st = gm.ocp_handler.settings
    nv = gm.ndx // 2
    na = nv - 6
    nf = gm.ocp_handler.model_handler.getFeetNb()
    fs = int(st.get("force_size", 3))
    return kind, st, nv, na, nf, fs


def blocks(gm):
    """Row and column partition of a handle: dict(x, u, c) of lists of (name, index array); c in the oracle's row order."""
    kind, st, nv, na, nf, fs = _dims(gm)
    r = lambda a, n: np.arange(a, a + n)
    x = [("base lin", r(0, 3)), ("base ang", r(3, 3)), ("joints", r(6, na)), ("base lin vel", r(nv, 3)), ("base ang vel", r(nv + 3, 3)),
         ("joint vel", r(nv + 6, na))]
    if kind == "full":
        u = [("torques", r(0, na))]
        nc1 = (17 if fs == 6 else 5) if st.get("force_cone", False) else 0
        nl1 = (6 if fs == 6 else 4) if st.get("land_cstr", False) else 0
        c = [("torque box", r(0, na)), ("joint box", r(na, na))]
        c += [("cone foot %d" % f, r(2 * na + nc1 * f, nc1)) for f in range(nf) if nc1]
        c += [("land foot %d" % f, r(2 * na + nc1 * nf + nl1 * f, nl1)) for f in range(nf) if nl1]
        assert 2 * na + (nc1 + nl1) * nf == gm.nc, (gm.nc, na, nc1, nl1)
    else:
        what = "wrench" if fs == 6 else "force"
        u = [("%s foot %d" % (what, f), r(fs * f, fs)) for f in range(nf)] + [("joint part", r(fs * nf, na))]
        c = [("joint box", r(0, na))] + [("frame vel foot %d" % f, r(na + fs * f, fs)) for f in range(nf)]
        if kind == "kino6" and st.get("force_cone", False):
            c += [("cone foot %d" % f, r(na + 6 * nf + 17 * f, 17)) for f in range(nf)]
    return dict(x=x, u=u, c=c)


def n_rows(gm):
    """Constraint rows of the oracle's layout."""
    return int(sum(len(i) for _, i in blocks(gm)["c"]))


# ---- the synced step ----
def synced_step(gm, oms, X):
    """One control step with every oracle of `oms` evaluated at the product's iterate (module docstring).  Leaves on each oracle and on the
    handle the synced iterate AFTER the recede (`kc_iterate`: xs, us, vs, lams), which the scales and the lpd / vpd references need.  Returns
    the next measured state, the product's plan."""
    assert int(gm.settings["max_iters"]) == 1
    xs, us, vs, lams = gm.xs, gm.us, gm.vs, gm.lams
    X = np.ascontiguousarray(X, float)
    it = dict(
        xs=np.concatenate([X[:, None, :], xs[:, 2:], xs[:, -1:]], 1), us=np.concatenate([us[:, 1:], us[:, -1:]], 1),
        vs=np.concatenate([vs[:, 1:], np.zeros_like(vs[:, -1:])], 1),
        lams=np.concatenate([lams[:, :1], lams[:, 2:], np.zeros_like(lams[:, -1:])], 1))
    for om in oms:
        om.set_iterate(xs, us, vs, lams)
        om.iterate(X)
        om.kc_iterate = it
    gm.iterate(X)
    gm.kc_iterate = it
    return gm.xs[:, 1, :].copy()


# ---- knots in the oracle's layout ----
def oracle_knot(om, b, t):
    """The oracle's knot (b, t) with the references of lpd and vpd and the activity pattern."""
    ko = om.knot(b, t)
    mu = float(om.mu)
    it = om.kc_iterate
    act = (np.abs(ko["C"]).sum(1) + np.abs(ko["D"]).sum(1)) != 0.0
    ko["act"] = act
    ko["lpd"] = it["lams"][b, t + 1] + 2.0 * ko["f"] / mu
    ko["vpd"] = np.where(act, it["vs"][b, t] + 2.0 * ko["d"] / mu, 0.0)
    return ko


def device_knot(gm, b, t, kg=None):
    """debug_lq(b, t) in the oracle's layout (module docstring); Talos kinodynamics: Q and q unfolded, the folded ones under Qf, qf, the fold
    terms under Qfold, qfold."""
    kind, st, nv, na, nf, fs = _dims(gm)
    kg = gm.debug_lq(b, t) if kg is None else kg
    ndx, nu = gm.ndx, gm.nu
    mu = float(gm.settings["mu_init"])
    out = {k: kg[k].copy() for k in ("A", "B", "Q", "S", "R", "q", "r", "f", "lpd")}
    if kind == "kino":
        out.update(C=kg["C"].copy(), D=np.zeros((gm.nc, nu)), d=kg["d"].copy(), vpd=kg["vpd"].copy())
        out["act"] = np.abs(kg["C"]).sum(1) != 0.0
        return out
    act = kg["act"]
    assert np.all((act == 0.0) | (act == 1.0)), ("activity flags must be 0 or 1", b, t)
    ncd = kg["Cd"].shape[0]
    if kind == "full":
        nc = gm.nc
        Cm, D = np.zeros((nc, ndx)), np.zeros((nc, nu))
        for i in range(nu):  # torque box: unit rows on u
            D[i, i] = act[i]
        for i in range(na):  # joint box: unit rows on the joint positions
            Cm[nu + i, 6 + i] = act[nu + i]
        Cm[2 * nu:] = kg["Cd"]
        D[2 * nu:] = kg["Dd"]
        assert not kg["Cd"][act[2 * nu:] == 0.0].any() and not kg["Dd"][act[2 * nu:] == 0.0].any(), ("an inactive dense row must be a zero row", b, t)
        out.update(C=Cm, D=D, d=kg["d"].copy(), vpd=kg["vpd"].copy(), act=act != 0.0)
        return out
    # Talos kinodynamics: device rows [control box (absent) | joint box | cone | velocity] -> oracle rows [joint box | velocity | cone]
    nvel = kg["Cv"].shape[0]
    assert not act[:nu].any() and not kg["d"][:nu].any() and not kg["vpd"][:nu].any(), ("the absent control-box rows must stay empty", b, t)
    cone = bool(st.get("force_cone", False))
    perm = np.r_[np.arange(nu, nu + na), np.arange(nu + na + ncd, nu + na + ncd + nvel), np.arange(nu + na, nu + na + ncd) if cone else []].astype(int)
    if not cone:
        assert not act[nu + na:nu + na + ncd].any() and not kg["Dd"].any(), ("force_cone = False: no cone row may be active", b, t)
    assert not kg["Cd"].any(), ("the wrench-cone rows of the kinodynamics variant act on u only", b, t)
    assert not kg["Cd"][act[nu + na:nu + na + ncd] == 0.0].any() and not kg["Dd"][act[nu + na:nu + na + ncd] == 0.0].any(), ("inactive cone row", b, t)
    Cv = kg["Cv"]
    nc = len(perm)
    Cm, D = np.zeros((nc, ndx)), np.zeros((nc, nu))
    for i in range(na):
        Cm[i, 6 + i] = act[nu + i]
    Cm[na:na + nvel] = Cv
    if cone:
        D[na + nvel:] = kg["Dd"]
    d = kg["d"][perm]
    Qfold, qfold = Cv.T @ Cv / mu, Cv.T @ d[na:na + nvel] / mu
    a = act[perm] != 0.0
    a[na:na + nvel] = np.abs(Cv).sum(1) != 0.0  # (equality rows of the feet in contact: present where the row is)
    if t == 0 and not kg["q"].any():
        qfold = np.zeros(ndx)  # (x_0 is fixed: both sides hold q_0 at exactly zero, the kernel folds nothing into it)
    out.update(C=Cm, D=D, d=d, vpd=kg["vpd"][perm], act=a, Qf=kg["Q"].copy(), qf=kg["q"].copy(), Qfold=Qfold, qfold=qfold,
               Q=kg["Q"] - Qfold, q=kg["q"] - qfold)
    return out


def scales(ko, it, b, t, nq):
    """Size of the terms the cancelling sums of stage t are differences of (module docstring), from the oracle's knot and the synced iterate."""
    xs, us, vs, lams = it["xs"][b], it["us"][b], it["vs"][b], it["lams"][b]
    nv = ko["A"].shape[0] // 2
    m = lambda a: float(np.abs(a).max()) if np.size(a) else 0.0
    mu = ko["mu"]
    s = dict(f=m(xs[t + 1]), d=max(m(ko["D"] @ us[t]), m(ko["C"][:, nv:] @ xs[t, nq:]), m(ko["C"][:, 6:nv] @ xs[t, 7:nq])),
             q=max(m(lams[t]), m(ko["A"].T @ lams[t + 1]), m(ko["C"].T @ vs[t])),
             r=max(m(ko["B"].T @ lams[t + 1]), m(ko["D"].T @ vs[t]), m(ko["R"] @ us[t])))
    s["lpd"], s["vpd"] = 2.0 * s["f"] / mu, 2.0 * s["d"] / mu
    return s


RESIDUE = 2.0 ** -40  # (9e-13: 4096 eps)


def _gap(a, b, what, scale=0.0, field_max=0.0, strict=True):
    """max|a - b| / max(max|b|, scale) of one block.  A block the oracle holds at exactly zero must be exactly zero (`strict`: the product
    against the oracle; between the two oracles of `floors` it must be a rounding residue).  A block of a matrix that is a ROUNDING RESIDUE in
    the oracle -- max|b| <= RESIDUE x the largest entry of the whole field at that stage: a structural zero that the oracle forms as a
    cancelling difference, 1e-17 in A next to its identity, 1e-33 in Q next to 1e5 -- has no size of its own to be relative to: it must be
    a residue on the other side too and counts as gap 0.  Every block above 9e-13 of the field's largest entry stays unfloored."""
    if not b.size:
        return 0.0
    den = float(np.abs(b).max())
    if den == 0.0 and scale == 0.0 and strict:
        assert np.all(a == 0.0), what + ("the oracle's block is exactly zero, the compared one is not", float(np.abs(a).max()))
        return 0.0
    if den <= RESIDUE * field_max:
        if float(np.abs(a).max()) <= RESIDUE * field_max:
            return 0.0
        assert scale > 0.0, what + ("the oracle's block is a rounding residue, the compared one is not", float(np.abs(a).max()), den, field_max)
    return float(np.abs(a - b).max() / max(den, scale))


def _block_list(part):
    x, u, c = part["x"], part["u"], part["c"]
    rows = dict(A=x, B=x, Q=x, S=x, R=u, C=c, D=c)
    cols = dict(A=x, B=u, Q=x, S=u, R=u, C=x, D=u)
    vpart = dict(f=x, q=x, lpd=x, r=u, d=c, vpd=c)
    return rows, cols, vpart


def held_at_zero(kos, part):
    """The blocks the oracle HOLDS at exactly zero: exactly zero at every stage of the instance.  (A block that is exactly zero at one stage and
    1e-33 at the next -- Q of base lin x base lin vel, a cancelling sum that sometimes cancels exactly -- is not held at zero: it is a
    rounding residue, see _gap.)  {field: set of block names}."""
    rows, cols, vpart = _block_list(part)
    out = {}
    for k in MATS:
        out[k] = {rn + " x " + cn for rn, ri in rows[k] for cn, ci in cols[k] if not any(ko[k][np.ix_(ri, ci)].any() for ko in kos)}
    for k in VECS:
        out[k] = {rn for rn, ri in vpart[k] if not any(ko[k][ri].any() for ko in kos)}
    return out


def knot_gaps(kg, ko, part, sc, what=(), strict=None):
    """Per-block gaps of one knot, both in the oracle's layout: {field: {block: gap}}, and the raw figures of the scaled vectors
    {field: {block: gap relative to the block's own size}}.  Asserts the activity pattern and the exactly-zero blocks."""
    assert np.array_equal(kg["act"], ko["act"]), what + ("activity", np.flatnonzero(kg["act"] != ko["act"]))
    rows, cols, vpart = _block_list(part)
    strict = {} if strict is None else strict  # {field: blocks that must be exactly zero}: held_at_zero of the oracle's knots
    gaps, raw = {}, {}
    for k in MATS:
        g = gaps.setdefault(k, {})
        fmax = float(np.abs(ko[k]).max()) if ko[k].size else 0.0
        for rn, ri in rows[k]:
            for cn, ci in cols[k]:
                blk = np.ix_(ri, ci)
                scale = float(np.abs(kg["Qfold"][blk]).max()) if (k == "Q" and "Qfold" in kg) else 0.0
                g[rn + " x " + cn] = _gap(kg[k][blk], ko[k][blk], what + (k, rn + " x " + cn), scale, fmax, rn + " x " + cn in strict.get(k, ()))
    for k in VECS:
        g, rw = gaps.setdefault(k, {}), raw.setdefault(k, {})
        for rn, ri in vpart[k]:
            scale = sc[k]
            if k == "q" and "qfold" in kg:
                scale = max(scale, float(np.abs(kg["qfold"][ri]).max()))
            g[rn] = _gap(kg[k][ri], ko[k][ri], what + (k, rn), scale, float(np.abs(ko[k]).max()) if ko[k].size else 0.0, rn in strict.get(k, ()))
            den = np.abs(ko[k][ri]).max() if len(ri) else 0.0
            rw[rn] = float(np.abs(kg[k][ri] - ko[k][ri]).max() / den) if den > 0 else 0.0
    return gaps, raw


def term_gaps(QN, qN, oQ, oq, part, lamH, what=(), strict=None):
    x = part["x"]
    fmax = float(np.abs(oQ).max())
    gaps, raw = dict(QN={}, qN={}), dict(qN={})
    for rn, ri in x:
        for cn, ci in x:
            blk = np.ix_(ri, ci)
            gaps["QN"][rn + " x " + cn] = _gap(QN[blk], oQ[blk], what + ("QN", rn + " x " + cn), 0.0, fmax,
                                                  strict is not None and rn + " x " + cn in strict["Q"] and not oQ[blk].any())
        gaps["qN"][rn] = _gap(qN[ri], oq[ri], what + ("qN", rn), lamH, float(np.abs(oq).max()), False)
        den = np.abs(oq[ri]).max()
        raw["qN"][rn] = float(np.abs(qN[ri] - oq[ri]).max() / den) if den > 0 else 0.0
    return gaps, raw


def _oracle_side(om, b, H, nq):
    kos = []
    for t in range(H):
        ko = oracle_knot(om, b, t)
        ko["mu"] = float(om.mu)
        kos.append(ko)
    oQ, oq, _ = om.terminal_knot(b)
    return kos, oQ, oq


def device_outputs(gm, insts=None):
    """What `check` compares: {(b, t): knot in the oracle's layout, (b, "N"): (QN, qN)}."""
    out = {}
    for b in range(gm.B) if insts is None else insts:
        for t in range(gm.H):
            out[(b, t)] = device_knot(gm, b, t)
        out[(b, "N")] = gm.debug_terminal(b)
    return out


def oracle_outputs(om, H, insts):
    """The same of an oracle (the twin of `floors`)."""
    out = {}
    for b in insts:
        for t in range(H):
            ko = oracle_knot(om, b, t)
            out[(b, t)] = ko
        oQ, oq, _ = om.terminal_knot(b)
        out[(b, "N")] = (oQ, oq)
    return out


def _worst(gm, om, outputs, insts, on_gap=None, strict=True):
    """Largest gap per field over all stages and blocks of the instances, with where it sits; `on_gap(field, b, stage, block, gap)` is called for
    every gap (the gate of `check`)."""
    part = blocks(gm)
    nq = gm.nx - gm.ndx // 2
    worst = {k: (0.0, None) for k in FIELDS}
    rawmax = {k: 0.0 for k in SCALED}
    it = om.kc_iterate
    for b in insts:
        kos, oQ, oq = _oracle_side(om, b, gm.H, nq)
        per_stage = []
        zero = held_at_zero(kos, part) if strict else None
        for t in range(gm.H):
            what = ("instance %d" % b, "stage %d" % t)
            per_stage.append(("stage %d" % t,) + knot_gaps(outputs[(b, t)], kos[t], part, scales(kos[t], it, b, t, nq), what, zero))
        QN, qN = outputs[(b, "N")]
        per_stage.append(("terminal node",) + term_gaps(QN, qN, oQ, oq, part, float(np.abs(it["lams"][b, -1]).max()), ("instance %d" % b, "terminal node"), zero))
        for stage, gaps, raw in per_stage:
            for k, g in gaps.items():
                for blk, v in g.items():
                    if on_gap is not None:
                        on_gap(k, b, stage, blk, v)
                    if v > worst[k][0]:
                        worst[k] = (v, (b, stage, blk))
            for k, g in raw.items():
                rawmax[k] = max(rawmax[k], max(g.values()) if g else 0.0)
    return worst, rawmax


def check_fold(gm, om, outputs, insts):
    """Talos kinodynamics: the device's folded Q against the oracle's Q + Cv^T Cv / mu formed from the oracle's velocity rows, relative to
    max|Q folded| (the bar of test_talos_kinodynamics.py: 1e-12)."""
    kind, st, nv, na, nf, fs = _dims(gm)
    if kind != "kino6":
        return 0.0
    mu = float(om.mu)
    worst = 0.0
    for b in insts:
        for t in range(gm.H):
            kg, ko = outputs[(b, t)], om.knot(b, t)
            Cvo = ko["C"][na:na + 6 * nf]
            e = np.abs(kg["Qf"] - ko["Q"] - Cvo.T @ Cvo / mu).max() / np.abs(kg["Qf"]).max()
            worst = max(worst, e)
            assert e < 1e-12, ("fold identity", "instance %d" % b, "stage %d" % t, e)
    return worst


def check(gm, om, scenario, insts=None, label="", outputs=None):
    """Every field of every stage of the named (or all) instances, and the terminal node, against the oracle's at the synced iterate, per
    block, gated by gate(scenario).  Prints the observed gap of every field next to its gate and as a multiple of its floor.  `outputs`:
    compare these in place of the handle's (device_outputs; the self-test hands in perturbed copies)."""
    insts = list(range(gm.B)) if insts is None else list(insts)
    out = device_outputs(gm, insts) if outputs is None else outputs
    gates = gate(scenario)
    fails = []

    def on_gap(k, b, stage, blk, v):
        if not v < gates[k]:
            fails.append((scenario, label, "instance %d" % b, k, stage, blk, v, gates[k]))

    worst, raw = _worst(gm, om, out, insts, on_gap)
    fold = check_fold(gm, om, out, insts)
    fl = dict(zip(FIELDS, FLOORS[scenario]))
    print("knot_check %s%s: gap | gate | multiple of the floor, per field: %s%s | raw gaps of the cancelling sums (not gated) %s"
          % (scenario, label, "  ".join("%s %.1e|%.0e|%s" % (k, worst[k][0], gates[k], ("%.2g" % (worst[k][0] / fl[k])) if fl[k] > 0 else "-") for k in FIELDS),
             (" | fold identity %.1e (bar 1e-12)" % fold) if fold else "", " ".join("%s %.1e" % kv for kv in raw.items())))
    if fails:
        fails.sort(key=lambda f: -f[6] / f[7])
        raise AssertionError(fails[0], "%d gaps above their gates" % len(fails), fails[1:6])
    return worst


def floors(gm, om, om2, insts=None):
    """Row of FLOORS: the largest per-stage, per-block gap of every field between the oracle `om` and its reframed twin `om2`, both at the
    synced iterate of `gm`.  Prints the row and where each floor sits."""
    insts = list(range(gm.B)) if insts is None else list(insts)
    worst, raw = _worst(gm, om, oracle_outputs(om2, gm.H, insts), insts, strict=False)
    row = tuple(worst[k][0] for k in FIELDS)
    print("knot_check.floors: (%s)" % ", ".join("%.1e" % v for v in row))
    print("   where: " + "; ".join("%s %s" % (k, worst[k][1]) for k in FIELDS if worst[k][1] is not None))
    return row


def active_rows(gm, insts=None):
    """Active rows over all knots of the instances, by family name of blocks(gm)['c']."""
    part = blocks(gm)["c"]
    n = {name.split(" foot")[0]: 0 for name, _ in part}
    for b in range(gm.B) if insts is None else insts:
        for t in range(gm.H):
            act = device_knot(gm, b, t)["act"]
            for name, idx in part:
                n[name.split(" foot")[0]] += int(act[idx].sum())
    return n


__doc__ = __doc__ % dict(table=_table(), observed=OBSERVED)
