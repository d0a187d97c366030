"""Sweep-level checker: the Riccati sweeps of a product handle against two plain FP64 solves of the handle's own LQ problem.
TEST INFRASTRUCTURE.

Every schedule of the stage engines ends a control step with derivative pass -> sweeps -> line search, so after iterate() the knots
(debug_lq), the terminal block (debug_terminal), the Newton step (debug_steps) and the gains (Ks) belong to one LQ problem.  `lq_inputs`
turns the device knots of one instance into (Q, S, R, q, r, A, B, f, C, D, d, QN, qN, mu) in the convention of oracle_lib.riccati (a row of
[C D] is zero where the row is inactive, oracle/orc_proxddp.hpp step 4); `check` solves that with

  * oracle_lib.riccati (orc_riccati: the serial proximal Riccati recursion), the reference the device is gated against, and
  * `dense_kkt` (the whole KKT system, LU), which also gives gains: K_t = d du_t / d dx_t of the tail problem t .. H-1 (`kkt_gain`),

and compares dxs, dus and Ks of ALL stages.  The norm is per quantity and per stage, max|a - b| / max|b| over that stage's block (`stage_gaps`);
it is not floored, so a wrong small gain row cannot hide behind the force columns.  A block the reference holds at exactly zero (dxs[0]) must be
exactly zero on the device.

Engine kinds
  * Go2 kinodynamics (KinoEngine): the fields as returned, D = 0.  With force_cone / land_cstr the extra rows are NOT in C (they live in
    separate buffers of the structured sweep): the checker REFUSES such a handle -- it is restricted to the settings of record, weight /
    limit overrides and kinematics_limits.
  * full dynamics (FullEngine, Go2 and Talos): C and D are built from the activity flags `act` -- torque-box rows are unit rows of D,
    joint-box rows are unit rows of C on dx[6 + i] (smpc_full_model.h) -- followed by the dense rows Cd | Dd (cone rows, land rows).
  * Talos kinodynamics (FullDims<..., KIN = 1>): as full dynamics; the frame-velocity rows Cv are already folded into Q / q by the stage
    kernel, so they do not enter C.  `lq_inputs(..., unfold_vel=True)` takes Cv^T Cv / mu and Cv^T d / mu out of Q / q again and hands the
    rows to the reference explicitly; `check_vel_fold` asserts that both forms give the same step (both sides on the CPU).
  * Go2 centroidal with point feet (the kernel pipeline of smpc_cent_split.h: cent_bwd_body, cent_fwd_body): debug_lq unpacks the stage record
    through CentRec's own maps; C = 0, D = the cone rows Dd (an inactive row is a zero row).  The momentum blocks of Q are not in the record:
    the accessor rebuilds them as the backward sweep does, w_lm | w_am + preg I, with the preg the line search parked.
  * Talos centroidal with 6-D feet (cent6_deriv_body -> riccati_dense_body<DD> -> cent6_forward_body): the dense knot cut to the nine real
    state rows and columns (the three pad rows / columns are exactly zero and decoupled: tests/test_centroidal_knots.py), C = Cd, D = Dd.
  For both centroidal kinds `check` also compares the multiplier steps dvs and dlams of all stages with oracle_lib.riccati's ([Z z] has no
  other read-out), and checks Ks at EVERY stage with `kkt_gain` (ndx = 9: cheap).

Tolerances are measured, not chosen.  FLOOR is the largest per-stage gap between the two CPU references on the device's knots (emulated
kernel bodies, measured at the parent of the commit that added this file, c443493) -- what two correct FP64 solvers disagree by at
mu = 1e-8.  Neither is the code under test.  GATE = 10 x FLOOR (summation order of a blocked matrix-core sweep), 1e-11 where the floor is
below 1e-12.  A device gap that needs more than 100 x its floor is a finding to explain, not a number to widen.

Ks floors: `kkt_gain` at EVERY stage for the Go2 kinodynamics scenarios; for the dense engines at the stages 0, H // 2 and H - 1 only (their
device gaps lie below even those).  `check` recomputes and prints the three-stage value in every run: it is NOT the floor of the table for Go2
kinodynamics -- there the largest reference gap sits at a stage in between (kino_record_k1 at control step 14: three-stage value 4.9e-10,
all-stage floor 6.8e-9, device 3.0e-8, i.e. 4.4 x the floor and 60 x the printed three-stage value).

talos_kino_cone: the KKT LU is the weak side of this floor.  Its matrix carries Cv^T Cv / mu = 1e8 in Q and the two references differ by
1e-7 .. 1e-6, while the folded and the unfolded Riccati solves agree to 3e-10 .. 9e-10 (`check_vel_fold`, printed) and the device is 1e-9 ..
3e-9 from the Riccati reference.  The gates below follow the rule as it stands and are three decades wide of the observed gap: in this
scenario a gain off by 1e-6 passes; every run prints the observed gaps next to the gates.

Observed on the emulated bodies at that commit, as multiples of the floor: Go2 kinodynamics dxs 0.4 - 5.7, dus 0.4 - 3.3, Ks 1.3 - 5.1; dense
engines <= 1.8, Talos kinodynamics 0.01 - 0.2.  On an MI355X (same commit, -m gpu): Go2 kinodynamics dxs 0.4 - 3.6,
dus 0.3 - 4.8, Ks 1.5 - 4.4; dense engines <= 2.2; Talos kinodynamics 0.01 - 0.2; residual of the rebuilt rows over |dx+| 6e-16 .. 2e-14.

Centroidal scenarios (floors measured on the emulated bodies at the commit that added them; absolute device gaps 1e-15 .. 2e-13 throughout, the
floors themselves 1e-15 .. 4e-10, so most gates sit at the 1e-11 minimum).  Observed as multiples of the floor, emulated bodies: point feet
dxs 0.001 - 1.3, dus 0.0001 - 0.97, Ks 0.014 - 0.85, dvs <= 0.41, dlams 0.014 - 1.8; 6-D feet <= 0.26.  On an MI355X (-m gpu): point feet dxs
0.002 - 1.3, dus 0.0004 - 2.1, Ks 0.04 - 0.75, dvs 0.04 - 0.64, dlams 0.04 - 1.8 (the figures above 1 belong to cent_h2 and
cent_cones_backtrack, whose floors are 1e-15 .. 1e-13); 6-D feet <= 0.13 except dvs of talos_cent_tight, 2.4 (2.3e-7 against a gate of 9.3e-7).
talos_cent_tight dvs: dnu = (C dx + D du + d) / mu with mu = 1e-8 is a cancelling sum divided by mu, so both references (floor 9.3e-8 on the
emulated knots, 1.3e-8 on the device's) and the device carry eps |D du| / (mu |dnu|); the rule stands as it is and every run prints the
observed gap next to the gate.  cent_two_parts runs B = 128 as two parts of 64 (SMPC_CENT_PARTS=2: the engine splits by itself only from
B = 1024 on) and checks the instances 0, 63, 64, 127.

FLOORS / GATES (per scenario; dxs, dus, Ks -- centroidal scenarios: dxs, dus, Ks, dvs, dlams)
%(table)s
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle_lib as O

# scenario -> (floor dxs, floor dus, floor Ks[, floor dvs, floor dlams]): see the module docstring.  Filled from tools of this file: `floors(gm)` prints a row.
FLOORS = {
    "kino_record_k1": (9.2e-9, 3.2e-8, 6.8e-9),
    "kino_record_k1_dense": (9.2e-9, 3.2e-8, 6.8e-9),  # (the same knots to rounding: the floor of kino_record_k1)
    "kino_record_k3": (6.9e-9, 4.2e-8, 8.4e-9),
    "kino_h3": (1.9e-9, 1.9e-9, 3.5e-10),
    "kino_h65": (2.9e-9, 2.3e-8, 1.4e-9),
    "kino_dense_w": (4.0e-9, 1.7e-8, 1.4e-9),
    "kino_tight_limits": (7.8e-10, 1.8e-9, 7.3e-10),
    "kino_backtrack": (2.2e-8, 1.1e-7, 1.3e-9),
    "full_go2_record": (1.1e-12, 6.1e-11, 9.0e-11),
    "full_go2_cone": (1.3e-12, 1.6e-11, 1.6e-11),
    "talos_walk": (8.4e-14, 9.8e-13, 4.1e-13),
    "talos_tight": (3.0e-13, 3.5e-13, 2.7e-13),
    "talos_kino_cone": (1.3e-7, 1.4e-6, 1.3e-8),
    "talos_walk_h100": (2.0e-12, 1.2e-12, 8.2e-13),
    # centroidal: (dxs, dus, Ks at every stage, dvs, dlams), SC.floors on the emulated bodies (the largest of the checked control steps)
    "cent_record_k1": (2.4e-12, 3.8e-12, 5.5e-13, 1.0e-13, 1.4e-13),
    "cent_record_k3": (4.2e-12, 1.5e-10, 2.7e-13, 3.1e-13, 3.3e-13),
    "cent_cones_backtrack": (7.2e-14, 3.9e-13, 8.4e-14, 5.4e-13, 1.3e-13),
    "cent_h2": (1.3e-15, 5.0e-15, 4.9e-15, 0.0, 3.2e-15),
    "cent_h63": (4.8e-12, 1.8e-11, 4.6e-14, 0.0, 1.1e-12),
    "cent_h65": (1.4e-12, 2.1e-11, 4.3e-14, 0.0, 6.1e-14),
    "cent_dense_w": (3.2e-13, 7.4e-13, 1.4e-14, 0.0, 3.6e-13),
    "cent_two_parts": (5.2e-14, 1.5e-13, 9.5e-14, 0.0, 3.0e-13),  # (instances 0, 63, 64, 127)
    "talos_cent_walk": (1.3e-12, 1.6e-11, 6.3e-14, 0.0, 1.7e-12),
    "talos_cent_tight": (5.1e-13, 8.3e-13, 3.3e-14, 9.3e-8, 1.4e-13),
    "talos_cent_h100": (6.7e-11, 4.1e-10, 8.9e-12, 0.0, 3.1e-11),
}


def gate(scenario):
    """(dxs, dus, Ks[, dvs, dlams]) gates of a scenario: 10 x its measured floor, 1e-11 where the floor is below 1e-12."""
    return tuple(1e-11 if f < 1e-12 else 10.0 * f for f in FLOORS[scenario])


def _table():
    e = lambda v: " ".join("%8.1e" % x for x in v)
    rows = ["  %-34s floor %s   gate %s" % (k, e(v), e(gate(k))) for k, v in FLOORS.items()]
    return "\n".join(rows)


def kkt_system(Q, S_, R, q, r, A, B, f, Cm, D, d, QN, qN, mu, sparse=False):
    """KKT matrix and right-hand side of the whole LQ problem (dx_0 = 0), unknowns per stage [du_t | dnu_t | dlam_{t+1} | dx_{t+1}]."""
    H, ndx, nu = B.shape
    nc = Cm.shape[1]
    per = nu + nc + 2 * ndx
    N = H * per
    K = sp.lil_matrix((N, N)) if sparse else np.zeros((N, N))
    rhs = np.zeros(N)
    iu = lambda t: t * per
    iv = lambda t: t * per + nu
    il = lambda t: t * per + nu + nc
    ix = lambda t: t * per + nu + nc + ndx
    for t in range(H):
        r0 = iu(t)
        K[r0:r0 + nu, iu(t):iu(t) + nu] = R[t]
        K[r0:r0 + nu, il(t):il(t) + ndx] = B[t].T
        K[r0:r0 + nu, iv(t):iv(t) + nc] = D[t].T
        if t > 0:
            K[r0:r0 + nu, ix(t - 1):ix(t - 1) + ndx] = S_[t].T
        rhs[r0:r0 + nu] = -r[t]
        r0 = iv(t)
        K[r0:r0 + nc, iv(t):iv(t) + nc] = -mu * np.eye(nc)
        K[r0:r0 + nc, iu(t):iu(t) + nu] = D[t]
        if t > 0:
            K[r0:r0 + nc, ix(t - 1):ix(t - 1) + ndx] = Cm[t]
        rhs[r0:r0 + nc] = -d[t]
        r0 = il(t)
        K[r0:r0 + ndx, iu(t):iu(t) + nu] = B[t]
        K[r0:r0 + ndx, ix(t):ix(t) + ndx] = -np.eye(ndx)
        K[r0:r0 + ndx, il(t):il(t) + ndx] = -mu * np.eye(ndx)
        if t > 0:
            K[r0:r0 + ndx, ix(t - 1):ix(t - 1) + ndx] = A[t]
        rhs[r0:r0 + ndx] = -f[t]
        r0 = ix(t)
        K[r0:r0 + ndx, il(t):il(t) + ndx] = -np.eye(ndx)
        if t + 1 < H:
            K[r0:r0 + ndx, ix(t):ix(t) + ndx] = Q[t + 1]
            K[r0:r0 + ndx, iu(t + 1):iu(t + 1) + nu] = S_[t + 1]
            K[r0:r0 + ndx, il(t + 1):il(t + 1) + ndx] = A[t + 1].T
            K[r0:r0 + ndx, iv(t + 1):iv(t + 1) + nc] = Cm[t + 1].T
            rhs[r0:r0 + ndx] = -q[t + 1]
        else:
            K[r0:r0 + ndx, ix(t):ix(t) + ndx] = QN
            rhs[r0:r0 + ndx] = -qN
    return K, rhs, (iu, iv, il, ix)


def dense_kkt(Q, S_, R, q, r, A, B, f, Cm, D, d, QN, qN, mu, sparse=False):
    """Newton step of the LQ problem from one LU solve of its KKT system: (dx, du, dnu, dlam).  `sparse`: the same system through
    scipy.sparse (SuperLU) -- the long horizons, whose dense matrix would not fit."""
    H, ndx, nu = B.shape
    nc = Cm.shape[1]
    K, rhs, (iu, iv, il, ix) = kkt_system(Q, S_, R, q, r, A, B, f, Cm, D, d, QN, qN, mu, sparse)
    assert abs(K - K.T).max() < 1e-12
    z = spla.spsolve(K.tocsc(), rhs) if sparse else sla.solve(K, rhs)
    dx = np.stack([np.zeros(ndx)] + [z[ix(t):ix(t) + ndx] for t in range(H)])
    du = np.stack([z[iu(t):iu(t) + nu] for t in range(H)])
    dv = np.stack([z[iv(t):iv(t) + nc] for t in range(H)])
    dl = np.stack([np.zeros(ndx)] + [z[il(t):il(t) + ndx] for t in range(H)])
    return dx, du, dv, dl


def kkt_gain(lq, t):
    """Feedback gain K_t without a Riccati recursion: du_t of the tail problem t .. H-1 is affine in dx_t; column j of K_t is the du_t of the
    homogeneous tail problem with dx_t = e_j (which enters through S_t^T dx_t, C_t dx_t and A_t dx_t)."""
    Q, S_, R, q, r, A, B, f, Cm, D, d, QN, qN, mu = lq
    H, ndx, nu = B.shape
    nc = Cm.shape[1]
    z = np.zeros
    n = H - t
    K, _, (iu, iv, il, ix) = kkt_system(Q[t:], S_[t:], R[t:], z((n, ndx)), z((n, nu)), A[t:], B[t:], z((n, ndx)), Cm[t:], D[t:], z((n, nc)),
                                        QN, z(ndx), mu, sparse=True)
    rhs = np.zeros((K.shape[0], ndx))
    rhs[iu(0):iu(0) + nu] = -S_[t].T
    rhs[iv(0):iv(0) + nc] = -Cm[t]
    rhs[il(0):il(0) + ndx] = -A[t]
    sol = spla.splu(K.tocsc()).solve(rhs)
    return sol[iu(0):iu(0) + nu]


def kind_of(gm):
    import simple_mpc

    ocp = gm.ocp_handler
    if isinstance(ocp, simple_mpc.FullDynamicsOCP):
        return "full"
    if isinstance(ocp, simple_mpc.KinodynamicsOCP):
        if int(ocp.settings.get("force_size", 3)) == 6:
            return "kino6"
        if ocp.settings.get("force_cone", False) or ocp.settings.get("land_cstr", False):
            raise ValueError("sweep_check: force_cone / land_cstr rows of the structured kinodynamics sweep are not in debug_lq's C")
        return "kino"
    if isinstance(ocp, simple_mpc.CentroidalOCP):
        return "cent6" if int(ocp.settings.get("force_size", 3)) == 6 else "cent"
    raise ValueError("sweep_check: the handle has no knot accessor")


def is_cent(gm):
    return kind_of(gm) in ("cent", "cent6")


def knots(gm, inst):
    return [gm.debug_lq(inst, t) for t in range(gm.H)]


def lq_inputs(gm, inst, kn=None, unfold_vel=False):
    """(Q, S, R, q, r, A, B, f, C, D, d, QN, qN, mu) of instance `inst` from the device knots, in oracle_lib.riccati's convention."""
    kind = kind_of(gm)
    kn = knots(gm, inst) if kn is None else kn
    H, ndx, nu, nc = gm.H, gm.ndx, gm.nu, gm.nc
    mu = float(gm.settings["mu_init"])
    st = lambda k: np.stack([g[k] for g in kn])
    Q, S_, R, q, r, A, B, f, d = (st(k) for k in ("Q", "S", "R", "q", "r", "A", "B", "f", "d"))
    Cm, D = np.zeros((H, nc, ndx)), np.zeros((H, nc, nu))
    if kind == "kino":
        Cm = st("C")
    elif kind in ("cent", "cent6"):
        for t, g in enumerate(kn):
            act = g["act"]
            assert np.all((act == 0.0) | (act == 1.0))
            assert not g["Dd"][act == 0.0].any(), ("an inactive cone row must be a zero row", t)
            D[t] = g["Dd"]
            if kind == "cent6":
                assert not g["Cd"][act == 0.0].any(), ("an inactive cone row must be a zero row", t)
                Cm[t] = g["Cd"]
    else:
        nvel = kn[0]["Cv"].shape[0] if kind == "kino6" else 0
        ncd = kn[0]["Cd"].shape[0]
        na = nc - nu - ncd - nvel
        for t, g in enumerate(kn):
            act = g["act"]
            assert np.all((act == 0.0) | (act == 1.0))
            for i in range(nu):  # torque box: unit rows on u (absent in the kinodynamics variant: flags stay 0)
                D[t, i, i] = act[i]
            for i in range(na):  # joint box: unit rows on the joint positions
                Cm[t, nu + i, 6 + i] = act[nu + i]
            Cm[t, nu + na:nu + na + ncd] = g["Cd"]
            D[t, nu + na:nu + na + ncd] = g["Dd"]
            if unfold_vel:
                Cv, dv = g["Cv"], g["d"][nu + na + ncd:]
                Cm[t, nu + na + ncd:] = Cv
                Q[t] = Q[t] - Cv.T @ Cv / mu
                q[t] = q[t] - Cv.T @ dv / mu
    QN, qN = gm.debug_terminal(inst)
    return Q, S_, R, q, r, A, B, f, Cm, D, d, QN, qN, mu


def stage_gaps(a, b):
    """Per-stage max|a - b| / max|b| of arrays [stages, ...] (b: the reference); a stage the reference holds at exactly zero must be exactly
    zero in `a` and counts as gap 0."""
    out = np.zeros(len(b))
    for t in range(len(b)):
        den = np.abs(b[t]).max()
        if den == 0.0:
            assert np.all(a[t] == 0.0), ("stage %d: the reference block is exactly zero, the compared one is not" % t, np.abs(a[t]).max())
            continue
        out[t] = np.abs(a[t] - b[t]).max() / den
    return out


def references(lq, k_stages=None, sparse=True, duals=False):
    """Both CPU solves: (dx, du, K, dlam) of oracle_lib.riccati and (dx, du, {t: K_t}) of the KKT system; with `duals` a third entry, the
    multiplier steps (dnu, dlam) of the Riccati solve and (dnu, dlam) of the KKT system."""
    rx, ru, rv, rl, rK = O.riccati(*lq)
    kx, ku, kv, kl = dense_kkt(*lq, sparse=sparse)
    H = ru.shape[0]
    ks = sorted({0, H // 2, H - 1}) if k_stages is None else k_stages
    kK = {t: kkt_gain(lq, t) for t in ks}
    if duals:
        return (rx, ru, rK, rl), (kx, ku, kK), ((rv, rl), (kv, kl))
    return (rx, ru, rK, rl), (kx, ku, kK)


def _ref_gaps(lq, cent, k_stages=None):
    """Both references of one instance and their mutual per-quantity gap (3 entries; 5 for the centroidal kinds)."""
    if not cent:
        ref, kkt = references(lq, k_stages)
        dual = None
    else:
        ref, kkt, dual = references(lq, range(lq[6].shape[0]) if k_stages is None else k_stages, duals=True)
    (rx, ru, rK, _), (kx, ku, kK) = ref, kkt
    g = [stage_gaps(kx, rx).max(), stage_gaps(ku, ru).max(), max(stage_gaps(kK[t][None], rK[t][None]).max() for t in kK)]
    if cent:
        (rv, rl), (kv, kl) = dual
        g += [stage_gaps(kv, rv).max(), stage_gaps(kl, rl).max()]
    return ref, kkt, dual, np.array(g)


def floors(gm, insts=None, k_stages=None):
    """Mutual gap of the two CPU references on the device's knots: (dxs, dus, Ks) -- centroidal kinds: (dxs, dus, Ks, dvs, dlams), Ks at every
    stage -- the largest stage of the largest instance."""
    cent = is_cent(gm)
    out = np.zeros(5 if cent else 3)
    for b in range(gm.B) if insts is None else insts:
        out = np.maximum(out, _ref_gaps(lq_inputs(gm, b), cent, k_stages)[3])
    return tuple(out)


def device_outputs(gm):
    """What `check` compares: the step and the gains of the last iteration (centroidal kinds: the multiplier steps too)."""
    dxs, dus = gm.debug_steps()
    out = dict(dxs=dxs, dus=dus, Ks=gm.Ks)
    if is_cent(gm):
        out["dvs"], out["dlams"] = gm.debug_dual_steps()
    return out


def check(gm, scenario, insts=None, label="", outputs=None, solved=None):
    """Device step and gains of every stage (centroidal kinds: and the multiplier steps dvs, dlams) against oracle_lib.riccati on the device's
    own knots, gated by gate(scenario); prints the observed gaps (and the floor of this run) so that a run records them.  Returns the
    per-instance (lq, reference, knots) for further checks.  `outputs`: compare these arrays in place of the handle's (device_outputs; the
    checker's self-test hands in perturbed copies); `solved`: the return value of an earlier call on the same state, whose knots and CPU
    solves are then reused."""
    cent = is_cent(gm)
    names = ("dxs", "dus", "Ks", "dvs", "dlams") if cent else ("dxs", "dus", "Ks")
    gates = gate(scenario)
    assert len(gates) == len(names), (scenario, "FLOORS row does not fit the handle kind")
    out = device_outputs(gm) if outputs is None else outputs
    res = []
    worst, floor = np.zeros(len(names)), np.zeros(len(names))
    for i, b in enumerate(range(gm.B) if insts is None else insts):
        if solved is None:
            kn = knots(gm, b)
            lq = lq_inputs(gm, b, kn)
            ref, kkt, dual, fl = _ref_gaps(lq, cent)
        else:
            sb, lq, ref, kn, _, kkt, dual, fl = solved[i]
            assert sb == b
        rx, ru, rK, rl = ref
        floor = np.maximum(floor, fl)
        assert np.all(rx[0] == 0.0)
        g = [stage_gaps(out["dxs"][b], rx), stage_gaps(out["dus"][b], ru), stage_gaps(out["Ks"][b], rK)]
        if cent:
            assert np.all(rl[0] == 0.0)
            g += [stage_gaps(out["dvs"][b], dual[0][0]), stage_gaps(out["dlams"][b], rl)]
        worst = np.maximum(worst, [x.max() for x in g])
        res.append((b, lq, ref, kn, g, kkt[:2], dual, fl))
    e = lambda v: " ".join("%.2e" % x for x in v)
    print("sweep_check %s%s: device vs riccati %s: %s | gates %s | reference floor of this run %s | multiples of the table's floor %s"
          % (scenario, label, " ".join(names), e(worst), e(gates), e(floor), " ".join(("%.2g" % (w / f)) if f > 0 else "-" for w, f in zip(worst, FLOORS[scenario]))))
    for r in res:
        b, g = r[0], r[4]
        for name, gap, lim in zip(names, g, gates):
            assert gap.max() < lim, (scenario, label, "instance %d" % b, name, "stage %d" % int(gap.argmax()), float(gap.max()), lim)
    return res


def rebuilt_rows(gm):
    """Rows of [A B] forward_full_body does not read but rebuilds (smpc_full_solver.h): the joint-position rows, and in the kinodynamics
    variant the joint-velocity rows."""
    kind = kind_of(gm)
    nv = gm.ndx // 2
    rows = list(range(6, nv))
    if kind == "kino6":
        rows += list(range(nv + 6, 2 * nv))
    assert kind != "kino"
    return np.array(rows)


def _residual_rows(lq, dx, du, rows):
    A, B, f = lq[5], lq[6], lq[7]
    return np.stack([(A[t] @ dx[t] + B[t] @ du[t] + f[t] - dx[t + 1])[rows] for t in range(len(du))])


def check_rebuilt_rows(gm, scenario, res, label=""):
    """The dynamics rows the forward sweep rebuilds instead of reading.  A change of the integrator or of the control layout that the backward
    sweep (dense rows of lq) and the forward sweep (rebuilt rows) do not share fails here by name.  Two assertions per instance:

    (a) the product: (A dx + B du) of those rows taken DENSE from debug_lq equals what forward_full_body forms instead -- joint positions
        dx_i + dt (A dx + B du)_{NV + i}, kinodynamics joint velocities dx_i + dt du_{NCM + i - 6} -- per stage to the dxs gate of the scenario;
    (b) the residual: A dx + B du + f - dx+ of those rows, formed from the dense rows of debug_lq and the device's step, equals mu dlam+ of the
        reference, per stage to the dxs gate of the scenario.  The residual is a difference of terms of the size of dx+ (it is mu |dlam+|, 1e-8
        to 1e-10 of them), so its error is measured against those terms: max|residual - mu dlam+| / max|dx+| over the rows of the stage.
        (Relative to mu |dlam+| itself the figure is bounded below by the rounding of dx+ to FP64, eps |dx+| / (mu |dlam+|): it is printed, not
        gated -- on the emulated bodies 8e-11 .. 2e-8 for the full-dynamics scenarios, 2e-10 for Talos kinodynamics.)"""
    gx = gate(scenario)[0]
    kind = kind_of(gm)
    rows = rebuilt_rows(gm)
    nv = gm.ndx // 2
    dt = float(gm.settings["timestep"])
    dxs, dus = gm.debug_steps()
    worst = np.zeros(3)
    for b, lq, (rx, ru, rK, rl), kn, *_ in res:
        A, B, mu = lq[5], lq[6], lq[13]
        for t in range(gm.H):
            dense = A[t] @ dxs[b, t] + B[t] @ dus[b, t]
            built = dxs[b, t, 6:nv] + dt * dense[nv + 6:]
            if kind == "kino6":
                ncm = gm.nu - (nv - 6)
                vel = dxs[b, t, nv + 6:] + dt * dus[b, t, ncm:]
                built = np.concatenate([dxs[b, t, 6:nv] + dt * vel, vel])
            den = np.abs(dense[rows]).max()
            gap = np.abs(built - dense[rows]).max() / den if den > 0 else float(np.abs(built).max() != 0)
            worst[0] = max(worst[0], gap)
            assert gap < gx, (scenario, label, "rebuilt product", "instance %d" % b, "stage %d" % t, gap, gx)
        ref = mu * rl[1:, rows]
        dev = _residual_rows(lq, dxs[b], dus[b], rows)
        worst[2] = max(worst[2], stage_gaps(dev, ref).max())
        for t in range(gm.H):
            den = np.abs(dxs[b, t + 1, rows]).max()
            gap = np.abs(dev[t] - ref[t]).max() / den if den > 0 else float(np.abs(dev[t] - ref[t]).max() != 0)
            worst[1] = max(worst[1], gap)
            assert gap < gx, (scenario, label, "residual of the rebuilt rows", "instance %d" % b, "stage %d" % t, gap, gx)
    print("sweep_check %s%s: rebuilt rows of [A B]: product vs dense %.2e | residual vs mu dlam+ over |dx+| %.2e | gate %.1e (both) | residual "
          "relative to mu |dlam+| %.2e (not gated)" % (scenario, label, worst[0], worst[1], gx, worst[2]))
    return worst


def check_vel_fold(gm, scenario, insts=None):
    """Talos kinodynamics: the stage kernel folds the frame-velocity rows (Q += Cv^T Cv / mu, q += Cv^T d / mu).  Taking the fold out of Q / q
    and giving the rows to the reference explicitly must give the same step.  Both sides are CPU solves of oracle_lib.riccati."""
    assert kind_of(gm) == "kino6"
    gx, gu, gK = gate(scenario)
    worst = np.zeros(3)
    for b in range(gm.B) if insts is None else insts:
        kn = knots(gm, b)
        assert max(np.abs(g["Cv"]).max() for g in kn) > 0.0
        fx, fu, _, _, fK = O.riccati(*lq_inputs(gm, b, kn))
        ex, eu, _, _, eK = O.riccati(*lq_inputs(gm, b, kn, unfold_vel=True))
        worst = np.maximum(worst, [stage_gaps(fx, ex).max(), stage_gaps(fu, eu).max(), stage_gaps(fK, eK).max()])
    print("sweep_check %s: folded vs explicit frame-velocity rows dxs %.2e dus %.2e Ks %.2e | gates %.1e %.1e %.1e" % (scenario, *worst, gx, gu, gK))
    assert worst[0] < gx and worst[1] < gu and worst[2] < gK, worst
    return worst


def active_rows(gm, insts=None):
    """Counts of active rows over all checked knots: (box rows, dense rows)."""
    kind = kind_of(gm)
    nbox = nden = 0
    for b in range(gm.B) if insts is None else insts:
        for g in knots(gm, b):
            if kind in ("cent", "cent6"):
                nden += int(g["act"].sum())
            elif kind == "kino":
                nbox += int((np.abs(g["C"][:12]).sum(1) > 0).sum())
            else:
                ncd = g["Cd"].shape[0]
                nvel = g["Cv"].shape[0] if "Cv" in g else 0
                na = gm.nc - gm.nu - ncd - nvel
                nbox += int(g["act"][:gm.nu + na].sum())
                nden += int(g["act"][gm.nu + na:gm.nu + na + ncd].sum())
    return nbox, nden


__doc__ = __doc__ % dict(table=_table())
