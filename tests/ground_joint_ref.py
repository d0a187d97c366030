"""The checker of the simulator's joint model: the ground step of tests/ground_ws_ref.py with effort limits, implicit joint
damping, armature and joint-limit stops, in numpy, the written model with its loops as written.  M, nle and the foot rows come from the
oracle through ground_env_ref.quantities.  Nothing of the product is imported except the table helpers.

The model.  A handle that has a ground gets a JOINT MODEL: five per-robot arrays [B][na], na = nv - 6, k the index of an actuated dof, and
a few scalars.  tau_max >= 0 (+inf allowed); damping d >= 0 finite; armature r_a >= 0 finite; q_lo <= q_hi (-inf / +inf allowed).  stops
is 0 or 1; activation (rad) > 0, 0 stands for 0.1; stop_erp in [0, 1], 0 stands for 0.2.  A null array pointer means tau_max = +inf,
d = 0, r_a = 0, limits from the robot table; per_robot says whether the given arrays are [na] (broadcast over the batch) or [B][na].
One step of robot i (everything not named is as in DESIGN 3.23 - 3.25):
  1 effort limit   tc_k = tau_k > tmax_k ? tmax_k : (tau_k < -tmax_k ? -tmax_k : tau_k), so a NaN passes through; tc is an output
                   (tau_applied).
  2 implicit damping and armature   Mh = M + diag(0_6, r_a + dt d); b = S tc - h - [0_6; d o v_joint] + Q_push; W = Mh^-1 [b | J^T];
                   v_f = v + dt W_0; G, c0, v+ = v_f + dt W_1 lambda and a = W_0 + W_1 lambda as before, with Mh in place of M.
  3 stop rows      only when stops = 1, in ascending k.  g- = q_k - q_lo_k, g+ = q_hi_k - q_k.  Joint k is a candidate iff
                   min(g-, g+) < activation; its side is lower (s = +1, g = g-) if g- <= g+, otherwise upper (s = -1, g = g+).  The
                   first NJ = 8 candidates get rows, appended after the contact rows; the rest are counted in `dropped`.  Row r of a
                   stop has J_r = s e_{6+k}; it shares W, G = J W_1 + compliance I and the sweeps' sums with the contact rows, so a stop
                   and a foot see each other.  c0_r = s v_f[6+k] + (g >= 0 ? g / dt : stop_erp g / dt).
  4 sweeps         each sweep runs the contact points of 3.23 in their order, their row sums over all rows, then the stop rows in
                   ascending order: lambda_r <- max(0, lambda_r - (c0_r + dt sum_j G_rj lambda_j) / (dt G_rr)).  Stop rows start from
                   exactly 0 every step; the warm buffer keeps its layout (contact rows only); rho_s takes the maximum over stop rows
                   too; the stopping rule, min_sweeps and the kernel's 1 / (dt G_rr) deviation are unchanged.
  5 outputs        per robot, besides those of 3.25: tau_applied [na]; stop_rows [8] (int32: +(k+1) lower, -(k+1) upper, 0 unused);
                   lam_stop [8]; dropped (int32)."""
import numpy as np

import ground_env_ref as ER
import ground_ws_ref as WR

NJ = 8
DEFAULT_ACTIVATION, DEFAULT_STOP_ERP = 0.1, 0.2


def clip(tau, tmax):
    out = np.array(tau, float)
    for k in range(len(out)):
        t = out[k]
        out[k] = tmax[k] if t > tmax[k] else (-tmax[k] if t < -tmax[k] else t)
    return out


def candidates(q_joint, q_lo, q_hi, activation):
    """([(k, s, g)] of the first NJ candidates in ascending k, dropped, margins): margins lists |min(g-, g+) - activation| and |g- - g+| of
    every joint with finite values, for the conditions on a test's inputs."""
    rows, dropped, margins = [], 0, []
    for k in range(len(q_joint)):
        gm, gp = q_joint[k] - q_lo[k], q_hi[k] - q_joint[k]
        if np.isfinite(min(gm, gp)):
            margins.append(abs(min(gm, gp) - activation))
        if np.isfinite(gm) and np.isfinite(gp):
            margins.append(abs(gm - gp))
        if min(gm, gp) < activation:
            if len(rows) < NJ:
                rows.append((k, 1, gm) if gm <= gp else (k, -1, gp))
            else:
                dropped += 1
    return rows, dropped, margins


def pgs(G, c0, dt, mu, npts, sweeps, lam0=None, tol=0.0, min_sweeps=1):
    """ground_ws_ref.pgs on the first 3 npts rows, their sums over all rows, then the stop rows (the rows behind them) in ascending order."""
    n = len(c0)
    lam = np.r_[WR.start_vector(lam0, 3 * npts), np.zeros(n - 3 * npts)]
    min_sweeps = max(1, min_sweeps)
    rhos = []
    for s in range(1, sweeps + 1):
        rho = 0.0
        for c in range(npts):
            rn = 3 * c + 2
            acc = 0.0
            for j in range(n):
                acc += G[rn, j] * lam[j]
            old = lam[rn]
            lam[rn] = max(0.0, old - (c0[rn] + dt * acc) / (dt * G[rn, rn]))
            rho = WR.sticky_max(rho, abs(lam[rn] - old) * (dt * G[rn, rn]))
            t = np.zeros(2)
            for i in range(2):
                ti = 3 * c + i
                acc = 0.0
                for j in range(n):
                    acc += G[ti, j] * lam[j]
                t[i] = lam[ti] - (c0[ti] + dt * acc) / (dt * G[ti, ti])
            nrm = np.sqrt(t[0] * t[0] + t[1] * t[1])
            if nrm > mu * lam[rn]:
                t = t * (mu * lam[rn] / nrm)
            if nrm == 0.0:
                t = np.zeros(2)
            for i in range(2):
                ti = 3 * c + i
                rho = WR.sticky_max(rho, abs(t[i] - lam[ti]) * (dt * G[ti, ti]))
            lam[3 * c], lam[3 * c + 1] = t[0], t[1]
        for r in range(3 * npts, n):
            acc = 0.0
            for j in range(n):
                acc += G[r, j] * lam[j]
            old = lam[r]
            lam[r] = max(0.0, old - (c0[r] + dt * acc) / (dt * G[r, r]))
            rho = WR.sticky_max(rho, abs(lam[r] - old) * (dt * G[r, r]))
        rhos.append(float(rho))
        if tol > 0.0 and s >= min_sweeps and rho <= tol:
            break
    return lam, len(rhos), rhos


def solve(rb, tab, x, tau, dt, plane, mu, push=None, joint=0, points=((0.0, 0.0, 0.0),), erp=0.2, compliance=1e-8, sweeps=30, lam0=None, tol=0.0,
          min_sweeps=1, tau_max=None, damping=None, armature=None, q_lo=None, q_hi=None, stops=0, activation=0.0, stop_erp=0.0):
    """One ground step of state x with its joint model: the dict of ground_ws_ref.solve (lam, lam_c: contact rows only) and tau_applied,
    stop_rows, lam_stop, dropped, margins."""
    nq, nv = rb.nq, rb.nv
    na = nv - 6
    tmax = np.full(na, np.inf) if tau_max is None else np.array(tau_max, float)
    d = np.zeros(na) if damping is None else np.array(damping, float)
    ra = np.zeros(na) if armature is None else np.array(armature, float)
    lo = np.array(tab.q_lo[:na]) if q_lo is None else np.array(q_lo, float)
    hi = np.array(tab.q_hi[:na]) if q_hi is None else np.array(q_hi, float)
    activation = activation if activation > 0.0 else DEFAULT_ACTIVATION
    stop_erp = stop_erp if stop_erp > 0.0 else DEFAULT_STOP_ERP
    tc = clip(tau, tmax)
    M, h, J, gap, Rc = ER.quantities(rb, tab, x, tc, plane, points)
    nr = J.shape[0]
    Q = np.zeros(nv) if push is None else ER.generalized_push(tab, x[:nq], joint, push[:3], push[3:6])
    Mh = M + np.diag(np.r_[np.zeros(6), ra + dt * d])
    b = np.r_[np.zeros(6), tc] - h - np.r_[np.zeros(6), d * x[nq + 6 :]] + Q
    rows, dropped, margins = candidates(x[7:nq], lo, hi, activation) if stops else ([], 0, [])
    Js = np.zeros((len(rows), nv))
    for r, (k, s, g) in enumerate(rows):
        Js[r, 6 + k] = s
    Ja = np.vstack([J, Js])
    Lc = np.linalg.cholesky(Mh)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, Ja.T]))
    vf = x[nq:] + dt * W[:, 0]
    nrt = nr + len(rows)
    G = Ja @ W[:, 1:] + compliance * np.eye(nrt)
    gapterm = np.zeros(nrt)
    for c in range(nr // 3):
        gapterm[3 * c + 2] = gap[c] / dt if gap[c] >= 0.0 else erp * gap[c] / dt
    c0 = np.zeros(nrt)
    c0[:nr] = J @ vf + gapterm[:nr]
    for r, (k, s, g) in enumerate(rows):
        gapterm[nr + r] = g / dt if g >= 0.0 else stop_erp * g / dt
        c0[nr + r] = s * vf[6 + k] + gapterm[nr + r]
    lam, used, rhos = pgs(G, c0, dt, mu, nr // 3, sweeps, lam0, tol, min_sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nr // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    lam_c = lam[:nr].copy()
    lam_w = (lam_c.reshape(-1, 3) @ Rc.T).reshape(-1)
    stop_rows, lam_stop = np.zeros(NJ, np.int32), np.zeros(NJ)
    for r, (k, s, g) in enumerate(rows):
        stop_rows[r] = s * (k + 1)
        lam_stop[r] = lam[nr + r]
    return dict(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam_w, lam_c=lam_c, gap=gap, contact=contact, sweeps=used, residual=rhos[-1], rhos=rhos,
                dtG=dt * np.diag(G), tau_applied=tc, stop_rows=stop_rows, lam_stop=lam_stop, dropped=dropped, margins=margins, stop_gaps=[g for _, _, g in rows],
                lam_all=lam)


def step(rb, tab, x, tau, dt, plane, mu, w=None, warm_start=False, **kw):
    """The state after one ground step and the warm row after it (contact rows only)."""
    r = solve(rb, tab, x, tau, dt, plane, mu, lam0=w if warm_start else None, **kw)
    vn = r["v_next"]
    return rb.integrate(np.r_[x[: rb.nq], vn], np.r_[vn * dt, np.zeros(rb.nv)]), r["lam_c"].copy(), r
