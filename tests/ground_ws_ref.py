"""The checker of the simulator's warm-started ground contact solve with a stopping rule: the model of tests/ground_env_ref.py
(one step of unilateral frictional contact on the plane {p : n . p = d}) with a start vector in the contact frame, rho of every sweep and
the stopping test, in numpy, the written model with its loops as written.  M, nle and the foot rows come from the oracle through
ground_env_ref.quantities.  Nothing of the product is imported except the table helpers."""
import numpy as np

import ground_env_ref as ER


def sticky_max(m, d):
    """max(m, d) that keeps a NaN once it has seen one."""
    return d if (d > m or d != d) else m


def start_vector(lam0, nr):
    """lambda0_r = lam0_r if it is given and finite, else exactly 0."""
    lam = np.zeros(nr)
    if lam0 is not None:
        for r in range(nr):
            if np.isfinite(lam0[r]):
                lam[r] = lam0[r]
    return lam


def pgs(G, c0, dt, mu, sweeps, lam0=None, tol=0.0, min_sweeps=1):
    """At most `sweeps` sweeps of projected Gauss-Seidel from the start vector, points in ascending order, layout [point][t1 t2 n]; sweep s
    yields rho_s = max_r |lambda_r(new) - lambda_r(old)| dt G_rr; the solve stops after sweep s if tol > 0, s >= min_sweeps and rho_s <= tol.
    Returns (lambda, sweeps run, [rho_1 .. rho_used])."""
    npts = len(c0) // 3
    lam = start_vector(lam0, 3 * npts)
    min_sweeps = max(1, min_sweeps)
    rhos = []
    for s in range(1, sweeps + 1):
        rho = 0.0
        for c in range(npts):
            n = 3 * c + 2
            acc = 0.0
            for j in range(3 * npts):
                acc += G[n, j] * lam[j]
            old = lam[n]
            lam[n] = max(0.0, old - (c0[n] + dt * acc) / (dt * G[n, n]))
            rho = sticky_max(rho, abs(lam[n] - old) * (dt * G[n, n]))
            t = np.zeros(2)
            for i in range(2):
                ti = 3 * c + i
                acc = 0.0
                for j in range(3 * npts):
                    acc += G[ti, j] * lam[j]
                t[i] = lam[ti] - (c0[ti] + dt * acc) / (dt * G[ti, ti])
            nrm = np.sqrt(t[0] * t[0] + t[1] * t[1])
            if nrm > mu * lam[n]:
                t = t * (mu * lam[n] / nrm)
            if nrm == 0.0:
                t = np.zeros(2)
            for i in range(2):
                ti = 3 * c + i
                rho = sticky_max(rho, abs(t[i] - lam[ti]) * (dt * G[ti, ti]))
            lam[3 * c], lam[3 * c + 1] = t[0], t[1]
        rhos.append(float(rho))
        if tol > 0.0 and s >= min_sweeps and rho <= tol:
            break
    return lam, len(rhos), rhos


def solve(rb, tab, x, tau, dt, plane, mu, push=None, joint=0, points=((0.0, 0.0, 0.0),), erp=0.2, compliance=1e-8, sweeps=30, lam0=None, tol=0.0,
          min_sweeps=1):
    """One ground step of state x on its own plane from the start vector lam0 (contact frame): the dict of ground_env_ref.solve and
    sweeps, residual (rho of the last sweep run), rhos (every sweep's), dtG (dt G_rr per row)."""
    nq = rb.nq
    M, h, J, gap, Rc = ER.quantities(rb, tab, x, tau, plane, points)
    nr = J.shape[0]
    Q = np.zeros(rb.nv) if push is None else ER.generalized_push(tab, x[:nq], joint, push[:3], push[3:6])
    b = np.r_[np.zeros(6), tau] - h + Q
    Lc = np.linalg.cholesky(M)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, J.T]))
    vf = x[nq:] + dt * W[:, 0]
    G = J @ W[:, 1:] + compliance * np.eye(nr)
    gapterm = np.zeros(nr)
    for c in range(nr // 3):
        gapterm[3 * c + 2] = gap[c] / dt if gap[c] >= 0.0 else erp * gap[c] / dt
    c0 = J @ vf + gapterm
    lam, used, rhos = pgs(G, c0, dt, mu, sweeps, lam0, tol, min_sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nr // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    lam_w = (lam.reshape(-1, 3) @ Rc.T).reshape(-1)
    return dict(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam_w, lam_c=lam, gap=gap, contact=contact, J=J, gapterm=gapterm, Q=Q, M=M, sweeps=used,
                residual=rhos[-1], rhos=rhos, dtG=dt * np.diag(G))


def step(rb, tab, x, tau, dt, plane, mu, w, warm_start, **kw):
    """The state after one ground step and the warm row after it: lam0 = w if warm_start, v+ of solve, q+ = q (+) v+ dt, w <- lambda in the
    contact frame."""
    r = solve(rb, tab, x, tau, dt, plane, mu, lam0=w if warm_start else None, **kw)
    vn = r["v_next"]
    return rb.integrate(np.r_[x[: rb.nq], vn], np.r_[vn * dt, np.zeros(rb.nv)]), r["lam_c"].copy(), r


def decided(rhos, tol, min_sweeps, margin=1e-3):
    """True if no rho_s with s >= min_sweeps lies within `margin` relative of tol: the number of sweeps is decided."""
    return all(abs(rho - tol) > margin * tol for s, rho in enumerate(rhos, 1) if s >= max(1, min_sweeps))
