"""The checker of the simulator's ground plane: one step of unilateral frictional contact in numpy, the written algorithm with
its loops as written.  M, nle and the world-aligned 6-D foot rows [J_lin; J_ang] come from the oracle's rigid-body code
(full_forward_dynamics(x, tau, all feet, fs=6): only its M, nle and J are used), the foot positions from centroidal(x)["feet"], the foot
rotations from a small forward kinematics over the robot table below.  Nothing of the product is imported except the table helpers."""
import numpy as np

import robot_tables as RT  # noqa: F401  (table helpers only)

DEFAULTS = dict(mu=0.7, erp=0.2, compliance=1e-8, sweeps=30)


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ])


def _axis_R(jtype, th):
    c, s = np.cos(th), np.sin(th)
    if jtype == 1:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if jtype == 2:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def foot_frames(tab, q):
    """(R [nfeet][3][3], p [nfeet][3]) of the feet of table `tab` at configuration q [nq]: joint 0 is the free-flyer (position, quaternion
    x y z w), joint j > 0 a revolute joint about axis jtype[j] (1 x, 2 y, 3 z) placed by (jp_R, jp_p) in its parent; a foot frame has the
    rotation of its joint."""
    nj = tab.njoints
    R, p = [None] * nj, [None] * nj
    R[0], p[0] = _quat_to_R(np.array(q[3:7], float)), np.array(q[:3], float)

    def place(j):
        if R[j] is None:
            pj = tab.parent[j]
            place(pj)
            R[j] = R[pj] @ np.array(tab.jp_R[j][:]).reshape(3, 3) @ _axis_R(tab.jtype[j], q[6 + j])
            p[j] = p[pj] + R[pj] @ np.array(tab.jp_p[j][:])
        return j

    Rf, pf = [], []
    for f in range(tab.nfeet):
        j = place(tab.foot_joint[f])
        Rf.append(R[j])
        pf.append(p[j] + R[j] @ np.array(tab.foot_p[f][:]))
    return np.array(Rf), np.array(pf)


def _skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])


def quantities(rb, tab, x, tau, ground_z, points):
    """M, h, J [3 nfeet P][nv] (world axes, rows x y z of point c = f P + k) and the gaps of every point."""
    nf = rb.nf
    r = rb.full_forward_dynamics(x, tau, (1 << nf) - 1, fs=6)
    feet = rb.centroidal(x)["feet"]
    Rf, _ = foot_frames(tab, x[: rb.nq])
    rows, gap = [], []
    for f in range(nf):
        Jl, Ja = r["J"][6 * f : 6 * f + 3], r["J"][6 * f + 3 : 6 * f + 6]
        for o in points:
            ow = Rf[f] @ np.array(o, float)
            rows.append(Jl - _skew(ow) @ Ja)
            gap.append(feet[f, 2] + ow[2] - ground_z)
    return np.array(r["M"]), np.array(r["nle"]), np.vstack(rows), np.array(gap)


def pgs(G, c0, dt, mu, sweeps):
    """`sweeps` sweeps of projected Gauss-Seidel from lambda = 0, points in ascending order, layout [point][x y z]."""
    npts = len(c0) // 3
    lam = np.zeros(3 * npts)
    for _ in range(sweeps):
        for c in range(npts):
            n = 3 * c + 2
            acc = 0.0
            for j in range(3 * npts):
                acc += G[n, j] * lam[j]
            lam[n] = max(0.0, lam[n] - (c0[n] + dt * acc) / (dt * G[n, n]))
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
            lam[3 * c], lam[3 * c + 1] = t[0], t[1]
    return lam


def solve(rb, tab, x, tau, dt, ground_z, points=((0.0, 0.0, 0.0),), mu=0.7, erp=0.2, compliance=1e-8, sweeps=30):
    """One ground step of state x under torques tau: dict(v_next, a, lam, gap, contact, and J, gapterm for checks on other answers)."""
    nq = rb.nq
    M, h, J, gap = quantities(rb, tab, x, tau, ground_z, points)
    nr = J.shape[0]
    b = np.r_[np.zeros(6), tau] - h
    Lc = np.linalg.cholesky(M)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, J.T]))
    vf = x[nq:] + dt * W[:, 0]
    G = J @ W[:, 1:] + compliance * np.eye(nr)
    gapterm = np.zeros(nr)
    for c in range(nr // 3):
        gapterm[3 * c + 2] = gap[c] / dt if gap[c] >= 0.0 else erp * gap[c] / dt
    c0 = J @ vf + gapterm
    lam = pgs(G, c0, dt, mu, sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nr // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    return dict(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam, gap=gap, contact=contact, J=J, gapterm=gapterm)


def step(rb, tab, x, tau, dt, ground_z, **kw):
    """The state after one ground step: v+ of solve, q+ = q (+) v+ dt."""
    r = solve(rb, tab, x, tau, dt, ground_z, **kw)
    vn = r["v_next"]
    return rb.integrate(np.r_[x[: rb.nq], vn], np.r_[vn * dt, np.zeros(rb.nv)]), r


def regimes(r, mu):
    """Which regimes one solve shows: all points free, some point sticking, some point sliding, some point penetrating."""
    lam = r["lam"].reshape(-1, 3)
    ln, lt = lam[:, 2], np.hypot(lam[:, 0], lam[:, 1])
    on = ln > 0.0
    stick = on & (lt < mu * ln * (1 - 1e-6))
    return dict(free=not on.any(), stick=bool(stick.any()), slide=bool((on & ~stick).any()), pen=bool((r["gap"] < 0.0).any()))
