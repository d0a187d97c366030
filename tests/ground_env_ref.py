"""The checker of the simulator's per-robot ground environment: one step of unilateral frictional contact on the plane
{p : n . p = d} with friction coefficient mu and one external force (f, o) on the body of joint j, in numpy, the written model with its
loops as written.  As tests/ground_ref.py it takes M, nle and the world-aligned 6-D foot rows from the oracle's rigid-body code and the
sweep from that file; the push point and its Jacobian come from a forward kinematics over the robot table of its own (joint_frames,
point_jacobian below).  Nothing of the product is imported except the table helpers."""
import numpy as np

import ground_ref as GR

_AXES = {1: np.array([1.0, 0.0, 0.0]), 2: np.array([0.0, 1.0, 0.0]), 3: np.array([0.0, 0.0, 1.0])}


def frame(n):
    """Rc = [t1 t2 n] of the unit normal n: t1 = (e_y x n) / |e_y x n|, t2 = n x t1."""
    n = np.array(n, float)
    t1 = np.cross(np.array([0.0, 1.0, 0.0]), n)
    t1 = t1 / np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    return np.column_stack([t1, t2, n])


def joint_frames(tab, q):
    """(R [nj][3][3], p [nj][3]) of every joint frame of table `tab` at configuration q, the conventions of ground_ref.foot_frames."""
    nj = tab.njoints
    R, p = [None] * nj, [None] * nj
    R[0], p[0] = GR._quat_to_R(np.array(q[3:7], float)), np.array(q[:3], float)
    for _ in range(nj):  # (parents need not precede their children in the table)
        for j in range(1, nj):
            pj = tab.parent[j]
            if R[j] is None and R[pj] is not None:
                R[j] = R[pj] @ np.array(tab.jp_R[j][:]).reshape(3, 3) @ GR._axis_R(tab.jtype[j], q[6 + j])
                p[j] = p[pj] + R[pj] @ np.array(tab.jp_p[j][:])
    return np.array(R), np.array(p)


def ancestors(tab, j):
    """Joint j and its ancestors."""
    out = [j]
    while j != 0:
        j = tab.parent[j]
        out.append(j)
    return out


def push_point(tab, q, j, o):
    R, p = joint_frames(tab, q)
    return p[j] + R[j] @ np.array(o, float)


def point_jacobian(tab, q, j, r):
    """[3][nv]: the world velocity of the point r (world coordinates) of the body of joint j per unit of every degree of freedom.  The
    base's six are its linear and angular velocity in the base frame; degree of freedom 5 + k is revolute joint k."""
    R, p = joint_frames(tab, q)
    nv = tab.njoints + 5
    J = np.zeros((3, nv))
    J[:, 0:3] = R[0]
    for i in range(3):
        J[:, 3 + i] = np.cross(R[0][:, i], r - p[0])
    for k in ancestors(tab, j):
        if k != 0:
            J[:, 5 + k] = np.cross(R[k] @ _AXES[tab.jtype[k]], r - p[k])
    return J


def generalized_push(tab, q, j, f, o):
    """Q [nv] of the force f (world axes) at the point p_j + R_j o."""
    r = push_point(tab, q, j, o)
    return point_jacobian(tab, q, j, r).T @ np.array(f, float)


def quantities(rb, tab, x, tau, plane, points):
    """M, h, J [3 nfeet P][nv] (rows t1, t2, n of point c = f P + k in the contact frame of the plane), the gaps n . p_c - d, Rc."""
    nf = rb.nf
    n, d = np.array(plane[:3], float), float(plane[3])
    Rc = frame(n)
    r = rb.full_forward_dynamics(x, tau, (1 << nf) - 1, fs=6)
    feet = rb.centroidal(x)["feet"]
    Rf, _ = GR.foot_frames(tab, x[: rb.nq])
    rows, gap = [], []
    for f in range(nf):
        Jl, Ja = r["J"][6 * f : 6 * f + 3], r["J"][6 * f + 3 : 6 * f + 6]
        for o in points:
            ow = Rf[f] @ np.array(o, float)
            lin = Jl - GR._skew(ow) @ Ja  # world axes
            rows.append(Rc.T @ lin)
            gap.append(n @ (feet[f] + ow) - d)
    return np.array(r["M"]), np.array(r["nle"]), np.vstack(rows), np.array(gap), Rc


def solve(rb, tab, x, tau, dt, plane, mu, push=None, joint=0, points=((0.0, 0.0, 0.0),), erp=0.2, compliance=1e-8, sweeps=30):
    """One ground step of state x on its own plane: dict(v_next, a, lam (world axes), lam_c (contact frame), gap, contact, J, gapterm, Q)."""
    nq = rb.nq
    M, h, J, gap, Rc = quantities(rb, tab, x, tau, plane, points)
    nr = J.shape[0]
    Q = np.zeros(rb.nv) if push is None else generalized_push(tab, x[:nq], joint, push[:3], push[3:6])
    b = np.r_[np.zeros(6), tau] - h + Q
    Lc = np.linalg.cholesky(M)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, J.T]))
    vf = x[nq:] + dt * W[:, 0]
    G = J @ W[:, 1:] + compliance * np.eye(nr)
    gapterm = np.zeros(nr)
    for c in range(nr // 3):
        gapterm[3 * c + 2] = gap[c] / dt if gap[c] >= 0.0 else erp * gap[c] / dt
    c0 = J @ vf + gapterm
    lam = GR.pgs(G, c0, dt, mu, sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nr // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    lam_w = (lam.reshape(-1, 3) @ Rc.T).reshape(-1)
    return dict(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam_w, lam_c=lam, gap=gap, contact=contact, J=J, gapterm=gapterm, Q=Q, M=M)


def regimes(r, mu):
    """ground_ref.regimes on the contact-frame forces."""
    return GR.regimes(dict(lam=r["lam_c"], gap=r["gap"]), mu)
