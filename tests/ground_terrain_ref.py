"""The checker of the simulator's per-robot height-field terrain: the ground step of tests/ground_joint_ref.py with the
normal, the contact frame and the gap of every contact point sampled from a height field, in numpy, the written model with its loops as
written.  M, nle and the foot rows come from the oracle; the sweep, the stop candidates and the clipping are those of ground_joint_ref.py,
imported and not edited.  Nothing of the product is imported except the table helpers.

The model.
Settings.  A terrain of a handle that has a ground: heights[T][ny][nx] doubles are world z at the grid nodes, row j along world y, column
i along world x.  cell > 0 is the node spacing in metres, the same in x and y.  tile[B] (int32) says which of the T tiles robot i stands
on; null means 0.  origin[B][2] is the world (x, y) of node (0, 0) of robot i's tile; null means (0, 0).  Tiles are shared: a thousand
robots may stand on the same tile at different origins.
Admission: nx, ny >= 2 and T >= 1; T ny nx under a cap; every height is finite; cell is finite and positive; tile lies in [0, T); origin
is finite; at each of the four corners of every cell hx^2 + hy^2 <= 3 (the rule n.z >= 0.5 of DESIGN 3.24; the gradient of a bilinear
patch is extremal at its corners).
Sampling.  For contact point c at p = p_c:
  1 x = (p.x - o.x) / cell, clamped to [0, nx - 1]; i = min(floor(x), nx - 2), u = x - i.  The same in y gives j and v.
  2 The clamping is done in double before any conversion to an integer; the selects are written so that a NaN or +-inf coordinate yields
    index 0.  The tile index is clamped to [0, T - 1] as well.  No value read from memory can index outside the array.
  3 With h00 = H[j][i], h10 = H[j][i+1], h01 = H[j+1][i], h11 = H[j+1][i+1]: dx0 = h10 - h00, dx1 = h11 - h01, dy0 = h01 - h00;
    h0 = h00 + u dx0, h1 = h01 + u dx1, h = h0 + v (h1 - h0); hx = (dx0 + v (dx1 - dx0)) / cell, hy = (dy0 + u ((h11 - h10) - dy0)) / cell.
  4 s = 1 / sqrt(hx hx + hy hy + 1), n_c = ((0 - hx) s, (0 - hy) s, s).
  5 The frame t1, t2 of point c comes from n_c by the formula of DESIGN 3.24.
  6 The gap is phi_c = n_c.z (p.z - h): the distance to the tangent plane of the terrain below the point.
The step is the step of DESIGN 3.23 - 3.27 with n_c, t1_c, t2_c, phi_c in place of the robot's n, t1, t2, phi: in the rows of point c, in
c0, and in lambda_world(c) = Rc_c lambda_c.  Unchanged: the sweep, erp, compliance, the per-robot mu and push, the solver settings, the
joint model, the stop rows and the body parameters."""
import math

import numpy as np

import ground_env_ref as ER
import ground_joint_ref as JR
import ground_ref as GR

DBL_MAX = 1.7976931348623157e308


def cell_index(p, o, cell, n):
    """(i, u, x): steps 1 and 2 along one axis of n nodes, in scalar Python; x is the unclamped grid coordinate (for a test's conditions)."""
    x = (p - o) / cell
    lo = x if x > 0.0 else 0.0
    cl = lo if lo < n - 1.0 else n - 1.0
    xc = cl if abs(x) <= DBL_MAX else 0.0
    fl = math.floor(xc)
    fi = fl if fl < n - 2.0 else n - 2.0
    return int(fi), xc - fi, x


def sample(H, cell, origin, p):
    """(h, n [3], info) of one tile H [ny][nx] at the world point p: steps 1 - 4.  info = (i, j, u, v, x, y, |grad h|)."""
    ny, nx = H.shape
    i, u, x = cell_index(float(p[0]), float(origin[0]), cell, nx)
    j, v, y = cell_index(float(p[1]), float(origin[1]), cell, ny)
    h00, h10, h01, h11 = float(H[j, i]), float(H[j, i + 1]), float(H[j + 1, i]), float(H[j + 1, i + 1])
    dx0, dx1, dy0 = h10 - h00, h11 - h01, h01 - h00
    h0, h1 = h00 + u * dx0, h01 + u * dx1
    h = h0 + v * (h1 - h0)
    hx = (dx0 + v * (dx1 - dx0)) / cell
    hy = (dy0 + u * ((h11 - h10) - dy0)) / cell
    s = 1.0 / math.sqrt(hx * hx + hy * hy + 1.0)
    return h, np.array([(0.0 - hx) * s, (0.0 - hy) * s, s]), (i, j, u, v, x, y, math.hypot(hx, hy))


def quantities(rb, tab, x, tau, heights, cell, tile, origin, points):
    """M, h, J [3 nfeet P][nv] (rows t1, t2, n of point c in ITS contact frame), the gaps, Rc [points][3][3], normals, heights, info."""
    nf = rb.nf
    T = heights.shape[0]
    H = heights[min(max(int(tile), 0), T - 1)]
    r = rb.full_forward_dynamics(x, tau, (1 << nf) - 1, fs=6)
    feet = rb.centroidal(x)["feet"]
    Rf, _ = GR.foot_frames(tab, x[: rb.nq])
    rows, gap, Rcs, normals, hs, info = [], [], [], [], [], []
    for f in range(nf):
        Jl, Ja = r["J"][6 * f : 6 * f + 3], r["J"][6 * f + 3 : 6 * f + 6]
        for o in points:
            ow = Rf[f] @ np.array(o, float)
            p = feet[f] + ow
            h, n, inf = sample(H, cell, origin, p)
            Rc = ER.frame(n)
            lin = Jl - GR._skew(ow) @ Ja  # world axes
            rows.append(Rc.T @ lin)
            gap.append(n[2] * (p[2] - h))
            Rcs.append(Rc)
            normals.append(n)
            hs.append(h)
            info.append(inf)
    return np.array(r["M"]), np.array(r["nle"]), np.vstack(rows), np.array(gap), np.array(Rcs), np.array(normals), np.array(hs), info


def solve(rb, tab, x, tau, dt, heights, cell, tile, origin, mu, push=None, joint=0, points=((0.0, 0.0, 0.0),), erp=0.2, compliance=1e-8, sweeps=30, lam0=None,
          tol=0.0, min_sweeps=1, tau_max=None, damping=None, armature=None, q_lo=None, q_hi=None, stops=0, activation=0.0, stop_erp=0.0):
    """ground_joint_ref.solve on the terrain: its dict, and normals [points][3], heights [points], info (per point: i, j, u, v, x, y, |grad h|)."""
    nq, nv = rb.nq, rb.nv
    na = nv - 6
    tmax = np.full(na, np.inf) if tau_max is None else np.array(tau_max, float)
    d = np.zeros(na) if damping is None else np.array(damping, float)
    ra = np.zeros(na) if armature is None else np.array(armature, float)
    lo = np.array(tab.q_lo[:na]) if q_lo is None else np.array(q_lo, float)
    hi = np.array(tab.q_hi[:na]) if q_hi is None else np.array(q_hi, float)
    activation = activation if activation > 0.0 else JR.DEFAULT_ACTIVATION
    stop_erp = stop_erp if stop_erp > 0.0 else JR.DEFAULT_STOP_ERP
    tc = JR.clip(tau, tmax)
    M, h, J, gap, Rcs, normals, hs, info = quantities(rb, tab, x, tc, np.asarray(heights, float), float(cell), tile, origin, points)
    nr = J.shape[0]
    Q = np.zeros(nv) if push is None else ER.generalized_push(tab, x[:nq], joint, push[:3], push[3:6])
    Mh = M + np.diag(np.r_[np.zeros(6), ra + dt * d])
    b = np.r_[np.zeros(6), tc] - h - np.r_[np.zeros(6), d * x[nq + 6 :]] + Q
    rows, dropped, margins = JR.candidates(x[7:nq], lo, hi, activation) if stops else ([], 0, [])
    Js = np.zeros((len(rows), nv))
    for r, (k, s, g) in enumerate(rows):
        Js[r, 6 + k] = s
    Ja = np.vstack([J, Js])
    Lc = np.linalg.cholesky(Mh)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, Ja.T]))
    vf = x[nq:] + dt * W[:, 0]
    nrt = nr + len(rows)
    G = Ja @ W[:, 1:] + compliance * np.eye(nrt)
    c0 = np.zeros(nrt)
    c0[:nr] = J @ vf
    for c in range(nr // 3):
        c0[3 * c + 2] += gap[c] / dt if gap[c] >= 0.0 else erp * gap[c] / dt
    for r, (k, s, g) in enumerate(rows):
        c0[nr + r] = s * vf[6 + k] + (g / dt if g >= 0.0 else stop_erp * g / dt)
    lam, used, rhos = JR.pgs(G, c0, dt, mu, nr // 3, sweeps, lam0, tol, min_sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nr // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    lam_c = lam[:nr].copy()
    lam_w = np.concatenate([Rcs[c] @ lam_c[3 * c : 3 * c + 3] for c in range(nr // 3)])
    stop_rows, lam_stop = np.zeros(JR.NJ, np.int32), np.zeros(JR.NJ)
    for r, (k, s, g) in enumerate(rows):
        stop_rows[r] = s * (k + 1)
        lam_stop[r] = lam[nr + r]
    return dict(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam_w, lam_c=lam_c, gap=gap, contact=contact, sweeps=used, residual=rhos[-1], rhos=rhos,
                dtG=dt * np.diag(G), tau_applied=tc, stop_rows=stop_rows, lam_stop=lam_stop, dropped=dropped, margins=margins, stop_gaps=[g for _, _, g in rows],
                lam_all=lam, normals=normals, heights=hs, info=info)


def step(rb, tab, x, tau, dt, heights, cell, tile, origin, mu, w=None, warm_start=False, **kw):
    """The state after one ground step on the terrain and the warm row after it (contact rows only)."""
    r = solve(rb, tab, x, tau, dt, heights, cell, tile, origin, mu, lam0=w if warm_start else None, **kw)
    vn = r["v_next"]
    return rb.integrate(np.r_[x[: rb.nq], vn], np.r_[vn * dt, np.zeros(rb.nv)]), r["lam_c"].copy(), r
