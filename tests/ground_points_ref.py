"""The checker of the simulator's body points: the ground step of tests/ground_joint_ref.py (on the plane) or of
tests/ground_terrain_ref.py (on a terrain) with contact candidates on any link in the free slots beside the foot points, in numpy, the
written model with its loops as written.  The foot quantities, the sweep, the stop candidates, the clipping and the sampling are those of
ground_terrain_ref.py, ground_joint_ref.py and ground_env_ref.py, imported and not edited; a point on any joint comes from
ground_env_ref.push_point / point_jacobian.  Nothing of the product is imported.

The model.
Settings.  A handle that has a ground gets BODY POINTS, shared by the batch: n in [0, 16] entries, joint[k] in [0, nj), offset[k][3]
  (metres, in the frame of that joint), and band >= 0 (metres; 0 stands for 0.02).  n = 0 or a null pointer clears them.
Slots.  The family's bound of 8 contact points (24 contact rows) per robot stays.  S = 8 - nfeet * points_per_foot slots are free beside
  the foot points.  S = 0 is refused.
One step of robot i (everything not named is as in DESIGN 3.23 - 3.28):
  1 position    p_k = p_j + R_j o_k with j = joint[k], from the tree walk that places the feet.
  2 gap         phi_k is the gap of a foot point at p_k.  Without a terrain: n . p_k - d with the robot's plane (setGroundEnv, else
                ground_z).  With a terrain: steps 1 - 6 of 3.28 at p_k, which also give the point its own n_k, t1_k, t2_k and h_k.
  3 candidates  in ascending k: k is a candidate iff phi_k < band (so a NaN gap is none).  The first S candidates get the slots
                s = 0, 1, ... in that order; the others are counted in body_dropped.
  4 rows        slot s is contact point c = nfeet P + s: three rows [t1 t2 n], exactly those of a foot point, at p_k, over the ancestors of
                joint[k], in the point's frame (the robot's plane frame, or its own on a terrain).  c0 gets phi_k / dt (phi_k >= 0) or
                erp phi_k / dt on the normal row.  The compliance and the robot's mu are the same.  The stop rows of 3.26 follow behind
                the last slot in use.
  5 sweeps      each sweep runs the foot points in their order, then the slots in ascending s (normal row, the two tangential rows,
                projection onto the disc of radius mu lambda_n: the update of a foot point), then the stop rows.  Slot rows start from
                exactly 0 every step.  The warm buffer keeps its layout (foot rows only).  rho takes the slot rows too.  The stopping
                rule, min_sweeps and the kernel's 1 / (dt G_rr) deviation are unchanged.
  6 outputs     per robot, besides those of 3.28 with their layouts unchanged:
                  body_slots [8] int32     k + 1 of the candidate in slot s, 0 = unused
                  lam_body [8][3]          forces ON the robot in world axes, 0 for unused slots
                  body_gap [16]            phi_k for k < n, 0 beyond
                  body_dropped             int32
                  body_touch               uint8: 1 iff lambda_n > 0 in some slot, else 0
                Bit nfeet P + s of the contact word is the slot's lambda_n > 0.
                lastTerrainNormals / lastTerrainHeights keep the foot points only.
With n = 0, or with every phi_k >= band, every added term is an exact zero and the shared outputs equal those of the kernel the handle
launched before, bit for bit."""
import numpy as np

import ground_env_ref as ER
import ground_joint_ref as JR
import ground_terrain_ref as TR
import ground_ws_ref as WR

MAX_POINTS, SLOTS, N_BODY = 8, 8, 16
DEFAULT_BAND = 0.02


def body_candidates(phi, band, free):
    """([k] of the slots in ascending k, dropped): step 3."""
    slots, dropped = [], 0
    for k in range(len(phi)):
        if phi[k] < band:
            if len(slots) < free:
                slots.append(k)
            else:
                dropped += 1
    return slots, dropped


def solve(rb, tab, x, tau, dt, mu, joints, offsets, band=0.0, plane=None, terrain=None, push=None, joint=0, points=((0.0, 0.0, 0.0),), erp=0.2, compliance=1e-8,
          sweeps=30, lam0=None, tol=0.0, min_sweeps=1, tau_max=None, damping=None, armature=None, q_lo=None, q_hi=None, stops=0, activation=0.0, stop_erp=0.0):
    """One ground step of state x with body points.  terrain = (heights [T][ny][nx], cell, tile, origin) or None: the plane [4].  The dict
    of ground_terrain_ref.solve (normals, heights, info only on a terrain; lam, lam_c, gap: foot points only) and body_slots, lam_body,
    body_gap, body_dropped, body_touch; for a test's conditions also band_margins (|phi_k - band|), slot_info (the terrain info of the slots)."""
    nq, nv = rb.nq, rb.nv
    na = nv - 6
    tmax = np.full(na, np.inf) if tau_max is None else np.array(tau_max, float)
    d = np.zeros(na) if damping is None else np.array(damping, float)
    ra = np.zeros(na) if armature is None else np.array(armature, float)
    lo = np.array(tab.q_lo[:na]) if q_lo is None else np.array(q_lo, float)
    hi = np.array(tab.q_hi[:na]) if q_hi is None else np.array(q_hi, float)
    activation = activation if activation > 0.0 else JR.DEFAULT_ACTIVATION
    stop_erp = stop_erp if stop_erp > 0.0 else JR.DEFAULT_STOP_ERP
    band = band if band > 0.0 else DEFAULT_BAND
    tc = JR.clip(tau, tmax)
    out = {}
    if terrain is not None:
        H, cell, tile, origin = terrain
        H = np.asarray(H, float)
        M, h, J, gap, Rcs, normals, hs, info = TR.quantities(rb, tab, x, tc, H, float(cell), tile, origin, points)
        out.update(normals=normals, heights=hs, info=info)
        Ht = H[min(max(int(tile), 0), H.shape[0] - 1)]
    else:
        M, h, J, gap, Rc = ER.quantities(rb, tab, x, tc, plane, points)
        Rcs = [Rc] * (J.shape[0] // 3)
    nrf = J.shape[0]  # foot rows
    npf = nrf // 3
    # steps 1, 2: every body point
    nb = len(joints)
    pk, phi, Rk, sinfo = [], np.zeros(nb), [], []
    for k in range(nb):
        p = ER.push_point(tab, x[:nq], int(joints[k]), offsets[k])
        if terrain is not None:
            hk, nk, inf = TR.sample(Ht, float(cell), origin, p)
            phi[k] = nk[2] * (p[2] - hk)
            Rk.append(ER.frame(nk))
            sinfo.append(inf)
        else:
            phi[k] = np.array(plane[:3], float) @ p - float(plane[3])
            Rk.append(Rc)
            sinfo.append(None)
        pk.append(p)
    # step 3
    slots, bdropped = body_candidates(phi, band, MAX_POINTS - npf)
    # step 4
    Jb = [Rk[k].T @ ER.point_jacobian(tab, x[:nq], int(joints[k]), pk[k]) for k in slots]
    Jc = np.vstack([J] + Jb) if Jb else J
    gapc = np.r_[gap, [phi[k] for k in slots]]
    nrp = Jc.shape[0]
    Q = np.zeros(nv) if push is None else ER.generalized_push(tab, x[:nq], joint, push[:3], push[3:6])
    Mh = M + np.diag(np.r_[np.zeros(6), ra + dt * d])
    b = np.r_[np.zeros(6), tc] - h - np.r_[np.zeros(6), d * x[nq + 6 :]] + Q
    rows, dropped, margins = JR.candidates(x[7:nq], lo, hi, activation) if stops else ([], 0, [])
    rows = rows[: 32 - nrp]  # (the rows of the instantiation: never binding, 24 + 8 = 32)
    Js = np.zeros((len(rows), nv))
    for r, (k, s, g) in enumerate(rows):
        Js[r, 6 + k] = s
    Ja = np.vstack([Jc, Js])
    Lc = np.linalg.cholesky(Mh)
    W = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.c_[b, Ja.T]))
    vf = x[nq:] + dt * W[:, 0]
    nrt = nrp + len(rows)
    G = Ja @ W[:, 1:] + compliance * np.eye(nrt)
    c0 = np.zeros(nrt)
    c0[:nrp] = Jc @ vf
    for c in range(nrp // 3):
        c0[3 * c + 2] += gapc[c] / dt if gapc[c] >= 0.0 else erp * gapc[c] / dt
    for r, (k, s, g) in enumerate(rows):
        c0[nrp + r] = s * vf[6 + k] + (g / dt if g >= 0.0 else stop_erp * g / dt)
    # step 5: the warm row holds foot rows only; slot rows start from exactly 0
    start = np.r_[WR.start_vector(lam0, nrf), np.zeros(nrp - nrf)]
    lam, used, rhos = JR.pgs(G, c0, dt, mu, nrp // 3, sweeps, start, tol, min_sweeps)
    Wl = W[:, 1:] @ lam
    contact = 0
    for c in range(nrp // 3):
        if lam[3 * c + 2] > 0.0:
            contact |= 1 << c
    lam_c = lam[:nrf].copy()
    lam_w = np.concatenate([Rcs[c] @ lam_c[3 * c : 3 * c + 3] for c in range(npf)])
    stop_rows, lam_stop = np.zeros(JR.NJ, np.int32), np.zeros(JR.NJ)
    for r, (k, s, g) in enumerate(rows):
        stop_rows[r] = s * (k + 1)
        lam_stop[r] = lam[nrp + r]
    body_slots, lam_body, body_gap = np.zeros(SLOTS, np.int32), np.zeros((SLOTS, 3)), np.zeros(N_BODY)
    touch = 0
    for s, k in enumerate(slots):
        body_slots[s] = k + 1
        lc = lam[nrf + 3 * s : nrf + 3 * s + 3]
        lam_body[s] = Rk[k] @ lc
        if lc[2] > 0.0:
            touch = 1
    body_gap[:nb] = phi
    out.update(v_next=vf + dt * Wl, a=W[:, 0] + Wl, lam=lam_w, lam_c=lam_c, gap=gap, contact=contact, sweeps=used, residual=rhos[-1], rhos=rhos,
               dtG=dt * np.diag(G), tau_applied=tc, stop_rows=stop_rows, lam_stop=lam_stop, dropped=dropped, margins=margins,
               stop_gaps=[g for _, _, g in rows], lam_all=lam, body_slots=body_slots, lam_body=lam_body, body_gap=body_gap, body_dropped=bdropped,
               body_touch=touch, band_margins=np.abs(phi - band), slot_info=[sinfo[k] for k in slots], slot_lam_n=[lam[nrf + 3 * s + 2] for s in range(len(slots))],
               slot_gap=[phi[k] for k in slots], points_world=pk)
    return out


def step(rb, tab, x, tau, dt, mu, joints, offsets, w=None, warm_start=False, **kw):
    """The state after one ground step with body points and the warm row after it (foot rows only)."""
    r = solve(rb, tab, x, tau, dt, mu, joints, offsets, lam0=w if warm_start else None, **kw)
    vn = r["v_next"]
    return rb.integrate(np.r_[x[: rb.nq], vn], np.r_[vn * dt, np.zeros(rb.nv)]), r["lam_c"].copy(), r
