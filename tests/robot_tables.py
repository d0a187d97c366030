"""Caller-filled robot tables for the centroidal MPC on a run-time joint tree (smpc_frontend_rt.h), derived from the project's built-in
tables through the ctypes mirror of smpc_robot_model.  TEST INFRASTRUCTURE.

  quad_arm    go2_like + a 6-joint serial arm on the base (Z-Y-Y-X-Y-X): 19 joints, 4 point feet
  biped_legs  talos_like without the joints above the pelvis, their mass lumped into the base body: 13 joints (Go2's count), 2 flat feet
  tree32      32 joints, 2 flat feet on joints 30 and 31, base and chest with three children each: the bound of every LDS array

The same struct goes to the oracle (oracle_robot) and to the library (simple_mpc.robot_from_table)."""
import ctypes as C

import numpy as np

import oracle_lib as O
import simple_mpc
from simple_mpc import RobotModelC

_keep = []  # tables handed to the oracle by pointer stay alive


def _builtin(name):
    src = O.lib().orc_builtin_robot(name.encode())  # (the same built-in table the library serves: include/smpc_robots_builtin.h)
    assert src, name
    return RobotModelC.from_buffer_copy(C.cast(src, C.POINTER(RobotModelC)).contents)


def _copy_joint(dst, j, src, k, parent):
    dst.parent[j], dst.jtype[j], dst.mass[j] = parent, src.jtype[k], src.mass[k]
    for i in range(9):
        dst.jp_R[j][i] = src.jp_R[k][i]
    for i in range(3):
        dst.jp_p[j][i], dst.com[j][i] = src.jp_p[k][i], src.com[k][i]
    for i in range(6):
        dst.inertia[j][i] = src.inertia[k][i]
    if j > 0:
        dst.q_ref[6 + j], dst.q_lo[j - 1], dst.q_hi[j - 1] = src.q_ref[6 + k], src.q_lo[k - 1], src.q_hi[k - 1]


def _new_joint(m, j, parent, jtype, p, mass, com, q_ref=0.0, lim=2.0):
    """A link of our own: identity placement rotation, a box-like inertia with small products so that no entry of the tensor is idle."""
    m.parent[j], m.jtype[j], m.mass[j] = parent, jtype, mass
    for i in range(9):
        m.jp_R[j][i] = 1.0 if i % 4 == 0 else 0.0
    for i in range(3):
        m.jp_p[j][i], m.com[j][i] = p[i], com[i]
    ixx, iyy, izz = mass * 0.012, mass * 0.009, mass * 0.007
    for i, v in enumerate((ixx, 0.03 * ixx, iyy, -0.02 * ixx, 0.01 * iyy, izz)):  # xx xy yy xz yz zz
        m.inertia[j][i] = v
    m.q_ref[6 + j], m.q_lo[j - 1], m.q_hi[j - 1] = q_ref, -lim, lim


def _finish(m, name, nj):
    m.name = name.encode()
    m.njoints, m.nq, m.nv = nj, nj + 6, nj + 5
    m.total_mass = float(sum(m.mass[:nj]))
    return m


def quad_arm():
    m = _builtin("go2_like")  # joints 0 .. 12, feet and reference placements stay
    arm = [  # parent, axis, placement in the parent, mass, CoM, reference angle
        (0, 3, (0.10, 0.0, 0.06), 1.2, (0.0, 0.0, 0.02), 0.0),
        (13, 2, (0.0, 0.0, 0.05), 1.0, (0.0, 0.0, 0.12), -0.6),
        (14, 2, (0.0, 0.0, 0.25), 0.8, (0.10, 0.0, 0.0), 1.2),
        (15, 1, (0.20, 0.0, 0.0), 0.5, (0.04, 0.0, 0.0), 0.0),
        (16, 2, (0.08, 0.0, 0.0), 0.3, (0.02, 0.0, 0.01), 0.4),
        (17, 1, (0.05, 0.0, 0.0), 0.2, (0.02, 0.005, 0.0), 0.0),
    ]
    for k, (par, jt, p, mass, com, qr) in enumerate(arm):
        _new_joint(m, 13 + k, par, jt, p, mass, com, qr)
    return _finish(m, "quad_arm", 19)


def biped_legs():
    t = _builtin("talos_like")
    m = RobotModelC.from_buffer_copy(t)  # base, legs (joints 1 .. 12), feet on joints 6 and 12, reference placements
    upper = float(sum(t.mass[13:23]))
    # the upper body as a point-like lump 0.25 m above the pelvis origin: mass, CoM and inertia of the base body
    mb = t.mass[0] + upper
    for i in range(3):
        m.com[0][i] = (t.mass[0] * t.com[0][i] + upper * (0.0, 0.0, 0.25)[i]) / mb
    m.mass[0] = mb
    for i, v in enumerate((1.9, 0.0, 1.6, 0.0, 0.0, 0.6)):
        m.inertia[0][i] = t.inertia[0][i] + v
    for j in range(13, 32):  # nothing of the removed joints stays behind
        m.parent[j] = m.jtype[j] = 0
        m.mass[j] = 0.0
    for i in range(19, 38):
        m.q_ref[i] = 0.0
    return _finish(m, "biped_legs", 13)


def tree32():
    t = _builtin("talos_like")
    m = RobotModelC.from_buffer_copy(t)
    _copy_joint(m, 1, t, 13, 0)  # torso
    _copy_joint(m, 2, t, 14, 1)  # chest: three children (joints 3, 10, 17)
    for side, (j0, k0, sgn) in enumerate(((3, 15, 1.0), (10, 19, -1.0))):  # arms: the four joints of the built-in table + a 3-joint wrist
        for i in range(4):
            _copy_joint(m, j0 + i, t, k0 + i, 2 if i == 0 else j0 + i - 1)
        _new_joint(m, j0 + 4, j0 + 3, 1, (0.0, 0.0, -0.12), 0.6, (0.0, 0.0, -0.05), 0.1 * sgn, 1.0)
        _new_joint(m, j0 + 5, j0 + 4, 2, (0.0, 0.0, -0.10), 0.4, (0.0, 0.01 * sgn, -0.04), -0.1, 1.0)
        _new_joint(m, j0 + 6, j0 + 5, 3, (0.0, 0.0, -0.08), 0.3, (0.01, 0.0, -0.03), 0.05 * sgn, 1.0)
    _new_joint(m, 17, 2, 3, (0.0, 0.0, 0.30), 1.5, (0.0, 0.0, 0.05), 0.0, 1.0)  # head
    _new_joint(m, 18, 17, 2, (0.0, 0.0, 0.05), 1.0, (0.01, 0.0, 0.05), 0.1, 1.0)
    _new_joint(m, 19, 18, 1, (0.0, 0.0, 0.05), 0.5, (0.0, 0.0, 0.04), 0.0, 1.0)
    for k in range(6):  # legs interleaved (left 20, 22, .., 30; right 21, 23, .., 31): the feet end up on the last two joints
        _copy_joint(m, 20 + 2 * k, t, 1 + k, 0 if k == 0 else 18 + 2 * k)
        _copy_joint(m, 21 + 2 * k, t, 7 + k, 0 if k == 0 else 19 + 2 * k)
    m.foot_joint[0], m.foot_joint[1] = 30, 31  # (foot_p, foot_ref_p: base and legs are those of the built-in table)
    m.parent[0], m.jtype[0] = -1, 0
    return _finish(m, "tree32", 32)


def _axis_rotation(axis, phi):
    """Rotation by phi about coordinate axis 1 / 2 / 3 (the jtype of a revolute joint)."""
    c, s = np.cos(phi), np.sin(phi)
    i, j, k = axis - 1, axis % 3, (axis + 1) % 3
    R = np.zeros((3, 3))
    R[i, i], R[j, j], R[k, k], R[j, k], R[k, j] = 1.0, c, c, -s, s
    return R


_SYM = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))  # the inertia's order: xx xy yy xz yz zz


def reframe(tab, seed):
    """The same robot with the frame of every joint turned about the joint's own axis: G_j = rot(jtype[j], phi_j), phi_j uniform in
    [-pi, pi], G = I on the base and on every foot joint.  A rotation about the axis commutes with the joint's motion, so q, v and tau keep
    their meaning, and with G = I on the feet so do foot frames, local contact forces and wrench cones:

        jp_R' = G_parent^T jp_R G_j     jp_p' = G_parent^T jp_p     com' = G_j^T com     I' = G_j^T I G_j

    foot_p, foot_ref_p, q_ref, q_lo, q_hi and the masses are untouched.  jp_R' is a dense rotation on every joint but the base: a seed
    that leaves one within 0.1 of the identity is refused."""
    rng = np.random.default_rng(seed)
    nj = tab.njoints
    feet = {tab.foot_joint[f] for f in range(tab.nfeet)}
    phi = rng.uniform(-np.pi, np.pi, nj)
    G = [np.eye(3) if j == 0 or j in feet else _axis_rotation(tab.jtype[j], phi[j]) for j in range(nj)]
    m = RobotModelC.from_buffer_copy(tab)
    for j in range(1, nj):
        Gp, Gj = G[tab.parent[j]], G[j]
        R = Gp.T @ np.array(tab.jp_R[j][:]).reshape(3, 3) @ Gj
        assert np.abs(R - np.eye(3)).max() > 0.1, ("seed %d leaves joint %d near the identity" % (seed, j), R)
        inertia = np.zeros((3, 3))
        for i, (r, c) in enumerate(_SYM):
            inertia[r, c] = inertia[c, r] = tab.inertia[j][i]
        inertia = Gj.T @ inertia @ Gj
        p, com = Gp.T @ np.array(tab.jp_p[j][:]), Gj.T @ np.array(tab.com[j][:])
        for i in range(9):
            m.jp_R[j][i] = R.flat[i]
        for i in range(3):
            m.jp_p[j][i], m.com[j][i] = p[i], com[i]
        for i, (r, c) in enumerate(_SYM):
            m.inertia[j][i] = inertia[r, c]
    m.name = (tab.name.decode() + "_rf").encode()
    return m


class Renumbering:
    """new_of_old[j]: the number that joint j of the original table has in the renumbered one.  Maps states, velocity-space vectors,
    torques and the velocity-space columns of matrices between the two numberings."""

    def __init__(self, new_of_old):
        self.new_of_old = np.asarray(new_of_old)
        nj = len(self.new_of_old)
        self.a = self.new_of_old[1:] - 1  # actuated joints: old position -> new position
        self.v = np.r_[np.arange(6), 6 + self.a]  # w_old = w_new[..., v]
        self.x = np.r_[np.arange(7), 7 + self.a, nj + 6 + self.v]

    def _to_new(self, old, idx):
        new = np.empty_like(old)
        new[..., idx] = old
        return new

    def state(self, X_old):
        return self._to_new(np.asarray(X_old), self.x)

    def velocity(self, v_old):
        return self._to_new(np.asarray(v_old), self.v)

    def torque(self, tau_old):
        return self._to_new(np.asarray(tau_old), self.a)

    def velocity_back(self, v_new):
        return np.asarray(v_new)[..., self.v]

    def torque_back(self, tau_new):
        return np.asarray(tau_new)[..., self.a]

    def state_back(self, X_new):
        return np.asarray(X_new)[..., self.x]

    def columns_back(self, M_new):
        """[.., nv] of the renumbered robot -> columns in the original order (J, Ag); apply twice (with .T) for M."""
        return np.asarray(M_new)[..., self.v]


def renumber(tab, seed):
    """(table, new_of_old): the same robot with its joints in another topological order, drawn at random (joint 0 stays, every parent
    comes before its children)."""
    rng = np.random.default_rng(seed)
    nj = tab.njoints
    order, ready = [0], [j for j in range(1, nj) if tab.parent[j] == 0]
    while ready:
        j = ready.pop(int(rng.integers(len(ready))))
        order.append(j)
        ready += [k for k in range(1, nj) if tab.parent[k] == j]
    assert sorted(order) == list(range(nj))
    new_of_old = np.empty(nj, int)
    new_of_old[order] = np.arange(nj)
    assert (new_of_old != np.arange(nj)).sum() > nj // 2, ("seed %d leaves most joints in place" % seed, new_of_old)
    m = RobotModelC.from_buffer_copy(tab)
    for new, old in enumerate(order):
        _copy_joint(m, new, tab, old, -1 if old == 0 else int(new_of_old[tab.parent[old]]))
    for f in range(tab.nfeet):
        m.foot_joint[f] = int(new_of_old[tab.foot_joint[f]])
    name = tab.name.decode()
    m.name = ((name[:-3] if name.endswith("_rf") else name) + "_rn").encode()
    return m, new_of_old


def _tree32p():
    import test_id_any_robot as T  # (the 32-joint point-foot table lives with the tests that introduced it)

    return T.table("tree32p")


MAKERS = {"quad_arm": quad_arm, "biped_legs": biped_legs, "tree32": tree32}
# <name>_rf: reframe(table(name)); <name>_rn: the re-framed table renumbered.  Seeds: the first that pass the helpers' own assertions.
REFRAME_SEED = {"quad_arm": 1, "biped_legs": 1, "tree32": 1, "tree32p": 1, "go2_like": 1, "talos_like": 1}
RENUMBER_SEED = {"quad_arm": 1, "biped_legs": 2, "tree32": 1, "tree32p": 1}
REFRAMED = [n + "_rf" for n in REFRAME_SEED]
RENUMBERED = [n + "_rn" for n in RENUMBER_SEED]
FEET = {4: ["FL_foot", "FR_foot", "RL_foot", "RR_foot"], 2: ["left_sole_link", "right_sole_link"]}
QUAD = np.array([[0.1, 0.075, 0], [-0.1, 0.075, 0], [-0.1, -0.075, 0], [0.1, -0.075, 0]])
_tables, _renumberings = {}, {}


def base_name(name):
    """("quad_arm", "rn") of "quad_arm_rn"; (name, "") of a table that is not derived by reframe / renumber."""
    return (name[:-3], name[-2:]) if name[-3:] in ("_rf", "_rn") else (name, "")


def table(name):
    """One table per robot for the whole session (never modified: the tests that need a bad table copy it)."""
    if name not in _tables:
        base, kind = base_name(name)
        if kind == "rf":
            _tables[name] = reframe(_tree32p() if base == "tree32p" else table(base), REFRAME_SEED[base])
        elif kind == "rn":
            _tables[name], new_of_old = renumber(table(base + "_rf"), RENUMBER_SEED[base])
            _renumberings[name] = Renumbering(new_of_old)
        else:
            _tables[name] = MAKERS[name]() if name in MAKERS else _builtin(name)
    return _tables[name]


def register(name, tab):
    """A table of a test's own making under a name, for the helpers that take names."""
    assert name not in _tables or _tables[name] is tab, name
    _tables[name] = tab
    return tab


def renumbering(name):
    """The Renumbering of a <name>_rn table against <name> (and <name>_rf)."""
    table(name)
    return _renumberings[name]


def oracle_robot(tab):
    """oracle_lib.Robot on a caller-filled table."""
    _keep.append(tab)
    rb = O.Robot.__new__(O.Robot)
    rb.ptr = C.cast(C.pointer(tab), C.c_void_p).value
    rb._init_from_ptr()
    return rb


def model_handler(tab, lib=None):
    """simple_mpc.RobotModelHandler on a caller-filled table, its feet added in table order."""
    mh = simple_mpc.RobotModelHandler(simple_mpc.robot_from_table(tab), "standing", "root_joint")
    for f in range(tab.nfeet):
        n = tab.foot_name[f].value.decode()
        if tab.nfeet == 2:
            mh.addQuadFoot(n, "root_joint", QUAD)
        else:
            mh.addPointFoot(n, "root_joint")
    return mh


def settings(rb, horizon, max_iters, short_gait=True):
    """Centroidal and MPC settings of record of the foot type (oracle_lib), horizon `horizon`; the short gait of the closed-loop tests:
    one stage of double support, two of flight."""
    if rb.nf == 4:
        s, ms = O.go2_centroidal_settings(rb), O.go2_mpc_settings(rb, max_iters=max_iters)
    else:
        s, ms = O.talos_centroidal_settings(rb), O.talos_mpc_settings(rb, max_iters=max_iters)
    ms["T"] = horizon
    if short_gait:
        ms["T_fly"], ms["T_contact"] = 2, 1
    return s, ms


def cycle(nf):
    """Trot (4 feet) / biped walk (2 feet) with T_ds = 1, T_ss = 2: six stages, so that six control steps feed a take-off and a touch-down of
    each foot pair into the horizon."""
    return O.trot_cycle(1, 2) if nf == 4 else O.walk_cycle(1, 2)


def make_product(tab, batch, max_iters=1, lib=None, horizon=10):
    rb = oracle_robot(tab)
    s, ms = settings(rb, horizon, max_iters)
    ocp = simple_mpc.CentroidalOCP(s, model_handler(tab, lib))
    ocp.createProblem(np.zeros(9), horizon, s["force_size"], -9.81, False)
    import mpc_setup as S

    gm = simple_mpc.BatchedMPC({k: ms[k] for k in S.MPC_KEYS}, ocp, batch, lib=lib)
    return gm, rb, s, ms


def make_pair(tab, batch, max_iters=1, lib=None, horizon=10, walk=(0.2, 0, 0, 0, 0, 0)):
    gm, rb, s, ms = make_product(tab, batch, max_iters, lib, horizon)
    om = O.OracleCentMPC(O.Cent(rb, s), ms, batch)
    for m in (om, gm):
        m.generateCycleHorizon(cycle(rb.nf))
        m.switchToWalk(np.array(walk, float))
    return om, gm, rb


def _quat(axis_angle):
    th = np.linalg.norm(axis_angle)
    if th < 1e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.r_[np.sin(th / 2) * axis_angle / th, np.cos(th / 2)]


def random_states(tab, n, seed, tilt=0.5, spread=0.8, vel=1.0):
    """n states [nq + nv]: base displaced and tilted by up to `tilt` rad about a random axis, every joint inside the middle `spread` of its
    limits, non-zero velocities everywhere."""
    rng = np.random.default_rng(seed)
    nj = tab.njoints
    lo, hi = np.array(tab.q_lo[: nj - 1]), np.array(tab.q_hi[: nj - 1])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * spread
    X = np.zeros((n, 2 * nj + 11))
    for b in range(n):
        ax = rng.normal(size=3)
        X[b, :3] = np.array(tab.q_ref[:3]) + rng.normal(size=3) * 0.05
        X[b, 3:7] = _quat(ax / np.linalg.norm(ax) * rng.uniform(0.1, tilt))
        X[b, 7 : nj + 6] = mid + half * rng.uniform(-1, 1, nj - 1)
        X[b, nj + 6 :] = rng.normal(size=nj + 5) * vel * np.r_[0.3 * np.ones(3), 0.5 * np.ones(3), np.ones(nj - 1)]
    return X


def near_reference_states(rb, n, seed, scale=0.5):
    """Measured states of the closed-loop tests: x_ref (+) N(0, sigma^2), the sigmas of mpc_setup.talos_random_states."""
    rng = np.random.default_rng(seed)
    sg = np.concatenate([np.ones(3) * 0.02, np.ones(3) * 0.05, np.ones(rb.nv - 6) * 0.1, np.ones(3) * 0.1, np.ones(3) * 0.2, np.ones(rb.nv - 6) * 0.5])
    return np.stack([rb.integrate(rb.x_ref, rng.normal(size=rb.ndx) * sg * scale) for _ in range(n)])
