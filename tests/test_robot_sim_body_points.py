"""BatchedRobotSim body points and the touch mask on the emulated kernels, against the checker tests/ground_points_ref.py.
Every case is a function of the library, so that tests/test_robot_sim_body_points_gpu.py runs the same functions on the HIP library.
The points, bands and seeds of case 1 are chosen on the checker alone; conditions() states what they have to meet."""
import ctypes as C

import numpy as np
import pytest

import ground_points_ref as PR
import ground_ws_ref as WR
import mpc_setup as S
import robot_tables as RT
import simple_mpc
import test_id_any_robot as T
import test_robot_sim_any_robot as SIM
import test_robot_sim_body_params as BP
import test_robot_sim_ground as G
import test_robot_sim_joint_model as J
import test_robot_sim_terrain as TT
from simple_mpc._capi import BodyPointsSettingsC, RobotModelC

_INVALID = -1  # SMPC_ERR_INVALID (include/smpc.h)
DT = G.DT
TOL, MIN_SWEEPS, SWEEPS = J.TOL, J.MIN_SWEEPS, J.SWEEPS
CELL = TT.CELL
# (robot, points per foot, seed of the states): 4, 4 and 6 free slots; the biped's rough case has a seed of its own (ROUGH_SEED)
CASES = [("go2_like", 1, 0), ("tree32p", 1, 3), ("biped_legs", 1, 1729)]
ROUGH_SEED = {"biped_legs": 95}
SHARED = J.SHARED + J.JOINT
NEW = ("body_slots", "lam_body", "body_gap", "body_dropped", "body_touch")
_cache = {}


# per quadruped: the two points beside every foot (in the shank joint's frame) and the depth of the skid below the trunk's frame
_QUADRUPED = {"go2_like": ((0.019, 0.056, -0.185), (-0.028, 0.02, -0.21), 0.3), "tree32p": ((-0.004, 0.026, -0.21), (0.06, 0.05, -0.212), 0.295)}


def _quadruped_points(name):
    """12 points: two on every shank beside the foot (the foot sits at (0, 0, -0.213) of the shank joint), one near two knees on the
    thighs, two corners of a skid below the trunk's frame (29.5 cm is 1.7 cm above the ground at the reference)."""
    a, b, skid = _QUADRUPED[name]
    joints, offsets = [], []
    for shank in (3, 6, 9, 12):
        joints += [shank, shank]
        offsets += [a, b]
    joints += [2, 8, 0, 0]
    offsets += [(0.0, 0.0, -0.2), (0.0, 0.0, -0.2), (0.18, 0.04, -skid), (-0.18, -0.04, -skid)]
    return np.array(joints, np.int32), np.array(offsets)


# the biped's points on the left and on the right leg: three on the foot link and one on the ankle link close to the sole (the sole's
# centre, the foot point, sits at (0, 0, -0.107) of the foot joint; some lie up to 2.4 cm below it, beside it), one on the shank
_BIPED = (((-0.053, -0.054, -0.096), (-0.105, -0.062, -0.131), (0.107, -0.066, -0.125), (0.122, -0.014, -0.099), (-0.005, -0.014, -0.259)),
          ((-0.08, 0.055, -0.093), (0.088, -0.055, -0.091), (-0.025, 0.068, -0.099), (0.119, 0.012, -0.128), (-0.035, 0.027, -0.297)))


def _biped_points():
    """12 points: _BIPED on the two legs, two on the trunk."""
    joints, offsets = [], []
    for (foot, ankle, shank), pts in zip(((6, 5, 4), (12, 11, 10)), _BIPED):
        joints += [foot, foot, foot, ankle, shank]
        offsets += list(pts)
    joints += [0, 0]
    offsets += [(0.1, 0.0, -0.15), (-0.1, 0.0, -0.15)]
    return np.array(joints, np.int32), np.array(offsets)


BAND = 0.05  # wide: the candidate set differs from state to state


def body_points(name):
    return _biped_points() if name == "biped_legs" else _quadruped_points(name)


def ref_kw(inp, i, P):
    X, tau, planes, mu, push, j, tmax, dmp, arm, qlo, qhi = inp[:11]
    return dict(push=push[i], joint=j, points=G.points(P), sweeps=SWEEPS, tol=TOL, min_sweeps=MIN_SWEEPS, tau_max=tmax[i], damping=dmp[i], armature=arm[i],
                q_lo=qlo[i], q_hi=qhi[i], stops=1)


def points_inputs(name, P, seed, rough, n=24):
    """The inputs of the body-parameter test (24 states, each with its own mu, push, joint rows and bodies; on the rough tiles of the
    terrain test if `rough`) with the body points of the robot and the checker's answers: computed once, shared, never modified."""
    key = (name, P, seed, rough, n)
    if key not in _cache:
        inp = BP.body_inputs(name, P, seed, n)
        X, tau, planes, mu, tabs = inp[0], inp[1], inp[2], inp[3], inp[12]
        joints, offsets = body_points(name)
        terr = TT.terrain(name, seed, X) if rough else None
        ref = []
        for i in range(n):
            where = dict(terrain=(terr[0], CELL, terr[1][i], terr[2][i])) if rough else dict(plane=planes[i])
            ref.append(PR.solve(RT.oracle_robot(tabs[i]), tabs[i], X[i], tau[i], DT, mu[i], joints, offsets, BAND, **where, **ref_kw(inp, i, P)))
        _cache[key] = (inp, joints, offsets, terr, ref)
    return _cache[key]


def solve_kw(inp, rows, terr):
    kw = BP.model_kw(inp, rows)
    kw["body"] = inp[11][rows]
    if terr is not None:
        del kw["planes"]
        kw.update(heights=terr[0], cell=CELL, tile=terr[1][rows], origin=terr[2][rows])
    return kw


def conditions(ref, rough):
    """The input conditions of parity(), on the checker alone."""
    loaded = sum(1 for r in ref if r["body_touch"])
    dropped = sum(1 for r in ref if r["body_dropped"] > 0)
    three = sum(1 for r in ref if r["body_touch"] and (r["contact"] & ((1 << (len(r["gap"]))) - 1)) != 0 and (r["lam_stop"] > 0.0).any())
    pen = sum(1 for r in ref if any(g < 0.0 for g in r["slot_gap"]))
    steep = sum(1 for r in ref for inf in r["slot_info"] if inf is not None and inf[6] > 0.2)
    band = min(float(r["band_margins"].min()) for r in ref)
    margins = float(np.concatenate([r["margins"] for r in ref]).min())
    decided = all(WR.decided(r["rhos"], TOL, MIN_SWEEPS) for r in ref)
    sets = len(set(tuple(r["body_slots"]) for r in ref))
    ok = loaded >= 10 and dropped >= 3 and three >= 3 and pen >= 3 and (not rough or steep >= 5) and band >= 1e-9 and margins >= 1e-9 and decided and sets >= 3
    return ok, (loaded, dropped, three, pen, steep, band, margins, decided, sets)


def _equal_ints(out, ref):
    assert np.array_equal(out["contact"], np.array([r["contact"] for r in ref], np.uint32))
    assert np.array_equal(out["tau_applied"], np.array([r["tau_applied"] for r in ref]))
    assert np.array_equal(out["stop_rows"], np.array([r["stop_rows"] for r in ref])) and out["stop_rows"].dtype == np.int32
    assert np.array_equal(out["dropped"], np.array([r["dropped"] for r in ref]))
    assert np.array_equal(out["sweeps"], np.array([r["sweeps"] for r in ref]))
    assert np.array_equal(out["body_slots"], np.array([r["body_slots"] for r in ref])) and out["body_slots"].dtype == np.int32
    assert np.array_equal(out["body_dropped"], np.array([r["body_dropped"] for r in ref])) and out["body_dropped"].dtype == np.int32
    assert np.array_equal(out["body_touch"], np.array([r["body_touch"] for r in ref], np.uint8)) and out["body_touch"].dtype == np.uint8


# ---------------------------------------------------------------------------------------------------------------------- 1
def parity(name, P, seed, rough, lib):
    """Case 1: groundPointsDynamics on 24 states, each with its own mu, push, joint rows, bodies and (rough) tile and origin, with stops on
    and 12 body points, against the checker.  No solve and no point is left out of a comparison."""
    inp, joints, offsets, terr, ref = points_inputs(name, P, seed, rough)
    X, tau = inp[0], inp[1]
    ok, what = conditions(ref, rough)
    print("%s P %d %s: checker: solves with a loaded slot %d, with dropped candidates %d, with slot + foot + stop loaded %d, with a penetrating candidate %d; slots on "
          "facets steeper than 0.2: %d; nearest |phi - band| %.2e; smallest stop margin %.2e; sweeps decided %s; distinct slot sets %d"
          % ((name, P, "rough" if rough else "plane") + what))
    assert ok, what
    assert len(joints) >= 12
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    out = sim.groundPointsDynamics(X, tau, DT, joints, offsets, BAND, **solve_kw(inp, slice(None), terr))
    keys = ("v_next", "a", "lam", "lam_contact", "lam_body", "lam_stop", "body_gap", "gap") + (("normals", "heights") if rough else ())
    worst = dict.fromkeys(keys, 0.0)
    for i, r in enumerate(ref):
        for k in keys:
            worst[k] = max(worst[k], G._rel(out[k][i], r["lam_c" if k == "lam_contact" else k]))
    print("%s P %d %s: %s" % (name, P, "rough" if rough else "plane", "  ".join("%s %.2e" % (k, worst[k]) for k in keys)))
    _equal_ints(out, ref)
    # (without the points the answers differ: they are read)
    plain = sim.groundTerrainDynamics(X, tau, DT, **solve_kw(inp, slice(None), terr)) if rough else sim.groundBodyDynamics(X, tau, DT, **solve_kw(inp, slice(None), terr))
    assert G._rel(plain["a"], out["a"]) > 1e-3
    assert max(worst.values()) < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------------- 2
FAR = 10.0  # metres above the trunk (whose tilt stays below 0.3 rad; a limb's frame may point anywhere): far outside every band


def far_points(name):
    joints, offsets = body_points(name)
    return np.zeros_like(joints), offsets + np.array([0.0, 0.0, FAR])


def inert_points(name, P, seed, lib, alloc, steps=20):
    """Case 2: body points far above the band give every shared output of groundTerrainDynamics and groundBodyDynamics bit for bit (the
    32-row kernel against the 24-row one the handle used before, where it did), slots and touch bytes 0; 20 steps at B = 3 equal a handle
    that never called the setter, with and without terrain, joint model and body parameters, set before or after; setBodyPoints(None)
    gives the handle that never called it."""
    joints, offsets = far_points(name)
    for rough in (False, True):
        inp, _, _, terr, _ = points_inputs(name, P, seed, rough)
        X, tau = inp[0], inp[1]
        tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
        kw = solve_kw(inp, slice(None), terr)
        want = sim.groundTerrainDynamics(X, tau, DT, **kw) if rough else sim.groundBodyDynamics(X, tau, DT, **kw)
        assert want["contact"].any() and want["stop_rows"].any()
        for jo, of in ((joints, offsets), ([], np.zeros((0, 3)))):
            got = sim.groundPointsDynamics(X, tau, DT, jo, of, 0.0, **kw)
            for k in SHARED + (("normals", "heights") if rough else ()):
                assert np.array_equal(got[k], want[k]), (k, rough)
            assert not got["body_slots"].any() and not got["body_touch"].any() and not got["lam_body"].any() and not got["body_dropped"].any()
            assert (got["body_gap"][:, : len(jo)] > FAR / 2).all() and not got["body_gap"][:, len(jo) :].any()
    inp = points_inputs(name, P, seed, False)[0]
    Bd = inp[11]
    B = 3
    tab, rb, sim, gz = G.make(name, P, lib, B)
    X0, tq = G.drop_states(rb, B, 71)
    na = rb.nv - 6
    jm = dict(tau_max=np.full(na, 3.0), damping=np.full((B, na), 0.2), armature=np.full(na, 0.01), stops=True)
    rough = np.ascontiguousarray(gz + np.random.default_rng(3).uniform(-0.02, 0.02, (1, 6, 6)))

    def handle(order):
        _, _, h, _ = G.make(name, P, lib, B)
        for what in order:
            if what == "warm":
                h.setGroundSolver(warm_start=True, tol=1e-6, min_sweeps=0)
            elif what == "joint":
                h.setJointModel(**jm)
            elif what == "body":
                h.setBodyParams(Bd[:B])
            elif what == "rough":
                h.setTerrain(rough, 0.15, origin=X0[:, :2] - 0.375)
            elif what == "far":
                h.setBodyPoints(joints, offsets)
            elif what == "near":
                h.setBodyPoints(*body_points(name), band=BAND)
            elif what == "clear":
                h.setBodyPoints(None)
        return h

    def run(h):
        Xd, td = alloc(X0), alloc(tq)
        trace = []
        for _ in range(steps):
            h.stepGroundDevice(Xd.ptr, td.ptr, DT)
            h.wait()
            trace.append((Xd.get(), h.lastGroundForces(), h.lastContacts(), h.lastAccelerations()))
        return trace, h.lastBodyContacts()

    groups = [
        [(), ("far",), ("near", "clear"), ("clear",)],
        [("rough",), ("rough", "far"), ("far", "rough"), ("near", "rough", "clear")],
        [("warm", "joint"), ("warm", "joint", "far"), ("far", "warm", "joint"), ("near", "joint", "warm", "clear")],
        [("warm", "joint", "body", "rough"), ("far", "warm", "joint", "body", "rough"), ("warm", "body", "far", "rough", "joint"),
         ("body", "rough", "near", "joint", "warm", "clear")],
    ]
    for group in groups:
        want, _ = run(handle(group[0]))
        assert any(t[2].all() for t in want) and np.abs(want[-1][0] - X0).max() > 1e-4  # (every robot has landed)
        for order in group[1:]:
            h = handle(order)
            got, last = run(h)
            for k, (g, w) in enumerate(zip(got, want)):
                assert all(np.array_equal(u, v) for u, v in zip(g, w)), (order, k)
            on = "far" in order
            ptrs = h.bodyPointsDevicePointers()
            assert all(bool(v) == on for v in ptrs.values()), (order, ptrs)
            assert not last["body_slots"].any() and not last["body_touch"].any() and not last["lam_body"].any() and not last["body_dropped"].any()
            assert on == bool((last["body_gap"][:, : len(joints)] > FAR / 2).all()) and not last["body_gap"][:, len(joints) :].any()


# ---------------------------------------------------------------------------------------------------------------------- 3
def two_feet_table(tab):
    """A copy of the go2_like table with its last two feet struck from the foot list."""
    t = RobotModelC.from_buffer_copy(tab)
    t.nfeet = 2
    return t


def body_point_is_a_foot_point(lib, rough):
    """Case 3 (no checker): the go2_like table with its last two feet struck from the foot list and two body points at those feet's joints
    and offsets, band 1 m, against the full table: same states, cold start, fixed sweeps."""
    name, seed, n = "go2_like", 0, 24
    tab = T.table(name)
    X, tau = G.ground_states(name, n, 12)[:2]
    rb = RT.oracle_robot(tab)
    gz = G.ground_height(rb)
    full = simple_mpc.BatchedRobotSim(RT.model_handler(tab, lib), force_size=3, batch=3, lib=lib)
    two = simple_mpc.BatchedRobotSim(RT.model_handler(two_feet_table(tab), lib), force_size=3, batch=3, lib=lib)
    full.setGround(ground_z=gz, sweeps=40)
    two.setGround(ground_z=gz, sweeps=40)
    assert (full.ground_points, two.ground_points) == (4, 2)
    joints = [tab.foot_joint[2], tab.foot_joint[3]]
    offsets = [list(tab.foot_p[2]), list(tab.foot_p[3])]
    kw = dict(stops=False)
    if rough:
        H, tile, origin = TT.terrain(name, seed, X)
        kw.update(heights=H[:1], cell=CELL, origin=origin)
        want = full.groundTerrainDynamics(X, tau, DT, **kw)
    else:
        want = full.groundBodyDynamics(X, tau, DT, **kw)
    got = two.groundPointsDynamics(X, tau, DT, joints, offsets, 1.0, **kw)
    assert (want["contact"] >> 2).any() and (want["contact"] & 3).any() and (want["gap"] < 1.0).all()
    lam = np.concatenate([got["lam"], got["lam_body"][:, :2].reshape(n, 6)], axis=1)
    worst = dict(v_next=G._rel(got["v_next"], want["v_next"]), a=G._rel(got["a"], want["a"]), lam=G._rel(lam, want["lam"]),
                 gap=G._rel(np.c_[got["gap"], got["body_gap"][:, :2]], want["gap"]))
    print("a body point is a foot point (%s): %s" % ("rough" if rough else "plane", "  ".join("%s %.2e" % kv for kv in worst.items())))
    assert np.array_equal(got["contact"], want["contact"])
    assert np.array_equal(got["body_slots"][:, :3], np.tile(np.array([1, 2, 0], np.int32), (n, 1)))
    assert np.array_equal(got["body_touch"], ((want["contact"] >> 2) != 0).astype(np.uint8))
    assert not got["lam_body"][:, 2:].any() and not got["body_dropped"].any()
    assert max(worst.values()) < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------------- 4
FALL_STEPS, FALL_LAST, FALL_SWEEPS = {False: 150, True: 250}, 50, 60  # (steps on the plane and on the rough tile, where the trunk rocks longer)
FALL_DAMPING, GRAVITY = BP.SCALE_DAMPING, BP.GRAVITY
FALL_BOX = ((0.0, 0.0, 0.0), (0.19, 0.05, 0.1))  # centre and half extents of the trunk box in the trunk's frame


def crouched(rb, gz, lift=0.001):
    """go2_like with its legs folded (thigh 1.2, knee -2.6 rad), the feet `lift` above the plane: the bottom of the trunk box is 7 mm
    above it, and the robot comes to lie on it within 0.1 s when the legs give way against the damping."""
    x = rb.x_ref.copy()
    for leg in range(4):
        x[7 + 3 * leg + 1], x[7 + 3 * leg + 2] = 1.2, -2.6
    x[2] += gz - rb.centroidal(x)["feet"][:, 2].min() + lift
    return x


def fall_ground(rb, gz, rough):
    """(where of the checker, setter arguments of the handle or None): the plane, or the first origin of the rough tile of the scale test."""
    if not rough:
        return dict(plane=[0.0, 0.0, 1.0, gz]), None
    H, origin = TT.scale_terrain(rb)
    return dict(terrain=(H, TT.SCALE_CELL, 0, origin[0])), (H, TT.SCALE_CELL, origin[:1])


def fall_loop(rough, with_points=True, x0=None):
    """The checker's host loop of case 4: zero torque, FALL_DAMPING on every joint, stops on, the eight corners of the trunk box, warm
    start, exactly FALL_SWEEPS sweeps.  (final state, deepest trunk-corner penetration and largest deviation of the summed contact force
    from (0, 0, m g) over the last FALL_LAST steps, final base height above the ground)."""
    key = ("fall", rough, with_points, None if x0 is None else x0.tobytes())
    if key not in _cache:
        tab = T.table("go2_like")
        rb = RT.oracle_robot(tab)
        gz = G.ground_height(rb)
        na = rb.nv - 6
        where, _ = fall_ground(rb, gz, rough)
        joints, offsets = simple_mpc.box_points(0, *FALL_BOX)
        if not with_points:
            joints, offsets = joints[:0], offsets[:0]
        x = crouched(rb, gz, 0.005 if rough else 0.001) if x0 is None else x0.copy()
        w, pen, dev = None, 0.0, 0.0
        mg = tab.total_mass * GRAVITY
        for k in range(FALL_STEPS[rough]):
            x, w, r = PR.step(rb, tab, x, np.zeros(na), DT, G.MU, joints, offsets, w=w, warm_start=k > 0, sweeps=FALL_SWEEPS, damping=np.full(na, FALL_DAMPING),
                              stops=1, **where)
            if k >= FALL_STEPS[rough] - FALL_LAST and with_points:
                pen = max(pen, -float(r["body_gap"][:8].min()))
                f = r["lam"].reshape(-1, 3).sum(0) + r["lam_body"].sum(0)
                dev = max(dev, float(np.linalg.norm(f - np.array([0.0, 0.0, mg])) / mg))
        low = min(float(r0[2]) for r0 in r["points_world"]) if with_points else x[2] - FALL_BOX[1][2]
        _cache[key] = (x, pen, dev, low)
    return _cache[key]


def fallen_robot_lies_on_its_trunk(lib, alloc, rough):
    """Case 4: a go2_like whose legs give way comes to lie on the corners of its trunk box with finite states; the deepest corner and the
    summed contact force over the last 50 of 150 (rough: 250) steps are gated at ten times the checker's own figures, the final state at 1e-9 times the
    checker's sensitivity to its start state; without the points the trunk ends below the ground (printed)."""
    name = "go2_like"
    tab, rb, sim, gz = G.make(name, 1, lib, 1, sweeps=FALL_SWEEPS)
    na = rb.nv - 6
    xr, pen_ref, dev_ref, low = fall_loop(rough)
    x0 = crouched(rb, gz, 0.005 if rough else 0.001)
    delta = 1e-7 * np.random.default_rng(4).uniform(-1.0, 1.0, rb.nv)
    xp = fall_loop(rough, x0=rb.integrate(x0, np.r_[delta, np.zeros(rb.nv)]))[0]
    sens = float(np.abs(xp - xr).max() / np.abs(delta).max())
    bar = 1e-9 * max(1.0, sens)
    mg = tab.total_mass * GRAVITY
    print("fall (%s): checker: deepest corner %.3e m, force deviation %.3e of m g, |v| at the end %.2e, sensitivity of the final state %.2f, bar %.2e"
          % ("rough" if rough else "plane", pen_ref, dev_ref, np.abs(xr[rb.nq : rb.nq + 6]).max(), sens, bar))
    if not rough:  # (what the points are for: printed, not gated)
        print("fall (plane): without body points the bottom of the trunk box ends %.4f m below the ground" % (gz - fall_loop(rough, with_points=False)[3]))
    # (the checker's trunk has come to rest: quasi-static as on the scale of DESIGN 3.27; on the rough tile it keeps rocking at some
    # 0.02 rad/s on two corners while the legs creep against the damping)
    assert np.abs(xr[rb.nq : rb.nq + 6]).max() < 0.05 and dev_ref < 0.05
    _, setter = fall_ground(rb, gz, rough)
    sim.setGroundSolver(warm_start=True)
    sim.setJointModel(damping=np.full(na, FALL_DAMPING), stops=True)
    if setter is not None:
        sim.setTerrain(setter[0], setter[1], origin=setter[2])
    sim.setBodyPoints(*simple_mpc.box_points(0, *FALL_BOX))
    Xd, td = alloc(x0[None]), alloc(np.zeros((1, na)))
    pen, dev = 0.0, 0.0
    for k in range(FALL_STEPS[rough]):
        sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
        if k >= FALL_STEPS[rough] - FALL_LAST:
            sim.wait()
            last = sim.lastBodyContacts()
            pen = max(pen, -float(last["body_gap"][0, :8].min()))
            f = sim.lastGroundForces().reshape(-1, 3).sum(0) + last["lam_body"][0].sum(0)
            dev = max(dev, float(np.linalg.norm(f - np.array([0.0, 0.0, mg])) / mg))
    sim.wait()
    x = Xd.get()[0]
    err = float(np.abs(x - xr).max())
    print("fall (%s): kernel: deepest corner %.3e m, force deviation %.3e of m g, final state against the checker's %.2e (bar %.2e); touch byte %d"
          % ("rough" if rough else "plane", pen, dev, err, bar, last["body_touch"][0]))
    assert np.isfinite(x).all() and last["body_touch"][0] == 1 and last["body_slots"][0, :4].all()
    assert pen <= 10.0 * pen_ref and dev <= 10.0 * dev_ref, (pen, pen_ref, dev, dev_ref)
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------------------------- 5
def mask_is_the_reset_mask(lib, alloc):
    """Case 5, first half: B = 5 with robots 1 and 3 on their trunks.  The touch bytes on the device equal the checker's; handed unchanged
    to reset_instances_device and resetGroundWarmStartDevice they reset exactly those two robots, and the other three continue bit for bit
    as in a run without the call."""
    import test_reset_instances as RI

    name, B, down, steps = "go2_like", 5, [1, 3], 12
    joints, offsets = simple_mpc.box_points(0, *FALL_BOX)
    tab = T.table(name)
    rb = RT.oracle_robot(tab)
    gz = G.ground_height(rb)
    na = rb.nv - 6
    X0, tq = G.drop_states(rb, B, 71)
    for i in down:
        X0[i] = crouched(rb, gz)
        X0[i, 8:19:3], X0[i, 9:19:3] = 1.35, -2.7  # (the feet drawn in above the bottom of the box: the robot lies on its trunk)
        X0[i, 2] = gz + FALL_BOX[1][2] + 0.0005
        X0[i, rb.nq + 2] = -0.2

    def handle():
        _, _, h, _ = G.make(name, 1, lib, B, sweeps=SWEEPS)
        h.setGroundSolver(warm_start=True, tol=TOL, min_sweeps=MIN_SWEEPS)
        h.setJointModel(damping=np.full(na, FALL_DAMPING), stops=True)
        h.setBodyPoints(joints, offsets)
        return h

    sims = [handle() for _ in range(3)]  # the mask on the device, the same robots from a host list, no reset
    mpcs = [RI.make("go2_kino", lib, B=B) for _ in range(3)]
    Xm = mpcs[0][2]
    for (m, _, _), h in zip(mpcs, sims):
        h.shareStream(m)
        m.iterate(Xm)
    Xd = [alloc(X0) for _ in sims]
    td = alloc(tq)
    for h, xd in zip(sims, Xd):
        for _ in range(steps):
            h.stepGroundDevice(xd.ptr, td.ptr, DT)
        h.wait()
    # the checker's touch bytes after the same steps
    want = np.zeros(B, np.uint8)
    for i in range(B):
        x, w = X0[i].copy(), None
        for k in range(steps):
            x, w, r = PR.step(rb, tab, x, tq[i], DT, G.MU, joints, offsets, w=w, warm_start=k > 0, plane=[0.0, 0.0, 1.0, gz], sweeps=SWEEPS, tol=TOL,
                              min_sweeps=MIN_SWEEPS, damping=np.full(na, FALL_DAMPING), stops=1)
        want[i] = r["body_touch"]
    assert want.tolist() == [0, 1, 0, 1, 0]
    touch = sims[0].lastBodyContacts()["body_touch"]
    assert np.array_equal(touch, want) and np.array_equal(sims[2].lastBodyContacts()["body_touch"], want)
    ptr = sims[0].bodyPointsDevicePointers()["body_touch"]
    mpcs[0][0].reset_instances_device(ptr)
    sims[0].resetGroundWarmStartDevice(ptr)
    mpcs[1][0].resetInstances(down)
    sims[1].resetGroundWarmStart(down)
    for (m, _, _), h in zip(mpcs, sims):
        m.wait()
        h.wait()
    keep = [0, 2, 4]
    warm = [alloc.read(h.groundSolverDevicePointers()[2], (B, 12)) for h in sims]
    assert not warm[0][down].any() and np.array_equal(warm[0], warm[1]) and np.array_equal(warm[0][keep], warm[2][keep]) and warm[0][keep].any()
    RI.assert_same(RI.snapshot(mpcs[0][0]), RI.snapshot(mpcs[1][0]), what="mask against list")
    assert mpcs[0][0].save_state() == mpcs[1][0].save_state() and mpcs[0][0].save_state() != mpcs[2][0].save_state()
    for (m, _, _) in mpcs:
        m.iterate(Xm)
    names = ("xs", "us", "Ks", "info")
    RI.assert_same(RI.snapshot(mpcs[0][0], names), RI.snapshot(mpcs[2][0], names), rows=keep, what="instances not in the mask")
    assert not np.array_equal(mpcs[0][0].us[down], mpcs[2][0].us[down])  # (the reset did something)
    traces = []
    for h, xd in zip(sims, Xd):
        t = []
        for _ in range(3):
            h.stepGroundDevice(xd.ptr, td.ptr, DT)
            h.wait()
            t.append((xd.get(), h.lastGroundForces(), h.lastAccelerations(), h.lastGroundSweeps(), h.lastBodyContacts()["lam_body"]))
        traces.append(t)
    for a, b, c in zip(*traces):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))  # (the mask resets what the list resets)
        assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(a, c))  # (the others never notice)


def batch_hygiene(name, P, seed, lib, alloc, emulated):
    """Case 5, second half: robot i is unchanged bit for bit when its neighbours' states change, on handles of batch 1, 3 and 5 and for
    n = 1, 3, 5 of the host-buffer solve, on the plane and on the rough tiles; on the emulated tier a NaN in robot 1's state leaves robots
    0 and 2 unchanged, and its own touch byte is then 0."""
    for rough in (False, True):
        inp, joints, offsets, terr, ref = points_inputs(name, P, seed, rough)
        X, tau = inp[0], inp[1]
        touched = [i for i, r in enumerate(ref) if r["body_touch"]]
        rows = (touched[:3] + [i for i in range(len(X)) if i not in touched][:2])[:5]
        rows = [rows[3], rows[0], rows[4], rows[1], rows[2]]
        keys = SHARED + NEW + (("normals", "heights") if rough else ())
        tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
        five = sim.groundPointsDynamics(X[rows], tau[rows], DT, joints, offsets, BAND, **solve_kw(inp, rows, terr))
        assert five["body_touch"].tolist() == [0, 1, 0, 1, 1]
        # the neighbours' states
        X2 = X[rows].copy()
        X2[[0, 2, 3, 4]] = X[[(r + 1) % len(X) for r in rows]][[0, 2, 3, 4]]
        other = sim.groundPointsDynamics(X2, tau[rows], DT, joints, offsets, BAND, **solve_kw(inp, rows, terr))
        for k in keys:
            assert np.array_equal(other[k][1], five[k][1]), k
        assert not np.array_equal(other["a"][0], five["a"][0])
        for batch in (1, 3, 5):
            _, _, h, _ = G.make(name, P, lib, batch, sweeps=SWEEPS)
            for n in (1, 3, 5):
                sub = rows[5 - n :]
                out = h.groundPointsDynamics(X[sub], tau[sub], DT, joints, offsets, BAND, **solve_kw(inp, sub, terr))
                for k in keys:
                    assert np.array_equal(out[k], five[k][5 - n :]), (k, batch, n)
            # the handle's step with the same settings
            sub = rows[:batch]
            kw = solve_kw(inp, sub, terr)
            h.setGroundEnv(mu=kw["mu"]) if rough else h.setGroundEnv(planes=kw["planes"], mu=kw["mu"])
            h.setPush(kw["push"], joint=kw["joint"])
            h.setGroundSolver(warm_start=False, tol=TOL, min_sweeps=MIN_SWEEPS)
            h.setBodyPoints(joints, offsets, band=BAND)
            if rough:
                h.setTerrain(terr[0], CELL, tile=terr[1][sub], origin=terr[2][sub])
            h.setBodyParams(kw["body"])
            h.setJointModel(**{k: kw[k] for k in ("tau_max", "damping", "armature", "q_lo", "q_hi", "stops")})
            Xd, td = alloc(X[sub]), alloc(tau[sub])
            h.stepGroundDevice(Xd.ptr, td.ptr, DT)
            h.wait()
            assert np.array_equal(h.lastAccelerations(), five["a"][:batch]) and np.array_equal(h.lastGroundForces(), five["lam"][:batch]), batch
            assert np.array_equal(Xd.get()[:, rb.nq :], five["v_next"][:batch]) and np.array_equal(h.lastContacts(), five["contact"][:batch])
            last = h.lastBodyContacts()
            for k in NEW:
                assert np.array_equal(last[k], five[k][:batch]), (k, batch)
        if emulated:
            sub = rows[:3]
            Xn = X[sub].copy()
            Xn[1, 0] = np.nan
            Xn[1, rb.nq + 7] = np.nan
            out = sim.groundPointsDynamics(Xn, tau[sub], DT, joints, offsets, BAND, **solve_kw(inp, sub, terr))
            for k in keys:
                assert np.array_equal(out[k][[0, 2]], five[k][[0, 2]]), k
            assert np.isnan(out["a"][1]).any() and out["body_touch"][1] == 0 and five["body_touch"][1] == 1


# ---------------------------------------------------------------------------------------------------------------------- 6
def admission(lib, alloc):
    """Case 6: every refusal through the C ABI names the field and the index and keeps the previous points; setBodyPoints before setGround
    is refused; no free slot is refused; setGround drops the points."""
    lib = lib or simple_mpc.default_lib()
    L = lib.L
    err = lambda: L.smpc_last_error().decode()
    name, B = "go2_like", 3
    tab, rb, sim = SIM.make(name, 3, lib, B)
    gz = G.ground_height(rb)
    nj = tab.njoints
    joints0, offsets0 = far_points(name)

    def raw(n=2, joint=(0, 3), offset=((0.0, 0.0, 0.0), (0.1, 0.0, -0.2)), band=0.03):
        s = BodyPointsSettingsC()
        s.n = n
        for k, j in enumerate(joint):
            s.joint[k] = j
        for k, o in enumerate(offset):
            for i in range(3):
                s.offset[k][i] = o[i]
        s.band = band
        return s

    X, tau = G.drop_states(rb, B, 71)
    none = [None] * 19

    def dyn(s):
        return L.smpc_robot_sim_ground_points_dynamics(sim._h, B, X, tau, DT, None, None, None, None, 0, None, None, None, None, C.byref(s), *none)

    # no ground yet
    s = raw()
    assert L.smpc_robot_sim_set_body_points(sim._h, C.byref(s)) == _INVALID and "no ground" in err()
    assert dyn(s) == _INVALID and "no ground" in err()
    with pytest.raises(RuntimeError, match="no ground"):
        sim.setBodyPoints(joints0, offsets0)
    with pytest.raises(RuntimeError, match="no ground"):
        sim.lastBodyContacts()
    assert not any(sim.bodyPointsDevicePointers().values())
    sim.setGround(ground_z=gz)
    sim.setBodyPoints(None)  # (nothing to clear)
    assert not any(sim.bodyPointsDevicePointers().values())
    assert not any(v.any() for v in sim.lastBodyContacts().values())  # (zeros while no points are set)
    near = body_points(name)
    sim.setBodyPoints(*near, band=BAND)
    ptrs = sim.bodyPointsDevicePointers()
    assert all(ptrs.values())
    assert not any(v.any() for v in sim.lastBodyContacts().values())  # (zeros before the first step)
    td = alloc(tau)

    def some_steps(h):
        Xd = alloc(X)
        for _ in range(12):  # (the robots land inside 20 ms)
            h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        return Xd.get(), h.lastGroundForces(), h.lastAccelerations(), h.lastBodyContacts()["body_slots"]

    twin = SIM.make(name, 3, lib, B)[2]
    twin.setGround(ground_z=gz)
    twin.setBodyPoints(*near, band=BAND)
    want = some_steps(twin)
    assert want[1].any() and want[3].any()
    nan, inf = float("nan"), float("inf")
    refusals = [
        (dict(n=-1), ("n = -1",)),
        (dict(n=17), ("n = 17",)),
        (dict(joint=(0, nj)), ("joint[1] = %d" % nj,)),
        (dict(joint=(-1, 3)), ("joint[0] = -1",)),
        (dict(offset=((0.0, 0.0, 0.0), (0.1, nan, 0.0))), ("offset[1][1]", "finite")),
        (dict(offset=((inf, 0.0, 0.0), (0.1, 0.0, 0.0))), ("offset[0][0]", "finite")),
        (dict(band=-0.01), ("band", "-0.01")),
        (dict(band=nan), ("band", "finite")),
        (dict(band=inf), ("band", "finite")),
    ]
    for kw, words in refusals:
        s = raw(**kw)
        assert L.smpc_robot_sim_set_body_points(sim._h, C.byref(s)) == _INVALID, words
        assert "body points" in err() and all(w in err() for w in words), (words, err())
        assert dyn(s) == _INVALID and all(w in err() for w in words), (words, err())
        assert sim.bodyPointsDevicePointers() == ptrs
    with pytest.raises(RuntimeError, match="n = 17"):
        sim.setBodyPoints(np.zeros(17, int), np.zeros((17, 3)))
    with pytest.raises(RuntimeError, match="expected"):
        sim.setBodyPoints([0, 1], np.zeros((3, 3)))
    got = some_steps(sim)  # (the previous points are in force)
    for u, v in zip(got, want):
        assert np.array_equal(u, v)
    # the host-buffer solve admits null outputs and null points
    s = raw()
    assert dyn(s) == 0, err()
    assert L.smpc_robot_sim_ground_points_dynamics(sim._h, B, X, tau, DT, None, None, None, None, 0, None, None, None, None, None, *none) == 0, err()
    assert sim.bodyPointsDevicePointers() == ptrs
    # no free slot: biped_legs with four points per foot
    _, _, full, _ = G.make("biped_legs", 4, lib, 1)
    s = raw(joint=(0, 1))
    assert L.smpc_robot_sim_set_body_points(full._h, C.byref(s)) == _INVALID and "no free slot" in err() and "2 * 4 = 8" in err()
    s0 = raw(n=0)
    assert L.smpc_robot_sim_set_body_points(full._h, C.byref(s0)) == 0  # (n = 0 clears, also there)
    # setGround drops the points
    sim.setGround(ground_z=gz)
    assert not any(sim.bodyPointsDevicePointers().values())
    plain = SIM.make(name, 3, lib, B)[2]
    plain.setGround(ground_z=gz)
    for u, v in zip(some_steps(sim)[:3], some_steps(plain)[:3]):
        assert np.array_equal(u, v)
    assert not np.array_equal(some_steps(plain)[0], want[0])


def test_box_points(built):
    """No GPU: the eight corners of a box, in the order of the docstring."""
    j, o = simple_mpc.box_points(3, (0.1, 0.0, -0.05), (0.2, 0.1, 0.04))
    assert j.dtype == np.int32 and (j == 3).all() and o.shape == (8, 3)
    assert np.array_equal(o[0], [0.1 - 0.2, 0.0 - 0.1, -0.05 - 0.04]) and np.array_equal(o[1], [0.1 + 0.2, 0.0 - 0.1, -0.05 - 0.04])
    assert np.array_equal(o[6], [0.1 - 0.2, 0.0 + 0.1, -0.05 + 0.04])
    assert len({tuple(r) for r in o}) == 8


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
Host = J.Host
GROUNDS = [False, True]


@pytest.mark.parametrize("rough", GROUNDS)
@pytest.mark.parametrize("name,P,seed", CASES)
def test_parity_with_the_checker(built, name, P, seed, rough):
    parity(name, P, ROUGH_SEED.get(name, seed) if rough else seed, rough, S.emu_lib())


@pytest.mark.parametrize("name,P,seed", CASES)
def test_points_outside_the_band_change_no_bit(built, name, P, seed):
    inert_points(name, P, seed, S.emu_lib(), Host)


@pytest.mark.parametrize("rough", GROUNDS)
def test_a_body_point_is_a_foot_point(built, rough):
    body_point_is_a_foot_point(S.emu_lib(), rough)


def test_admission_and_errors(built):
    admission(S.emu_lib(), Host)


@pytest.mark.parametrize("rough", GROUNDS)
def test_a_fallen_robot_lies_on_its_trunk(built, rough):
    fallen_robot_lies_on_its_trunk(S.emu_lib(), Host, rough)


def test_the_touch_mask_is_the_reset_mask(built):
    mask_is_the_reset_mask(S.emu_lib(), Host)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_batch_hygiene(built, name, P, seed):
    batch_hygiene(name, P, seed, S.emu_lib(), Host, True)
