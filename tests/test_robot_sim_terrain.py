"""Per-robot height-field terrain of the simulator (simple_mpc.BatchedRobotSim.setTerrain / terrainDevicePointers / lastTerrainNormals /
lastTerrainHeights / groundTerrainDynamics, simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h: sim_ground_terrain_rt_body<24> and <32>, DESIGN
3.28) against the numpy checker tests/ground_terrain_ref.py, against the kernels on a plane bit for bit (a flat tile) and at the project's
bar (a sampled tilted plane), and against itself across batch sizes.

CPU tier: the kernel body compiled with the sequential-lane test backend (tests/emu); tests/test_robot_sim_terrain_gpu.py runs the same
cases on the HIP library.  Bars (those of DESIGN 3.26 / 3.27): 1e-9 relative with max(1, |.|_inf) as the scale on v+, a, lambda, lam_stop,
normals and heights of one solve; integer outputs and contact words equal exactly (the terrain's seed is chosen on the checker so that no
decision is marginal); np.array_equal where the model promises equal bits."""
import ctypes as C

import numpy as np
import pytest

import ground_env_ref as ER
import ground_terrain_ref as TR
import ground_ws_ref as WR
import mpc_setup as S
import robot_tables as RT
import simple_mpc
import test_id_any_robot as T
import test_robot_sim_any_robot as SIM
import test_robot_sim_body_params as BP
import test_robot_sim_ground as G
import test_robot_sim_ground_env as E
import test_robot_sim_joint_model as J
from simple_mpc._capi import TerrainSettingsC

_INVALID = -1  # SMPC_ERR_INVALID (include/smpc.h)
DT, MU = G.DT, G.MU
CASES = J.CASES
TOL, MIN_SWEEPS, SWEEPS = J.TOL, J.MIN_SWEEPS, J.SWEEPS
ALL = J.SHARED + J.JOINT
NEW = ("normals", "heights")
TILES, NY, NX, CELL = 3, 4, 5, 0.12  # (T = 3 rough tiles of 5 x 4 nodes; a sole of 20 x 10 cm spans more than one cell)
ROUGH = 0.03                         # heights within +-3 cm of the reference foot height: slopes up to 0.5 per axis
TERRAIN_SEED = 5200  # (chosen on the checker alone: the conditions of parity() hold for the three cases)
_cache = {}


def terrain(name, seed, X):
    """(heights [3, 4, 5], tile [n], origin [n, 2]): every state its own tile and origin.  The grid (48 x 36 cm) lies below the robot,
    shifted by up to 8 cm per axis; every sixth state's grid is shifted by a further 25 / 20 cm, so that some of its points lie outside."""
    tab = T.table(name)
    gz = G.ground_height(RT.oracle_robot(tab))
    rng = np.random.default_rng(TERRAIN_SEED + seed)
    n = len(X)
    H = gz + rng.uniform(-ROUGH, ROUGH, (TILES, NY, NX))
    tile = rng.integers(0, TILES, n).astype(np.int32)
    origin = X[:, :2] - 0.5 * CELL * np.array([NX - 1, NY - 1]) + rng.uniform(-0.08, 0.08, (n, 2))
    far = np.arange(n) % 6 == 5
    origin[far] += np.array([0.25, 0.2]) * np.where(rng.uniform(size=(n, 2)) < 0.5, -1.0, 1.0)[far]
    return np.ascontiguousarray(H), tile, np.ascontiguousarray(origin)


def terrain_inputs(name, P, seed, n=24):
    """The inputs of the body-parameter test (states, mu, push, joint rows, bodies) on a terrain, with the checker's answers: computed
    once, shared, never modified."""
    key = ("inputs", name, P, seed, n)
    if key not in _cache:
        inp = BP.body_inputs(name, P, seed, n)
        X, tau, mu, push, j, tmax, dmp, arm, qlo, qhi, Bd, tabs = inp[0], inp[1], inp[3], inp[4], inp[5], inp[6], inp[7], inp[8], inp[9], inp[10], inp[11], inp[12]
        H, tile, origin = terrain(name, seed, X)
        ref = [TR.solve(RT.oracle_robot(tabs[i]), tabs[i], X[i], tau[i], DT, H, CELL, tile[i], origin[i], mu[i], push[i], j, points=G.points(P), sweeps=SWEEPS,
                        tol=TOL, min_sweeps=MIN_SWEEPS, tau_max=tmax[i], damping=dmp[i], armature=arm[i], q_lo=qlo[i], q_hi=qhi[i], stops=1) for i in range(n)]
        _cache[key] = (inp, H, tile, origin, ref)
    return _cache[key]


def kw_of(inp, rows, with_body=True):
    kw = BP.model_kw(inp, rows)
    del kw["planes"]
    if with_body:
        kw["body"] = inp[11][rows]
    return kw


def conditions(ref, P, name):
    """The input conditions of parity(), on the checker alone."""
    count = dict(free=0, stick=0, slide=0, pen=0)
    for r, m in ref:
        for k, v in ER.regimes(r, m).items():
            count[k] += int(v)
    split, outside, steep, edge = 0, 0, 0, np.inf
    for r, _ in ref:
        info = r["info"]
        two = False
        for f in range(len(info) // P):
            for a in range(f * P, (f + 1) * P):
                for b in range(a + 1, (f + 1) * P):
                    if info[a][:2] != info[b][:2] and np.abs(r["normals"][a] - r["normals"][b]).max() > 1e-6:
                        two = True
        split += int(two)
        for (i, j, u, v, x, y, slope) in info:
            out = not (0.0 <= x <= NX - 1 and 0.0 <= y <= NY - 1)
            outside += int(out)
            steep += int(slope > 0.2)
            for c, nn in ((x, NX), (y, NY)):
                if 0.0 <= c <= nn - 1:
                    edge = min(edge, abs(c - round(c)))
    decided = all(WR.decided(r["rhos"], TOL, MIN_SWEEPS) for r, _ in ref)
    margins = np.concatenate([r["margins"] for r, _ in ref])
    ok = (min(count.values()) >= 3 and (name != "biped_legs" or 2 * split >= len(ref)) and outside >= 3 and steep >= 10 and edge >= 1e-9 and decided
          and margins.min() >= 1e-9)
    return ok, (count, split, outside, steep, float(edge), decided, float(margins.min()))


# ---------------------------------------------------------------------------------------------------------------------- 1
def parity(name, P, seed, lib):
    """Case 1: groundTerrainDynamics on 24 states, each with its own tile, origin, mu, push, joint rows and bodies, against the checker.
    No solve and no point is left out of a comparison."""
    inp, H, tile, origin, ref = terrain_inputs(name, P, seed)
    X, tau, mu = inp[0], inp[1], inp[3]
    ok, what = conditions(list(zip(ref, mu)), P, name)
    print("%s P %d: checker: regimes %s; solves with two points of a foot on different facets %d; points outside the grid %d; on facets steeper than 0.2: %d; "
          "nearest cell boundary %.2e cells; sweeps decided %s; smallest stop margin %.2e" % ((name, P) + what))
    assert ok, what
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    out = sim.groundTerrainDynamics(X, tau, DT, H, CELL, tile=tile, origin=origin, **kw_of(inp, slice(None)))
    npts = P * tab.nfeet
    assert out["normals"].shape == (len(X), npts, 3) and out["heights"].shape == (len(X), npts)
    worst = dict(v_next=0.0, a=0.0, lam=0.0, lam_contact=0.0, lam_stop=0.0, normals=0.0, heights=0.0, gap=0.0)
    for i, r in enumerate(ref):
        for k in worst:
            worst[k] = max(worst[k], G._rel(out[k][i], r["lam_c" if k == "lam_contact" else k]))
    print("%s P %d: v+ %.2e  a %.2e  lambda %.2e  lambda (contact frame) %.2e  lam_stop %.2e  normals %.2e  heights %.2e  gap %.2e"
          % ((name, P) + tuple(worst[k] for k in ("v_next", "a", "lam", "lam_contact", "lam_stop", "normals", "heights", "gap"))))
    # (the plane gives other answers: the terrain is read)
    plain = sim.groundBodyDynamics(X, tau, DT, **kw_of(inp, slice(None)))
    assert G._rel(plain["a"], out["a"]) > 1e-3
    assert np.array_equal(out["contact"], np.array([r["contact"] for r in ref], np.uint32))
    assert np.array_equal(out["tau_applied"], np.array([r["tau_applied"] for r in ref]))
    assert np.array_equal(out["stop_rows"], np.array([r["stop_rows"] for r in ref])) and out["stop_rows"].dtype == np.int32
    assert np.array_equal(out["dropped"], np.array([r["dropped"] for r in ref]))
    assert np.array_equal(out["sweeps"], np.array([r["sweeps"] for r in ref]))
    assert max(worst.values()) < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------------- 2
def flat_tiles(gz):
    """A single 2 x 2 tile and a 3 x 2 one (nx = 3, ny = 2), every height ground_z."""
    return [(np.full((1, 2, 2), gz), 0.5), (np.full((1, 2, 3), gz), 0.07)]


def flat_tile_is_the_plane(name, P, seed, lib, alloc, steps=20):
    """Case 2: a tile whose heights all equal ground_z gives the bits of the kernels on the plane: the solve on 24 states against
    groundBodyDynamics on every shared output, 20 steps at B = 3 against a handle that never set a terrain (with and without a joint model
    and body parameters, set before or after), and setTerrain(None) gives the handle that never called it."""
    inp = terrain_inputs(name, P, seed)[0]
    X, tau, Bd = inp[0], inp[1], inp[11]
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    n, B = len(X), 3
    rng = np.random.default_rng(3)
    want = sim.groundBodyDynamics(X, tau, DT, **kw_of(inp, slice(None)))
    assert want["contact"].any() and want["stop_rows"].any()
    for H, cell in flat_tiles(gz):
        for origin in (None, X[:, :2] + rng.uniform(-0.3, 0.3, (n, 2))):
            got = sim.groundTerrainDynamics(X, tau, DT, H, cell, origin=origin, **kw_of(inp, slice(None)))
            for k in ALL:
                assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got["heights"], np.full_like(got["heights"], gz))
            assert np.array_equal(got["normals"], np.broadcast_to(np.array([0.0, 0.0, 1.0]), got["normals"].shape)) and not np.signbit(got["normals"]).any()
    X0, tq = G.drop_states(rb, B, 71)
    na = rb.nv - 6
    jm = dict(tau_max=np.full(na, 3.0), damping=np.full((B, na), 0.2), armature=np.full(na, 0.01), stops=True)
    H, cell = flat_tiles(gz)[1]
    rough = np.ascontiguousarray(gz + rng.uniform(-0.02, 0.02, (1, 6, 6)))

    def handle(order):
        _, _, h, _ = G.make(name, P, lib, B)
        for what in order:
            if what == "warm":
                h.setGroundSolver(warm_start=True, tol=1e-6, min_sweeps=0)
            elif what == "joint":
                h.setJointModel(**jm)
            elif what == "body":
                h.setBodyParams(Bd[:B])
            elif what == "flat":
                h.setTerrain(H, cell, origin=X0[:, :2] - 0.05)
            elif what == "rough":
                h.setTerrain(rough, 0.15, origin=X0[:, :2] - 0.375)
            elif what == "clear":
                h.setTerrain(None)
        return h

    def run(h):
        Xd, td = alloc(X0), alloc(tq)
        trace = []
        for _ in range(steps):
            h.stepGroundDevice(Xd.ptr, td.ptr, DT)
            h.wait()
            trace.append((Xd.get(), h.lastGroundForces(), h.lastContacts(), h.lastAccelerations()))
        return trace

    groups = [
        [(), ("flat",), ("rough", "clear"), ("clear",)],
        [("warm", "joint"), ("warm", "joint", "flat"), ("flat", "warm", "joint"), ("rough", "joint", "warm", "clear")],
        [("warm", "joint", "body"), ("flat", "warm", "joint", "body"), ("warm", "body", "flat", "joint"), ("body", "rough", "joint", "warm", "clear")],
    ]
    for group in groups:
        want = run(handle(group[0]))
        assert any(t[2].all() for t in want) and np.abs(want[-1][0] - X0).max() > 1e-4  # (every robot has landed)
        for order in group[1:]:
            h = handle(order)
            got = run(h)
            for k, (g, w) in enumerate(zip(got, want)):
                assert all(np.array_equal(u, v) for u, v in zip(g, w)), (order, k)
            on = order[-1] != "clear" and "flat" in order
            ptrs = h.terrainDevicePointers()
            assert bool(ptrs["heights"]) == on and bool(ptrs["tile"]) == on and bool(ptrs["origin"]) == on
            assert (ptrs["nx"], ptrs["ny"], ptrs["tiles"], ptrs["cell"]) == ((3, 2, 1, cell) if on else (0, 0, 0, 0.0))
            if on:
                assert np.array_equal(h.lastTerrainHeights(), np.full((B, P * tab.nfeet), gz))
                assert np.array_equal(h.lastTerrainNormals(), np.broadcast_to(np.array([0.0, 0.0, 1.0]), (B, P * tab.nfeet, 3)))
                assert np.array_equal(alloc.read(ptrs["origin"], (B, 2)), X0[:, :2] - 0.05) and np.array_equal(alloc.read(ptrs["heights"], (1, 2, 3)), H)
    # (and a rough tile moves the robots elsewhere)
    moved = run(handle(("rough",)))
    assert np.abs(moved[-1][0] - run(handle(()))[-1][0]).max() > 1e-5


# ---------------------------------------------------------------------------------------------------------------------- 3
PLANE_TILT = 0.3


def sampled_plane_is_the_plane(name, P, seed, lib):
    """Case 3: the plane n . p = d (tilted by 0.3 rad) sampled onto a tile against groundEnvDynamics on that plane, 1e-9 relative; contact
    words equal.  No checker takes part."""
    inp = terrain_inputs(name, P, seed)[0]
    X, tau, mu, push, j = inp[0], inp[1], inp[3], inp[4], inp[5]
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    n = len(X)
    ax = np.array([np.cos(0.7), np.sin(0.7), 0.0])
    c, s = np.cos(PLANE_TILT), np.sin(PLANE_TILT)
    nrm = np.array([ax[1] * s, -ax[0] * s, c])  # (e_z turned by the tilt about the horizontal axis ax)
    nrm = nrm / np.linalg.norm(nrm)
    d = float(nrm @ np.r_[X[0, :2], gz])
    cell, nn = 0.15, 21  # (3 m square: every contact point of every state lies inside, also with a leg stretched out at a joint limit)
    origin = np.tile(X[0, :2] - 0.5 * cell * (nn - 1), (n, 1))
    H = simple_mpc.terrain_from_function(lambda x, y: (d - nrm[0] * (x + origin[0, 0]) - nrm[1] * (y + origin[0, 1])) / nrm[2], nn, nn, cell)
    want = sim.groundEnvDynamics(X, tau, DT, planes=np.tile(np.r_[nrm, d], (n, 1)), mu=mu, push=push, joint=j)
    got = sim.groundTerrainDynamics(X, tau, DT, H, cell, origin=origin, mu=mu, push=push, joint=j, stops=False)
    worst = {k: G._rel(got[k], want[k]) for k in ("v_next", "a", "lam", "gap")}
    worst["normals"] = float(np.abs(got["normals"] - nrm).max())
    print("%s P %d: sampled plane against the plane: v+ %.2e  a %.2e  lambda %.2e  gap %.2e  normals %.2e; contacts %d of %d states"
          % (name, P, worst["v_next"], worst["a"], worst["lam"], worst["gap"], worst["normals"], int((want["contact"] != 0).sum()), n))
    assert (want["contact"] != 0).sum() >= 3
    assert np.array_equal(got["contact"], want["contact"])
    assert max(worst.values()) < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------------- 4
SCALE_DAMPING, SCALE_STEPS, SCALE_LAST, GRAVITY = BP.SCALE_DAMPING, BP.SCALE_STEPS, BP.SCALE_LAST, BP.GRAVITY
SCALE_CELL, SCALE_N, SCALE_ROUGH = 0.1, 9, 0.015
SCALE_SHIFT = np.array([[0.0, 0.0], [0.033, -0.021], [-0.047, 0.038]])


def scale_terrain(rb):
    gz = G.ground_height(rb)
    H = gz + np.random.default_rng(77).uniform(-SCALE_ROUGH, SCALE_ROUGH, (1, SCALE_N, SCALE_N))
    origin = rb.x_ref[:2] - 0.5 * SCALE_CELL * (SCALE_N - 1) + SCALE_SHIFT
    return np.ascontiguousarray(H), np.ascontiguousarray(origin)


def scale_loop(steps=SCALE_STEPS):
    """The checker's host loop of case 4: go2_like on one rough tile at three origins, zero torque, the legs sinking against SCALE_DAMPING
    N m s / rad, warm-started solves of exactly SWEEPS sweeps: the summed world force over the last SCALE_LAST steps per robot [3][3]."""
    key = ("scale", steps)
    if key not in _cache:
        tab = T.table("go2_like")
        rb = RT.oracle_robot(tab)
        H, origin = scale_terrain(rb)
        na = rb.nv - 6
        sums = []
        for i in range(len(origin)):
            x, w, acc = rb.x_ref.copy(), None, np.zeros(3)
            for k in range(steps):
                x, w, r = TR.step(rb, tab, x, np.zeros(na), DT, H, SCALE_CELL, 0, origin[i], MU, w=w, warm_start=k > 0, sweeps=SWEEPS,
                                  damping=np.full(na, SCALE_DAMPING), stops=0)
                if k >= steps - SCALE_LAST:
                    acc += r["lam"].reshape(-1, 3).sum(0)
            sums.append(acc)
        _cache[key] = np.array(sums)
    return _cache[key]


def scale_reads_the_weight(lib, alloc, steps=SCALE_STEPS):
    """Case 4: three go2_like on one rough tile at three origins stand on a scale: the sum over the points of lambda_world, averaged over
    the last 50 of 300 steps, against (0, 0, m g), horizontal components included; the gate is ten times the checker's own deviation."""
    name, B = "go2_like", 3
    ref = scale_loop(steps) / SCALE_LAST
    tab = T.table(name)
    want = np.array([0.0, 0.0, tab.total_mass * GRAVITY])
    dev_ref = np.linalg.norm(ref - want, axis=1) / want[2]
    print("go2_like on the rough scale: checker: mean force %s N, m g %.4f N, relative deviation %s" % (ref.tolist(), want[2], dev_ref))
    assert (dev_ref < 0.05).all()  # (quasi-static)
    _, rb, sim, gz = G.make(name, 1, lib, B, sweeps=SWEEPS)
    H, origin = scale_terrain(rb)
    na = rb.nv - 6
    sim.setGroundSolver(warm_start=True)
    sim.setJointModel(damping=np.full(na, SCALE_DAMPING), stops=False)
    sim.setTerrain(H, SCALE_CELL, origin=origin)
    Xd, td = alloc(np.tile(rb.x_ref, (B, 1))), alloc(np.zeros((B, na)))
    acc = np.zeros((B, 3))
    tilted = 0.0
    for k in range(steps):
        sim.stepGroundDevice(Xd.ptr, td.ptr, DT)
        if k >= steps - SCALE_LAST:
            sim.wait()
            acc += sim.lastGroundForces().reshape(B, -1, 3).sum(1)
            tilted = max(tilted, float(np.abs(sim.lastTerrainNormals()[..., :2]).max()))
    sim.wait()
    got = acc / SCALE_LAST
    dev = np.linalg.norm(got - want, axis=1) / want[2]
    err = np.abs(got - ref).max(1) / want[2]
    print("go2_like on the rough scale: kernel: mean force %s N; against the checker %s; relative deviation from m g %s; largest tilt of a normal %.3f"
          % (got.tolist(), err, dev, tilted))
    assert tilted > 0.05  # (the individual normals are tilted: the horizontal components cancel only if every point is rotated by its own frame)
    assert (dev <= 10.0 * dev_ref).all(), (dev, dev_ref)


# ---------------------------------------------------------------------------------------------------------------------- 5
def batch_hygiene(name, P, seed, lib, alloc, emulated):
    """Case 5: robot i's outputs depend on its own tile and origin only: not on the neighbours', not on the batch of the handle (1, 3, 5),
    not on n of the host-buffer solve (T = 3, nx != ny); a robot 1e6 m outside its grid gets finite outputs equal to the checker's; on the
    emulated tier a NaN in robot 1's state leaves robots 0 and 2 unchanged bit for bit."""
    inp, H, tile, origin, ref = terrain_inputs(name, P, seed)
    X, tau, mu, push, j = inp[0], inp[1], inp[3], inp[4], inp[5]
    keys = ALL + NEW
    rows = [1, 2, 7, 4, 10]
    tab, rb, sim, gz = G.make(name, P, lib, 3, sweeps=SWEEPS)
    five = sim.groundTerrainDynamics(X[rows], tau[rows], DT, H, CELL, tile=tile[rows], origin=origin[rows], **kw_of(inp, rows))
    assert five["contact"].any() and len(set(tile[rows])) > 1
    # the neighbours' tiles and origins
    t2, o2 = tile[rows].copy(), origin[rows].copy()
    t2[[0, 2, 3, 4]] = (t2[[0, 2, 3, 4]] + 1) % TILES
    o2[[0, 2, 3, 4]] += 0.05
    other = sim.groundTerrainDynamics(X[rows], tau[rows], DT, H, CELL, tile=t2, origin=o2, **kw_of(inp, rows))
    for k in keys:
        assert np.array_equal(other[k][1], five[k][1]), k
    assert not np.array_equal(other["heights"][0], five["heights"][0])
    # n of the solve, on handles of batch 1, 3 and 5
    for batch in (1, 3, 5):
        _, _, h, _ = G.make(name, P, lib, batch, sweeps=SWEEPS)
        for n in (1, 3, 5):
            sub = rows[5 - n :]
            out = h.groundTerrainDynamics(X[sub], tau[sub], DT, H, CELL, tile=tile[sub], origin=origin[sub], **kw_of(inp, sub))
            for k in keys:
                assert np.array_equal(out[k], five[k][5 - n :]), (k, batch, n)
        # the handle's step with the same settings: robot i reads tile[i] and origin[i]
        sub = rows[:batch]
        kw = kw_of(inp, sub)
        h.setGroundEnv(mu=kw["mu"])
        h.setPush(kw["push"], joint=kw["joint"])
        h.setGroundSolver(warm_start=False, tol=TOL, min_sweeps=MIN_SWEEPS)
        h.setTerrain(H, CELL, tile=tile[sub], origin=origin[sub])
        h.setBodyParams(kw["body"])
        h.setJointModel(**{k: kw[k] for k in ("tau_max", "damping", "armature", "q_lo", "q_hi", "stops")})
        Xd, td = alloc(X[sub]), alloc(tau[sub])
        h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        assert np.array_equal(h.lastAccelerations(), five["a"][:batch]) and np.array_equal(h.lastGroundForces(), five["lam"][:batch]), batch
        assert np.array_equal(Xd.get()[:, rb.nq :], five["v_next"][:batch]) and np.array_equal(h.lastGroundSweeps(), five["sweeps"][:batch])
        assert np.array_equal(h.lastTerrainNormals(), five["normals"][:batch]) and np.array_equal(h.lastTerrainHeights(), five["heights"][:batch])
        ptrs = h.terrainDevicePointers()
        assert np.array_equal(alloc.read(ptrs["heights"], (TILES, NY, NX)), H) and np.array_equal(alloc.read(ptrs["origin"], (batch, 2)), origin[sub])
        assert (ptrs["nx"], ptrs["ny"], ptrs["tiles"], ptrs["cell"]) == (NX, NY, TILES, CELL)
    # 1e6 m outside the grid: every coordinate is clamped, the outputs are finite and the checker's
    i = rows[1]
    tabs = inp[12]
    for shift in (np.array([1e6, -1e6]), np.array([-1e6, 1e6])):
        far = origin[[i]] + shift
        out = sim.groundTerrainDynamics(X[[i]], tau[[i]], DT, H, CELL, tile=tile[[i]], origin=far, **kw_of(inp, [i]))
        kw = kw_of(inp, [i])
        r = TR.solve(RT.oracle_robot(tabs[i]), tabs[i], X[i], tau[i], DT, H, CELL, tile[i], far[0], mu[i], push[i], j, points=G.points(P), sweeps=SWEEPS, tol=TOL,
                     min_sweeps=MIN_SWEEPS, tau_max=kw["tau_max"][0], damping=kw["damping"][0], armature=kw["armature"][0], q_lo=kw["q_lo"][0],
                     q_hi=kw["q_hi"][0], stops=1)
        assert all(np.isfinite(out[k]).all() for k in keys)
        for k in ("v_next", "a", "lam", "lam_stop", "normals", "heights", "gap"):
            assert G._rel(out[k][0], r[k]) < 1e-9, k
        assert out["contact"][0] == r["contact"] and out["sweeps"][0] == r["sweeps"]
        assert all(inf[0] in (0, NX - 2) and inf[1] in (0, NY - 2) and inf[2] in (0.0, 1.0) and inf[3] in (0.0, 1.0) for inf in r["info"])
    if emulated:
        sub = rows[:3]
        Xn = X[sub].copy()
        Xn[1, 0] = np.nan
        Xn[1, rb.nq + 7] = np.nan
        out = sim.groundTerrainDynamics(Xn, tau[sub], DT, H, CELL, tile=tile[sub], origin=origin[sub], **kw_of(inp, sub))
        for k in keys:
            assert np.array_equal(out[k][[0, 2]], five[k][[0, 2]]), k
        assert np.isnan(out["a"][1]).any()


# ---------------------------------------------------------------------------------------------------------------------- 7
def admission(lib, alloc):
    """Case 7: every refusal through the C ABI names the field and the index and keeps the previous terrain; setTerrain before setGround
    is refused; setGround drops the terrain."""
    lib = lib or simple_mpc.default_lib()
    L = lib.L
    err = lambda: L.smpc_last_error().decode()
    name, B = "go2_like", 3
    tab, rb, sim = SIM.make(name, 3, lib, B)
    gz = G.ground_height(rb)
    rng = np.random.default_rng(5)
    good = np.ascontiguousarray(gz + rng.uniform(-0.02, 0.02, (2, 4, 6)))
    tile0 = np.array([0, 1, 1], np.int32)
    origin0 = np.ascontiguousarray(np.tile(rb.x_ref[:2], (B, 1)) - np.array([0.3, 0.18]))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)

    def raw(H, cell=0.12, tile=tile0, origin=origin0, dims=None):
        H = np.ascontiguousarray(H)
        t, ny, nx = dims or H.shape
        return TerrainSettingsC(nx, ny, t, cell, p(H), p(tile), p(origin)), (H, tile, origin)

    def set_raw(*a, **k):
        t, keep = raw(*a, **k)
        return L.smpc_robot_sim_set_terrain(sim._h, C.byref(t))

    # no ground yet
    assert set_raw(good) == _INVALID and "no ground" in err()
    with pytest.raises(RuntimeError, match="no ground"):
        sim.setTerrain(good, 0.12)
    X, tau = G.drop_states(rb, B, 71)
    none = [None] * 14
    t, keep = raw(good)
    assert L.smpc_robot_sim_ground_terrain_dynamics(sim._h, B, X, tau, DT, C.byref(t), None, None, 0, None, None, None, None, *none) == _INVALID and "no ground" in err()
    assert sim.terrainDevicePointers()["heights"] == 0
    sim.setGround(ground_z=gz)
    sim.setTerrain(None)  # (nothing to clear)
    assert sim.terrainDevicePointers()["heights"] == 0
    with pytest.raises(RuntimeError, match="no terrain"):
        sim.lastTerrainNormals()
    assert L.smpc_robot_sim_ground_terrain_dynamics(sim._h, B, X, tau, DT, None, None, None, 0, None, None, None, None, *none) == _INVALID and "terrain is null" in err()
    sim.setTerrain(good, 0.12, tile=tile0, origin=origin0)
    ptrs = sim.terrainDevicePointers()
    assert ptrs["heights"] and (ptrs["nx"], ptrs["ny"], ptrs["tiles"]) == (6, 4, 2)
    assert not sim.lastTerrainNormals().any() and not sim.lastTerrainHeights().any()  # (zeros before the first step)
    td = alloc(tau)

    def some_steps(h):
        Xd = alloc(X)
        for _ in range(12):  # (the robots land inside 20 ms)
            h.stepGroundDevice(Xd.ptr, td.ptr, DT)
        h.wait()
        return Xd.get(), h.lastGroundForces(), h.lastAccelerations()

    twin = SIM.make(name, 3, lib, B)[2]
    twin.setGround(ground_z=gz)
    twin.setTerrain(good, 0.12, tile=tile0, origin=origin0)
    want = some_steps(twin)
    assert want[1].any()
    nan, inf = float("nan"), float("inf")

    def bad(at, value):
        a = good.copy()
        a[at] = value
        return a

    steep = good.copy()
    steep[1, 2, 3] += 0.3  # (0.3 m over a cell of 0.12 m in x and in y: hx^2 + hy^2 = 12.5)
    refusals = [
        (dict(H=good, dims=(2, 4, 1)), ("nx = 1",)),
        (dict(H=good, dims=(2, 1, 6)), ("ny = 1",)),
        (dict(H=good, dims=(0, 4, 6)), ("tiles = 0",)),
        (dict(H=good, dims=(4096, 2048, 2048)), ("nodes", "cap")),
        (dict(H=good, cell=0.0), ("cell", "positive")),
        (dict(H=good, cell=-0.1), ("cell", "positive")),
        (dict(H=good, cell=nan), ("cell",)),
        (dict(H=good, cell=inf), ("cell", "finite")),
        (dict(H=bad((1, 2, 3), nan)), ("heights[1][2][3]", "finite")),
        (dict(H=bad((0, 3, 5), -inf)), ("heights[0][3][5]", "finite")),
        (dict(H=good, tile=np.array([0, 2, 1], np.int32)), ("tile[1] = 2",)),
        (dict(H=good, tile=np.array([0, 1, -1], np.int32)), ("tile[2] = -1",)),
        (dict(H=good, origin=np.array([[0.0, 0.0], [0.0, nan], [0.0, 0.0]])), ("origin[1][1]", "finite")),
        (dict(H=good, origin=np.array([[0.0, 0.0], [0.0, 0.0], [inf, 0.0]])), ("origin[2][0]", "finite")),
        (dict(H=steep), ("slope[1][1][2]", "above 3")),
    ]
    for kw, words in refusals:
        assert set_raw(**kw) == _INVALID, words
        assert "terrain" in err() and all(w in err() for w in words), (words, err())
        t, keep = raw(**kw)
        assert L.smpc_robot_sim_ground_terrain_dynamics(sim._h, B, X, tau, DT, C.byref(t), None, None, 0, None, None, None, None, *none) == _INVALID
        assert all(w in err() for w in words), (words, err())
        assert sim.terrainDevicePointers() == ptrs and np.array_equal(alloc.read(ptrs["heights"], good.shape), good)
    with pytest.raises(RuntimeError, match="slope"):
        sim.setTerrain(steep, 0.12)
    t, keep = raw(good, origin=None, tile=None)
    t.heights = None
    assert L.smpc_robot_sim_set_terrain(sim._h, C.byref(t)) == _INVALID and "heights is null" in err()
    for wrong in (dict(tile=tile0[:2]), dict(origin=origin0[:, :1]), dict(origin=origin0[:2])):
        with pytest.raises(RuntimeError, match="expected"):
            sim.setTerrain(good, 0.12, **wrong)
    with pytest.raises(RuntimeError, match="heights"):
        sim.setTerrain(good[0, 0], 0.12)
    got = some_steps(sim)
    for u, v in zip(got, want):
        assert np.array_equal(u, v)
    assert np.abs(sim.lastTerrainNormals()[..., :2]).max() > 1e-3 and np.abs(sim.lastTerrainHeights() - gz).max() <= 0.02
    # the host-buffer solve admits null outputs, a null tile and a null origin
    t, keep = raw(good, tile=None, origin=None)
    assert L.smpc_robot_sim_ground_terrain_dynamics(sim._h, B, X, tau, DT, C.byref(t), None, None, 0, None, None, None, None, *none) == 0, err()
    # setGround drops the terrain
    sim.setGround(ground_z=gz)
    assert sim.terrainDevicePointers()["heights"] == 0
    plain = SIM.make(name, 3, lib, B)[2]
    plain.setGround(ground_z=gz)
    for u, v in zip(some_steps(sim), some_steps(plain)):
        assert np.array_equal(u, v)
    assert not np.array_equal(some_steps(plain)[0], want[0])


# ---------------------------------------------------------------------------------------------------------------------- helpers
def test_helpers(built):
    """No GPU: terrain_height is the checker's sampling bit for bit (NaN, +-inf, -0.0, 1e300, nodes and borders among the points);
    terrain_rough and terrain_stairs pass admission by construction, also where the request is too steep; amplitude 0 is exactly flat."""
    lib = S.emu_lib()
    rng = np.random.default_rng(9)
    H = rng.uniform(-0.05, 0.05, (4, 5))
    o = np.array([0.3, -0.2])
    xy = np.r_[rng.uniform(-0.3, 0.9, (40, 2)), [[0.3, -0.2], [0.3 + 4 * CELL, -0.2 + 3 * CELL], [0.3 + CELL, -0.2 + 2 * CELL], [np.nan, 0.0], [np.inf, -np.inf],
                                                   [-0.0, 1e300], [-1e300, 0.0]]]
    h, n = simple_mpc.terrain_height(H, CELL, o, xy)
    for k in range(len(xy)):
        hk, nk, info = TR.sample(H, CELL, o, xy[k])
        assert h[k] == hk and np.array_equal(n[k], nk), (k, xy[k])
        assert 0 <= info[0] <= 3 and 0 <= info[1] <= 2 and 0.0 <= info[2] <= 1.0 and 0.0 <= info[3] <= 1.0
    nan_x, inf_xy = TR.sample(H, CELL, o, xy[-4])[2], TR.sample(H, CELL, o, xy[-3])[2]
    assert (nan_x[0], nan_x[2]) == (0, 0.0) and inf_xy[:4] == (0, 0, 0.0, 0.0)
    h1, n1 = simple_mpc.terrain_height(H, CELL, o, xy[3])
    assert h1 == h[3] and np.array_equal(n1, n[3])
    flat, nf = simple_mpc.terrain_height(np.full((2, 2), 0.37), 0.5, np.zeros(2), xy)
    assert (flat == 0.37).all() and np.array_equal(nf, np.broadcast_to(np.array([0.0, 0.0, 1.0]), nf.shape)) and not np.signbit(nf).any()
    f = simple_mpc.terrain_from_function(lambda x, y: 0.1 * x - 0.2 * y, 6, 4, 0.25)
    assert f.shape == (4, 6) and f[2, 3] == 0.1 * 0.75 - 0.2 * 0.5
    hp, npl = simple_mpc.terrain_height(f, 0.25, np.zeros(2), np.array([0.4, 0.3]))
    assert abs(hp - (0.04 - 0.06)) < 1e-15 and np.abs(npl - np.array([-0.1, 0.2, 1.0]) / np.sqrt(1.05)).max() < 1e-15
    tab, rb, sim = SIM.make("go2_like", 3, lib, 1)
    sim.setGround(ground_z=0.0)
    for amp, wl in ((0.0, 0.5), (0.03, 0.5), (0.5, 0.05), (5.0, 0.3)):
        R = simple_mpc.terrain_rough(np.random.default_rng(1), 12, 9, 0.1, amp, wl)
        assert R.shape == (9, 12) and np.abs(R).max() <= amp * (1 + 1e-12)
        assert amp > 0.0 or not R.any()
        assert amp != 0.03 or abs(np.abs(R).max() - amp) < 1e-12
        sim.setTerrain(R, 0.1)
    for rise, run, ramp in ((0.05, 0.4, 0.1), (0.15, 0.3, 0.01), (0.5, 0.2, 0.05), (-0.1, 0.35, 0.1)):
        St = simple_mpc.terrain_stairs(20, 3, 0.05, rise, run, ramp)
        assert St.shape == (3, 20) and (St == St[0]).all() and (np.diff(St[0]) * np.sign(rise) >= 0.0).all()
        sim.setTerrain(St, 0.05)
    St = simple_mpc.terrain_stairs(20, 3, 0.05, 0.05, 0.4, 0.1)
    assert St[0, 0] == 0.0 and abs(St[0, 8] - 0.05) < 1e-15 and abs(St[0, 7] - 0.025) < 1e-15 and St[0, 6] == 0.0 and abs(St[0, 16] - 0.1) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
Host = J.Host


@pytest.mark.parametrize("name,P,seed", CASES)
def test_parity_with_the_checker(built, name, P, seed):
    parity(name, P, seed, S.emu_lib())


@pytest.mark.parametrize("name,P,seed", CASES)
def test_a_flat_tile_is_the_plane_bit_for_bit(built, name, P, seed):
    flat_tile_is_the_plane(name, P, seed, S.emu_lib(), Host)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_a_sampled_plane_is_the_plane(built, name, P, seed):
    sampled_plane_is_the_plane(name, P, seed, S.emu_lib())


def test_the_scale_reads_the_weight_on_rough_ground(built):
    scale_reads_the_weight(S.emu_lib(), Host)


@pytest.mark.parametrize("name,P,seed", CASES)
def test_batch_hygiene(built, name, P, seed):
    batch_hygiene(name, P, seed, S.emu_lib(), Host, True)


def test_admission_and_errors(built):
    admission(S.emu_lib(), Host)
