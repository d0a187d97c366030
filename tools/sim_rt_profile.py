"""Launch times of the simulator step: the templated pair of a kinodynamics handle (full_fd_body + sim_integrate_body) and the one-launch
kernel on a run-time joint tree (sim_rt_body) side by side.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o sim -- python3 tools/sim_rt_profile.py run [batch]
    python3 tools/sim_rt_profile.py summary <kernel_trace.csv> [batch]

`run`: go2_like through BatchedMPC.simStepDevice of a kinodynamics handle (the yardstick), then BatchedRobotSim.stepDevice on go2_like,
quad_arm, the 32-joint point-foot table of tests/test_id_any_robot.py and tree32 with two 6-D contacts, one after the other; every foot in
contact, Baumgarte gains (0, 50), small random torques; per robot WARM steps, then READINGS x LAUNCHES steps -- the states move between
launches because every step integrates them.  `summary`: the dispatches of the trace whose grid is the full batch, per kernel in launch
order, cut into the robots' runs; per reading the mean of its LAUNCHES dispatches, then the minimum of the readings and their spread.

The ground plane, same method:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o ground -- python3 tools/sim_rt_profile.py run-ground [batch]
    python3 tools/sim_rt_profile.py summary-ground <kernel_trace.csv> [batch]

`run-ground`: per robot of GROUND_RUNS BatchedRobotSim.stepDevice (sim_rt_body, every foot in contact: the yardstick of the same run), then
stepGroundDevice with the plane at the reference foot height on both instantiations (a points-per-foot count that gives at most 12 rows,
one that gives more) at each of GROUND_SWEEPS sweeps.  `summary-ground`: one row per run, and the cost of a sweep as the slope between
the smallest and the largest sweep count.

The per-robot environment, same method:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o env -- python3 tools/sim_rt_profile.py run-env [batch]
    python3 tools/sim_rt_profile.py summary-env <kernel_trace.csv> [batch]

`run-env`: per robot of GROUND_RUNS, instantiation and sweep count stepGroundDevice on a handle without an environment (sim_ground_rt_body:
the yardstick of the same run), then on the same handle after setGroundEnv / setPush with the uniform environment (sim_ground_env_rt_body:
the same answers bit for bit).  `summary-env`: both columns, their ratio, the cost of a sweep and the intercept at zero sweeps of each.

The warm-started solve with a stopping rule, same method:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o ws -- python3 tools/sim_rt_profile.py run-ws [batch]
    python3 tools/sim_rt_profile.py summary-ws <kernel_trace.csv> [batch]

`run-ws`, per robot of WS_RUNS: (a) the cost of the bookkeeping -- at each of GROUND_SWEEPS sweeps stepGroundDevice after setGroundEnv / setPush
with the uniform environment (sim_ground_env_rt_body: the yardstick of the same run), then on the same handle after setGroundSolver with
warm_start = 0, tol = 0 (sim_ground_ws_rt_body: the same answers bit for bit); (b) what the feature buys -- robots at rest on the plane under
small random torques, tol = 1e-6, sweeps = 60, once cold and once warm, with the distribution of sweeps_used printed at launches 1, 5 and 20
after the warm-up.  `summary-ws`: (a) both columns, per-sweep cost and intercept of each; (b) launch µs cold and warm as the minimum of
the readings, and at launches 1, 5 and 20."""
import collections
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, READINGS, LAUNCHES = 5, 3, 20
RUNS = [("go2_like", 3, False), ("go2_like", 3, True), ("quad_arm", 3, True), ("tree32p", 3, True), ("tree32", 6, True)]  # (robot, contact size, run-time kernel)
GROUND_SWEEPS = (10, 30, 60)
# (robot, contact size of the bilateral yardstick, points per foot on sim_ground_rt_body<12>, on <24>)
GROUND_RUNS = [("go2_like", 3, 1, 2), ("quad_arm", 3, 1, 2), ("tree32p", 3, 1, 2), ("biped_legs", 6, 1, 4)]
GROUND_POINTS = {1: [(0.0, 0.0, 0.0)], 2: [(0.02, 0.0, 0.0), (-0.02, 0.0, 0.0)], 4: [(0.1, 0.05, 0.0), (0.1, -0.05, 0.0), (-0.1, 0.05, 0.0), (-0.1, -0.05, 0.0)]}


def run(B):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import mpc_setup as S
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T

    for name, fs, rt in RUNS:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        if rt:
            sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
            step = lambda x, t: sim.stepDevice(x, t, [True] * tab.nfeet, 1e-3, Kp=[0.0] * fs, Kd=[50.0] * fs)
        else:
            sim = S.make_product(B)[0]
            step = lambda x, t: sim.simStepDevice(x, t, [True] * 4, 1e-3, Kp=[0.0] * 3, Kd=[50.0] * 3)
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, rb.nv - 6))).cuda()
        torch.cuda.synchronize()
        for _ in range(WARM + READINGS * LAUNCHES):
            step(Xd.data_ptr(), td.data_ptr())
        sim.wait()
        Xh = Xd.cpu().numpy()
        print(name, "fs", fs, "run-time" if rt else "templated", "finite:", bool(np.isfinite(Xh).all()), "largest state change %.3f" % np.abs(Xh - X).max(), flush=True)


def run_ground(B):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T

    for name, fs, p12, p24 in GROUND_RUNS:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
        gz = float(rb.centroidal(rb.x_ref)["feet"][:, 2].min())
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, rb.nv - 6))).cuda()
        runs = [("sim_rt_body", None, None)] + [("ground", P, sw) for P in (p12, p24) for sw in GROUND_SWEEPS]
        for kind, P, sw in runs:
            if kind == "ground":
                sim.setGround(ground_z=gz, points=GROUND_POINTS[P], sweeps=sw)
                step = lambda x, t: sim.stepGroundDevice(x, t, 1e-3)
            else:
                step = lambda x, t: sim.stepDevice(x, t, [True] * tab.nfeet, 1e-3, Kp=[0.0] * fs, Kd=[50.0] * fs)
            Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            torch.cuda.synchronize()
            for _ in range(WARM + READINGS * LAUNCHES):
                step(Xd.data_ptr(), td.data_ptr())
            sim.wait()
            Xh = Xd.cpu().numpy()
            note = "" if kind != "ground" else " robots with a contact %d of %d" % (int((sim.lastContacts() != 0).sum()), B)
            print(name, kind, "P", P, "sweeps", sw, "finite:", bool(np.isfinite(Xh).all()), "largest state change %.3f" % np.abs(Xh - X).max() + note, flush=True)


def run_env(B):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T

    for name, fs, p12, p24 in GROUND_RUNS:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
        gz = float(rb.centroidal(rb.x_ref)["feet"][:, 2].min())
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, rb.nv - 6))).cuda()
        for P in (p12, p24):
            for sw in GROUND_SWEEPS:
                ends = []
                for env in (False, True):
                    sim.setGround(ground_z=gz, points=GROUND_POINTS[P], sweeps=sw)  # (drops the environment of the run before)
                    if env:
                        sim.setGroundEnv(planes=np.tile([0.0, 0.0, 1.0, gz], (B, 1)), mu=np.full(B, 0.7))
                        sim.setPush(np.zeros((B, 6)))
                    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
                    torch.cuda.synchronize()
                    for _ in range(WARM + READINGS * LAUNCHES):
                        sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
                    sim.wait()
                    ends.append(Xd.cpu().numpy())
                print(name, "P", P, "sweeps", sw, "finite:", bool(np.isfinite(ends[0]).all()), "the two kernels agree bit for bit:", bool(np.array_equal(ends[0], ends[1])),
                      flush=True)


WS_RUNS = [("go2_like", 3, 1), ("biped_legs", 6, 4)]  # (robot, contact size of the handle, points per foot): 4 points on <12>, 8 points on <24>
WS_TOL, WS_SWEEPS, WS_SAMPLES = 1e-6, 60, (1, 5, 20)


def run_ws(B):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T

    for name, fs, P in WS_RUNS:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
        gz = float(rb.centroidal(rb.x_ref)["feet"][:, 2].min())
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, rb.nv - 6))).cuda()
        # (a) the bookkeeping: inert settings against the kernel of the per-robot environment
        for sw in GROUND_SWEEPS:
            ends = []
            for ws in (False, True):
                sim.setGround(ground_z=gz, points=GROUND_POINTS[P], sweeps=sw)  # (drops the settings of the run before)
                sim.setGroundEnv(planes=np.tile([0.0, 0.0, 1.0, gz], (B, 1)), mu=np.full(B, 0.7))
                sim.setPush(np.zeros((B, 6)))
                if ws:
                    sim.setGroundSolver(warm_start=False, tol=0.0)
                Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
                torch.cuda.synchronize()
                for _ in range(WARM + READINGS * LAUNCHES):
                    sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
                sim.wait()
                ends.append(Xd.cpu().numpy())
            print(name, "P", P, "sweeps", sw, "inert settings: finite:", bool(np.isfinite(ends[0]).all()), "the two kernels agree bit for bit:",
                  bool(np.array_equal(ends[0], ends[1])), flush=True)
        # (b) at rest on the plane, cold and warm
        X0 = np.tile(rb.x_ref, (B, 1))
        for warm in (False, True):
            sim.setGround(ground_z=gz, points=GROUND_POINTS[P], sweeps=WS_SWEEPS)
            sim.setGroundSolver(warm_start=warm, tol=WS_TOL)
            Xd = torch.from_numpy(np.ascontiguousarray(X0)).cuda()
            torch.cuda.synchronize()
            for k in range(WARM + READINGS * LAUNCHES):
                sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
                if k + 1 - WARM in WS_SAMPLES:
                    s = sim.lastGroundSweeps()  # (joins the stream)
                    q = np.percentile(s, [0, 10, 50, 90, 100]).astype(int).tolist()
                    print(name, "P", P, "warm" if warm else "cold", "launch", k + 1 - WARM, "sweeps_used min / 10 % / median / 90 % / max", q, "mean %.2f" % s.mean(),
                          "largest residual %.2e" % np.nanmax(sim.lastGroundResiduals()), flush=True)
            sim.wait()
            print(name, "P", P, "warm" if warm else "cold", "finite:", bool(np.isfinite(Xd.cpu().numpy()).all()), flush=True)


def summary_ws(trace, B):
    d = []  # (kernel, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_ground_env_rt_body|sim_ground_ws_rt_body)(?:<|ILi)(\d+)", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("%s<%s>" % m.groups(), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(WS_RUNS) * (2 * len(GROUND_SWEEPS) + 2), len(d)

    def reading(blk):
        t = [v for _, v in blk[WARM:]]
        means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
        return min(means), 100 * (max(means) / min(means) - 1.0), t

    print("| robot | rows | points | sweeps | `sim_ground_env_rt_body` µs (spread) | `sim_ground_ws_rt_body`, inert µs (spread) | ratio |")
    print("|---|---|---|---|---|---|---|")
    k, rest = 0, []
    for name, fs, P in WS_RUNS:
        cols = ([], [])
        for sw in GROUND_SWEEPS:
            cell = []
            for ws in (0, 1):
                blk = d[k * per: (k + 1) * per]
                k += 1
                assert len(set(n for n, _ in blk)) == 1 and ("ws" in blk[0][0]) == bool(ws), set(n for n, _ in blk)
                t, sp, _ = reading(blk)
                cols[ws].append(t)
                cell.append("%.1f (%.1f %%)" % (t, sp))
            print("| %s | %s | %d | %d | %s | %s | %.3f |" % (name, blk[0][0][-3:-1], P * T_NFEET[name], sw, cell[0], cell[1], cols[1][-1] / cols[0][-1]))
        span = GROUND_SWEEPS[-1] - GROUND_SWEEPS[0]
        slopes = [(c[-1] - c[0]) / span for c in cols]
        print("| %s |  | %d | per sweep / intercept | %.2f / %.1f | %.2f / %.1f | |"
              % (name, P * T_NFEET[name], slopes[0], cols[0][0] - GROUND_SWEEPS[0] * slopes[0], slopes[1], cols[1][0] - GROUND_SWEEPS[0] * slopes[1]))
        for warm in (0, 1):
            blk = d[k * per: (k + 1) * per]
            k += 1
            assert len(set(n for n, _ in blk)) == 1 and "ws" in blk[0][0], set(n for n, _ in blk)
            rest.append((name, P * T_NFEET[name], "warm" if warm else "cold") + reading(blk))
    print()
    print("| robot | points | start | launch µs, minimum of the readings (spread) | at launch %s |" % " / ".join(str(s) for s in WS_SAMPLES))
    print("|---|---|---|---|---|")
    for name, pts, start, t, sp, all_t in rest:
        print("| %s | %d | %s | %.1f (%.1f %%) | %s |" % (name, pts, start, t, sp, " / ".join("%.1f" % all_t[s - 1] for s in WS_SAMPLES)))


def summary_env(trace, B):
    d = []  # (kernel, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_ground_rt_body|sim_ground_env_rt_body)(?:<|ILi)(\d+)", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("%s<%s>" % m.groups(), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(GROUND_RUNS) * 2 * len(GROUND_SWEEPS) * 2, len(d)
    print("| robot | rows | points | sweeps | `sim_ground_rt_body` µs (spread) | `sim_ground_env_rt_body` µs (spread) | ratio |")
    print("|---|---|---|---|---|---|---|")
    k = 0
    for name, fs, p12, p24 in GROUND_RUNS:
        for P in (p12, p24):
            cols = ([], [])
            for sw in GROUND_SWEEPS:
                cell = []
                for env in (0, 1):
                    blk = d[k * per: (k + 1) * per]
                    k += 1
                    assert len(set(n for n, _ in blk)) == 1 and ("env" in blk[0][0]) == bool(env), set(n for n, _ in blk)
                    t = [v for _, v in blk[WARM:]]
                    means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
                    cols[env].append(min(means))
                    cell.append("%.1f (%.1f %%)" % (min(means), 100 * (max(means) / min(means) - 1.0)))
                print("| %s | %s | %d | %d | %s | %s | %.3f |" % (name, blk[0][0][-3:-1], P * T_NFEET[name], sw, cell[0], cell[1], cols[1][-1] / cols[0][-1]))
            span = GROUND_SWEEPS[-1] - GROUND_SWEEPS[0]
            slopes = [(c[-1] - c[0]) / span for c in cols]
            print("| %s |  | %d | per sweep / intercept | %.2f / %.1f | %.2f / %.1f | |"
                  % (name, P * T_NFEET[name], slopes[0], cols[0][0] - GROUND_SWEEPS[0] * slopes[0], slopes[1], cols[1][0] - GROUND_SWEEPS[0] * slopes[1]))


def summary_ground(trace, B):
    d = []  # (kernel, rows of the instantiation, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_rt_body|sim_ground_rt_body(?:<|ILi)(\d+))", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("sim_rt_body" if m.group(2) is None else "sim_ground_rt_body<%s>" % m.group(2), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(GROUND_RUNS) * (1 + 2 * len(GROUND_SWEEPS)), len(d)
    print("| robot | kernel | points | sweeps | step µs | spread of the readings | per sweep µs |")
    print("|---|---|---|---|---|---|---|")
    k = 0
    for name, fs, p12, p24 in GROUND_RUNS:
        for P in (None, p12, p24):
            times = []
            for sw in ((None,) if P is None else GROUND_SWEEPS):
                blk = d[k * per: (k + 1) * per]
                k += 1
                assert len(set(n for n, _ in blk)) == 1, set(n for n, _ in blk)
                t = [v for _, v in blk[WARM:]]
                means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
                times.append(min(means))
                slope = "" if sw != GROUND_SWEEPS[-1] else "%.2f" % ((times[-1] - times[0]) / (GROUND_SWEEPS[-1] - GROUND_SWEEPS[0]))
                print("| %s | `%s` | %s | %s | %.1f | %.1f %% | %s |" % (name, blk[0][0], "%d-D bilateral" % fs if P is None else str(P * T_NFEET[name]), sw or "", min(means),
                                                                       100 * (max(means) / min(means) - 1.0), slope))


T_NFEET = {"go2_like": 4, "quad_arm": 4, "tree32p": 4, "biped_legs": 2}


def summary(trace, B):
    fam = collections.defaultdict(list)  # kernel -> durations in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_rt_body|full_fd_body|sim_integrate_body)", r["Kernel_Name"])
        if m and grid == B * 64:
            fam[m.group(1)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    per = WARM + READINGS * LAUNCHES

    def reading(d):
        means = [sum(d[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
        return min(means), max(means) / min(means) - 1.0

    print("| robot | contacts | kernels | step µs | spread of the readings |")
    print("|---|---|---|---|---|")
    k, yard = 0, None
    for name, fs, rt in RUNS:
        if rt:
            d = fam["sim_rt_body"]
            assert len(d) == per * sum(r for _, _, r in RUNS), len(d)
            t, sp = reading(d[k * per + WARM: (k + 1) * per])
            ratio = "" if yard is None or name != "go2_like" else " (%.2fx the yardstick)" % (t / yard)
            print("| %s | %d-D | `sim_rt_body` | %.1f%s | %.1f %% |" % (name, fs, t, ratio, 100 * sp))
            k += 1
        else:
            a, b = fam["full_fd_body"], fam["sim_integrate_body"]
            assert len(a) >= per and len(b) >= per, (len(a), len(b))
            (ta, sa), (tb, sb) = reading(a[-per:][WARM:]), reading(b[-per:][WARM:])
            yard = ta + tb
            print("| %s (yardstick) | %d-D | `full_fd_body` %.1f + `sim_integrate_body` %.1f | %.1f | %.1f %% |" % (name, fs, ta, tb, yard, 100 * max(sa, sb)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif sys.argv[1] == "run-ground":
        run_ground(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif sys.argv[1] == "run-env":
        run_env(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif sys.argv[1] == "run-ws":
        run_ws(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif sys.argv[1] == "summary-ws":
        summary_ws(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
    elif sys.argv[1] == "summary-env":
        summary_env(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
    elif sys.argv[1] == "summary-ground":
        summary_ground(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
    else:
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
