"""Launch times of the ground step with per-robot body parameters, the method of tools/sim_joint_profile.py:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o body -- python3 tools/sim_body_profile.py run [batch]
    python3 tools/sim_body_profile.py summary <kernel_trace.csv> [batch]

`run`, per robot of RUNS, 30 fixed sweeps, WARM steps and then READINGS x LAUNCHES steps each, for the two joint models of
tools/sim_joint_profile.py (the inert one; damping, armature, effort limits and the stops on, from states with ten joints 0.03 rad inside a
limit): stepGroundDevice after setJointModel (sim_ground_joint_rt_body: the yardstick of the same run, the kernel of the parent commit
unchanged), then the same handle after setBodyParams with the table's rows repeated (sim_ground_body_rt_body: the same answers bit for bit).
`summary`: the dispatches of the trace whose grid is the full batch, in launch order, cut into the runs; per reading the mean of its LAUNCHES
dispatches, then the minimum of the readings and their spread."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, READINGS, LAUNCHES = 5, 3, 20
SWEEPS = 30
RUNS = [("go2_like", 3, 1), ("tree32p", 3, 1), ("biped_legs", 6, 4)]  # (robot, contact size of the handle, points per foot)
POINTS = {1: [(0.0, 0.0, 0.0)], 4: [(0.1, 0.05, 0.0), (0.1, -0.05, 0.0), (-0.1, 0.05, 0.0), (-0.1, -0.05, 0.0)]}
MODES = [("inert", False), ("inert", True), ("stops", False), ("stops", True)]  # (joint model, body parameters)


def run(B):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T

    for name, fs, P in RUNS:
        tab = T.table(name)
        rb = RT.oracle_robot(tab)
        na = rb.nv - 6
        lo, hi = np.array(tab.q_lo[:na]), np.array(tab.q_hi[:na])
        sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
        gz = float(rb.centroidal(rb.x_ref)["feet"][:, 2].min())
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        Xs = X.copy()
        for m, k in enumerate(np.random.default_rng(7).permutation(na)[:10]):
            Xs[:, 7 + k] = lo[k] + 0.03 if m % 2 == 0 else hi[k] - 0.03
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, na))).cuda()
        nominal = np.ascontiguousarray(np.tile(simple_mpc.body_params(tab), (B, 1, 1)))
        ends = {}
        for model, with_body in MODES:
            sim.setGround(ground_z=gz, points=POINTS[P], sweeps=SWEEPS)  # (drops the settings, the model and the bodies of the run before)
            sim.setGroundSolver(warm_start=False, tol=0.0)
            if model == "inert":
                sim.setJointModel(stops=False)
            else:
                sim.setJointModel(tau_max=np.full(na, 0.5), damping=np.full(na, 0.1), armature=np.full(na, 0.01), stops=True)
            if with_body:
                sim.setBodyParams(nominal)
            Xd = torch.from_numpy(np.ascontiguousarray(Xs if model == "stops" else X)).cuda()
            torch.cuda.synchronize()
            for k in range(WARM + READINGS * LAUNCHES):
                sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
            sim.wait()
            ends[(model, with_body)] = Xd.cpu().numpy()
        print(name, "P", P, "finite:", all(bool(np.isfinite(v).all()) for v in ends.values()), "the table's rows agree with no rows bit for bit:",
              all(bool(np.array_equal(ends[(m, False)], ends[(m, True)])) for m in ("inert", "stops")), flush=True)


def summary(trace, B):
    d = []  # (kernel, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_ground_joint_rt_body|sim_ground_body_rt_body)(?:<|ILi)(\d+)", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("%s<%s>" % m.groups(), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(RUNS) * len(MODES), len(d)
    print("| robot | points per foot | inert: `sim_ground_joint_rt_body` µs (spread) | `sim_ground_body_rt_body` µs (spread) | ratio | stops on: joint µs (spread) | body µs (spread) | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    k = 0
    for name, fs, P in RUNS:
        cells, names = [], []
        for model, with_body in MODES:
            blk = d[k * per: (k + 1) * per]
            k += 1
            assert len(set(n for n, _ in blk)) == 1 and ("body_rt" in blk[0][0]) == with_body, set(n for n, _ in blk)
            t = [v for _, v in blk[WARM:]]
            means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
            cells.append((min(means), 100 * (max(means) / min(means) - 1.0)))
            names.append(blk[0][0])
        print("| %s | %d | %s %.1f (%.1f %%) | %s %.1f (%.1f %%) | %.3f | %.1f (%.1f %%) | %.1f (%.1f %%) | %.3f |"
              % (name, P, names[0][-4:], cells[0][0], cells[0][1], names[1][-4:], cells[1][0], cells[1][1], cells[1][0] / cells[0][0], cells[2][0], cells[2][1],
                 cells[3][0], cells[3][1], cells[3][0] / cells[2][0]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
