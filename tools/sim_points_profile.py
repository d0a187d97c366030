"""Launch times of the ground step with body points, the method of tools/sim_terrain_profile.py:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o points -- python3 tools/sim_points_profile.py run [batch]
    python3 tools/sim_points_profile.py summary <kernel_trace.csv> [batch]

`run`, per robot of RUNS, 30 fixed sweeps, the inert joint model, the table's body rows repeated, WARM steps and then READINGS x LAUNCHES
steps each: stepGroundDevice after setBodyParams (sim_ground_body_rt_body: the kernel of the parent commit unchanged, <24> for the
quadrupeds, <32> for the biped), then the same handle after setBodyPoints with every point 10 m above the trunk (sim_ground_points_rt_body<32>
with no candidate: the same states bit for bit), then with a skid of S points 2 mm below the height of the feet under the trunk, S the
free slots of the robot (every slot taken, the robot resting on its trunk).  `summary`: the dispatches of the trace whose grid is the full
batch, in launch order, cut into the runs; per reading the mean of its LAUNCHES dispatches, then the minimum of the readings and their
spread."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, READINGS, LAUNCHES = 5, 3, 20
SWEEPS = 30
RUNS = [("go2_like", 3, 1), ("tree32p", 3, 1), ("biped_legs", 6, 1)]  # (robot, contact size of the handle, points per foot)
MODES = ["parent", "outside", "loaded"]


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
        sim = simple_mpc.BatchedRobotSim(RT.model_handler(tab), force_size=fs, batch=B)
        gz = float(rb.centroidal(rb.x_ref)["feet"][:, 2].min())
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        td = torch.from_numpy(np.random.default_rng(6).normal(0.0, 1.0, (B, na))).cuda()
        nominal = np.ascontiguousarray(np.tile(simple_mpc.body_params(tab), (B, 1, 1)))
        S = 8 - tab.nfeet * P
        ang = 2.0 * np.pi * np.arange(S) / S
        skid = np.c_[0.1 * np.cos(ang), 0.1 * np.sin(ang), np.full(S, gz - rb.x_ref[2] - 0.002)]
        ends, slots = {}, 0
        for mode in MODES:
            sim.setGround(ground_z=gz, sweeps=SWEEPS)  # (drops the settings, the model, the bodies and the points of the run before)
            sim.setGroundSolver(warm_start=False, tol=0.0)
            sim.setJointModel(stops=False)
            sim.setBodyParams(nominal)
            if mode == "outside":
                sim.setBodyPoints(np.zeros(S, np.int32), skid + np.array([0.0, 0.0, 10.0]))
            elif mode == "loaded":
                sim.setBodyPoints(np.zeros(S, np.int32), skid)
            Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            torch.cuda.synchronize()
            for k in range(WARM + READINGS * LAUNCHES):
                sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
            sim.wait()
            ends[mode] = Xd.cpu().numpy()
            if mode == "loaded":
                slots = float((sim.lastBodyContacts()["body_slots"] != 0).sum(1).mean())
        print(name, "P", P, "finite:", all(bool(np.isfinite(v).all()) for v in ends.values()), "points outside the band agree with the parent bit for bit:",
              bool(np.array_equal(ends["parent"], ends["outside"])), "the skid differs:", not np.array_equal(ends["parent"], ends["loaded"]),
              "mean slots in use at the last step: %.2f of %d" % (slots, S), flush=True)


def summary(trace, B):
    d = []  # (kernel, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_ground_body_rt_body|sim_ground_points_rt_body)(?:<|ILi)(\d+)", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("%s<%s>" % m.groups(), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(RUNS) * len(MODES), len(d)
    print("| robot | free slots | parent: `sim_ground_body_rt_body` µs (spread) | `sim_ground_points_rt_body<32>`, every point outside the band µs (spread) | ratio | every slot "
          "loaded µs (spread) | ratio |")
    print("|---|---|---|---|---|---|---|")
    k = 0
    for name, fs, P in RUNS:
        cells, names = [], []
        for mode in MODES:
            blk = d[k * per: (k + 1) * per]
            k += 1
            assert len(set(n for n, _ in blk)) == 1 and ("points_rt" in blk[0][0]) == (mode != "parent"), set(n for n, _ in blk)
            t = [v for _, v in blk[WARM:]]
            means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
            cells.append((min(means), 100 * (max(means) / min(means) - 1.0)))
            names.append(blk[0][0])
        print("| %s | %d | %s %.1f (%.1f %%) | %.1f (%.1f %%) | %.3f | %.1f (%.1f %%) | %.3f |"
              % (name, 4 if P == 1 and name != "biped_legs" else 6, names[0][-4:], cells[0][0], cells[0][1], cells[1][0], cells[1][1], cells[1][0] / cells[0][0],
                 cells[2][0], cells[2][1], cells[2][0] / cells[0][0]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
