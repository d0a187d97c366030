"""Launch times of the ground step on a per-robot height-field terrain, the method of tools/sim_body_profile.py:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o terrain -- python3 tools/sim_terrain_profile.py run [batch]
    python3 tools/sim_terrain_profile.py summary <kernel_trace.csv> [batch]

`run`, per robot of RUNS, 30 fixed sweeps, the inert joint model, the table's body rows repeated, WARM steps and then READINGS x LAUNCHES
steps each: stepGroundDevice after setBodyParams (sim_ground_body_rt_body: the yardstick of the same run, the kernel of the parent commit
unchanged), then the same handle after setTerrain with a flat tile at the ground's height (sim_ground_terrain_rt_body: the same states bit
for bit), then on a rough tile (heights within 2 cm of the ground's, T = 4 tiles of 64 x 64 nodes 5 cm apart, every robot at its own
origin).  `summary`: the dispatches of the trace whose grid is the full batch, in launch order, cut into the runs; per reading the mean of
its LAUNCHES dispatches, then the minimum of the readings and their spread."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, READINGS, LAUNCHES = 5, 3, 20
SWEEPS = 30
RUNS = [("go2_like", 3, 1), ("tree32p", 3, 1), ("biped_legs", 6, 4)]  # (robot, contact size of the handle, points per foot)
POINTS = {1: [(0.0, 0.0, 0.0)], 4: [(0.1, 0.05, 0.0), (0.1, -0.05, 0.0), (-0.1, 0.05, 0.0), (-0.1, -0.05, 0.0)]}
MODES = ["plane", "flat", "rough"]
TILES, NODES, CELL, ROUGH = 4, 64, 0.05, 0.02


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
        rng = np.random.default_rng(8)
        rough = gz + rng.uniform(-ROUGH, ROUGH, (TILES, NODES, NODES))
        tile = (np.arange(B) % TILES).astype(np.int32)
        origin = X[:, :2] - 0.5 * CELL * (NODES - 1) + rng.uniform(-0.5, 0.5, (B, 2))
        ends = {}
        for mode in MODES:
            sim.setGround(ground_z=gz, points=POINTS[P], sweeps=SWEEPS)  # (drops the settings, the model, the bodies and the terrain of the run before)
            sim.setGroundSolver(warm_start=False, tol=0.0)
            sim.setJointModel(stops=False)
            sim.setBodyParams(nominal)
            if mode == "flat":
                sim.setTerrain(np.full((1, 2, 2), gz), 1.0, origin=origin)
            elif mode == "rough":
                sim.setTerrain(rough, CELL, tile=tile, origin=origin)
            Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            torch.cuda.synchronize()
            for k in range(WARM + READINGS * LAUNCHES):
                sim.stepGroundDevice(Xd.data_ptr(), td.data_ptr(), 1e-3)
            sim.wait()
            ends[mode] = Xd.cpu().numpy()
        print(name, "P", P, "finite:", all(bool(np.isfinite(v).all()) for v in ends.values()), "the flat tile agrees with the plane bit for bit:",
              bool(np.array_equal(ends["plane"], ends["flat"])), "the rough tile differs:", not np.array_equal(ends["plane"], ends["rough"]), flush=True)


def summary(trace, B):
    d = []  # (kernel, duration) in launch order
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(sim_ground_body_rt_body|sim_ground_terrain_rt_body)(?:<|ILi)(\d+)", r["Kernel_Name"])
        if m and grid == B * 64:
            d.append(("%s<%s>" % m.groups(), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    per = WARM + READINGS * LAUNCHES
    assert len(d) == per * len(RUNS) * len(MODES), len(d)
    print("| robot | points per foot | plane: `sim_ground_body_rt_body` µs (spread) | flat tile: `sim_ground_terrain_rt_body` µs (spread) | ratio | rough tile µs (spread) | ratio |")
    print("|---|---|---|---|---|---|---|")
    k = 0
    for name, fs, P in RUNS:
        cells, names = [], []
        for mode in MODES:
            blk = d[k * per: (k + 1) * per]
            k += 1
            assert len(set(n for n, _ in blk)) == 1 and ("terrain_rt" in blk[0][0]) == (mode != "plane"), set(n for n, _ in blk)
            t = [v for _, v in blk[WARM:]]
            means = [sum(t[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
            cells.append((min(means), 100 * (max(means) / min(means) - 1.0)))
            names.append(blk[0][0])
        print("| %s | %d | %s %.1f (%.1f %%) | %s %.1f (%.1f %%) | %.3f | %.1f (%.1f %%) | %.3f |"
              % (name, P, names[0][-4:], cells[0][0], cells[0][1], names[1][-4:], cells[1][0], cells[1][1], cells[1][0] / cells[0][0], cells[2][0], cells[2][1],
                 cells[2][0] / cells[0][0]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    else:
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
