"""Launch times of the three inverse-dynamics kernels, templated and run-time engines side by side (flat feet: 3.22).

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o id -- python3 tools/id_rt_profile.py run [batch]
    python3 tools/id_rt_profile.py summary <kernel_trace.csv> [batch]
    ... run6 / summary6: the same for flat feet -- talos_like (templated engine, then the run-time flat-foot engine), biped_legs, tree32

`run`: KinodynamicsID at 100 fixed iterations on go2_like (templated engine, then the run-time engine through smpc_debug_id_force_rt),
quad_arm and the 32-joint point-foot table of tests/test_id_any_robot.py, one after the other; per robot WARM solves, then READINGS x
LAUNCHES solves on states that move between ticks.  `summary`: the dispatches of the trace whose grid is the full batch, per kernel family in
launch order, cut into the robots' runs (the run-time quantities / assembly kernels are one symbol for every robot); per reading the mean
of its LAUNCHES dispatches, then the minimum of the readings and their spread."""
import collections
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, READINGS, LAUNCHES = 5, 3, 20
RUNS = [("go2_like", False), ("go2_like", True), ("quad_arm", True), ("tree32p", True)]  # (robot, through the run-time engine)
RUNS6 = [("talos_like", False), ("talos_like", True), ("biped_legs", True), ("tree32", True)]
# kernel families (quantities, assembly, solve) of the templated / run-time engine
FAMILIES = {False: (("id_quant", "id_assemble", "qp_admm"), ("id_quant_rt", "id_assemble_rt", "qp_admm_rt")),
            True: (("id_quant", "id6_assemble", "qp6_admm"), ("id6_quant_rt", "id6_assemble_rt", "qp6_admm_rt"))}


def run(B, flat=False):
    sys.path[:0] = [os.path.join(ROOT, "simple-mpc_amd", "python"), os.path.join(ROOT, "tests")]
    import numpy as np
    import robot_tables as RT
    import simple_mpc
    import test_id_any_robot as T
    import test_id_flat_any_robot as T6

    L = simple_mpc.default_lib().L
    for name, rt in (RUNS6 if flat else RUNS):
        tab = RT.table(name) if flat else T.table(name)
        rb = RT.oracle_robot(tab)
        tau_max, v_max = T6.limits(name) if flat else T.limits(rb)
        was = L.smpc_debug_id_force_rt(int(rt))
        try:
            kid = simple_mpc.KinodynamicsID(RT.model_handler(tab), 1e-3, T6.KINO if flat else T.ALL, tau_max, v_max, batch=B, admm_iters=100, admm_tol=-1.0)
        finally:
            L.smpc_debug_id_force_rt(was)
        X = RT.near_reference_states(rb, min(B, 64), seed=5, scale=0.3)
        X = np.tile(X, (-(-B // X.shape[0]), 1))[:B]
        rng = np.random.default_rng(6)
        for _ in range(WARM + READINGS * LAUNCHES):
            Xk = X + np.concatenate([np.zeros((B, 7)), rng.normal(0.0, 2e-3, (B, X.shape[1] - 7))], axis=1)
            kid.solve(0.0, Xk[:, : rb.nq], Xk[:, rb.nq:])
        print(name, "run-time" if rt else "templated", "max residual %.2e" % kid.getResiduals().max(), flush=True)


def summary(trace, B, flat=False):
    fam = collections.defaultdict(list)  # kernel family -> durations in launch order
    runs = RUNS6 if flat else RUNS
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        m = re.search(r"(id6?_quant|id6?_assemble|qp6?_admm)(_rt)?_body(ILi(\d+)E)?", r["Kernel_Name"])
        if m and grid == B * 64:
            fam[m.group(1) + (m.group(2) or "")].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    per = WARM + READINGS * LAUNCHES
    nrt = sum(rt for _, rt in runs)
    print("| robot | engine | quantities µs | assembly µs | solve µs | spread of the readings |")
    print("|---|---|---|---|---|---|")
    k = 0
    for name, rt in runs:
        cells, spread = [], 0.0
        for f in FAMILIES[flat][int(rt)]:
            d = fam[f]
            assert len(d) == per * (nrt if rt else 1), (f, rt, len(d))
            d = d[k * per + WARM: (k + 1) * per] if rt else d[WARM:per]
            means = [sum(d[i * LAUNCHES: (i + 1) * LAUNCHES]) / LAUNCHES for i in range(READINGS)]
            cells.append("%.1f" % min(means))
            spread = max(spread, max(means) / min(means) - 1.0)
        print("| %s | %s | %s | %.1f %% |" % (name, "run-time" if rt else "templated", " | ".join(cells), 100 * spread))
        k += rt


if __name__ == "__main__":
    if sys.argv[1] in ("run", "run6"):
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, flat=sys.argv[1] == "run6")
    else:
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4096, flat=sys.argv[1] == "summary6")
