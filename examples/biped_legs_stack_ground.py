"""The resident control stack of examples/biped_legs_stack_resident.py, standing, on the GROUND: biped_legs (the talos_like table without the
joints above the pelvis, 13 joints, 2 flat feet) under the centroidal MPC with 6-D feet at 100 Hz and CentroidalID with flat-foot contacts
at 1 kHz, with BatchedRobotSim.stepGroundDevice as the robot -- a plane with unilateral contact and Coulomb friction detected from the
state, four corner points per sole (8 points, a rank-deficient contact problem).  The fixed-sweep solve from zero does not converge on such
soles; here the solve starts from the forces of the previous tick and stops by its own residual
(setGroundSolver, simple-mpc_amd/csrc/smpc_sim_ground_ws_rt.h).  The stack runs twice, once cold (every tick from lambda = 0) and once warm,
with the same tol, and prints for both: robots up, base height, largest penetration, mean and largest sweeps_used, largest residual,
robot-seconds per second.  The controller's gains are those of the bilateral example, untuned for a unilateral ground: what happens is
reported, not gated.

    python examples/biped_legs_stack_ground.py [batch] [mpc_steps] [tol]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import BatchedMPC, BatchedRobotSim, CentroidalID, CentroidalOCP, RobotModelC, RobotModelHandler, load_robot, presets, robot_from_table  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
tol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-6
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "100"))
SWEEPS = 60

# ---- the robot table: base and legs (joints 1 .. 12, feet on joints 6 and 12) of the built-in biped; the upper body as a lump on the base ----
src = load_robot("talos_like", LIB).contents
table = RobotModelC.from_buffer_copy(src)
upper = float(sum(src.mass[13:23]))
mb = src.mass[0] + upper
for i in range(3):
    table.com[0][i] = (src.mass[0] * src.com[0][i] + upper * (0.0, 0.0, 0.25)[i]) / mb
table.mass[0] = mb
for i, v in enumerate((1.9, 0.0, 1.6, 0.0, 0.0, 0.6)):
    table.inertia[0][i] = src.inertia[0][i] + v
for j in range(13, 32):  # nothing of the removed joints stays behind
    table.parent[j] = table.jtype[j] = 0
    table.mass[j] = 0.0
for i in range(19, 38):
    table.q_ref[i] = 0.0
table.name = b"biped_legs"
table.njoints, table.nq, table.nv = 13, 19, 18
table.total_mass = float(sum(table.mass[:13]))

dt_mpc, N_simu = 0.01, 10
dt_simu = dt_mpc / N_simu
id_settings = dict(kp_base=7.0, kp_com=7.0, kp_posture=10.0, kp_contact=10.0, kp_feet_tracking=2000.0, w_base=50.0, w_com=100.0, w_posture=1.0,
                   w_contact_force=1e-6, w_contact_motion=1e-3, w_feet_tracking=100.0)  # those of biped_legs_stack_resident.py, untuned for the ground
effort, vmax = presets.TALOS_EFFORT[:12], presets.TALOS_VMAX[:12]  # the legs of the built-in biped


def run(warm):
    mh = RobotModelHandler(robot_from_table(table), "standing", "root_joint")
    for n in presets.TALOS_FEET:
        mh.addQuadFoot(n, "root_joint", presets.TALOS_QUAD)
    nv = mh.nv
    mpc_conf = {k: v for k, v in presets.talos_mpc_settings(mh, max_iters=1).items() if k in presets.MPC_KEYS}
    ocp = CentroidalOCP(presets.talos_centroidal_settings(mh), mh)  # force_size 6: u = [(f, tau) per foot]
    ocp.createProblem(np.zeros(9), T, 6, -9.81, False)
    mpc = BatchedMPC(mpc_conf, ocp, B, lib=LIB)
    mpc.generateCycleHorizon(presets.walk_cycle())
    mpc.switchToStand()
    centroidal_ID = CentroidalID(mh, dt_simu, id_settings, effort, vmax, batch=B, lib=LIB)
    sim = BatchedRobotSim(mh, force_size=6, batch=B, lib=LIB)
    X0 = np.tile(mh.getReferenceState(), (B, 1))
    X0[:, 7 + 2] += np.linspace(-0.02, 0.02, B)  # (a hip pitch: the robots differ)
    z0 = X0[0, 2]
    # the plane under the soles of the reference pose: over the plane z = 0 the gaps are the heights of the corners
    sim.setGround(ground_z=0.0, points=presets.TALOS_QUAD)
    ground_z = float(sim.groundDynamics(np.tile(mh.getReferenceState(), (1, 1)), np.zeros((1, nv - 6)), dt_simu)["gap"].min())
    sim.setGround(ground_z=ground_z, points=presets.TALOS_QUAD, sweeps=SWEEPS)
    sim.setGroundSolver(warm_start=warm, tol=tol)
    if not warm:
        print("controller of %d joints; simulator: %d robots on the plane z = %.4f m, %d contact points each, at most %d sweeps, tol %.1e m/s"
              % (table.njoints, sim.B, ground_z, sim.ground_points, SWEEPS, tol))
    centroidal_ID.shareStream(mpc)  # MPC step, targets, QP solves and simulator steps in one in-order queue
    sim.shareStream(mpc)
    if LIB is None:  # states and torques in torch tensors
        import torch

        X = torch.from_numpy(X0).cuda()
        tau = torch.zeros((B, nv - 6), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        x_ptr, tau_ptr = X.data_ptr(), tau.data_ptr()
    else:  # (the CPU test build of the kernel bodies: its "device" memory is the host's)
        X, tau = X0.copy(), np.zeros((B, nv - 6))
        x_ptr, tau_ptr = X.ctypes.data, tau.ctypes.data
    zero_tau = np.zeros((B, nv - 6))
    worst_pen, worst_res, sweeps_sum, sweeps_max, samples = 0.0, 0.0, 0, 0, 0
    t0 = time.time()
    t_stats = 0.0
    for step in range(steps):
        mpc.iterate_device(x_ptr)
        mpc.wait()
        for sub in range(N_simu):
            centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)
            centroidal_ID.solve_device(x_ptr, tau_ptr)
            sim.stepGroundDevice(x_ptr, tau_ptr, dt_simu)
        # once per MPC period (its time is taken out of the throughput figure): the solver's read-outs of the last tick, the penetration
        sim.wait()
        ts = time.time()
        sw, res = sim.lastGroundSweeps(), sim.lastGroundResiduals()
        sweeps_sum, sweeps_max, samples = sweeps_sum + int(sw.sum()), max(sweeps_max, int(sw.max())), samples + B
        Xh = X.cpu().numpy() if LIB is None else X
        ok = np.isfinite(Xh).all(1)
        if np.isfinite(res).any():
            worst_res = max(worst_res, float(np.nanmax(res)))
        if ok.any():
            worst_pen = max(worst_pen, float(-sim.groundDynamics(Xh[ok], zero_tau[ok], dt_simu)["gap"].min()))
        t_stats += time.time() - ts
    sim.wait()
    wall = time.time() - t0 - t_stats
    centroidal_ID.shareStream(None)
    sim.shareStream(None)
    if LIB is None:
        torch.cuda.synchronize()
        X = X.cpu().numpy()
    sim_time = steps * dt_mpc
    R22 = 1.0 - 2.0 * (X[:, 3] ** 2 + X[:, 4] ** 2)  # cosine of the base's tilt
    up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.05) & (R22 > np.cos(0.3))
    name = "warm" if warm else "cold"
    print("%s: robots that stay up: %d of %d; base height %.3f .. %.3f m (start %.3f)" % (name, int(up.sum()), B, np.nanmin(X[:, 2]), np.nanmax(X[:, 2]), z0))
    print("%s: largest penetration %.3e m" % (name, max(worst_pen, 0.0)))
    print("%s: sweeps_used mean %.2f, largest %d (of %d); largest residual %.3e m/s (the last tick of every MPC period, %d robot-ticks)"
          % (name, sweeps_sum / max(samples, 1), sweeps_max, SWEEPS, worst_res, samples))
    print("%s: %.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s: %.1f ms per MPC period, %.0f robot-seconds per second"
          % (name, sim_time, steps, N_simu, wall, 1e3 * wall / steps, B * sim_time / wall))
    return X


X_cold = run(False)
X = run(True)
assert np.all(np.isfinite(X)) and np.all(np.isfinite(X_cold))
