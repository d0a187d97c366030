"""The resident control stack of examples/quadruped_arm_stack_resident.py on the GROUND: the 19-joint quadruped with an arm under the
centroidal MPC at 100 Hz and CentroidalID at 1 kHz, with BatchedRobotSim.stepGroundDevice as the robot -- a plane with unilateral contact
and Coulomb friction detected from the state (simple-mpc_amd/csrc/smpc_sim_ground_rt.h), one launch per tick.  The MPC's contact plan goes
to the controller only: the simulator takes no mask, so a controller that pulls on the floor, pushes outside the friction cone or touches
down late shows here, where the bilateral contacts of stepDevice hide it.  MPC step, targets, QP solve and simulator step share one stream;
states and torques stay on the device.  Per run it prints the robots that stay up, the largest penetration and the share of control ticks
on which planned and detected contacts differ.

    python examples/quadruped_arm_stack_ground.py [batch] [mpc_steps] [stand|walk]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import BatchedMPC, BatchedRobotSim, CentroidalID, CentroidalOCP, RobotModelC, RobotModelHandler, load_robot, robot_from_table  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
mode = sys.argv[3] if len(sys.argv) > 3 else "stand"
if mode not in ("stand", "walk"):
    raise SystemExit("mode: stand or walk")
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))

# ---- the robot table: the built-in quadruped + a serial arm Z-Y-Y-X-Y-X on the base (that of quadruped_arm_stack_resident.py) ----
table = RobotModelC.from_buffer_copy(load_robot("go2_like", LIB).contents)
arm = [  # parent joint, axis (1 / 2 / 3 = X / Y / Z), placement in the parent, mass, centre of mass, reference angle
    (0, 3, (0.10, 0.0, 0.06), 1.2, (0.0, 0.0, 0.02), 0.0),
    (13, 2, (0.0, 0.0, 0.05), 1.0, (0.0, 0.0, 0.12), -0.6),
    (14, 2, (0.0, 0.0, 0.25), 0.8, (0.10, 0.0, 0.0), 1.2),
    (15, 1, (0.20, 0.0, 0.0), 0.5, (0.04, 0.0, 0.0), 0.0),
    (16, 2, (0.08, 0.0, 0.0), 0.3, (0.02, 0.0, 0.01), 0.4),
    (17, 1, (0.05, 0.0, 0.0), 0.2, (0.02, 0.005, 0.0), 0.0),
]
for k, (parent, axis, p, mass, com, q_ref) in enumerate(arm):
    j = 13 + k
    table.parent[j], table.jtype[j], table.mass[j] = parent, axis, mass
    for i in range(9):
        table.jp_R[j][i] = 1.0 if i % 4 == 0 else 0.0
    for i in range(3):
        table.jp_p[j][i], table.com[j][i] = p[i], com[i]
    for i, v in enumerate((0.012 * mass, 0.0, 0.009 * mass, 0.0, 0.0, 0.007 * mass)):
        table.inertia[j][i] = v
    table.q_ref[6 + j], table.q_lo[j - 1], table.q_hi[j - 1] = q_ref, -2.0, 2.0
table.name = b"quad_arm"
table.njoints, table.nq, table.nv = 19, 25, 24
table.total_mass = sum(table.mass[:19])

mh = RobotModelHandler(robot_from_table(table), "standing", "root_joint")
feet = ["FL_foot", "FR_foot", "RL_foot", "RR_foot"]
for n in feet:
    mh.addPointFoot(n, "root_joint")
nq, nv, mass = mh.nq, mh.nv, mh.getMass()
gravity = np.array([0, 0, -9.81])
problem = CentroidalOCP(dict(
    timestep=0.01, w_u=np.eye(12) * 1e-3, w_com=np.zeros((3, 3)), w_linear_mom=np.diag([0.01, 0.01, 100]),
    w_angular_mom=np.diag([0.1, 0.1, 1000]), w_linear_acc=0.01 * np.eye(3), w_angular_acc=0.01 * np.eye(3), gravity=gravity, mu=0.8,
    Lfoot=0.01, Wfoot=0.01, force_size=3), mh)
problem.createProblem(np.zeros(9), T, 3, gravity[2], False)
mpc = BatchedMPC(dict(support_force=-mass * gravity[2], TOL=1e-4, mu_init=1e-8, max_iters=1, num_threads=1, swing_apex=0.10, T_fly=30, T_contact=10,
                      timestep=0.01), problem, B, lib=LIB)
quadru = dict.fromkeys(feet, True)
mpc.generateCycleHorizon([quadru] * 10 + [dict(quadru, FL_foot=False, RR_foot=False)] * 30 + [quadru] * 10 + [dict(quadru, FR_foot=False, RL_foot=False)] * 30)
if mode == "walk":
    V = np.zeros((B, 6))
    V[:, 0] = np.linspace(0.0, 0.2, B)
    mpc.switchToWalk(V[0])
    mpc.setVelocityBaseBatched(V)
else:
    mpc.switchToStand()

dt_mpc, N_simu = 0.01, 10
dt_simu = dt_mpc / N_simu
id_settings = dict(kp_base=7.0, kp_com=7.0, kp_posture=10.0, kp_contact=10.0, kp_feet_tracking=2000.0, w_base=50.0, w_com=100.0, w_posture=1.0,
                   w_contact_force=1e-6, w_contact_motion=1e-3, w_feet_tracking=100.0)  # those of quadruped_arm_stack_resident.py, untuned for the ground
effort = np.r_[np.array([23.7, 23.7, 45.43] * 4), np.full(6, 30.0)]
vmax = np.r_[np.array([30.1, 30.1, 15.7] * 4), np.full(6, 20.0)]
centroidal_ID = CentroidalID(mh, dt_simu, id_settings, effort, vmax, batch=B, lib=LIB)
sim = BatchedRobotSim(mh, force_size=3, batch=B, lib=LIB)

X0 = np.tile(mh.getReferenceState(), (B, 1))
X0[:, 7 + 12] = np.linspace(-0.5, 0.5, B)  # first arm joint (yaw): every robot holds its arm differently
z0 = X0[0, 2]
# the plane under the feet of the reference pose: over the plane z = 0 the gaps are the heights of the feet
sim.setGround(ground_z=0.0)
ground_z = float(sim.groundDynamics(X0[:1], np.zeros((1, nv - 6)), dt_simu)["gap"].min())
sim.setGround(ground_z=ground_z, mu=0.8)  # (the friction coefficient the MPC plans with)
print("controller of %d joints; simulator: %d robots on the plane z = %.4f m, %d contact points each, mu = 0.8, mode: %s"
      % (table.njoints, sim.B, ground_z, sim.ground_points, mode))

centroidal_ID.shareStream(mpc)  # MPC step, targets, QP solves and simulator steps in one in-order queue
sim.shareStream(mpc)
if LIB is None:  # states, torques and the running statistics in torch tensors, torch's work on the same queue
    import torch

    X = torch.from_numpy(X0).cuda()
    tau = torch.zeros((B, nv - 6), dtype=torch.float64, device="cuda")
    tau_max = torch.zeros((), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    queue = torch.cuda.ExternalStream(mpc.stream())
    x_ptr, tau_ptr = X.data_ptr(), tau.data_ptr()
else:  # (the CPU test build of the kernel bodies: its "device" memory is the host's)
    X, tau, tau_max = X0.copy(), np.zeros((B, nv - 6)), 0.0
    x_ptr, tau_ptr = X.ctypes.data, tau.ctypes.data
zero_tau = np.zeros((B, nv - 6))
worst_pen, mismatch, ticks = 0.0, 0, 0
t0 = time.time()
t_stats = 0.0
for step in range(steps):
    mpc.iterate_device(x_ptr)
    mpc.wait()
    contact = mpc.ocp_handler.getContactState(0)
    planned = sum(1 << i for i, c in enumerate(contact) if c)
    for sub in range(N_simu):
        centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)  # CoM, its velocity, foot references, forces: interpolated and written on the device
        centroidal_ID.solve_device(x_ptr, tau_ptr)
        sim.stepGroundDevice(x_ptr, tau_ptr, dt_simu)
        if LIB is None:
            with torch.cuda.stream(queue):
                tau_max = torch.maximum(tau_max, tau.abs().max())
        else:
            tau_max = max(tau_max, np.abs(tau).max())
    # once per MPC period (its time is taken out of the throughput figure): detected against planned contacts of the last tick, the penetration
    sim.wait()  # (the ticks of this period are done: what follows is bookkeeping)
    ts = time.time()
    detected = sim.lastContacts()
    mismatch += int((detected != planned).sum())
    ticks += B
    Xh = X.cpu().numpy() if LIB is None else X
    ok = np.isfinite(Xh).all(1)
    if ok.any():
        worst_pen = max(worst_pen, float(-sim.groundDynamics(Xh[ok], zero_tau[ok], dt_simu)["gap"].min()))
    t_stats += time.time() - ts
sim.wait()
wall = time.time() - t0 - t_stats
resid = centroidal_ID.getResiduals().max()
centroidal_ID.shareStream(None)
sim.shareStream(None)
if LIB is None:
    torch.cuda.synchronize()
    X, tau, tau_max = X.cpu().numpy(), tau.cpu().numpy(), float(tau_max.cpu())
sim_time = steps * dt_mpc
R22 = 1.0 - 2.0 * (X[:, 3] ** 2 + X[:, 4] ** 2)  # cosine of the base's tilt
up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.08) & (R22 > np.cos(0.3))
print("%d robots, %.2f s of %s: base x %.3f m ... %.3f m; base height %.3f .. %.3f m (start %.3f); max |tau| %.1f N m; QP residual %.1e"
      % (B, sim_time, "walking" if mode == "walk" else "standing", X[0, 0], X[-1, 0], np.nanmin(X[:, 2]), np.nanmax(X[:, 2]), z0, tau_max, resid))
print("robots that stay up: %d of %d" % (int(up.sum()), B))
print("largest penetration: %.3e m" % max(worst_pen, 0.0))
print("planned and detected contacts differ on %.1f %% of the sampled control ticks (the last tick of every MPC period, %d robot-ticks)"
      % (100.0 * mismatch / max(ticks, 1), ticks))
print("%.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s: %.1f ms per MPC period, %.0f robot-seconds per second"
      % (sim_time, steps, N_simu, wall, 1e3 * wall / steps, B * sim_time / wall))
if mode == "stand":
    assert np.all(np.isfinite(X)) and np.all(np.abs(tau) <= effort + 1e-6)
