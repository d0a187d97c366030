"""The resident ground stack of examples/quadruped_arm_stack_ground.py, standing, under a grid of actuators: how weak and how sticky may the
joints be before the controller falls over?  Every robot of the batch gets its own effort limits (tau_max = scale x the limits the
controller plans with) and its own joint damping (BatchedRobotSim.setJointModel), the joint-limit stops of the robot table are on, and one
launch per tick (sim_ground_joint_rt_body, simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h) covers the whole grid.  The cell (scale inf,
damping 0) is the run of quadruped_arm_stack_ground.py for as long as none of its joints comes within the activation distance (0.1 rad) of
a limit: the stops are on for every robot, and a joint that gets a stop row is no longer the ideal joint of that example.  The largest
number of stop rows of every robot is recorded, and the example says so if a robot of that cell got one.  For every robot it prints the peak
demanded torque, the peak applied torque (per joint in the trace), the largest stop force and whether the robot is still up.

    python examples/quadruped_arm_stack_actuators.py [batch] [mpc_steps]

SMPC_EXAMPLE_TRACE=<file.npz>: the final states, tau_max, the joint limits, the peaks (applied torques per joint [batch][na]), the largest
number of stop rows and the scale and damping of every robot.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import BatchedMPC, BatchedRobotSim, CentroidalID, CentroidalOCP, RobotModelC, RobotModelHandler, load_robot, robot_from_table  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))
MU_PLAN = 0.8
SCALES = [np.inf, 1.0, 0.2, 0.1]  # tau_max over the controller's effort limits; inf: ideal actuators
DAMPS = [0.0, 0.2]                 # N m s / rad on every joint

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
na = nv - 6
# the plane under the feet of the reference pose: over the plane z = 0 the gaps are the heights of the feet
sim.setGround(ground_z=0.0)
ground_z = float(sim.groundDynamics(X0[:1], np.zeros((1, na)), dt_simu)["gap"].min())
sim.setGround(ground_z=ground_z, mu=MU_PLAN)
# the grid: robot i sits in cell i mod (scales x dampings), the scale varying fastest; robots of one cell differ by their arm
cell = np.arange(B) % (len(SCALES) * len(DAMPS))
scale, damp = np.array(SCALES)[cell % len(SCALES)], np.array(DAMPS)[cell // len(SCALES)]
tau_max = scale[:, None] * effort[None, :]
q_lo, q_hi = np.array(table.q_lo[:na]), np.array(table.q_hi[:na])
sim.setJointModel(tau_max=tau_max, damping=np.tile(damp[:, None], (1, na)), stops=True)
print("controller of %d joints; simulator: %d robots on the plane z = %.4f m, %d contact points each; grid: tau_max scale %s x damping %s N m s / rad; stops on"
      % (table.njoints, sim.B, ground_z, sim.ground_points, SCALES, DAMPS))

centroidal_ID.shareStream(mpc)  # MPC step, targets, QP solves and simulator steps in one in-order queue
sim.shareStream(mpc)
if LIB is None:  # states and torques in torch tensors
    import torch

    X = torch.from_numpy(X0).cuda()
    tau = torch.zeros((B, na), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    x_ptr, tau_ptr = X.data_ptr(), tau.data_ptr()
else:  # (the CPU test build of the kernel bodies: its "device" memory is the host's)
    X, tau = X0.copy(), np.zeros((B, na))
    x_ptr, tau_ptr = X.ctypes.data, tau.ctypes.data
peak_dem, peak_stop, beyond = np.zeros(B), np.zeros(B), np.zeros(B)
peak_app_joint = np.zeros((B, na))  # the largest |tau_applied| of every joint over all ticks
stop_rows_max = np.zeros(B, int)    # the largest number of stop rows of a tick
t0 = time.time()
for step in range(steps):
    mpc.iterate_device(x_ptr)
    mpc.wait()
    for sub in range(N_simu):
        centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)
        centroidal_ID.solve_device(x_ptr, tau_ptr)
        sim.stepGroundDevice(x_ptr, tau_ptr, dt_simu)
        # every tick (host copies: this example is about the figures, not about throughput)
        sim.wait()
        th = tau.cpu().numpy() if LIB is None else tau
        peak_dem = np.fmax(peak_dem, np.abs(th).max(axis=1))
        peak_app_joint = np.fmax(peak_app_joint, np.abs(sim.lastAppliedTorques()))
        st = sim.lastJointStops()
        peak_stop = np.fmax(peak_stop, st["lam_stop"].max(axis=1))
        stop_rows_max = np.maximum(stop_rows_max, (st["stop_rows"] != 0).sum(axis=1) + st["dropped"])
    Xh = X.cpu().numpy() if LIB is None else X
    q = Xh[:, 7:nq]
    beyond = np.fmax(beyond, np.maximum(q_lo[None, :] - q, q - q_hi[None, :]).max(axis=1))
sim.wait()
wall = time.time() - t0
centroidal_ID.shareStream(None)
sim.shareStream(None)
if LIB is None:
    torch.cuda.synchronize()
    X = X.cpu().numpy()
sim_time = steps * dt_mpc
R22 = 1.0 - 2.0 * (X[:, 3] ** 2 + X[:, 4] ** 2)  # cosine of the base's tilt
up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.08) & (R22 > np.cos(0.3))
peak_app = peak_app_joint.max(axis=1)
ideal = np.isinf(scale) & (damp == 0.0)
print("%d robots, %.2f s of standing:" % (B, sim_time))
for i in range(B):
    print("robot %d (tau_max scale %s, damping %.2f): peak demanded torque %.3f N m, peak applied torque %.3f N m, largest stop force %.3e N m, %s"
          % (i, "%.2f" % scale[i] if np.isfinite(scale[i]) else "inf", damp[i], peak_dem[i], peak_app[i], peak_stop[i], "up" if up[i] else "down"))
print("robots of the cell (scale inf, damping 0) that got a stop row: %d of %d" % (int((stop_rows_max[ideal] > 0).sum()), int(ideal.sum())))
print("robots that stay up: %d of %d; largest excursion beyond a joint limit %.3e rad" % (int(up.sum()), B, max(float(beyond.max()), 0.0)))
print("%.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s" % (sim_time, steps, N_simu, wall))
if os.environ.get("SMPC_EXAMPLE_TRACE"):
    np.savez(os.environ["SMPC_EXAMPLE_TRACE"], X=X, tau_max=tau_max, q_lo=q_lo, q_hi=q_hi, peak_demanded=peak_dem, peak_applied=peak_app, peak_applied_joint=peak_app_joint, peak_stop=peak_stop,
             stop_rows_max=stop_rows_max,
             beyond=beyond, scale=scale, damping=damp, up=up)
