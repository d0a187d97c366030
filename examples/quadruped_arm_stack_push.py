"""The resident ground stack of examples/quadruped_arm_stack_ground.py, standing, under a grid of friction coefficients against lateral
pushes: does the controller survive a shove on a slippery floor?  Every robot of the batch gets its own mu (BatchedRobotSim.setGroundEnv) and
its own push on the base (setPush: a force along +y at the base origin, held for 100 ms from 200 ms on), and one launch per tick
(sim_ground_env_rt_body, simple-mpc_amd/csrc/smpc_sim_ground_env_rt.h) covers the whole grid.  One row of the grid has no push and one
column the friction coefficient the MPC plans with, so the cell (no push, default mu) is the run of quadruped_arm_stack_ground.py.  Per
grid cell it prints how many robots are up at the end, the largest excursion of the base and the largest penetration.

The MPC plans for flat ground: every plane stays horizontal here.  Slopes are exercised by the tests (tests/test_robot_sim_ground_env.py),
not by this example.

    python examples/quadruped_arm_stack_push.py [batch] [mpc_steps] [push_start_ms] [push_ms]

SMPC_EXAMPLE_TRACE=<file.npz>: the base positions [mpc_steps + 1][batch][3], the final states and the index of the end of the push.
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
push_start = int(sys.argv[3]) if len(sys.argv) > 3 else 200  # ms, a multiple of the MPC period
push_len = int(sys.argv[4]) if len(sys.argv) > 4 else 100
if push_start % 10 or push_len % 10 or push_len < 10:
    raise SystemExit("push_start_ms, push_ms: multiples of the MPC period of 10 ms")
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))
MU_PLAN = 0.8  # the friction coefficient the MPC plans with: the default column
MUS = [MU_PLAN, 0.4, 0.2, 1.2]
FORCES = [0.0, 30.0, 60.0, 90.0, 120.0]  # N along +y on the base; the first row has no push

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
# the plane under the feet of the reference pose: over the plane z = 0 the gaps are the heights of the feet
sim.setGround(ground_z=0.0)
ground_z = float(sim.groundDynamics(X0[:1], np.zeros((1, nv - 6)), dt_simu)["gap"].min())
sim.setGround(ground_z=ground_z, mu=MU_PLAN)
# the grid: robot i sits in cell i mod (rows x columns), the push varying fastest; robots of one cell differ by their arm
cell = np.arange(B) % (len(FORCES) * len(MUS))
row, col = cell % len(FORCES), cell // len(FORCES)
push = np.zeros((B, 6))
push[:, 1] = np.array(FORCES)[row]
sim.setGroundEnv(mu=np.array(MUS)[col])
sim.setPush(np.zeros((B, 6)), joint=0)
print("controller of %d joints; simulator: %d robots on the plane z = %.4f m, %d contact points each; grid: mu %s x push %s N along +y from %d ms for %d ms"
      % (table.njoints, sim.B, ground_z, sim.ground_points, MUS, FORCES, push_start, push_len))

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
trace = [X0[:, :3].copy()]
excursion, pen = np.zeros(B), np.zeros(B)
t0 = time.time()
t_stats = 0.0
for step in range(steps):
    if step * 10 == push_start:
        sim.setPush(push, joint=0)  # (joins the stream: the period before is done)
    if step * 10 == push_start + push_len:
        sim.setPush(np.zeros((B, 6)), joint=0)
    mpc.iterate_device(x_ptr)
    mpc.wait()
    for sub in range(N_simu):
        centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)
        centroidal_ID.solve_device(x_ptr, tau_ptr)
        sim.stepGroundDevice(x_ptr, tau_ptr, dt_simu)
    # once per MPC period (its time is taken out of the throughput figure): base excursion and penetration of every robot
    sim.wait()
    ts = time.time()
    Xh = X.cpu().numpy() if LIB is None else X
    trace.append(Xh[:, :3].copy())
    ok = np.isfinite(Xh).all(1)
    excursion[ok] = np.maximum(excursion[ok], np.linalg.norm(Xh[ok, :3] - X0[ok, :3], axis=1))
    if ok.any():
        pen[ok] = np.maximum(pen[ok], -sim.groundDynamics(Xh[ok], zero_tau[ok], dt_simu)["gap"].min(axis=1))
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
up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.08) & (R22 > np.cos(0.3))
print("%d robots, %.2f s of standing; robots up / robots, largest base excursion [m], largest penetration [m] per cell:" % (B, sim_time))
print("%10s" % "push \\ mu" + "".join("%28.1f" % m for m in sorted(MUS)))
for r, f in enumerate(FORCES):
    line = "%8.0f N" % f
    for m in sorted(MUS):
        sel = (row == r) & (col == MUS.index(m))
        line += "%10s %8.3f %8.1e" % ("%d/%d" % (up[sel].sum(), sel.sum()), excursion[sel].max(), max(pen[sel].max(), 0.0)) if sel.any() else "%28s" % "-"
    print(line)
print("robots that stay up: %d of %d" % (int(up.sum()), B))
k_end = min((push_start + push_len) // 10, steps)
for i in range(min(B, 2)):
    print("robot %d (push %.0f N, mu %.1f): base displacement along the push at the end of the push %+.6f m, largest penetration %.3e m"
          % (i, push[i, 1], MUS[col[i]], trace[k_end][i, 1] - X0[i, 1], max(pen[i], 0.0)))
print("%.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s: %.1f ms per MPC period, %.0f robot-seconds per second"
      % (sim_time, steps, N_simu, wall, 1e3 * wall / steps, B * sim_time / wall))
if os.environ.get("SMPC_EXAMPLE_TRACE"):
    np.savez(os.environ["SMPC_EXAMPLE_TRACE"], base=np.array(trace), X=X, push_end=k_end)
