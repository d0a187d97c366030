"""The resident ground stack of examples/quadruped_arm_stack_payload.py, walking, on a grid of roughness amplitudes: the controllers plan
on flat ground, the robot they drive walks over a height field: how far does it get?  Every robot of the batch stands on its own tile
(BatchedRobotSim.setTerrain with tiles built by terrain_rough, one tile per amplitude, amplitude 0 among them), the centroidal MPC and
CentroidalID keep the flat-ground model, and one launch per tick (sim_ground_terrain_rt_body,
simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h) covers the whole grid.  The tile of amplitude 0 is flat at the ground's height and its
robots are the run without a terrain bit for bit.  For every robot it prints how far it got along x, the largest tilt of a terrain normal
under its feet, and whether it is still up.

    python examples/quadruped_arm_stack_terrain.py [batch] [mpc_steps] [flat]

`flat`: the same run without a terrain.  SMPC_EXAMPLE_TRACE=<file.npz>: the final states, the amplitude of every robot, the distances, the
largest horizontal component of a recorded normal per robot and who is up.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import BatchedMPC, BatchedRobotSim, CentroidalID, CentroidalOCP, RobotModelC, RobotModelHandler, load_robot, robot_from_table, terrain_rough  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))
MU_PLAN = 0.8
FLAT = len(sys.argv) > 3 and sys.argv[3] == "flat"  # the same run without a terrain: every robot walks on the plane
AMPLITUDES = [0.0, 0.01, 0.02, 0.04]  # m: the peak of the rough tile's heights about the ground's height
WAVELENGTH = 0.3                      # m
CELL, NX, NY = 0.05, 81, 25           # a tile of 4 m x 1.2 m; node (0, 0) lies 0.5 m behind and 0.6 m beside the robot's start
SPEED = 0.2                           # m/s, commanded along x

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
V = np.zeros((B, 6))
V[:, 0] = SPEED
mpc.switchToWalk(V[0])
mpc.setVelocityBaseBatched(V)

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
# the grid: robot i walks on the tile of amplitude i mod len(AMPLITUDES); robots of one tile differ by their arm.  Tile 0 (amplitude 0) is
# ground_z at every node: the flat plane exactly
tile = (np.arange(B) % len(AMPLITUDES)).astype(np.int32)
amplitude = np.array(AMPLITUDES)[tile]
rng = np.random.default_rng(0)
heights = np.stack([ground_z + terrain_rough(rng, NX, NY, CELL, a, WAVELENGTH) for a in AMPLITUDES])  # [tiles, NY, NX]
origin = X0[:, :2] - np.array([0.5, 0.6])
if not FLAT:
    sim.setTerrain(heights, CELL, tile=tile, origin=origin)
print("controller of %d joints on flat ground; simulator: %d robots on %d tiles of %d x %d nodes (%.2f m apart) about z = %.4f m, %d contact points each; "
      "amplitudes %s m%s" % (table.njoints, sim.B, len(AMPLITUDES), NX, NY, CELL, ground_z, sim.ground_points, AMPLITUDES, "; FLAT: no terrain" if FLAT else ""))

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
tilt = np.zeros(B)  # the largest horizontal component of a terrain normal under a foot, sampled once per MPC step
t0 = time.time()
for step in range(steps):
    mpc.iterate_device(x_ptr)
    mpc.wait()
    for sub in range(N_simu):
        centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)
        centroidal_ID.solve_device(x_ptr, tau_ptr)
        sim.stepGroundDevice(x_ptr, tau_ptr, dt_simu)
    if not FLAT:  # (a host copy per MPC step: this example is about the figures, not about throughput)
        sim.wait()
        nrm = sim.lastTerrainNormals()
        tilt = np.maximum(tilt, np.hypot(nrm[..., 0], nrm[..., 1]).max(axis=1))
sim.wait()
wall = time.time() - t0
centroidal_ID.shareStream(None)
sim.shareStream(None)
if LIB is None:
    torch.cuda.synchronize()
    X = X.cpu().numpy()
sim_time = steps * dt_mpc
distance = X[:, 0] - X0[:, 0]
R22 = 1.0 - 2.0 * (X[:, 3] ** 2 + X[:, 4] ** 2)  # cosine of the base's tilt
up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.08 + amplitude) & (R22 > np.cos(0.3))
print("%d robots, %.2f s of walking at %.2f m/s commanded:" % (B, sim_time, SPEED))
for i in range(B):
    print("robot %d (amplitude %.3f m): got %.3f m along x (commanded %.3f m), largest tilt of a normal under a foot %.3f, %s"
          % (i, amplitude[i], distance[i], SPEED * sim_time, tilt[i], "up" if up[i] else "down"))
print("robots that stay up: %d of %d" % (int(up.sum()), B))
print("%.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s" % (sim_time, steps, N_simu, wall))
if os.environ.get("SMPC_EXAMPLE_TRACE"):
    np.savez(os.environ["SMPC_EXAMPLE_TRACE"], X=X, amplitude=amplitude, distance=distance, tilt=tilt, up=up, heights=heights, origin=origin)
