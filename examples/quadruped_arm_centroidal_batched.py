"""Batched centroidal MPC of a robot that is not one of the built-in shapes: the go2_like quadruped with a 6-joint arm on its base
(19 joints, 4 point feet), described by a caller-filled robot table.  The loop is that of examples/go2_centroidal_batched.py; the
centroidal problem takes any table with 4 point feet or 2 flat feet and up to 32 joints (its state front end reads the joint tree at run time).

    python examples/quadruped_arm_centroidal_batched.py [batch] [steps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import BatchedMPC, CentroidalOCP, RobotDataHandler, RobotModelC, RobotModelHandler, load_robot, robot_from_table  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))

# ---- the robot table: the built-in quadruped + a serial arm Z-Y-Y-X-Y-X on the base (include/smpc_robot.h says what every field means) ----
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
    for i, v in enumerate((0.012 * mass, 0.0, 0.009 * mass, 0.0, 0.0, 0.007 * mass)):  # Ixx Ixy Iyy Ixz Iyz Izz about the CoM
        table.inertia[j][i] = v
    table.q_ref[6 + j], table.q_lo[j - 1], table.q_hi[j - 1] = q_ref, -2.0, 2.0
table.name = b"quad_arm"
table.njoints, table.nq, table.nv = 19, 25, 24
table.total_mass = sum(table.mass[:19])

model_handler = RobotModelHandler(robot_from_table(table), "standing", "root_joint")
feet = ["FL_foot", "FR_foot", "RL_foot", "RR_foot"]
for n in feet:
    model_handler.addPointFoot(n, "root_joint")
gravity = np.array([0, 0, -9.81])
problem_conf = dict(
    timestep=0.01, w_u=np.eye(12) * 1e-3, w_com=np.zeros((3, 3)), w_linear_mom=np.diag([0.01, 0.01, 100]),
    w_angular_mom=np.diag([0.1, 0.1, 1000]), w_linear_acc=0.01 * np.eye(3), w_angular_acc=0.01 * np.eye(3), gravity=gravity, mu=0.8,
    Lfoot=0.01, Wfoot=0.01, force_size=3,
)
problem = CentroidalOCP(problem_conf, model_handler)
problem.createProblem(np.zeros(9), T, 3, gravity[2], False)
mpc_conf = dict(support_force=-model_handler.getMass() * gravity[2], TOL=1e-4, mu_init=1e-8, max_iters=1, num_threads=1, swing_apex=0.15,
                T_fly=30, T_contact=10, timestep=0.01)
mpc = BatchedMPC(mpc_conf, problem, B, lib=LIB)
quadru = dict.fromkeys(feet, True)
mpc.generateCycleHorizon([quadru] * 10 + [dict(quadru, FL_foot=False, RR_foot=False)] * 30 + [quadru] * 10 + [dict(quadru, FR_foot=False, RL_foot=False)] * 30)
V = np.zeros((B, 6))
V[:, 0] = np.linspace(0.0, 0.4, B)
mpc.switchToWalk(V[0])
mpc.setVelocityBaseBatched(V)

# measured multibody states [B][nq + nv] = [B][49]: the reference posture with the arm swung differently on every robot
X = np.tile(model_handler.getReferenceState(), (B, 1))
X[:, 7 + 12] = np.linspace(-1.0, 1.0, B)  # first arm joint (yaw)
t0 = time.time()
for step in range(steps):
    mpc.iterate(X)
dt = (time.time() - t0) / steps
print("%d quadrupeds with an arm (%d joints), %d control steps: %.2f ms per batched step (%.0f control-steps/s incl. host copies)"
      % (B, table.njoints, steps, dt * 1e3, B / dt))
us = mpc.us.reshape(B, T, 4, 3)
print("vertical force per robot at t = 0: %.1f .. %.1f N (weight %.1f N)" % (us[:, 0, :, 2].sum(1).min(), us[:, 0, :, 2].sum(1).max(), model_handler.getMass() * 9.81))
dev = mpc.updateInternalData(X)["centroidal_state"]
host = RobotDataHandler(model_handler)
host.updateInternalData(X[B - 1])
print("centre of mass of the last robot: device %s, host %s" % (np.round(dev[B - 1, :3], 4), np.round(host.getCentroidalState()[:3], 4)))
x_i, xdot_i, f_i = mpc.interpolate(0.004)
u_fb = mpc.riccatiFeedback(0.004, X)
print("interpolated centroidal state", x_i.shape, "forces", f_i.shape, "Riccati-feedback forces", u_fb.shape)
