"""The whole control stack for a flat-foot biped that is not the built-in shape, with nothing crossing the host inside the loop: biped_legs --
the talos_like table without the joints above the pelvis, their mass lumped into the base body (13 joints, 2 flat feet) -- under the centroidal
MPC with 6-D feet at 100 Hz, CentroidalID with flat-foot contacts (tsid Contact6d) at 1 kHz with its targets written by the MPC's
interpolation kernel (setTargetsFromMPC), and BatchedRobotSim.stepDevice with 6-D contacts as the robot.  Every leg of the loop runs on the
run-time joint tree of the caller's table; MPC step, targets, QP solve and simulator step share one stream; states and torques stay on the
device.  The loop is that of the reference's examples/talos_centroidal.py (MPC :200-216, CentroidalID :218-246) with the simulator in place
of PyBullet; gains: those of examples/talos_centroidal_id_batched.py.

    python examples/biped_legs_stack_resident.py [batch] [mpc_steps]
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
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "100"))

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

mh = RobotModelHandler(robot_from_table(table), "standing", "root_joint")
for n in presets.TALOS_FEET:
    mh.addQuadFoot(n, "root_joint", presets.TALOS_QUAD)
nq, nv, mass = mh.nq, mh.nv, mh.getMass()
mpc_conf = {k: v for k, v in presets.talos_mpc_settings(mh, max_iters=1).items() if k in presets.MPC_KEYS}
ocp = CentroidalOCP(presets.talos_centroidal_settings(mh), mh)  # force_size 6: u = [(f, tau) per foot]
ocp.createProblem(np.zeros(9), T, 6, -9.81, False)
mpc = BatchedMPC(mpc_conf, ocp, B, lib=LIB)
mpc.generateCycleHorizon(presets.walk_cycle())
V = np.zeros((B, 6))
V[:, 0] = np.linspace(0.0, 0.1, B)
mpc.switchToWalk(V[0])
mpc.setVelocityBaseBatched(V)

dt_mpc, N_simu = 0.01, 10
dt_simu = dt_mpc / N_simu
id_settings = dict(kp_base=7.0, kp_com=7.0, kp_posture=10.0, kp_contact=10.0, kp_feet_tracking=2000.0, w_base=50.0, w_com=100.0, w_posture=1.0,
                   w_contact_force=1e-6, w_contact_motion=1e-3, w_feet_tracking=100.0)  # those of examples/talos_centroidal_id_batched.py
effort, vmax = presets.TALOS_EFFORT[:12], presets.TALOS_VMAX[:12]  # the legs of the built-in biped
centroidal_ID = CentroidalID(mh, dt_simu, id_settings, effort, vmax, batch=B, lib=LIB)
sim = BatchedRobotSim(mh, force_size=6, batch=B, lib=LIB)
Kp, Kd = [0.0] * 6, [50.0] * 6  # Baumgarte gains of the contacts (those of examples/talos_centroidal_id_batched.py)
print("controller of %d joints: %d variables, %d rows per QP; simulator: %d robots, %d contact rows each"
      % (table.njoints, nv + 24, nv + 24 + 6 + 12 + 34 + nv - 6, sim.B, 6 * sim.nf))

X0 = np.tile(mh.getReferenceState(), (B, 1))
z0 = X0[0, 2]
centroidal_ID.shareStream(mpc)  # MPC step, targets, QP solves and simulator steps in one in-order queue
sim.shareStream(mpc)
if LIB is None:  # states, torques and the running maximum of |tau| / limit in torch tensors, torch's work on the same queue
    import torch

    X = torch.from_numpy(X0).cuda()
    tau = torch.zeros((B, nv - 6), dtype=torch.float64, device="cuda")
    lim = torch.from_numpy(np.ascontiguousarray(effort)).cuda()
    over = torch.zeros((), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    queue = torch.cuda.ExternalStream(mpc.stream())
    x_ptr, tau_ptr = X.data_ptr(), tau.data_ptr()
else:  # (the CPU test build of the kernel bodies: its "device" memory is the host's)
    X, tau, over = X0.copy(), np.zeros((B, nv - 6)), 0.0
    x_ptr, tau_ptr = X.ctypes.data, tau.ctypes.data
t0 = time.time()
for step in range(steps):
    mpc.iterate_device(x_ptr)
    mpc.wait()
    contact = mpc.ocp_handler.getContactState(0)
    for sub in range(N_simu):
        centroidal_ID.setTargetsFromMPC(mpc, sub * dt_simu)  # CoM, its velocity, foot references, wrenches: interpolated and written on the device
        centroidal_ID.solve_device(x_ptr, tau_ptr)
        sim.stepDevice(x_ptr, tau_ptr, contact, dt_simu, Kp=Kp, Kd=Kd)
        if LIB is None:
            with torch.cuda.stream(queue):
                over = torch.maximum(over, (tau.abs() / lim).max())
        else:
            over = max(over, np.abs(tau / effort).max())
sim.wait()
wall = time.time() - t0
resid = centroidal_ID.getResiduals().max()
centroidal_ID.shareStream(None)
sim.shareStream(None)
if LIB is None:
    torch.cuda.synchronize()
    X, tau, over = X.cpu().numpy(), tau.cpu().numpy(), float(over.cpu())
sim_time = steps * dt_mpc
up = np.isfinite(X).all(1) & (np.abs(X[:, 2] - z0) < 0.05)
print("%d bipeds, %.2f s of walking: base x %.3f m (0 m/s command) ... %.3f m (0.1 m/s command)" % (B, sim_time, X[0, 0], X[-1, 0]))
print("robots that stay up: %d of %d" % (int(up.sum()), B))
print("base height %.3f .. %.3f m (reference %.3f); largest |tau| / limit %.3f; QP residual %.1e" % (np.nanmin(X[:, 2]), np.nanmax(X[:, 2]), z0, over, resid))
print("%.2f s of simulated time (%d MPC steps x %d controller ticks) in %.2f s: %.1f ms per MPC period, %.0f robot-seconds per second"
      % (sim_time, steps, N_simu, wall, 1e3 * wall / steps, B * sim_time / wall))
assert np.all(np.isfinite(X)) and over <= 1.0 + 1e-6
