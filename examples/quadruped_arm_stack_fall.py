"""The push grid of examples/quadruped_arm_stack_push.py with a fall detector on the device: the eight corners of a trunk box and the four
knees are body points (BatchedRobotSim.setBodyPoints), so a robot that a push knocks over lands on its trunk or its knees
instead of sinking through the floor with everything but its feet, and the ground step itself writes a touch byte per robot.  After every
MPC period the robots whose byte is set are put back to their start state on the shared stream (torch.where on the device tier, numpy on
the CPU test build), and the same device mask goes to BatchedMPC.reset_instances_device and BatchedRobotSim.resetGroundWarmStartDevice:
nothing crosses the host inside the loop.  Per push force it prints how many robots touched down and how often, and the rate in simulated
robot-seconds per second beside the same run with the resets off (both are measurements).

    python examples/quadruped_arm_stack_fall.py [batch] [mpc_steps] [push_start_ms] [push_ms] [force_scale]

SMPC_EXAMPLE_TRACE=<file.npz>: the states after every MPC period [mpc_steps][batch][nq + nv] (after the resets), the touch bytes at the
end of every period, the start states and the final states of the run with the resets on.  SMPC_EXAMPLE_NO_POINTS=1: no body points (the
robots of quadruped_arm_stack_push.py).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-mpc_amd", "python"))
from simple_mpc import box_points, BatchedMPC, BatchedRobotSim, CentroidalID, CentroidalOCP, RobotModelC, RobotModelHandler, load_robot, robot_from_table  # noqa: E402

LIB = None  # the shipped HIP library
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
push_start = int(sys.argv[3]) if len(sys.argv) > 3 else 200  # ms, a multiple of the MPC period
push_len = int(sys.argv[4]) if len(sys.argv) > 4 else 100
scale = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
POINTS_ON = not os.environ.get("SMPC_EXAMPLE_NO_POINTS")
if push_start % 10 or push_len % 10 or push_len < 10:
    raise SystemExit("push_start_ms, push_ms: multiples of the MPC period of 10 ms")
T = int(os.environ.get("SMPC_EXAMPLE_HORIZON", "50"))
MU_PLAN = 0.8  # the friction coefficient the MPC plans with: the default column
MUS = [MU_PLAN, 0.4, 0.2, 1.2]
FORCES = [scale * f for f in (0.0, 60.0, 120.0, 180.0, 240.0)]  # N along +y and as much along -z on the base; the first row has no push

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

X0 = np.tile(mh.getReferenceState(), (B, 1))
X0[:, 7 + 12] = np.linspace(-0.5, 0.5, B)  # first arm joint (yaw): every robot holds its arm differently
cell = np.arange(B) % (len(FORCES) * len(MUS))
row, col = cell % len(FORCES), cell // len(FORCES)
push = np.zeros((B, 6))
push[:, 1] = np.array(FORCES)[row]
push[:, 2] = -push[:, 1]  # (the shove comes from the side and from above in equal parts: it presses the robot down rather than sliding it away)
# the body points: the corners of a box around the trunk and the four knees (the origins of the shank joints 3, 6, 9, 12)
bj, bo = box_points(0, (0.0, 0.0, 0.0), (0.19, 0.05, 0.057))
bj, bo = np.r_[bj, [3, 6, 9, 12]], np.r_[bo, np.zeros((4, 3))]


class _DeviceBytes:
    """A uint8 device array behind a raw pointer, for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="|u1", data=(ptr, False), version=2)


def run(resets):
    mpc = BatchedMPC(dict(support_force=-mass * gravity[2], TOL=1e-4, mu_init=1e-8, max_iters=1, num_threads=1, swing_apex=0.10, T_fly=30, T_contact=10,
                          timestep=0.01), problem, B, lib=LIB)
    mpc.generateCycleHorizon([quadru] * 10 + [dict(quadru, FL_foot=False, RR_foot=False)] * 30 + [quadru] * 10 + [dict(quadru, FR_foot=False, RL_foot=False)] * 30)
    mpc.switchToStand()
    centroidal_ID = CentroidalID(mh, dt_simu, id_settings, effort, vmax, batch=B, lib=LIB)
    sim = BatchedRobotSim(mh, force_size=3, batch=B, lib=LIB)
    # the plane under the feet of the reference pose: over the plane z = 0 the gaps are the heights of the feet
    sim.setGround(ground_z=0.0)
    ground_z = float(sim.groundDynamics(X0[:1], np.zeros((1, nv - 6)), dt_simu)["gap"].min())
    sim.setGround(ground_z=ground_z, mu=MU_PLAN)
    sim.setGroundEnv(mu=np.array(MUS)[col])
    sim.setPush(np.zeros((B, 6)), joint=0)
    if POINTS_ON:
        sim.setBodyPoints(bj, bo)
    centroidal_ID.shareStream(mpc)  # MPC step, targets, QP solves, simulator steps and resets in one in-order queue
    sim.shareStream(mpc)
    touch_ptr = sim.bodyPointsDevicePointers()["body_touch"]
    if LIB is None:  # states, torques, the mask and the counters in torch tensors on the shared stream
        import torch

        stream = torch.cuda.ExternalStream(mpc.stream())
        X = torch.from_numpy(X0).cuda()
        Xs = torch.from_numpy(X0).cuda()
        tau = torch.zeros((B, nv - 6), dtype=torch.float64, device="cuda")
        count = torch.zeros(B, dtype=torch.int64, device="cuda")
        touch = torch.as_tensor(_DeviceBytes(touch_ptr, B), device="cuda") if touch_ptr else torch.zeros(B, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        x_ptr, tau_ptr = X.data_ptr(), tau.data_ptr()
    else:  # (the CPU test build of the kernel bodies: its "device" memory is the host's)
        import ctypes

        X, tau, count = X0.copy(), np.zeros((B, nv - 6)), np.zeros(B, np.int64)
        touch = np.ctypeslib.as_array((ctypes.c_uint8 * B).from_address(touch_ptr)) if touch_ptr else np.zeros(B, np.uint8)
        x_ptr, tau_ptr = X.ctypes.data, tau.ctypes.data
    states, masks = [], []
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
        # the touch bytes of the period's last step: the fallen robots go back to their start state, their MPC instance to its cold start and
        # their warm row to zero, all on the shared stream
        if LIB is None:
            with torch.cuda.stream(stream):
                count += touch
                if resets:
                    X.copy_(torch.where(touch[:, None] != 0, Xs, X))
        else:
            sim.wait()
            count += touch
            if resets:
                X[touch != 0] = X0[touch != 0]
        if resets and touch_ptr:
            mpc.reset_instances_device(touch_ptr)
            sim.resetGroundWarmStartDevice(touch_ptr)
        if os.environ.get("SMPC_EXAMPLE_TRACE") and resets:  # (the trace reads the host: its time is taken out of the rate)
            sim.wait()
            mpc.wait()
            ts = time.time()
            states.append(X.cpu().numpy() if LIB is None else X.copy())
            masks.append(touch.cpu().numpy() if LIB is None else touch.copy())
            t_stats += time.time() - ts
    sim.wait()
    mpc.wait()
    wall = time.time() - t0 - t_stats
    centroidal_ID.shareStream(None)
    sim.shareStream(None)
    if LIB is None:
        torch.cuda.synchronize()
        X, count = X.cpu().numpy(), count.cpu().numpy()
    return X, count, wall, states, masks, ground_z, sim.ground_points


quadru = dict.fromkeys(feet, True)
dt_mpc, N_simu = 0.01, 10
dt_simu = dt_mpc / N_simu
id_settings = dict(kp_base=7.0, kp_com=7.0, kp_posture=10.0, kp_contact=10.0, kp_feet_tracking=2000.0, w_base=50.0, w_com=100.0, w_posture=1.0,
                   w_contact_force=1e-6, w_contact_motion=1e-3, w_feet_tracking=100.0)  # those of quadruped_arm_stack_resident.py, untuned for the ground
effort = np.r_[np.array([23.7, 23.7, 45.43] * 4), np.full(6, 30.0)]
vmax = np.r_[np.array([30.1, 30.1, 15.7] * 4), np.full(6, 20.0)]
sim_time = steps * dt_mpc
X, count, wall, states, masks, ground_z, npts = run(True)
print("controller of %d joints; simulator: %d robots on the plane z = %.4f m, %d contact points and %d body points each (%s); grid: mu %s x push %s N along +y and -z "
      "from %d ms for %d ms" % (table.njoints, B, ground_z, npts, len(bj), "on" if POINTS_ON else "off", MUS, FORCES, push_start, push_len))
print("%d robots, %.2f s; per push force: robots that touched down with their trunk or a knee / robots, MPC periods that ended with a touch:" % (B, sim_time))
for r, f in enumerate(FORCES):
    sel = row == r
    if sel.any():
        print("%8.0f N %10s %8d" % (f, "%d/%d" % ((count[sel] > 0).sum(), sel.sum()), count[sel].sum()))
for i in np.flatnonzero(count > 0)[:8]:
    print("robot %d (push %.0f N, mu %.1f) touched down: %d resets" % (i, push[i, 1], MUS[col[i]], count[i]))
print("every state finite at the end: %s" % bool(np.isfinite(X).all()))
rate_on = B * sim_time / wall
_, count_off, wall_off, _, _, _, _ = run(False)
print("%.2f s of simulated time (%d MPC steps x %d controller ticks): %.1f robot-seconds per second with the resets on, %.1f with the resets off "
      "(%d robots down at some time there)" % (sim_time, steps, N_simu, rate_on, B * sim_time / wall_off, int((count_off > 0).sum())))
if os.environ.get("SMPC_EXAMPLE_TRACE"):
    np.savez(os.environ["SMPC_EXAMPLE_TRACE"], states=np.array(states), touch=np.array(masks), X0=X0, X=X)
