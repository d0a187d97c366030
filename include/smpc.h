/*
 * smpc.h -- C ABI of the MI355X batched locomotion-MPC engine (libsmpc_hip.so).
 *
 * Drop-in boundary for the hot path of Simple-Robotics/simple-mpc: `MPC::iterate()` and what it drives
 * (reference src/mpc.cpp:189-218).  Plain pointers and sizes only; all arrays are row-major,
 * instance-major ([B][...]), IEEE double.  Host C++ (simple-mpc_amd/csrc/simple_mpc.hpp) and the
 * Python module `simple_mpc` bind these symbols; INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Every function returns 0 on success and a negative code on failure; smpc_last_error() then holds the
 * message (the reference throws std::runtime_error at the same places: src/kinodynamics.cpp:175,235,
 * 279,299; src/ocp-handler.cpp:28,32,76).
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef SMPC_H
#define SMPC_H
#include "smpc_robot.h"
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_OK 0
#define SMPC_ERR_INVALID (-1)
#define SMPC_ERR_RUNTIME (-2)
#define SMPC_ERR_NO_DEVICE (-3)

typedef struct smpc_handle smpc_handle;

/* KinodynamicsSettings: reference include/simple-mpc/kinodynamics.hpp:24-51 (same field names).
 * Matrices are dense row-major: w_x (ndx x ndx), w_u (nu x nu), w_frame (3x3), w_cent, w_centder (6x6). */
typedef struct smpc_kinodynamics_settings
{
  double timestep;
  const double * w_x;
  const double * w_u;
  const double * w_frame;
  const double * w_cent;
  const double * w_centder;
  const double * qmin;
  const double * qmax;
  double gravity[3];
  double mu;
  double Lfoot;
  double Wfoot;
  int force_size;
  int kinematics_limits;
  int force_cone;
  int land_cstr;
  /* createProblem(x0, T, force_size, gravity, terminal_constraint): the last argument (reference src/ocp-handler.cpp:96-137).
   * Non-zero adds the DCM equality com + tau vcom = com_ref at the terminal node (src/kinodynamics.cpp:366-388). */
  int terminal_constraint;
} smpc_kinodynamics_settings;

/* CentroidalSettings: reference include/simple-mpc/centroidal-dynamics.hpp:27-43 (same field names).
 * w_u (nu x nu, nu = force_size * nfeet) dense row-major; the other weights are 3 x 3. */
typedef struct smpc_centroidal_settings
{
  double timestep;
  const double * w_u;
  const double * w_com;
  const double * w_linear_mom;
  const double * w_angular_mom;
  const double * w_linear_acc;
  const double * w_angular_acc;
  double gravity[3];
  double mu;
  double Lfoot;
  double Wfoot;
  int force_size;
} smpc_centroidal_settings;

/* FullDynamicsSettings: reference include/simple-mpc/fulldynamics.hpp:28-65 (same field names).
 * w_x (ndx x ndx), w_u (nu x nu, nu = nv - 6), w_cent (6 x 6), w_forces, w_frame (force_size x force_size), dense row-major;
 * umin / umax (nu), qmin / qmax (nv - 6), Kp_correction / Kd_correction (force_size). */
typedef struct smpc_fulldynamics_settings
{
  double timestep;
  const double * w_x;
  const double * w_u;
  const double * w_cent;
  const double * w_forces;
  const double * w_frame;
  const double * umin;
  const double * umax;
  const double * qmin;
  const double * qmax;
  const double * Kp_correction;
  const double * Kd_correction;
  double gravity[3];
  double mu;
  double Lfoot;
  double Wfoot;
  int force_size;
  int torque_limits;
  int kinematics_limits;
  int force_cone;
  int land_cstr;
  int terminal_constraint; /* createProblem's last argument: DCM terminal equality (reference src/fulldynamics.cpp:433-455) */
} smpc_fulldynamics_settings;

/* MPCSettings: reference include/simple-mpc/mpc.hpp:29-49 (same field names). */
typedef struct smpc_mpc_settings
{
  double swing_apex;
  double support_force;
  double TOL;
  double mu_init;
  int max_iters;
  int num_threads; /* accepted for API compatibility; the GPU path ignores it */
  int T_fly;
  int T_contact;
  int T;
  double timestep;
} smpc_mpc_settings;

/* Built-in robot tables ("go2_like", "biped_like"); NULL if unknown.
 * Replaces RobotModelHandler(model, "standing", base) + addPointFoot
 * (reference src/robot-handler.cpp:12-60; examples/go2_kinodynamics.py:23-27). */
const smpc_robot_model * smpc_builtin_robot(const char * name);

const char * smpc_last_error(void);
/* SolverProxDDP's convergence test inside iterate (reference src/mpc.cpp:43 hands TOL to the solver, :212 runs it: `run` returns as soon
 * as the primal and dual infeasibilities are below TOL).  Off by default -- the metric of record is "at fixed ProxDDP iterations"; on: an
 * instance that is converged at the start of an iteration takes no further step in this control step (its iterate, multipliers and
 * regularisation stay; the feedback gains are those of the sweep at the converged point).  Kinodynamics and full-dynamics handles. */
int smpc_set_early_exit_on_tol(smpc_handle * h, int on);
/* number of HIP devices visible (0 => every compute entry point fails loudly) */
int smpc_device_count(void);

/* KinodynamicsOCP(settings, model) + createProblem(x_ref, T, force_size, gravity, false) + MPC(settings, ocp):
 * reference src/kinodynamics.cpp:29-38, src/ocp-handler.cpp:96-137, src/mpc.cpp:19-99.
 * `gravity_arg` is the 4th argument of createProblem (its sign convention differs between callers,
 * SURVEY App. C.8).  Performs the cold solve (<= 100 ProxDDP iterations). */
int smpc_create(
  const smpc_robot_model * robot, const smpc_kinodynamics_settings * ocp, const smpc_mpc_settings * mpc, int batch,
  double gravity_arg, int device_id, smpc_handle ** out);
/* CentroidalOCP(settings, model) + createProblem(getCentroidalState(), T, force_size, gravity, false) + MPC(settings, ocp):
 * reference src/centroidal-dynamics.cpp:27-37, src/ocp-handler.cpp:96-137, src/mpc.cpp:19-99 (SURVEY 8a rows a6, a8, a9;
 * BASELINE config "Go2 centroidal (9-dim state), H = 50").  The handle is used through the same entry points as a
 * kinodynamics handle: smpc_iterate still takes the measured MULTIBODY states [B][nq + nv] (the reference reduces them with
 * getCentroidalState, src/mpc.cpp:200); the problem state is [com; h_lin; h_ang], so xs is [B][H+1][9], us [B][H][3 nfeet],
 * K0 [B][3 nfeet][9], vs [B][H][2 nfeet] (friction-cone rows), smpc_get_state_derivative01 [B][2][9],
 * smpc_get_reference_poses the contact positions [B][H][nfeet][3], smpc_set_x_reference takes 9 doubles.
 * smpc_get_dims reports nq, nv of the robot and nx = ndx = 9.  Entry points that are specific to the kinodynamics
 * problem (debug_get_lq, debug_get_terminal, get_x_device) fail with SMPC_ERR_INVALID on such a handle.
 * Robots: the OCP depends on the robot through its mass, its feet and the force size only, so ANY table of smpc_robot.h with
 * (4 feet, force_size 3) or (2 feet, force_size 6) and 2 <= njoints <= SMPC_MAX_JOINTS is accepted.  The two built-in shapes (13 joints /
 * 4 point feet, 23 joints / 2 flat feet) use the state front end of their stage-kernel family; every other table uses the front end on
 * the run-time joint tree and is validated before anything is allocated -- parent[0] == -1, 0 <= parent[j] < j, jtype[0] == 0,
 * jtype[j] in 1..3, nq == njoints + 6, nv == njoints + 5, foot_joint in range, every number finite, masses positive, total_mass equal to
 * the sum of the masses to 1e-9 relative: SMPC_ERR_INVALID with a message that names the field.  Other foot counts are refused. */
int smpc_create_centroidal(
  const smpc_robot_model * robot, const smpc_centroidal_settings * ocp, const smpc_mpc_settings * mpc, int batch,
  double gravity_arg, int device_id, smpc_handle ** out);
/* FullDynamicsOCP(settings, model) + createProblem(x_ref, T, force_size, gravity, false) + MPC(settings, ocp):
 * reference src/fulldynamics.cpp:30-76 (contact models, ProximalSettings(1e-9, 1e-10, 10)), :78-214 (createStage),
 * :418-455 (terminal cost), src/mpc.cpp:19-99 (BASELINE's full-dynamics configuration).  State (q, v),
 * control = the nv - 6 joint torques; nc = nu (torque box) + nv - 6 (joint box) [+ cone rows of 6-D feet].  Used through the
 * same entry points as a kinodynamics handle; smpc_set_stage_reference takes what = 2 for the contact-force references
 * (setReferenceForces, src/fulldynamics.cpp:258-300) and smpc_get_contact_forces reads MPC::getContactForces. */
int smpc_create_fulldynamics(
  const smpc_robot_model * robot, const smpc_fulldynamics_settings * ocp, const smpc_mpc_settings * mpc, int batch,
  double gravity_arg, int device_id, smpc_handle ** out);
/* MPC::getContactForces(t) for every stage (reference src/mpc.cpp:354-380): contact forces of the constrained dynamics at the
 * solution, out [B][H][nfeet][force_size], zero for feet that are not in contact at that stage.  Full-dynamics handles only. */
int smpc_get_contact_forces(smpc_handle * h, double * out);
int smpc_destroy(smpc_handle * h);

/* dims[0..7] = nq, nv, nx, ndx, nu, nc, nfeet, H */
int smpc_get_dims(const smpc_handle * h, int * dims);

/* MPC::generateCycleHorizon (reference src/mpc.cpp:101-187). contact_states: [n_states][nfeet], 0/1. */
int smpc_generate_cycle_horizon(smpc_handle * h, const uint8_t * contact_states, int n_states);
/* MPC::switchToWalk / switchToStand (reference src/mpc.cpp:382-392) */
int smpc_switch_to_walk(smpc_handle * h, const double * velocity_base6);
int smpc_switch_to_stand(smpc_handle * h);
/* One velocity command per instance, V: [B][6] (MPC::velocity_base_ is a public member the callers of the reference assign
 * directly, bindings/expose-mpc.cpp:86; a batch of robots is not steered by one joystick).  The walking / standing state is
 * unchanged.  smpc_switch_to_walk / smpc_switch_to_stand broadcast one command to every instance. */
int smpc_set_velocity_base_batched(smpc_handle * h, const double * V);
/* Per-stage references of the horizon -- the OCPHandler setters / getters (reference include/simple-mpc/ocp-handler.hpp:
 * 66-127; src/kinodynamics.cpp:154-306, src/centroidal-dynamics.cpp:120-304, src/ocp-handler.cpp:58-81), broadcast over the
 * batch; t >= horizon is the reference's "Stage index exceeds stage vector size" error.
 *   what = 0: control target (setReferenceControl; setReferenceForce(s) are segments of it), n = nu
 *   what = 1: reference state as setReferenceState / getReferenceState define it, n = nx (kinodynamics: the state_cost
 *             target; centroidal: [com_ref; v_lin; v_ang], stored as momenta m v like the reference does)
 * setPoseBase / setVelocityBase are read-modify-write of what = 1, as in the reference.  Getters return instance 0.
 * Like in the reference, the next smpc_iterate overwrites the foot references of every stage and the state target of the
 * last stage (MPC::updateStepTrackerReferences, src/mpc.cpp:278-313). */
int smpc_set_stage_reference(smpc_handle * h, int t, int what, const double * v, int n);
int smpc_get_stage_reference(smpc_handle * h, int t, int what, double * v, int n);
/* setReferencePose / getReferencePose (translation; src/kinodynamics.cpp:154-169, src/centroidal-dynamics.cpp:151-188) */
int smpc_set_reference_pose(smpc_handle * h, int t, int foot, const double * p3);
int smpc_get_reference_pose(smpc_handle * h, int t, int foot, int instance, double * p3);
/* ... with the rotation of the SE3 (R9: row-major 3 x 3; src/kinodynamics.cpp:154-170, reference tests/problem.cpp:157-160: what was set is
 * what is returned).  MPC::iterate overwrites every stage's pose with (identity rotation, Bezier position) before it solves
 * (src/mpc.cpp:303-309): so does smpc_iterate -- no solve behind this boundary ever evaluates another rotation (the stage kernels use
 * M_ref = (I, p)); a rotation set here lives until the next control step, exactly as in the reference.  smpc_set_reference_pose (translation
 * only) sets the identity rotation. */
int smpc_set_reference_pose_se3(smpc_handle * h, int t, int foot, const double * p3, const double * R9);
int smpc_get_reference_pose_se3(smpc_handle * h, int t, int foot, int instance, double * p3, double * R9);
/* getContactState(t): contact flag per foot (src/kinodynamics.cpp:343-349); getContactSupport = their sum */
int smpc_get_contact_state(smpc_handle * h, int t, uint8_t * out_nfeet);
/* MPC::getCyclingContactState(t, ee_name) for every foot: entry t of the (rotating) contact sequence the cycle horizon was generated
 * from (reference include/simple-mpc/mpc.hpp:144-147, src/mpc.cpp:103-110,230); returns the sequence length, or the length alone
 * when out is NULL.  Error before generateCycleHorizon or for t outside the sequence. */
int smpc_get_cycling_contact_state(smpc_handle * h, int t, uint8_t * out_nfeet);
/* MPC::x_reference_ (public member, reference include/simple-mpc/mpc.hpp:191) */
int smpc_set_x_reference(smpc_handle * h, const double * x_ref);

/* MPC::iterate for the whole batch (reference src/mpc.cpp:189-218). X: [B][nx] measured states (host).
 * Synchronous: returns when the solve is complete. */
int smpc_iterate(smpc_handle * h, const double * X);
/* Same with X already resident in HBM; asynchronous on the handle's stream (pair with smpc_wait). */
int smpc_iterate_device(smpc_handle * h, const double * X_device);
int smpc_wait(smpc_handle * h);
/* The hipStream_t (as void *) every launch of this handle is issued on.  A caller that produces the measured states on the device -- a
 * batched simulator, torch through torch.cuda.ExternalStream -- enqueues its own kernels there: the closed loop
 * iterate_device -> get_x_device -> (caller's kernels) -> iterate_device is then one in-order queue with no host-side wait between control
 * steps.  The stream belongs to the handle.  NULL in the CPU test build. */
void * smpc_get_stream(smpc_handle * h);
/* smpc_iterate without the final synchronisation (X must stay valid until smpc_wait): one host thread keeps several handles -- one per
 * device, each with its share of the batch -- busy at once (include/simple-mpc/batched-mpc.hpp BatchedMPCGroup). */
int smpc_iterate_async(smpc_handle * h, const double * X);
/* The small return set of a control step -- xs[1], us[0], K_0 (what MPC::iterate's caller consumes: reference examples/go2_kinodynamics.py
 * :254-292) -- of every instance of this handle as rows [x1 (nx) | u0 (nu) | K0 (nu x ndx, row-major)] of `out`, `row_doubles` (>= nx + nu
 * + nu ndx) doubles apart.  `out` is typically one slice of a single pinned host buffer that the handles of all devices fill side by
 * side ("async D2H into one pinned host buffer").  Asynchronous on the handle's stream: smpc_wait completes it.
 * Kinodynamics handles. */
int smpc_gather_outputs(smpc_handle * h, double * out, size_t row_doubles);
/* The same rows packed into a DEVICE buffer [batch][row_doubles] by one kernel on the handle's stream, for a caller that moves them itself:
 * a collective towards the process that owns the controllers (one process per device: torch.distributed gather over RCCL), a peer copy, or
 * one copy into pinned memory from a side stream so that the transfer overlaps the next control step.  Kinodynamics handles. */
int smpc_gather_outputs_device(smpc_handle * h, double * out_device, size_t row_doubles);
/* ... and into a buffer on ANOTHER device of the node (hipMemcpyPeerAsync over xGMI on the handle's stream, after the pack kernel): one
 * process, one handle per device, every device's rows gathered on the device that runs the controllers.  `out_peer` points to
 * [batch][nx + nu + nu ndx] doubles on device `dst_device`, rows contiguous.  Kinodynamics handles. */
int smpc_gather_outputs_peer(smpc_handle * h, double * out_peer, int dst_device);
/* Checkpoint / resume (the reference has none; a batched simulator needs it to roll back or migrate a batch).
 * The state is everything a later smpc_iterate depends on: iterate, multipliers, swing trajectories, references, velocity
 * commands, gait bookkeeping -- not the feedback gains of the last solve (the next iterate recomputes them).
 *   smpc_state_size   bytes needed for this handle (it grows with the gait cycle: call it after generateCycleHorizon)
 *   smpc_save_state   writes at most `capacity` bytes to `buffer` (host), returns the number written through *written
 *   smpc_load_state   restores; the buffer must come from a handle of the same kind, batch, horizon and robot
 * After smpc_load_state the handle continues bit-identically to the handle the state was saved from. */
int smpc_state_size(smpc_handle * h, size_t * bytes);
int smpc_save_state(smpc_handle * h, void * buffer, size_t capacity, size_t * written);
int smpc_load_state(smpc_handle * h, const void * buffer, size_t size);
/* Reset single instances of the batch to the cold start (the reference has no such call: one MPC object is one robot, and a user
 * constructs a new one).  After a reset, the solver state of the instance is what the constructor left in it; the problem data are
 * untouched.  Solver state: xs, us, vs, lams, the augmented-Lagrangian centres, the per-instance scalars of smpc_get_info (hence the
 * status word: 0), the line-search selection, the state derivatives of stages 0, 1 and the swing start / end of every foot -- written
 * relative to the current ring head, so that a reset at any control step gives the same trajectory t = 0 .. H.  Problem data: the
 * instance's velocity command and its references, the shared stage list, gait timers, walking / standing state, reference poses and
 * the two switches (early exit, retained state derivatives).  The cold solution is a function of the settings only: it is kept on the
 * device by every handle and is not part of the checkpoint.  With smpc_set_retain_state_derivatives on, the getters of every stage
 * refuse after a reset until the next iterate, as after smpc_load_state.
 *   smpc_reset_instances          re-applies src/mpc.cpp:72-89 to the n instances of a host list (unsorted, duplicates allowed); an index
 *                                 outside [0, B) returns SMPC_ERR_INVALID and changes nothing; n = 0 succeeds and does nothing.  The mask
 *                                 is built on the host and uploaded on the handle's stream, then as below
 *   smpc_reset_instances_device   re-applies src/mpc.cpp:72-89 to every instance with a non-zero byte in mask_device [B] (device memory):
 *                                 one kernel on the handle's stream, no host synchronisation -- a fall detector on the device writes the
 *                                 mask and nothing crosses the host.  The kernel reads the mask: it must stay valid until smpc_wait.
 *                                 The detector this speaks of is body_touch of smpc_robot_sim_get_body_points_last (uint8_t [B]) */
int smpc_reset_instances(smpc_handle * h, const int * instances, int n);
int smpc_reset_instances_device(smpc_handle * h, const uint8_t * mask_device);
/* xs_[t] of every instance into a dense device buffer [B][nx]; asynchronous on the handle's stream.
 * Lets a closed loop keep the measured states resident in HBM (x_meas = xs[1] + noise). */
int smpc_get_x_device(smpc_handle * h, int t, double * out_device);

/* MPC::xs_ / us_ / Ks_ (reference include/simple-mpc/mpc.hpp:187-189; filled at src/mpc.cpp:215-217).
 * out: xs [B][H+1][nx], us [B][H][nu], K0 [B][nu][ndx], Ks [B][H][nu][ndx] */
int smpc_get_xs(smpc_handle * h, double * out);
int smpc_get_us(smpc_handle * h, double * out);
int smpc_get_K0(smpc_handle * h, double * out);
int smpc_get_Ks(smpc_handle * h, double * out);
/* solver multipliers (results_.vs / results_.lams): vs [B][H][nc], lams [B][H+1][ndx] (lams[0] = 0) */
int smpc_get_vs(smpc_handle * h, double * out);
/* (tests) multipliers of the optional rows of a kinodynamics handle: which = 0 friction-cone rows [B][H][2 nfeet],
 * 1 land rows [B][H][nfeet] */
int smpc_debug_get_extra_multipliers(smpc_handle * h, int which, double * out);
int smpc_get_lams(smpc_handle * h, double * out);
/* MPC::getStateDerivative(t) for t = 0,1 (reference src/mpc.cpp:346-352). out: [B][2][2 nv] */
int smpc_get_state_derivative01(smpc_handle * h, double * out);
/* MPC::getStateDerivative(t) for EVERY stage t (reference src/mpc.cpp:346-352: Et.ev[t].xdot of the accepted iterate).
 * Opt-in per handle: with the switch on, every control step (smpc_iterate, smpc_iterate_device, smpc_iterate_async) enqueues one more
 * kernel on the handle's stream after the solve, which evaluates the continuous dynamics of every (instance, stage) at the returned
 * xs[t], us[t] with the stage's contact mask and parameters; off (the default), nothing is launched or allocated.
 *   smpc_set_retain_state_derivatives   on = 1 allocates [B][H][dim] doubles on the first enable (SMPC_ERR_RUNTIME if that fails;
 *                                       the handle stays usable); on = 0 stops the launches
 *   smpc_get_state_derivatives          out [B][H][dim] (host); dim = 2 nv (kinodynamics, full dynamics), 9 (centroidal)
 *   smpc_get_state_derivatives_device   the same into a device buffer, asynchronous on the handle's stream
 * The getters return SMPC_ERR_INVALID when the switch is off, when no iterate has run since it was enabled, and after smpc_load_state
 * or smpc_reset_instances until the next iterate (the buffer is not part of the checkpoint: smpc_state_size does not change).  Stages 0, 1 equal
 * smpc_get_state_derivative01. */
int smpc_set_retain_state_derivatives(smpc_handle * h, int on);
int smpc_get_state_derivatives(smpc_handle * h, double * out);
int smpc_get_state_derivatives_device(smpc_handle * h, double * out_device);
/* MPC::getReferencePose(t, foot).translation() for all t, feet (reference src/mpc.cpp:336-339). out: [B][H][nfeet][3] */
int smpc_get_reference_poses(smpc_handle * h, double * out);
/* MPC::foot_takeoff_times_ / foot_land_times_ (reference include/simple-mpc/mpc.hpp:184-185). which: 0 takeoff, 1 land.
 * Returns the number of entries (<= cap copied). */
int smpc_get_foot_timing(smpc_handle * h, int foot, int which, int * out, int cap);
/* per-instance solver scalars of the last iteration, [B][16]:
 * phi0, dphi0, alpha, phi_new, prim_infeas, dual_infeas, ls_failed, preg, prim_new, cost, cost_new, ls_index */
int smpc_get_info(smpc_handle * h, double * out);
/* Per-instance status word of the last control step (the reference ignores the solver's return value, src/mpc.cpp:212; a batch needs to
 * know which of its members went wrong), out [B]: bit 0 = a non-finite number among the solver scalars (the instance's trajectory
 * must not be used), bit 1 = the last line search failed (the smallest step was taken), bit 2 = the primal regularisation has reached
 * its upper limit.  Returns the number of instances with a non-zero word, or a negative error code. */
#define SMPC_STATUS_NONFINITE 1
#define SMPC_STATUS_LS_FAILED 2
#define SMPC_STATUS_REG_SATURATED 4
int smpc_get_status(smpc_handle * h, int * out);
/* cold-solve trace of the constructor: returns n iterations; out [n][4] = phi0, prim, dual, alpha (cap rows) */
int smpc_get_cold_trace(smpc_handle * h, double * out, int cap);

/* test / debug access to one LQ knot (stage t of instance inst) as assembled by the stage kernel in the
 * LAST iteration: out must hold smpc_lq_size() doubles, laid out A,B,Q,S,R,C,q,r,f,d,lx,lu,lpd,vpd.
 * Centroidal handles answer too (row-major, vector conventions of the oracle's Knot):
 *   point feet: A 9x9, B 9xnu, Q 9x9, S 9xnu, R nuxnu, Dd ncxnu (cone rows; Cd is structurally zero; an inactive row is zero), q 9, r nu, f 9,
 *               d nc, act nc (1.0 / 0.0), any ("a cone row of the stage is active"), preg (the regularisation the iteration used) --
 *               the stage record of the kernel pipeline, unpacked on the host through the maps the backward sweep gathers through;
 *   6-D feet:   the dense knot of the sweep: the full-dynamics layout A,B,Q,S,R,Cd,Dd,q,r,f,d,lx,lu,lpd,vpd,act,cdirty with ndx = 12 (the state
 *               padded from 9 to 12) and nu + 17 nfeet rows (the nu control-box rows are absent);
 *   a handle created with SMPC_CENT_FUSED=1 (cross-check build) keeps no record and answers SMPC_ERR_INVALID. */
int smpc_lq_size(const smpc_handle * h);
int smpc_debug_get_lq(smpc_handle * h, int inst, int t, double * out);
/* last line-search steps: dxs [B][H+1][ndx], dus [B][H][nu] */
int smpc_debug_get_steps(smpc_handle * h, double * dxs, double * dus);
/* terminal node of the last iteration for one instance: QN [ndx][ndx], qN [ndx] (centroidal handles with 6-D feet: ndx = 12, as their knot) */
int smpc_debug_get_terminal(smpc_handle * h, int inst, double * QN, double * qN);
/* last multiplier steps of a centroidal handle: dvs [B][H][nc], dlams [B][H][9] with dlams[t] = step of lambda_{t+1} */
int smpc_debug_get_dual_steps(smpc_handle * h, double * dvs, double * dlams);

/* in-kernel phase timers of the Riccati sweep (shader cycles, block 0 only); needs SMPC_PHASE_PROFILE=1
 * in the environment at smpc_create time. out: 64 doubles */
int smpc_debug_get_phase_cycles(smpc_handle * h, double * out64);

/* profiling: when enabled every kernel launch is bracketed by HIP events on the handle's stream.
 * smpc_get_kernel_times: ms[9], calls[9] for recede, deriv, riccati, forward, trial, select, apply, tree, tree_ls (the lane-per-problem tree
 * pass that precedes the derivative resp. the line-search kernel of a kinodynamics handle). */
int smpc_set_profiling(smpc_handle * h, int enabled);
/* number of kernel slots this library reports (9 today; grows when kernels are added) */
int smpc_kernel_time_slots(void);
/* the first min(n, smpc_kernel_time_slots()) slots into ms[n], calls[n].  Centroidal handles: frontend, step (6-D feet: recede), deriv, riccati,
 * forward, line search, and for 6-D feet the candidate kernel of the line search in the slot behind them. */
int smpc_get_kernel_times_n(smpc_handle * h, double * ms, long * calls, int n);
/* the same without a capacity: writes smpc_kernel_time_slots() entries -- size the arrays with that call, or use the _n form */
int smpc_get_kernel_times(smpc_handle * h, double * ms, long * calls);
int smpc_reset_kernel_times(smpc_handle * h);

/* ---- interpolation between MPC knots (replaces the Interpolator class,
 *      reference include/simple-mpc/interpolator.hpp, src/interpolator.cpp:5-78) ----
 * smpc_interpolate: batched targets for the whole-body controller that follows the MPC, from the solution held by the
 *   handle, as the reference examples compute them (examples/go2_kinodynamics.py:276-284):
 *     x_out     [B][nx]    interpolateState over xs[0 .. knots-1] (configuration on the manifold, velocity linear)
 *     acc_out   [B][nv]    interpolateLinear over getStateDerivative(t)[nv:] with the joint part replaced by
 *                          us[t][3 nf:], t = 0, 1
 *     force_out [B][3 nf]  interpolateLinear over us[t][: 3 nf], t = 0, 1
 *   delay >= 0 (seconds after the last smpc_iterate); beyond the last interval the last knot is returned, like the
 *   reference.  Any output pointer may be NULL.  Host buffers.
 *   Centroidal handle (examples/talos_centroidal.py: interpolateLinear over states, state derivatives and forces):
 *     x_out [B][9], acc_out [B][9] = interpolated getStateDerivative, force_out [B][3 nf].
 * smpc_interpolate_knots: the Interpolator methods on explicit host knot lists [n][dim]:
 *     kind 0 interpolateState (dim = nq + nv), 1 interpolateConfiguration (dim = nq), 2 interpolateLinear (any dim).
 *   Errors mirror the reference's assertions ("State is not of the right size"). */
int smpc_interpolate(smpc_handle * h, double delay, int knots, double * x_out, double * acc_out, double * force_out);

/* ---- full-dynamics model, first block: constrained forward dynamics of n states -- replaces
 *      pinocchio::constraintDynamics as called by Aligator's MultibodyConstraintFwdDynamics for the contacts
 *      FullDynamicsOCP builds (reference src/fulldynamics.cpp:39,50-75,139): CONTACT_3D, LOCAL frame, Baumgarte corrector
 *      Kp / Kd [3] (NULL = 0), actuation [0; I].  X [n][nq + nv], tau [n][nv - 6], contact_mask [n] (bit f = foot f in
 *      contact), all host.  Outputs (host): a_out [n][nv]; lambda_out [n][3 nfeet] contact forces ON the robot in the contact
 *      frames, the feet in contact first (in foot order), remaining entries 0; iters_out [n] proximal iterations (may be
 *      NULL); kernel_ms: wall time of the launch (may be NULL).  prox_accuracy / prox_mu / prox_max_iter <= 0 select the
 *      reference's ProximalSettings(1e-9, 1e-10, 10).  n need not be the handle's batch size; the handle supplies the
 *      robot table and gravity.  Kinodynamics handles (the quadruped, CONTACT_3D) and -- round 4 -- full-dynamics handles of either
 *      robot: the contact model is the handle's (3-D LOCAL point feet, or 6-D LOCAL_WORLD_ALIGNED flat feet with Kp / Kd [6] and
 *      lambda_out [n][6 nfeet] contact wrenches). */
int smpc_full_forward_dynamics(
  smpc_handle * h, int n, const double * X, const double * tau, const unsigned * contact_mask, const double * Kp,
  const double * Kd, double prox_accuracy, double prox_mu, int prox_max_iter, double * a_out, double * lambda_out,
  int * iters_out, double * kernel_ms);

/* ---- state feedback front-end (replaces RobotDataHandler::updateInternalData(x, false) and
 *      getCentroidalState, reference src/robot-handler.cpp:106-127,142-149) for a batch of measured multibody states
 *      X [B][nx] (host): feet [B][nf][3] foot positions (world), com [B][3], hg [B][6] centroidal momentum
 *      [linear; angular about the CoM], centroidal_state [B][9] = [com; h_lin; h_ang].  Any output may be NULL.
 *      Every kind of handle: the kinodynamics, centroidal and full-dynamics OCPs of the quadruped and of the biped. */
int smpc_update_internal_data(smpc_handle * h, const double * X, double * feet, double * com, double * hg, double * centroidal_state);
/* (tests) smpc_update_internal_data computed by the front end on the run-time joint tree (the one a centroidal handle of a robot other
 * than the two built-in shapes runs in every control step) on the robot table of ANY centroidal handle, the built-in shapes included:
 * same arguments, same outputs.  Other handle kinds: SMPC_ERR_INVALID. */
int smpc_debug_frontend_rt(smpc_handle * h, const double * X, double * feet, double * com, double * hg, double * centroidal_state);
/* Riccati feedback application between MPC knots (reference examples/go2_fulldynamics.py:271-285):
 *   u_out[b] = interpolateLinear(us)[b] - Ks[0][b] * difference(X_meas[b], interpolateState(xs)[b])
 * X_meas [B][nx], u_out [B][nu] (host).  Centroidal handle: X_meas are still the measured multibody states [B][nq + nv];
 * the feedback acts on their centroidal state, u_out[b] = f(d) - K0 (x(d) - getCentroidalState(X_meas[b])). */
int smpc_riccati_feedback(smpc_handle * h, double delay, const double * X_meas, double * u_out);
int smpc_interpolate_knots(int kind, double delay, double timestep, const double * knots, int n, int dim, double * out, int device_id);

/* ---- friction compensation (replaces FrictionCompensation::computeFriction, reference
 *      src/friction-compensation.cpp:22-37): torque[b][j] += viscous[j] * velocity[b][j] + dry[j] * sign(velocity[b][j])
 *      for a batch of joint velocity / torque vectors of size nu (host buffers, torque in / out).  velocity_size /
 *      torque_size are the per-instance vector lengths the caller holds: a mismatch with nu is the reference's
 *      "Velocity has wrong size" / "Torque has wrong size" error. */
int smpc_friction_compensation(
  const double * dry, const double * viscous, int nu, const double * velocity, int velocity_size, double * torque, int torque_size,
  int batch, int device_id);

/* ---- centroidal model (replaces CentroidalFwdDynamics + IntegratorEuler as composed in
 *      reference src/centroidal-dynamics.cpp:79-81; the centroidal state itself comes from smpc_update_internal_data) ----
 * Batched forward step with derivatives, 3-D contact forces:
 *     x = [c; h; L] (CoM, linear momentum, angular momentum about the CoM),  u = [f_1 .. f_nfeet]
 *     xdot = [h / m ;  m g + sum_{contact} f_i ;  sum_{contact} (p_i - c) x f_i],   Xnext = x + timestep * xdot
 *     A = d Xnext / dx  [B][9][9],   B = d Xnext / du  [B][9][3 nfeet]   (row-major; columns of feet in the air are zero)
 * X [B][9], U [B][3 nfeet], contact [B][nfeet] (0 / 1), contact_pos [B][nfeet][3]; host buffers; A and B may be NULL. */
int smpc_centroidal_dynamics(
  double mass, const double * gravity, double timestep, int nfeet, const double * X, const double * U, const unsigned char * contact,
  const double * contact_pos, int batch, double * Xnext, double * A, double * B, int device_id);

/* ---- whole-body inverse-dynamics QP: KinodynamicsID (reference include/simple-mpc/inverse-dynamics/kinodynamics-id.hpp:17-92,
 *      src/inverse-dynamics/kinodynamics-id.cpp:7-237), batched: one QP per robot and control tick, 3-D point feet.
 *      Field names of KinodynamicsID::Settings; the limits the reference reads from the pinocchio model (effortLimit, velocityLimit,
 *      lower / upperPositionLimit of the actuated joints) are passed explicitly; admm_* are the solver's own (0 = defaults). ---- */
typedef struct smpc_id_settings
{
  double friction_coefficient;
  double contact_weight_ratio_max;
  double contact_weight_ratio_min;
  double kp_base, kp_posture, kp_contact;
  double w_base, w_posture, w_contact_motion, w_contact_force; /* <= 0: task disabled, as in the reference */
  int contact_motion_equality;
  double control_dt;
  const double * effort_limit;   /* nv - 6 */
  const double * velocity_limit; /* nv - 6 */
  const double * q_min;          /* nv - 6 */
  const double * q_max;          /* nv - 6 */
  int admm_iters;                /* cap on the ADMM iterations per solve (default 400; residuals are checked every 20 iterations and the loop
                                    stops below 1e-7; warm-started from the previous tick) */
  double admm_rho, admm_sigma, admm_alpha; /* defaults 0.1, 1e-6, 1.6 */
  double admm_tol;               /* 0: default 1e-7 ; < 0: never stop early (exactly admm_iters iterations) */
  /* CentroidalID::Settings (include/simple-mpc/inverse-dynamics/centroidal-id.hpp): centroidal != 0 selects that controller -- the base
   * task keeps its orientation rows, a centre-of-mass task and a position-tracking task per foot out of contact are added; the posture
   * and base targets stay at the reference state (centroidal-id.cpp:60-84) */
  int centroidal;
  double kp_com, kp_feet_tracking;
  double w_com, w_feet_tracking; /* <= 0: task disabled */
  /* The reference AS CODED (src/inverse-dynamics/kinodynamics-id.cpp:222-223: setDerivative is called twice, so the base acceleration
   * target becomes the velocity reference of the base task and its acceleration reference stays zero).  0 (default): velocity and
   * acceleration references from the respective targets -- with zero base targets, as in the reference's tests, both coincide. */
  int base_reference_as_coded;
  /* TSID's TaskJointPosVelAccBounds in full (time step 2 control_dt, braking-distance position bounds, viability bounds with the default
   * acceleration limit; setImposeBounds(true, true, true, false) of kinodynamics-id.cpp:80-88).  0 (default): position / velocity limits
   * as acceleration bounds over one control period. */
  int tsid_joint_bounds;
  /* Robots with flat (QUAD) feet -- RobotModelHandler::addQuadFoot, tsid::contacts::Contact6d (kinodynamics-id.cpp:41-49, 163-167, 204-208):
   * force_size 6 and the four corners of every sole in its foot frame, quad_contact_points [nfeet][4][3] (getQuadFootContactPoints).  The QP then
   * holds the forces at the corners (12 per foot, foot frame), the 6-D LOCAL contact motion, a friction pyramid per corner and the bound on the
   * total normal force; force targets and reported contact forces are 6-D wrenches per foot (foot frame).  0 or 3: point feet. */
  int force_size;
  const double * quad_contact_points;
} smpc_id_settings;
typedef struct smpc_id_handle smpc_id_handle;
/* KinodynamicsID(model_handler, control_dt, settings): the default target is the reference state, every foot in contact with an equal
 * share of the weight (kinodynamics-id.cpp:96-112). */
int smpc_id_create(const smpc_robot_model * robot, const smpc_id_settings * settings, int batch, int device_id, smpc_id_handle ** out);
void smpc_id_destroy(smpc_id_handle * h);
/* setTarget(q, v, a, contact_state, f) (kinodynamics-id.cpp:120-183) of one instance, or of every instance (instance < 0):
 * q (nq), v (nv), a (nv), contact flag per foot, f (3 per foot, world frame; flat feet: the 6-D wrench per foot, foot frame -- wherever
 * this section says "3 per foot" / "3 nfeet" for a force, a flat-foot handle takes 6) */
int smpc_id_set_target(smpc_id_handle * h, int instance, const double * q, const double * v, const double * a, const uint8_t * contact, const double * f);
/* one target per robot of the batch: Q [B][nq], V [B][nv], A [B][nv], contact [B][nfeet], F [B][3 nfeet] */
int smpc_id_set_targets(smpc_id_handle * h, const double * Q, const double * V, const double * A, const uint8_t * contact, const double * F);
/* CentroidalID::setTarget(com_position, com_velocity, feet_pose_vec, feet_velocity_vec, contact_state_target, f_target)
 * (centroidal-id.cpp:86-147) of one instance or of every instance (instance < 0): com, vcom (3), feet_p, feet_v (3 per foot, world
 * frame: the translations / linear velocities of the reference's SE3 / Motion arguments), contact flag per foot, f (3 per foot).
 * SMPC_ERR_INVALID on a KinodynamicsID handle. */
int smpc_id_set_target_centroidal(smpc_id_handle * h, int instance, const double * com, const double * vcom, const double * feet_p,
                                  const double * feet_v, const uint8_t * contact, const double * f);
/* one target per robot: COM, VCOM [B][3], FEET_P, FEET_V [B][3 nfeet], contact [B][nfeet], F [B][3 nfeet] */
int smpc_id_set_targets_centroidal(smpc_id_handle * h, const double * COM, const double * VCOM, const double * FEET_P, const double * FEET_V,
                                   const uint8_t * contact, const double * F);
/* solve(t, q_meas, v_meas, tau) + getAccelerations for the batch (kinodynamics-id.cpp:185-237): X [B][nq + nv] (host) ->
 * tau [B][nv - 6], a [B][nv] (may be NULL), f [B][3 nfeet] contact forces of the solution (may be NULL), resid [B] the larger of the
 * QP's primal / dual residuals (may be NULL) */
int smpc_id_solve(smpc_id_handle * h, const double * X, double * tau, double * a, double * f, double * resid);
/* Same with the states resident in HBM: X_device [B][nq + nv]; asynchronous on the handle's stream (pair with smpc_id_wait).  tau_device
 * [B][nv - 6] may be NULL: the torques then stay in the handle's own buffer, smpc_id_get_tau_device. */
int smpc_id_solve_device(smpc_id_handle * h, const double * X_device, double * tau_device);
int smpc_id_wait(smpc_id_handle * h);
/* residuals of the last solve, resid [B] (the larger of the QP's primal / dual residuals; not finite: the solve of that robot failed,
 * its warm start was dropped and its next solve starts from scratch); joins the handle's stream */
int smpc_id_get_resid(smpc_id_handle * h, double * resid);
/* forget the warm start (ADMM iterate, step-size parameter) of one robot, or of every robot (instance < 0) */
int smpc_id_reset(smpc_id_handle * h, int instance);
const double * smpc_id_get_tau_device(smpc_id_handle * h);
/* the handle's own state buffer [B][nq + nv] in HBM (smpc_id_solve copies the host states there; a simulator may keep its states in it) */
double * smpc_id_get_x_device(smpc_id_handle * h);
/* The 1 kHz loop of the reference's examples (examples/go2_kinodynamics.py:264-300) without host round trips, for a kinodynamics MPC handle
 * and a KinodynamicsID handle of the same batch on the same device:
 *   smpc_id_set_targets_from_mpc  interpolateState / interpolateLinear of the MPC's solution at `delay` seconds after its last iterate
 *                                 (as smpc_interpolate, `knots` as there) written straight into the controller's target buffers; the
 *                                 contact flags are those of the MPC's stage 0.  Ordered after the MPC's work, before the next solve.
 *                                 A centroidal MPC handle feeds a CentroidalID handle the same way (examples/talos_centroidal.py:218-243):
 *                                 centre of mass, its velocity (momentum / mass), the foot references between stages 0 and 1 and
 *                                 their velocities, the interpolated forces.
 *   smpc_sim_step_device          one step of a simulated batch: constrained forward dynamics of the feet in contact (flags per foot;
 *                                 Baumgarte gains Kp, Kd [3], NULL = 0; ProximalSettings of record) under torques tau_device, then
 *                                 semi-implicit Euler over dt; X_device [B][nq + nv] is updated in place.  Asynchronous on the MPC
 *                                 handle's stream (smpc_wait joins).  Kinodynamics handles of the quadruped, and full-dynamics handles of
 *                                 either robot (their own contact model: Kp, Kd of force_size entries).
 * Round 4: the MPC handle of smpc_id_set_targets_from_mpc / smpc_id_share_stream may be of any kind -- the kinodynamics OCP of the biped
 * with flat feet and the full-dynamics OCPs feed a KinodynamicsID controller of the same robot (states, accelerations, contact forces /
 * wrenches of stage 0 .. 1 interpolated on the device). */
int smpc_id_set_targets_from_mpc(smpc_id_handle * id, smpc_handle * mpc, double delay, int knots);
/* From now on the controller issues its work on the MPC handle's stream (kinodynamics or centroidal handle; NULL: back to its own):
 * MPC step, targets, QP solves and simulator steps then form one in-order queue -- smpc_id_wait / smpc_wait are needed only before the
 * host reads a result, not between the legs of a tick.  The stream belongs to the MPC handle: go back (NULL) before that handle is
 * destroyed. */
int smpc_id_share_stream(smpc_id_handle * id, smpc_handle * mpc);
int smpc_sim_step_device(smpc_handle * h, double * X_device, const double * tau_device, const uint8_t * contact, const double * Kp, const double * Kd, double dt);
/* (tests) intermediate results of the last solve, padded layouts of simple-mpc_amd/csrc/smpc_id.h: what = 0 M, 1 nle, 2 J, 3 dJ v, 4 foot
 * velocities, 5 H [32][32], 6 g [32], 7 C [80][32], 8 l [80], 9 u [80], 10 centre of mass [3], 11 foot positions [3 nfeet], 12 torques [nv - 6]; every one [B][...] */
int smpc_id_debug_get(smpc_id_handle * h, int what, double * out);
/* Any robot table with 4 point feet (force_size 3) and 2 .. SMPC_MAX_JOINTS joints (simple-mpc_amd/csrc/smpc_id_rt.h): the reference takes
 * any pinocchio::Model in KinodynamicsID / CentroidalID (src/inverse-dynamics/kinodynamics-id.cpp:7-237, centroidal-id.cpp:6-147).
 * smpc_id_create keeps its two built shapes (13 joints / 4 point feet, 23 joints / 2 flat feet) on their templated kernels; every other
 * point-foot table is validated like the centroidal MPC's (SMPC_ERR_INVALID naming the field, nothing allocated) and served by kernels
 * that read the joint tree at run time.  Flat feet on any other tree are refused by smpc_id_create and served by smpc_id_create_any (below).
 *   smpc_id_get_dims        dims[10] = B, nq, nv, nfeet, force size of a target, n (variables), m (rows), n and m padded to 16, contact-
 *                           motion rows per foot: what the buffers of this section are sized by (kinodynamics-id.cpp:24-38 reads them
 *                           from the model)
 *   smpc_debug_id_force_rt  (tests) on != 0: handles created from now on for the built point-foot shape use the run-time kernels too;
 *                           returns the previous setting.  One process-wide atomic flag: a handle created by another thread while it is
 *                           set takes the run-time kernels as well.
 * The limit vectors of smpc_id_settings are raw pointers: the C ABI reads nv - 6 entries of each and cannot check their lengths; the
 * Python and C++ mirrors, which hold the containers, refuse a vector of another length before they call smpc_id_create_any. */
int smpc_id_get_dims(smpc_id_handle * h, int * dims);
int smpc_debug_id_force_rt(int on);
/* everything smpc_id_create accepts, served by the same engines and kernel symbols, plus: flat feet (force_size 6, 2 feet) on any validated
 * table with 2 .. SMPC_MAX_JOINTS joints, served by the run-time flat-foot engine (n = nv + 24 variables, m = n + 52 + nv - 6 rows; wrench
 * targets [2][6]).  A table it refuses: SMPC_ERR_INVALID naming the field (parent[5], njoints, "nfeet = 4 ... built for 2 flat feet"), nothing
 * allocated.  There are two entries because smpc_id_create's answer to flat feet on any other tree than the built one -- the refusal above -- is
 * pinned by existing callers and tests; the mirrors call this one.  Under smpc_debug_id_force_rt(1) this entry also sends the built flat-foot shape
 * (23 joints / 2 flat feet) through the run-time engine.  smpc_id_debug_get, what = 13: foot rotations [B][nfeet][9] (run-time flat-foot engine). */
int smpc_id_create_any(const smpc_robot_model * robot, const smpc_id_settings * settings, int batch, int device_id, smpc_id_handle ** out);

/* ---- batched rigid-body simulator for any robot table (simple-mpc_amd/csrc/smpc_sim_rt.h) ----
 * A stand-alone handle that carries a robot table and nothing else (no OCP, no MPC settings): the constrained forward dynamics of
 * smpc_full_forward_dynamics and the simulator step of smpc_sim_step_device for ANY validated table of smpc_robot.h, on a joint tree that
 * is read at run time.  One kernel launch per step (dynamics and integration together).
 *   smpc_robot_sim_create    force_size 3: point contacts (CONTACT_3D, LOCAL), 1 .. SMPC_MAX_FEET feet; force_size 6: flat contacts
 *                            (CONTACT_6D, LOCAL_WORLD_ALIGNED), 1 .. 2 feet, so that a robot has at most 12 contact rows; 2 <= njoints <=
 *                            SMPC_MAX_JOINTS, batch >= 1; gravity NULL = (0, 0, -9.81).  The table is validated like the centroidal MPC's.
 *                            Anything else: SMPC_ERR_INVALID with a message that names the field, *out = NULL, nothing allocated.  The
 *                            built-in tables are accepted and run the same kernel.
 *   smpc_robot_sim_get_dims  dims[5] = B, nq, nv, nfeet, force_size
 *   smpc_robot_sim_share_stream      as smpc_id_share_stream: from now on the simulator issues its work on the MPC handle's stream (NULL:
 *                            back to its own) -- MPC step, targets, QP solve and simulator step form one in-order queue.  The stream
 *                            belongs to the MPC handle: go back (NULL) before that handle is destroyed.
 *   smpc_robot_sim_forward_dynamics  host buffers, layouts and defaults of smpc_full_forward_dynamics: X [n][nq + nv], tau [n][nv - 6],
 *                            contact_mask [n] (bit per foot), Kp / Kd [force_size] (NULL = 0), ProximalSettings(1e-9, 1e-10, 10) for
 *                            arguments <= 0; a_out [n][nv], lambda_out [n][force_size nfeet] (forces ON the robot in the contact frame,
 *                            feet in contact first, the rest exactly 0), iters_out [n] (may be NULL).  n need not be B.
 *   smpc_robot_sim_step_device       constrained forward dynamics, then v <- v + a dt, q <- integrate(q, v dt) (semi-implicit Euler);
 *                            X_device [B][nq + nv] is updated in place, tau_device [B][nv - 6].  contact: nfeet flags on the host, the same
 *                            for every robot; mask_device [B] (device, bit per foot), when not NULL, overrides it with one mask per robot.
 *                            Asynchronous on the handle's stream (smpc_robot_sim_wait joins).  dt <= 0: SMPC_ERR_INVALID.
 *   smpc_robot_sim_get_last  accelerations [B][nv] and contact forces [B][force_size nfeet] of the last step (device pointers owned by the
 *                            handle, written by the step on its stream): logging without a second solve.
 *   smpc_robot_sim_read_last the same copied to host buffers a_out [B][nv], lambda_out [B][force_size nfeet] (either may be NULL); joins
 *                            the handle's stream. */
typedef struct smpc_robot_sim smpc_robot_sim;
int smpc_robot_sim_create(const smpc_robot_model * robot, int force_size, int batch, const double * gravity, int device_id, smpc_robot_sim ** out);
void smpc_robot_sim_destroy(smpc_robot_sim * sim);
int smpc_robot_sim_get_dims(smpc_robot_sim * sim, int * dims);
int smpc_robot_sim_wait(smpc_robot_sim * sim);
void * smpc_robot_sim_get_stream(smpc_robot_sim * sim);
int smpc_robot_sim_share_stream(smpc_robot_sim * sim, smpc_handle * mpc);
int smpc_robot_sim_forward_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, const unsigned * contact_mask, const double * Kp,
                                    const double * Kd, double prox_accuracy, double prox_mu, int prox_max_iter, double * a_out, double * lambda_out,
                                    int * iters_out);
int smpc_robot_sim_step_device(smpc_robot_sim * sim, double * X_device, const double * tau_device, const uint8_t * contact, const uint32_t * mask_device,
                               const double * Kp, const double * Kd, double dt);
int smpc_robot_sim_get_last(smpc_robot_sim * sim, double ** a_device, double ** lambda_device);
int smpc_robot_sim_read_last(smpc_robot_sim * sim, double * a_out, double * lambda_out);

/* ---- ground plane with unilateral frictional contact for the simulator above (simple-mpc_amd/csrc/smpc_sim_ground_rt.h) ----
 * smpc_robot_sim_step_device applies the BILATERAL contacts its caller names; the entries below put the robot on a plane z = ground_z with
 * unilateral contact and Coulomb friction DETECTED FROM THE STATE: no mask.  Every foot carries points_per_foot contact points (offsets
 * in the foot frame, the same for every foot), numbered c = foot * points_per_foot + k; every point is always a row block [x y z] of a
 * velocity-level complementarity problem that `sweeps` sweeps of projected Gauss-Seidel solve from lambda = 0 (no early exit), one kernel
 * launch per step.  Independent of the handle's force_size.  A handle that never calls smpc_robot_sim_set_ground behaves as before.
 *   smpc_ground_settings     ground_z; mu (friction coefficient); erp (share of a penetration removed per step); compliance (added to the
 *                            diagonal of the Delassus matrix); sweeps; points_per_foot (1 .. 4); points[k][3].  An argument that is 0
 *                            stands for its default: mu 0.7, erp 0.2, compliance 1e-8, sweeps 30, points_per_foot 1 with the point at
 *                            the foot frame's origin (a frictionless or erp-free plane is a tiny positive value).
 *   smpc_robot_sim_set_ground        stores the settings and (re)allocates the force and contact-word buffers; may be called again with
 *                            other settings (another points_per_foot resizes the buffers); joins the handle's stream first.  Refused
 *                            with SMPC_ERR_INVALID and a message that names the field, before anything is allocated and with the
 *                            previous settings kept: a number that is not finite, mu < 0, erp outside [0, 1], compliance < 0,
 *                            sweeps < 0, points_per_foot outside [0, 4], nfeet * points_per_foot > 8 (the message names the product).
 *   smpc_robot_sim_get_ground_dims   dims[2] = points_per_foot, contact points per robot (nfeet points_per_foot); 0, 0 before set_ground
 *   smpc_robot_sim_step_ground_device   one step of the batch: X_device [B][nq + nv] updated in place, tau_device [B][nv - 6].
 *                            Asynchronous on the handle's stream.  dt <= 0, or a call before smpc_robot_sim_set_ground: SMPC_ERR_INVALID
 *                            with a message.  Writes the accelerations a = M^-1 (S tau - h + J^T lambda) that smpc_robot_sim_get_last
 *                            returns, the forces and the contact words.
 *   smpc_robot_sim_ground_dynamics   the same solve on host buffers X [n][nq + nv], tau [n][nv - 6] (n need not be B); the state is not
 *                            advanced.  v_next_out [n][nv], a_out [n][nv], lambda_out [n][3 points] (forces ON the robot in world axes,
 *                            [point][x y z]), gap_out [n][points] (height of every point above the plane), contact_out [n] (bit c: the
 *                            normal force of point c is positive); any output may be NULL.
 *   smpc_robot_sim_get_ground_last   forces [B][3 points] and contact words [B] of the last ground step (device pointers owned by the
 *                            handle; they change when smpc_robot_sim_set_ground is called again)
 *   smpc_robot_sim_read_ground_last  the same copied to host buffers (either may be NULL); joins the handle's stream. */
typedef struct smpc_ground_settings
{
  double ground_z, mu, erp, compliance;
  int sweeps, points_per_foot;
  double points[4][3];
} smpc_ground_settings;
int smpc_robot_sim_set_ground(smpc_robot_sim * sim, const smpc_ground_settings * settings);
int smpc_robot_sim_get_ground_dims(smpc_robot_sim * sim, int * dims);
int smpc_robot_sim_step_ground_device(smpc_robot_sim * sim, double * X_device, const double * tau_device, double dt);
int smpc_robot_sim_ground_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, double * v_next_out, double * a_out,
                                   double * lambda_out, double * gap_out, uint32_t * contact_out);
int smpc_robot_sim_get_ground_last(smpc_robot_sim * sim, double ** lambda_device, uint32_t ** contact_device);
int smpc_robot_sim_read_ground_last(smpc_robot_sim * sim, double * lambda_out, uint32_t * contact_out);

/* ---- per-robot slopes, friction and pushes on that ground (simple-mpc_amd/csrc/smpc_sim_ground_env_rt.h) ----
 * After smpc_robot_sim_set_ground every robot stands on the plane z = ground_z with the settings' mu and nothing but its joint torques acts
 * on it.  The entries below give robot i its own plane, plane[i] = (n, d): the ground is {p : n . p = d} with n a unit normal in world
 * axes; its own friction coefficient mu[i]; and one external force, push[i] = (f, o): f (world axes, N) acts on the body of joint
 * push_joint (one index per handle, 0 = the base) at the point o given in that joint's frame.  The contact problem lives in the frame
 * Rc = [t1 t2 n], t1 = (e_y x n) / |e_y x n|, t2 = n x t1 (the identity for n = e_z); forces are still reported in world axes.  A quantity
 * left unset takes the handle's setting for every robot: (0, 0, 1, ground_z), the settings' mu, no push.  Each entry validates before it
 * allocates, answers SMPC_ERR_INVALID with a message that names the field and the robot, and leaves the previous environment in force; each
 * needs smpc_robot_sim_set_ground first.
 *   smpc_robot_sim_set_ground_env    host arrays plane [B][4] and mu [B]; either may be NULL for "uniform" (a call replaces both: a NULL
 *                            array drops what an earlier call had set for it).  Admitted: every number finite, | |n| - 1 | <= 1e-9,
 *                            n.z >= 0.5, mu > 0.  Copies into device buffers owned by the handle; joins the handle's stream first.
 *   smpc_robot_sim_set_ground_push   push_joint in 0 .. njoints - 1 and a host array push [B][6] of finite numbers; NULL clears the push.
 *   smpc_robot_sim_get_ground_push   the device pointer of the handle-owned push buffer [B][6] (NULL while no push is set): a resident loop
 *                            may rewrite the pushes on the shared stream without the host.  Values written there are not validated; a
 *                            value that is not finite spoils the robot it belongs to and no other.  The pointer stays valid until
 *                            the push is cleared, smpc_robot_sim_set_ground is called or the handle is destroyed.
 *   smpc_robot_sim_step_ground_device  (above) is unchanged: on a handle on which neither setter has been called it runs the kernel of the
 *                            uniform ground exactly as before, afterwards the kernel that reads the per-robot values.
 *                            smpc_robot_sim_get_ground_last / _read_ground_last and smpc_robot_sim_get_last serve both.
 *   smpc_robot_sim_set_ground        (above) called afterwards DROPS the per-robot environment and the push: both revert to uniform / none.
 *   smpc_robot_sim_ground_env_dynamics  the solve of smpc_robot_sim_ground_dynamics on n host states with explicit plane [n][4], mu [n],
 *                            push [n][6] (any may be NULL: the handle's setting, whatever the setters have stored) and push_joint; n need
 *                            not be B, nothing is advanced, and the handle's environment is neither read nor changed.  Outputs as
 *                            smpc_robot_sim_ground_dynamics: lambda_out in world axes, gap_out = n . p - d, any output may be NULL. */
int smpc_robot_sim_set_ground_env(smpc_robot_sim * sim, const double * plane, const double * mu);
int smpc_robot_sim_set_ground_push(smpc_robot_sim * sim, int push_joint, const double * push);
int smpc_robot_sim_get_ground_push(smpc_robot_sim * sim, double ** push_device);
int smpc_robot_sim_ground_env_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                       const double * push, int push_joint, double * v_next_out, double * a_out, double * lambda_out, double * gap_out,
                                       uint32_t * contact_out);

/* ---- warm-started contact solve with a stopping rule on that ground (simple-mpc_amd/csrc/smpc_sim_ground_ws_rt.h) ----
 * After smpc_robot_sim_set_ground every robot runs exactly `sweeps` sweeps of projected Gauss-Seidel from lambda = 0.  The entries below let
 * robot i start from its own forces of the previous step, stop when a sweep has stopped moving them, and report how far it got.
 *   start    lambda0_r = w[i][r] if warm_start is set and w[i][r] is finite, else 0.  w is the handle-owned warm buffer [B][3 points], laid out
 *            IN THE CONTACT FRAME, [point][t1 t2 n], so a slope needs no rotation; an entry that is not finite reads as 0.
 *   sweeps   s = 1 .. sweeps as before; sweep s also yields rho_s = max_r |lambda_r(new) - lambda_r(old)| dt G_rr (m/s) over the robot's rows,
 *            `old` the row's value before the sweep touches it, `new` the value written (after the projection for tangential rows).
 *   stop     after sweep s if tol > 0, s >= min_sweeps and rho_s <= tol.  tol = 0: exactly `sweeps` sweeps.  A NaN rho never stops.
 *   outputs  per robot sweeps_used (int32) and residual (rho of the last sweep run); on a step, w[i] <- lambda in the contact frame.
 * Each entry needs smpc_robot_sim_set_ground first, validates before it allocates, answers SMPC_ERR_INVALID with a message that names the
 * field and leaves the previous settings in force.
 *   smpc_robot_sim_set_ground_solver   warm_start 0 / 1; tol >= 0 finite; min_sweeps in 1 .. sweeps of the ground (0 stands for 1).  Zeroes
 *                            the warm buffer; joins the handle's stream first.  From this call on smpc_robot_sim_step_ground_device
 *                            launches sim_ground_ws_rt_body, which reads the per-robot environment and push if they are set.  With
 *                            {0, 0, 0} the results equal those of the kernels above bit for bit.
 *   smpc_robot_sim_set_ground          (above) called afterwards DROPS the solver settings and the warm buffer, as it drops the environment.
 *   smpc_robot_sim_reset_ground_warm_start   zeroes the warm rows of the n robots of a host list (unsorted, duplicates allowed; an index
 *                            outside 0 .. B - 1 refuses the whole call); n = 0 resets every robot.  Asynchronous on the handle's stream.
 *   smpc_robot_sim_reset_ground_warm_start_device   the same for every robot with a non-zero byte in mask_device [B] (device memory), one
 *                            kernel on the handle's stream, no host round trip.  body_touch of smpc_robot_sim_get_body_points_last
 *                            (uint8_t [B], written by the ground step itself) is a mask in this layout: the fall detector on the device.
 *   smpc_robot_sim_get_ground_solver_last  device pointers of sweeps_used [B], residual [B] and the warm buffer [B][3 points] (owned by the
 *                            handle; they change when smpc_robot_sim_set_ground is called again; NULL before the setter or the first
 *                            smpc_robot_sim_ground_solve_dynamics: a getter allocates nothing); any output may be NULL.
 *   smpc_robot_sim_read_ground_solver_last  sweeps_used and residual of the last ground step copied to host buffers (either may be NULL);
 *                            joins the handle's stream.  Zeros before the first step after the setter (before the setter without
 *                            touching the device).  The resets are no-ops that succeed while there is no warm buffer.
 *   smpc_robot_sim_ground_solve_dynamics  smpc_robot_sim_ground_env_dynamics with explicit solver settings (NULL: {0, 0, 0}) and an
 *                            explicit start vector lambda0 [n][3 points] in the contact frame (NULL: zeros; read only if
 *                            settings->warm_start is set).  Further outputs lambda_contact_out [n][3 points] (contact frame),
 *                            sweeps_out [n], residual_out [n]; any output may be NULL.  The handle's settings and warm buffer are neither
 *                            read nor changed. */
typedef struct smpc_ground_solver_settings
{
  int warm_start;
  double tol;
  int min_sweeps;
} smpc_ground_solver_settings;
int smpc_robot_sim_set_ground_solver(smpc_robot_sim * sim, const smpc_ground_solver_settings * settings);
int smpc_robot_sim_reset_ground_warm_start(smpc_robot_sim * sim, const int * indices, int n);
int smpc_robot_sim_reset_ground_warm_start_device(smpc_robot_sim * sim, const uint8_t * mask_device);
int smpc_robot_sim_get_ground_solver_last(smpc_robot_sim * sim, int32_t ** sweeps_device, double ** residual_device, double ** warm_device);
int smpc_robot_sim_read_ground_solver_last(smpc_robot_sim * sim, int32_t * sweeps_out, double * residual_out);
int smpc_robot_sim_ground_solve_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                         const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                         double * v_next_out, double * a_out, double * lambda_out, double * lambda_contact_out, double * gap_out,
                                         uint32_t * contact_out, int32_t * sweeps_out, double * residual_out);

/* ---- effort limits, joint damping, armature and joint-limit stops on that ground (simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h,
 * DESIGN 3.26) ----
 * A handle that has a ground gets a JOINT MODEL: five per-robot arrays [B][na], na = nv - 6, k the index of an actuated dof, and a few
 * scalars.  tau_max >= 0 (+inf allowed); damping d >= 0 finite; armature r_a >= 0 finite; q_lo <= q_hi (-inf / +inf allowed).  stops is 0
 * or 1; activation (rad) > 0, 0 stands for 0.1; stop_erp in [0, 1], 0 stands for 0.2.  A null array pointer means tau_max = +inf, d = 0,
 * r_a = 0, limits from the robot table; per_robot says whether the given arrays are [na] (broadcast over the batch) or [B][na].
 * One step of robot i (everything not named is as in DESIGN 3.23 - 3.25):
 *   1 effort limit   tc_k = tau_k > tmax_k ? tmax_k : (tau_k < -tmax_k ? -tmax_k : tau_k), so a NaN passes through; tc is an output
 *                    (tau_applied).
 *   2 implicit damping and armature   Mh = M + diag(0_6, r_a + dt d); b = S tc - h - [0_6; d o v_joint] + Q_push; W = Mh^-1 [b | J^T];
 *                    v_f = v + dt W_0; G, c0, v+ = v_f + dt W_1 lambda and a = W_0 + W_1 lambda as before, with Mh in place of M.
 *   3 stop rows      only when stops = 1, in ascending k.  g- = q_k - q_lo_k, g+ = q_hi_k - q_k.  Joint k is a candidate iff
 *                    min(g-, g+) < activation; its side is lower (s = +1, g = g-) if g- <= g+, otherwise upper (s = -1, g = g+).  The
 *                    first NJ = 8 candidates get rows, appended after the contact rows; the rest are counted in `dropped`.  Row r of a
 *                    stop has J_r = s e_{6+k}; it shares W, G = J W_1 + compliance I and the sweeps' sums with the contact rows, so a stop
 *                    and a foot see each other.  c0_r = s v_f[6+k] + (g >= 0 ? g / dt : stop_erp g / dt).
 *   4 sweeps         each sweep runs the contact points of 3.23 in their order, their row sums over all rows, then the stop rows in
 *                    ascending order: lambda_r <- max(0, lambda_r - (c0_r + dt sum_j G_rj lambda_j) / (dt G_rr)).  Stop rows start from
 *                    exactly 0 every step; the warm buffer keeps its layout (contact rows only); rho_s takes the maximum over stop rows
 *                    too; the stopping rule, min_sweeps and the kernel's 1 / (dt G_rr) deviation are unchanged.
 *   5 outputs        per robot, besides those of 3.25: tau_applied [na]; stop_rows [8] (int32: +(k+1) lower, -(k+1) upper, 0 unused);
 *                    lam_stop [8]; dropped (int32).
 * Each entry needs smpc_robot_sim_set_ground first, validates before it allocates, answers SMPC_ERR_INVALID with a message that names the
 * field and the first offending index, and leaves the previous model in force.
 *   smpc_robot_sim_set_joint_model   stores the model (host arrays, copied).  From this call on smpc_robot_sim_step_ground_device launches
 *                            sim_ground_joint_rt_body, which honours the per-robot environment, the push and the solver settings if they
 *                            are set.  With tau_max = +inf, d = r_a = 0 and stops = 0 the results equal those of the kernels above bit
 *                            for bit.  Joins the handle's stream first.
 *   smpc_robot_sim_set_ground        (above) called afterwards DROPS the joint model, as it drops the environment and the solver settings.
 *   smpc_robot_sim_get_joint_last    device pointers of tau_applied [B][na], stop_rows [B][8], lam_stop [B][8], dropped [B] (owned by the
 *                            handle; NULL before the setter: a getter allocates nothing); any output may be NULL.
 *   smpc_robot_sim_read_joint_last   the same copied to host buffers (any may be NULL); joins the handle's stream.  Zeros before the setter,
 *                            without touching the device.
 *   smpc_robot_sim_ground_joint_dynamics   smpc_robot_sim_ground_solve_dynamics with an explicit joint model (arrays [na], or [n][na] with
 *                            per_robot; NULL model: the inert one) and the four further outputs; any output may be NULL.  The handle's
 *                            model, settings and buffers are neither read nor changed. */
#define SMPC_JOINT_MAX_STOPS 8
typedef struct smpc_joint_model_settings
{
  const double * tau_max;
  const double * damping;
  const double * armature;
  const double * q_lo;
  const double * q_hi;
  int per_robot;
  int stops;
  double activation;
  double stop_erp;
} smpc_joint_model_settings;
int smpc_robot_sim_set_joint_model(smpc_robot_sim * sim, const smpc_joint_model_settings * model);
int smpc_robot_sim_get_joint_last(smpc_robot_sim * sim, double ** tau_applied_device, int32_t ** stop_rows_device, double ** lam_stop_device,
                                  int32_t ** dropped_device);
int smpc_robot_sim_read_joint_last(smpc_robot_sim * sim, double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out);
int smpc_robot_sim_ground_joint_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                         const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                         const smpc_joint_model_settings * model, double * v_next_out, double * a_out, double * lambda_out,
                                         double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out, double * residual_out,
                                         double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out);

/* ---- per-robot link masses, centres of mass and inertias on that ground (simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h:
 * sim_ground_body_rt_body) ----
 * A handle that has a ground gets optional BODY PARAMETERS: body [B][njoints][10] doubles, njoints the robot's own joint count (nq - 6,
 * the free-flyer included).  Row j of robot i is [mass, com_x, com_y, com_z, Ixx, Ixy, Iyy, Ixz, Iyz, Izz]: order and meaning of mass[j],
 * com[j], inertia[j] of smpc_robot.h (com in the joint frame, inertia about the body's CoM in the joint frame).  A row is admitted exactly
 * when a robot table carrying it would be: mass finite and > 0, com finite, inertia finite.
 * When body parameters are set, robot i's ground step uses row [i][j] wherever the kernels use the table's mass[j], com[j], inertia[j]:
 * the spatial inertia of body j, hence M, h and everything computed from them.  Nothing else of the model changes: tree, placements,
 * feet, the contact model of DESIGN 3.23 - 3.25 and the joint model of 3.26 stay as written.  A step with the rows of a table equals, bit
 * for bit, the step of a handle created from that table.  The MPC and the inverse-dynamics controllers keep the table they were created
 * with.  The free-flight entries (smpc_robot_sim_step_device, smpc_robot_sim_forward_dynamics) do not read body parameters.
 * Each entry validates before it allocates, answers SMPC_ERR_INVALID with a message that names the field and the first offending
 * [robot][joint], and leaves the previous parameters in force.
 *   smpc_robot_sim_set_body_params    stores body [B][njoints][10] (host, copied); NULL clears.  Needs smpc_robot_sim_set_ground first;
 *                            smpc_robot_sim_set_ground called afterwards DROPS the parameters.  Independent of
 *                            smpc_robot_sim_set_joint_model, in either order.  While they are set smpc_robot_sim_step_ground_device launches
 *                            sim_ground_body_rt_body with the handle's joint model, or with the inert one if it has none; once cleared, the
 *                            handle launches exactly what it launched before.  Joins the handle's stream first.
 *   smpc_robot_sim_read_body_params   a host copy [B][njoints][10]; the table's rows repeated B times while nothing is set.
 *   smpc_robot_sim_get_body_params    the handle-owned device pointer, NULL while unset.  A resident loop may rewrite the array on the shared
 *                            stream; values written there are NOT validated (a non-finite value gives NaNs in that robot's outputs).
 *   smpc_robot_sim_ground_body_dynamics   smpc_robot_sim_ground_joint_dynamics plus body [n][njoints][10] (NULL: the table's).  The handle's
 *                            own parameters are neither read nor changed, and n need not be the batch. */
int smpc_robot_sim_set_body_params(smpc_robot_sim * sim, const double * body);
int smpc_robot_sim_read_body_params(smpc_robot_sim * sim, double * body_out);
int smpc_robot_sim_get_body_params(smpc_robot_sim * sim, double ** body_device);
int smpc_robot_sim_ground_body_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                        const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                        const smpc_joint_model_settings * model, const double * body, double * v_next_out, double * a_out,
                                        double * lambda_out, double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out,
                                        double * residual_out, double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out,
                                        int32_t * dropped_out);

/* ---- per-robot height-field terrain under that ground (simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h: sim_ground_terrain_rt_body,
 * DESIGN 3.28) ----
 * Settings.  A terrain of a handle that has a ground: heights[T][ny][nx] doubles are world z at the grid nodes, row j along world y,
 * column i along world x.  cell > 0 is the node spacing in metres, the same in x and y.  tile[B] (int32) says which of the T tiles robot i
 * stands on; null means 0.  origin[B][2] is the world (x, y) of node (0, 0) of robot i's tile; null means (0, 0).  Tiles are shared: a
 * thousand robots may stand on the same tile at different origins.
 * Admission (host only, smpc_sim_terrain_dims.h; it answers before anything is allocated, names the field and the first offending index,
 * and leaves the previous terrain in force): nx, ny >= 2 and T >= 1; T ny nx <= 4 194 304 nodes; every height is finite; cell is finite
 * and positive; tile lies in [0, T); origin is finite; at each of the four corners of every cell hx^2 + hy^2 <= 3, which is the rule
 * n.z >= 0.5 of DESIGN 3.24 (the gradient of a bilinear patch is extremal at its corners).
 * Sampling.  For contact point c at p = p_c:
 *   1 x = (p.x - o.x) / cell, clamped to [0, nx - 1]; i = min(floor(x), nx - 2), u = x - i.  The same in y gives j and v.
 *   2 The clamping is done in double before any conversion to an integer; the selects are written so that a NaN or +-inf coordinate
 *     yields index 0.  The tile index is clamped to [0, T - 1] in the kernel as well.  No value read from memory can index outside the
 *     array.
 *   3 With h00 = H[j][i], h10 = H[j][i+1], h01 = H[j+1][i], h11 = H[j+1][i+1]: dx0 = h10 - h00, dx1 = h11 - h01, dy0 = h01 - h00;
 *     h0 = h00 + u dx0, h1 = h01 + u dx1, h = h0 + v (h1 - h0); hx = (dx0 + v (dx1 - dx0)) / cell, hy = (dy0 + u ((h11 - h10) - dy0)) / cell.
 *   4 s = 1 / sqrt(hx hx + hy hy + 1), n_c = ((0 - hx) s, (0 - hy) s, s).
 *   5 The frame t1, t2 of point c comes from n_c by the formula of DESIGN 3.24.
 *   6 The gap is phi_c = n_c.z (p.z - h): the distance to the tangent plane of the terrain below the point.
 * This order of operations is chosen so that a tile whose heights all equal ground_z gives n = (0, 0, 1), h = ground_z and the frame of
 * the flat plane exactly.
 * The step is the step of DESIGN 3.23 - 3.27 with n_c, t1_c, t2_c, phi_c in place of the robot's n, t1, t2, phi: in the rows of point c,
 * in c0, and in lambda_world(c) = Rc_c lambda_c.  Unchanged: the sweep, erp, compliance, the per-robot mu and push of
 * smpc_robot_sim_set_ground_env / smpc_robot_sim_set_push, the solver settings, the joint model, the stop rows and the body parameters.
 * WHILE A TERRAIN IS SET THE `planes` OF smpc_robot_sim_set_ground_env ARE NOT READ.  The warm buffer stays "in the point's own contact
 * frame", which now moves with the foot.  Vertical faces, contacts other than at the foot points and the free-flight entries do not know
 * the terrain.
 *   smpc_robot_sim_set_terrain   stores the settings (host arrays, copied); NULL clears.  Needs smpc_robot_sim_set_ground first;
 *                            smpc_robot_sim_set_ground called afterwards DROPS the terrain.  Independent of smpc_robot_sim_set_joint_model,
 *                            smpc_robot_sim_set_body_params and smpc_robot_sim_set_ground_solver, in any order.  While it is set
 *                            smpc_robot_sim_step_ground_device launches sim_ground_terrain_rt_body with the handle's joint model and body
 *                            parameters, or with the inert model and the table's bodies where those are unset; once cleared, the handle
 *                            launches exactly what it launched before.  Joins the handle's stream first.
 *   smpc_robot_sim_get_terrain   the handle-owned device pointers heights [T][ny][nx], tile [B], origin [B][2] and the dims (NULL / 0
 *                            while unset).  A resident loop may rewrite the arrays on the shared stream, unvalidated: the clamps above keep
 *                            every index inside the array whatever is written.
 *   smpc_robot_sim_read_terrain_last / smpc_robot_sim_get_terrain_last   normals [B][points][3] and heights [B][points] of the last step
 *                            (n_c and h of every contact point; zeros before the first step), as a host copy / as device pointers.
 *   smpc_robot_sim_ground_terrain_dynamics   smpc_robot_sim_ground_body_dynamics with the terrain settings in place of `plane`
 *                            (tile [n] and origin [n][2] here; `terrain` must not be NULL) and the two new outputs normals_out
 *                            [n][points][3] and heights_out [n][points].  The handle's own terrain is neither read nor changed. */
typedef struct smpc_terrain_settings
{
  int32_t nx, ny, tiles;
  double cell;
  const double * heights; /* [tiles][ny][nx] */
  const int32_t * tile;   /* [B] (or [n]), NULL: 0 */
  const double * origin;  /* [B][2] (or [n][2]), NULL: (0, 0) */
} smpc_terrain_settings;
int smpc_robot_sim_set_terrain(smpc_robot_sim * sim, const smpc_terrain_settings * terrain);
int smpc_robot_sim_get_terrain(smpc_robot_sim * sim, double ** heights_device, int32_t ** tile_device, double ** origin_device, int32_t * nx, int32_t * ny,
                               int32_t * tiles, double * cell);
int smpc_robot_sim_read_terrain_last(smpc_robot_sim * sim, double * normals_out, double * heights_out);
int smpc_robot_sim_get_terrain_last(smpc_robot_sim * sim, double ** normals_device, double ** heights_device);
int smpc_robot_sim_ground_terrain_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const smpc_terrain_settings * terrain,
                                           const double * mu, const double * push, int push_joint, const smpc_ground_solver_settings * settings,
                                           const double * lambda0, const smpc_joint_model_settings * model, const double * body, double * v_next_out,
                                           double * a_out, double * lambda_out, double * lambda_contact_out, double * gap_out, uint32_t * contact_out,
                                           int32_t * sweeps_out, double * residual_out, double * tau_applied_out, int32_t * stop_rows_out,
                                           double * lam_stop_out, int32_t * dropped_out, double * normals_out, double * heights_out);

/* ---- body points: contact candidates on any link, and the touch mask (simple-mpc_amd/csrc/smpc_sim_ground_joint_rt.h:
 * sim_ground_points_rt_body / sim_ground_points_terrain_rt_body) ----
 * Settings.  A handle that has a ground gets BODY POINTS, shared by the batch: n in [0, 16] entries, joint[k] in [0, nj), offset[k][3]
 *   (metres, in the frame of that joint), and band >= 0 (metres; 0 stands for 0.02).  n = 0 or a null pointer clears them.
 * Slots.  The family's bound of 8 contact points (24 contact rows) per robot stays.  S = 8 - nfeet * points_per_foot slots are free beside
 *   the foot points.  S = 0 is refused.
 * One step of robot i (everything not named is as in DESIGN 3.23 - 3.28):
 *   1 position    p_k = p_j + R_j o_k with j = joint[k], from the tree walk that places the feet.
 *   2 gap         phi_k is the gap of a foot point at p_k.  Without a terrain: n . p_k - d with the robot's plane (setGroundEnv, else
 *                 ground_z).  With a terrain: steps 1 - 6 of 3.28 at p_k, which also give the point its own n_k, t1_k, t2_k and h_k.
 *   3 candidates  in ascending k: k is a candidate iff phi_k < band (so a NaN gap is none).  The first S candidates get the slots
 *                 s = 0, 1, ... in that order; the others are counted in body_dropped.
 *   4 rows        slot s is contact point c = nfeet P + s: three rows [t1 t2 n], exactly those of a foot point, at p_k, over the ancestors of
 *                 joint[k], in the point's frame (the robot's plane frame, or its own on a terrain).  c0 gets phi_k / dt (phi_k >= 0) or
 *                 erp phi_k / dt on the normal row.  The compliance and the robot's mu are the same.  The stop rows of 3.26 follow behind
 *                 the last slot in use.
 *   5 sweeps      each sweep runs the foot points in their order, then the slots in ascending s (normal row, the two tangential rows,
 *                 projection onto the disc of radius mu lambda_n: the update of a foot point), then the stop rows.  Slot rows start from
 *                 exactly 0 every step.  The warm buffer keeps its layout (foot rows only).  rho takes the slot rows too.  The stopping
 *                 rule, min_sweeps and the kernel's 1 / (dt G_rr) deviation are unchanged.
 *   6 outputs     per robot, besides those of 3.28 with their layouts unchanged:
 *                   body_slots [8] int32     k + 1 of the candidate in slot s, 0 = unused
 *                   lam_body [8][3]          forces ON the robot in world axes, 0 for unused slots
 *                   body_gap [16]            phi_k for k < n, 0 beyond
 *                   body_dropped             int32
 *                   body_touch               uint8: 1 iff lambda_n > 0 in some slot, else 0
 *                 Bit nfeet P + s of the contact word is the slot's lambda_n > 0.
 *                 lastTerrainNormals / lastTerrainHeights keep the foot points only.
 * With n = 0, or with every phi_k >= band, every added term is an exact zero and the shared outputs equal those of the kernel the handle
 * launched before, bit for bit.
 * Admission (host only, smpc_sim_points_dims.h; it answers before anything is allocated, names the field and the first offending index, and
 * leaves the previous points in force).  A handle with body points always launches a 32-row kernel.  Not modelled: radii on the points, a
 * friction coefficient of their own, more than 8 contact points per robot; the free-flight entries do not know the points.
 *   smpc_robot_sim_set_body_points   stores the settings (copied); NULL or n = 0 clears, and the handle then launches exactly what it
 *                            launched before.  Needs smpc_robot_sim_set_ground first; smpc_robot_sim_set_ground called afterwards DROPS
 *                            the points.  Independent of the terrain, the joint model, the body parameters, the environment, the push and
 *                            the solver settings, in any order.  Joins the handle's stream first.
 *   smpc_robot_sim_get_body_points_last / smpc_robot_sim_read_body_points_last   the five outputs of the last step as device pointers
 *                            (NULL while no points are set) / as host copies (joins the stream; zeros while no points are set):
 *                            body_slots [B][8], lam_body [B][8][3], body_gap [B][16], body_dropped [B], body_touch [B].  body_touch is
 *                            uint8_t [B], the mask layout smpc_reset_instances_device and smpc_robot_sim_reset_ground_warm_start_device
 *                            read: handed to them on the shared stream it resets the robots that touched down, nothing crossing the host.
 *   smpc_robot_sim_ground_points_dynamics   smpc_robot_sim_ground_terrain_dynamics with the points settings and the five outputs
 *                            ([n] in place of [B]).  A NULL terrain means the plane (`plane` [n][4] or NULL as in
 *                            smpc_robot_sim_ground_body_dynamics; not read with a terrain); normals_out / heights_out are written only
 *                            with a terrain.  It neither reads nor changes the handle's points. */
typedef struct smpc_body_points_settings
{
  int32_t n;
  int32_t joint[16];
  double offset[16][3];
  double band;
} smpc_body_points_settings;
int smpc_robot_sim_set_body_points(smpc_robot_sim * sim, const smpc_body_points_settings * points);
int smpc_robot_sim_get_body_points_last(smpc_robot_sim * sim, int32_t ** body_slots_device, double ** lam_body_device, double ** body_gap_device,
                                        int32_t ** body_dropped_device, uint8_t ** body_touch_device);
int smpc_robot_sim_read_body_points_last(smpc_robot_sim * sim, int32_t * body_slots_out, double * lam_body_out, double * body_gap_out,
                                         int32_t * body_dropped_out, uint8_t * body_touch_out);
int smpc_robot_sim_ground_points_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const smpc_terrain_settings * terrain,
                                          const double * plane, const double * mu, const double * push, int push_joint,
                                          const smpc_ground_solver_settings * settings, const double * lambda0, const smpc_joint_model_settings * model,
                                          const double * body, const smpc_body_points_settings * points, double * v_next_out, double * a_out,
                                          double * lambda_out, double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out,
                                          double * residual_out, double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out,
                                          int32_t * dropped_out, double * normals_out, double * heights_out, int32_t * body_slots_out,
                                          double * lam_body_out, double * body_gap_out, int32_t * body_dropped_out, uint8_t * body_touch_out);

#ifdef __cplusplus
}
#endif
#endif
