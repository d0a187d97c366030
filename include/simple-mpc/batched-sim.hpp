// simple-mpc/batched-sim.hpp -- header-only C++ host mirror of the batched rigid-body simulator over the C ABI of smpc.h
// (smpc_robot_sim_*): the constrained forward dynamics the reference's FullDynamicsOCP obtains from pinocchio::constraintDynamics
// (src/fulldynamics.cpp:39,50-75,139) and a semi-implicit Euler step, for any validated robot table, `batch` robots per launch.  The handle
// carries the robot and nothing else.  Eigen types replaced by std::vector<double>; errors are rethrown as std::runtime_error.
#pragma once
#include "../smpc.h"
#include "batched-mpc.hpp"
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace simple_mpc
{
  class BatchedRobotSim
  {
  public:
    // force_size 3: point contacts (LOCAL frame), 1 .. 4 feet; 6: flat contacts (LOCAL_WORLD_ALIGNED), 1 .. 2 feet.  gravity: empty = (0, 0, -9.81)
    BatchedRobotSim(const smpc_robot_model * robot, int force_size, int batch, const std::vector<double> & gravity = {}, int device_id = 0)
    {
      if (!gravity.empty() && gravity.size() != 3)
        throw std::runtime_error("gravity: 3 entries expected");
      check(smpc_robot_sim_create(robot, force_size, batch, gravity.empty() ? nullptr : gravity.data(), device_id, &h_));
      int d[5];
      check(smpc_robot_sim_get_dims(h_, d));
      batch_ = d[0];
      nq_ = d[1];
      nv_ = d[2];
      nf_ = d[3];
      fs_ = d[4];
    }
    ~BatchedRobotSim()
    {
      if (h_)
        smpc_robot_sim_destroy(h_);
    }
    BatchedRobotSim(const BatchedRobotSim &) = delete;
    BatchedRobotSim & operator=(const BatchedRobotSim &) = delete;
    int batch() const { return batch_; }
    int nq() const { return nq_; }
    int nv() const { return nv_; }
    int nfeet() const { return nf_; }
    int force_size() const { return fs_; }

    // X [n][nq + nv], tau [n][nv - 6], contact_mask [n] (bit per foot), Kp / Kd: force_size entries or empty (= 0) ->
    // a [n][nv], lambda [n][force_size nfeet] (feet in contact first, the rest 0), iters [n]; n need not be the batch
    void forwardDynamics(const std::vector<double> & X, const std::vector<double> & tau, const std::vector<unsigned> & contact_mask, const std::vector<double> & Kp,
                         const std::vector<double> & Kd, std::vector<double> & a, std::vector<double> & lambda, std::vector<int> & iters,
                         double prox_accuracy = 0.0, double prox_mu = 0.0, int prox_max_iter = 0)
    {
      const size_t n = contact_mask.size();
      if (n == 0 || X.size() != n * (size_t)(nq_ + nv_) || tau.size() != n * (size_t)(nv_ - 6))
        throw std::runtime_error("X [n][nq + nv], tau [n][nv - 6], contact_mask [n] expected");
      gains(Kp, Kd);
      a.resize(n * nv_);
      lambda.resize(n * (size_t)(fs_ * nf_));
      iters.resize(n);
      check(smpc_robot_sim_forward_dynamics(h_, (int)n, X.data(), tau.data(), contact_mask.data(), Kp.empty() ? nullptr : Kp.data(), Kd.empty() ? nullptr : Kd.data(),
                                            prox_accuracy, prox_mu, prox_max_iter, a.data(), lambda.data(), iters.data()));
    }
    // one step of the batch, states [B][nq + nv] and torques [B][nv - 6] resident on the device, X updated in place; asynchronous on the
    // handle's stream.  mask_device: [B] uint32 on the device (bit per foot), overrides contact_state when not null
    void stepDevice(double * X_device, const double * tau_device, const std::vector<bool> & contact_state, double dt, const std::vector<double> & Kp = {},
                    const std::vector<double> & Kd = {}, const uint32_t * mask_device = nullptr)
    {
      if (!(dt > 0.0))
        throw std::runtime_error("dt must be positive");
      if (!mask_device && (int)contact_state.size() != nf_)
        throw std::runtime_error("contact_state must have one entry per foot");
      gains(Kp, Kd);
      std::vector<uint8_t> c(contact_state.size());
      for (size_t i = 0; i < c.size(); i++)
        c[i] = contact_state[i] ? 1 : 0;
      check(smpc_robot_sim_step_device(h_, X_device, tau_device, (int)c.size() == nf_ ? c.data() : nullptr, mask_device, Kp.empty() ? nullptr : Kp.data(),
                                       Kd.empty() ? nullptr : Kd.data(), dt));
    }
    // issue the simulator's work on the MPC's stream from now on (nullptr: back to its own)
    void shareStream(BatchedMPC * mpc) { check(smpc_robot_sim_share_stream(h_, mpc ? mpc->handle() : nullptr)); }
    void wait() { check(smpc_robot_sim_wait(h_)); }
    void * stream() { return smpc_robot_sim_get_stream(h_); }
    // accelerations [B][nv] / contact forces [B][force_size nfeet] of the last step (host copies; join the handle's stream)
    std::vector<double> lastAccelerations()
    {
      std::vector<double> a((size_t)batch_ * nv_);
      check(smpc_robot_sim_read_last(h_, a.data(), nullptr));
      return a;
    }
    std::vector<double> lastForces()
    {
      std::vector<double> f((size_t)batch_ * fs_ * nf_);
      check(smpc_robot_sim_read_last(h_, nullptr, f.data()));
      return f;
    }
    // the same as device pointers owned by the handle
    void lastDevicePointers(double ** a_device, double ** lambda_device) { check(smpc_robot_sim_get_last(h_, a_device, lambda_device)); }
    smpc_robot_sim * handle() { return h_; }

    // ---- ground plane with unilateral frictional contact detected from the state (smpc_robot_sim_set_ground and the entries after it) ----
    // fields that are 0 stand for their defaults (mu 0.7, erp 0.2, compliance 1e-8, sweeps 30, one point at the foot frame's origin);
    // may be called again; nfeet * points_per_foot <= 8
    void setGround(const smpc_ground_settings & settings)
    {
      check(smpc_robot_sim_set_ground(h_, &settings));
      int d[2];
      check(smpc_robot_sim_get_ground_dims(h_, d));
      gp_ = d[0];
      gn_ = d[1];
    }
    int groundPointsPerFoot() const { return gp_; }
    int groundPoints() const { return gn_; }
    // one step of the batch on the ground, X [B][nq + nv] updated in place, tau [B][nv - 6] (device); asynchronous on the handle's stream
    void stepGroundDevice(double * X_device, const double * tau_device, double dt)
    {
      if (!(dt > 0.0))
        throw std::runtime_error("dt must be positive");
      check(smpc_robot_sim_step_ground_device(h_, X_device, tau_device, dt));
    }
    struct GroundDynamics
    {
      std::vector<double> v_next, a, lambda, gap; // [n][nv], [n][nv], [n][3 points] (on the robot, world axes), [n][points]
      std::vector<uint32_t> contact;              // [n] bit per point: positive normal force
    };
    // the solve of one ground step on host buffers X [n][nq + nv], tau [n][nv - 6]; n need not be the batch, nothing is advanced
    GroundDynamics groundDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt)
    {
      const size_t nx = (size_t)(nq_ + nv_), n = X.size() / nx;
      if (n == 0 || X.size() != n * nx || tau.size() != n * (size_t)(nv_ - 6))
        throw std::runtime_error("X [n][nq + nv], tau [n][nv - 6] expected");
      GroundDynamics g;
      g.v_next.resize(n * nv_);
      g.a.resize(n * nv_);
      g.lambda.resize(n * 3 * (size_t)gn_);
      g.gap.resize(n * (size_t)gn_);
      g.contact.resize(n);
      check(smpc_robot_sim_ground_dynamics(h_, (int)n, X.data(), tau.data(), dt, g.v_next.data(), g.a.data(), g.lambda.data(), g.gap.data(), g.contact.data()));
      return g;
    }
    // forces [B][3 points] / contact words [B] of the last ground step (host copies; join the handle's stream)
    std::vector<double> lastGroundForces()
    {
      std::vector<double> f((size_t)batch_ * 3 * gn_);
      check(smpc_robot_sim_read_ground_last(h_, f.data(), nullptr));
      return f;
    }
    std::vector<uint32_t> lastContacts()
    {
      std::vector<uint32_t> c((size_t)batch_);
      check(smpc_robot_sim_read_ground_last(h_, nullptr, c.data()));
      return c;
    }
    // the same as device pointers owned by the handle (they change when setGround is called again)
    void groundForceDevicePointers(double ** lambda_device, uint32_t ** contact_device) { check(smpc_robot_sim_get_ground_last(h_, lambda_device, contact_device)); }

    // ---- per-robot slopes, friction and pushes on that ground (smpc_robot_sim_set_ground_env and the entries after it) ----
    // planes [B][4] = (n, d): robot i stands on {p : n . p = d}, n a unit normal in world axes with n.z >= 0.5; mu [B] > 0.  An empty vector
    // stands for the handle's setting for every robot ((0, 0, 1, ground_z), the mu of setGround); a call replaces both.  Needs setGround
    // first; setGround called afterwards drops the per-robot ground and the push.
    void setGroundEnv(const std::vector<double> & planes = {}, const std::vector<double> & mu = {})
    {
      if ((!planes.empty() && planes.size() != (size_t)batch_ * 4) || (!mu.empty() && mu.size() != (size_t)batch_))
        throw std::runtime_error("planes [B][4], mu [B] expected (or empty)");
      check(smpc_robot_sim_set_ground_env(h_, planes.empty() ? nullptr : planes.data(), mu.empty() ? nullptr : mu.data()));
    }
    // push [B][6] = (f, o): the force f (world axes, N) on the body of joint `joint` (0 = the base) at the point o given in that joint's
    // frame; an empty vector clears the push
    void setPush(const std::vector<double> & push = {}, int joint = 0)
    {
      if (!push.empty() && push.size() != (size_t)batch_ * 6)
        throw std::runtime_error("push [B][6] expected (or empty)");
      check(smpc_robot_sim_set_ground_push(h_, joint, push.empty() ? nullptr : push.data()));
    }
    // the handle-owned push buffer [B][6] on the device (null while no push is set): a resident loop may rewrite it on the shared stream;
    // values written there are not validated
    double * pushDevicePointer()
    {
      double * p = nullptr;
      check(smpc_robot_sim_get_ground_push(h_, &p));
      return p;
    }
    // groundDynamics with an explicit environment per state: planes [n][4], mu [n], push [n][6] (each may be empty: the handle's setting of
    // setGround, no push); the handle's own environment is not read
    GroundDynamics groundEnvDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const std::vector<double> & planes = {},
                                     const std::vector<double> & mu = {}, const std::vector<double> & push = {}, int joint = 0)
    {
      const size_t nx = (size_t)(nq_ + nv_), n = X.size() / nx;
      if (n == 0 || X.size() != n * nx || tau.size() != n * (size_t)(nv_ - 6))
        throw std::runtime_error("X [n][nq + nv], tau [n][nv - 6] expected");
      if ((!planes.empty() && planes.size() != n * 4) || (!mu.empty() && mu.size() != n) || (!push.empty() && push.size() != n * 6))
        throw std::runtime_error("planes [n][4], mu [n], push [n][6] expected (or empty)");
      GroundDynamics g;
      g.v_next.resize(n * nv_);
      g.a.resize(n * nv_);
      g.lambda.resize(n * 3 * (size_t)gn_);
      g.gap.resize(n * (size_t)gn_);
      g.contact.resize(n);
      check(smpc_robot_sim_ground_env_dynamics(h_, (int)n, X.data(), tau.data(), dt, planes.empty() ? nullptr : planes.data(), mu.empty() ? nullptr : mu.data(),
                                               push.empty() ? nullptr : push.data(), joint, g.v_next.data(), g.a.data(), g.lambda.data(), g.gap.data(),
                                               g.contact.data()));
      return g;
    }

    // ---- warm-started contact solve with a stopping rule on that ground (smpc_robot_sim_set_ground_solver and the entries after it) ----
    // warm_start: every robot starts its sweeps from its own forces of the previous step (the handle-owned warm buffer, contact frame);
    // tol > 0 (m/s): a robot's sweeps stop after sweep s >= min_sweeps once rho_s <= tol (tol = 0: exactly `sweeps` sweeps; min_sweeps in
    // 1 .. sweeps, 0 stands for 1).  Zeroes the warm buffer.  Needs setGround first; setGround called afterwards drops the settings.
    void setGroundSolver(bool warm_start = false, double tol = 0.0, int min_sweeps = 0)
    {
      const smpc_ground_solver_settings s = {warm_start ? 1 : 0, tol, min_sweeps};
      check(smpc_robot_sim_set_ground_solver(h_, &s));
    }
    // zero the warm rows of the listed robots (an empty list: every robot); asynchronous on the handle's stream
    void resetGroundWarmStart(const std::vector<int> & indices = {})
    {
      check(smpc_robot_sim_reset_ground_warm_start(h_, indices.empty() ? nullptr : indices.data(), (int)indices.size()));
    }
    // the same for every robot with a non-zero byte in mask_device [B] (device memory)
    void resetGroundWarmStartDevice(const uint8_t * mask_device) { check(smpc_robot_sim_reset_ground_warm_start_device(h_, mask_device)); }
    // sweeps run [B] / rho of the last sweep run [B] in the last ground step (host copies; join the handle's stream)
    std::vector<int32_t> lastGroundSweeps()
    {
      std::vector<int32_t> s((size_t)batch_);
      check(smpc_robot_sim_read_ground_solver_last(h_, s.data(), nullptr));
      return s;
    }
    std::vector<double> lastGroundResiduals()
    {
      std::vector<double> r((size_t)batch_);
      check(smpc_robot_sim_read_ground_solver_last(h_, nullptr, r.data()));
      return r;
    }
    // the same and the warm buffer [B][3 points] as device pointers owned by the handle (they change when setGround is called again)
    void groundSolverDevicePointers(int32_t ** sweeps_device, double ** residual_device, double ** warm_device)
    {
      check(smpc_robot_sim_get_ground_solver_last(h_, sweeps_device, residual_device, warm_device));
    }
    struct GroundSolve
    {
      GroundDynamics g;
      std::vector<double> lambda_contact, residual; // [n][3 points] in the contact frame [point][t1 t2 n], [n]
      std::vector<int32_t> sweeps;                  // [n]
    };
    // groundEnvDynamics with explicit solver settings and an explicit start vector lam0 [n][3 points] in the contact frame (empty: zeros;
    // read only if warm_start); the handle's settings and warm buffer are neither read nor changed
    GroundSolve groundSolveDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const std::vector<double> & planes = {},
                                    const std::vector<double> & mu = {}, const std::vector<double> & push = {}, int joint = 0, const std::vector<double> & lam0 = {},
                                    bool warm_start = true, double tol = 0.0, int min_sweeps = 0)
    {
      const size_t nx = (size_t)(nq_ + nv_), n = X.size() / nx, nr = 3 * (size_t)gn_;
      if (n == 0 || X.size() != n * nx || tau.size() != n * (size_t)(nv_ - 6))
        throw std::runtime_error("X [n][nq + nv], tau [n][nv - 6] expected");
      if ((!planes.empty() && planes.size() != n * 4) || (!mu.empty() && mu.size() != n) || (!push.empty() && push.size() != n * 6))
        throw std::runtime_error("planes [n][4], mu [n], push [n][6] expected (or empty)");
      if (!lam0.empty() && lam0.size() != n * nr)
        throw std::runtime_error("lam0 [n][3 points] expected (or empty)");
      const smpc_ground_solver_settings s = {warm_start && !lam0.empty() ? 1 : 0, tol, min_sweeps};
      GroundSolve r;
      r.g.v_next.resize(n * nv_);
      r.g.a.resize(n * nv_);
      r.g.lambda.resize(n * nr);
      r.g.gap.resize(n * (size_t)gn_);
      r.g.contact.resize(n);
      r.lambda_contact.resize(n * nr);
      r.residual.resize(n);
      r.sweeps.resize(n);
      check(smpc_robot_sim_ground_solve_dynamics(h_, (int)n, X.data(), tau.data(), dt, planes.empty() ? nullptr : planes.data(), mu.empty() ? nullptr : mu.data(),
                                                 push.empty() ? nullptr : push.data(), joint, &s, lam0.empty() ? nullptr : lam0.data(), r.g.v_next.data(),
                                                 r.g.a.data(), r.g.lambda.data(), r.lambda_contact.data(), r.g.gap.data(), r.g.contact.data(), r.sweeps.data(),
                                                 r.residual.data()));
      return r;
    }

    // ---- effort limits, joint damping, armature and joint-limit stops (smpc_robot_sim_set_joint_model and the entries after it) ----
    // The arrays of a joint model: each empty (tau_max = inf, damping = armature = 0, the limits of the robot table), [na] (broadcast over
    // the batch) or [rows][na] (per robot), na = nv - 6.  activation (rad; 0 stands for 0.1): the distance to a limit below which a joint
    // gets a stop row (at most 8 per robot and step); stop_erp (0 stands for 0.2): the part of a penetration removed per step.
    struct JointModel
    {
      std::vector<double> tau_max, damping, armature, q_lo, q_hi;
      bool stops = true;
      double activation = 0.0, stop_erp = 0.0;
    };
    // From this call on stepGroundDevice clips the torques to [-tau_max, tau_max], damps the joints implicitly and holds them at their
    // limits with unilateral rows that share the contact solve with the feet.  Needs setGround first; setGround called afterwards drops
    // the model.
    void setJointModel(const JointModel & model)
    {
      std::vector<double> keep[5];
      const smpc_joint_model_settings m = jointModel(model, (size_t)batch_, keep);
      check(smpc_robot_sim_set_joint_model(h_, &m));
    }
    // the torques applied in the last ground step [B][na] (host copy; joins the handle's stream); zeros before setJointModel
    std::vector<double> lastAppliedTorques()
    {
      std::vector<double> t((size_t)batch_ * (size_t)(nv_ - 6));
      check(smpc_robot_sim_read_joint_last(h_, t.data(), nullptr, nullptr, nullptr));
      return t;
    }
    struct JointStops
    {
      std::vector<int32_t> stop_rows, dropped; // [n][8]: +(k + 1) joint k at its lower stop, -(k + 1) at its upper stop, 0 unused; [n]
      std::vector<double> lam_stop;            // [n][8]
    };
    JointStops lastJointStops()
    {
      JointStops s;
      s.stop_rows.resize((size_t)batch_ * SMPC_JOINT_MAX_STOPS);
      s.lam_stop.resize((size_t)batch_ * SMPC_JOINT_MAX_STOPS);
      s.dropped.resize((size_t)batch_);
      check(smpc_robot_sim_read_joint_last(h_, nullptr, s.stop_rows.data(), s.lam_stop.data(), s.dropped.data()));
      return s;
    }
    // the same as device pointers owned by the handle (null before setJointModel; they change when setGround is called again)
    void jointModelDevicePointers(double ** tau_applied_device, int32_t ** stop_rows_device, double ** lam_stop_device, int32_t ** dropped_device)
    {
      check(smpc_robot_sim_get_joint_last(h_, tau_applied_device, stop_rows_device, lam_stop_device, dropped_device));
    }
    struct GroundJoint
    {
      GroundSolve s;
      std::vector<double> tau_applied; // [n][na]
      JointStops stops;
    };
    // groundSolveDynamics with an explicit joint model per state; the handle's model, settings and buffers are neither read nor changed
    GroundJoint groundJointDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const JointModel & model,
                                    const std::vector<double> & planes = {}, const std::vector<double> & mu = {}, const std::vector<double> & push = {},
                                    int joint = 0, const std::vector<double> & lam0 = {}, bool warm_start = true, double tol = 0.0, int min_sweeps = 0)
    {
      return groundJointBody(X, tau, dt, model, nullptr, planes, mu, push, joint, lam0, warm_start, tol, min_sweeps);
    }

    // ---- per-robot link masses, centres of mass and inertias (smpc_robot_sim_set_body_params and the entries after it) ----
    // body [B][njoints][10], njoints = nq - 6: row j of robot i = mass | com x y z | Ixx Ixy Iyy Ixz Iyz Izz of the body of joint j (the
    // layout of body_params() below).  From this call on robot i's ground step uses its rows wherever the robot table's mass, com and
    // inertia were used; nothing else of the model changes, and the MPC and ID controllers keep the nominal table.  An empty vector clears
    // them.  Needs setGround first; setGround called afterwards drops them.  Independent of setJointModel.
    void setBodyParams(const std::vector<double> & body)
    {
      if (!body.empty() && body.size() != (size_t)batch_ * (size_t)(nq_ - 6) * 10)
        throw std::runtime_error("body [B][njoints][10] expected (or empty)");
      check(smpc_robot_sim_set_body_params(h_, body.empty() ? nullptr : body.data()));
    }
    // the body parameters in force [B][njoints][10] (host copy): those of setBodyParams, or the table's rows repeated B times
    std::vector<double> bodyParams()
    {
      std::vector<double> b((size_t)batch_ * (size_t)(nq_ - 6) * 10);
      check(smpc_robot_sim_read_body_params(h_, b.data()));
      return b;
    }
    // the handle-owned device array [B][njoints][10] (null while none are set): a resident loop may rewrite it on the shared stream;
    // values written there are not validated
    double * bodyParamsDevicePointer()
    {
      double * p = nullptr;
      check(smpc_robot_sim_get_body_params(h_, &p));
      return p;
    }
    // groundJointDynamics with explicit body parameters per state: body [n][njoints][10] (empty: the robot table's); the handle's own
    // parameters are neither read nor changed
    GroundJoint groundBodyDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const JointModel & model,
                                   const std::vector<double> & body, const std::vector<double> & planes = {}, const std::vector<double> & mu = {},
                                   const std::vector<double> & push = {}, int joint = 0, const std::vector<double> & lam0 = {}, bool warm_start = true,
                                   double tol = 0.0, int min_sweeps = 0)
    {
      return groundJointBody(X, tau, dt, model, &body, planes, mu, push, joint, lam0, warm_start, tol, min_sweeps);
    }

    // ---- per-robot height-field terrain (smpc_robot_sim_set_terrain and the entries after it) ----
    // heights [tiles][ny][nx] are world z at the grid nodes (row j along world y, column i along world x, `cell` metres apart); tile [B]
    // says which tile robot i stands on (empty: 0) and origin [B][2] is the world (x, y) of node (0, 0) of its tile (empty: (0, 0)).
    struct Terrain
    {
      int nx = 0, ny = 0, tiles = 1;
      double cell = 0.0;
      std::vector<double> heights;
      std::vector<int32_t> tile;
      std::vector<double> origin;
    };
    // From this call on every contact point has its own normal, contact frame and gap, sampled from the bilinear patch below it
    // (terrain_height() below is the same sampling); mu, the push, the solver settings, the joint model and the body parameters are
    // unchanged, and the planes of setGroundEnv are not read.  Needs setGround first; setGround called afterwards drops the terrain.
    void setTerrain(const Terrain & t)
    {
      const smpc_terrain_settings c = terrainSettings(t, (size_t)batch_);
      check(smpc_robot_sim_set_terrain(h_, &c));
    }
    // the handle launches what it launched before setTerrain
    void clearTerrain() { check(smpc_robot_sim_set_terrain(h_, nullptr)); }
    // the handle-owned device arrays and the dims (null / 0 while no terrain is set): a resident loop may rewrite the arrays on the shared
    // stream; values written there are not validated, and the kernel's clamps keep every index inside the array
    struct TerrainDevice
    {
      double * heights = nullptr;
      int32_t * tile = nullptr;
      double * origin = nullptr;
      int32_t nx = 0, ny = 0, tiles = 0;
      double cell = 0.0;
    };
    TerrainDevice terrainDevicePointers()
    {
      TerrainDevice d;
      check(smpc_robot_sim_get_terrain(h_, &d.heights, &d.tile, &d.origin, &d.nx, &d.ny, &d.tiles, &d.cell));
      return d;
    }
    // the unit normal of the terrain below every contact point at the last ground step [B][points][3] (host copy)
    std::vector<double> lastTerrainNormals()
    {
      std::vector<double> n((size_t)batch_ * (size_t)gn_ * 3);
      check(smpc_robot_sim_read_terrain_last(h_, n.data(), nullptr));
      return n;
    }
    // the terrain height below every contact point at the last ground step [B][points] (host copy)
    std::vector<double> lastTerrainHeights()
    {
      std::vector<double> h((size_t)batch_ * (size_t)gn_);
      check(smpc_robot_sim_read_terrain_last(h_, nullptr, h.data()));
      return h;
    }
    struct GroundTerrain
    {
      GroundJoint j;
      std::vector<double> normals, heights; // [n][points][3], [n][points]
    };
    // groundBodyDynamics on a terrain instead of planes (tile [n], origin [n][2]); the handle's own terrain is neither read nor changed
    GroundTerrain groundTerrainDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const Terrain & terrain,
                                        const JointModel & model, const std::vector<double> & body = {}, const std::vector<double> & mu = {},
                                        const std::vector<double> & push = {}, int joint = 0, const std::vector<double> & lam0 = {}, bool warm_start = true,
                                        double tol = 0.0, int min_sweeps = 0)
    {
      const size_t n = X.size() / (size_t)(nq_ + nv_);
      const smpc_terrain_settings c = terrainSettings(terrain, n);
      GroundTerrain r;
      r.normals.resize(n * (size_t)gn_ * 3);
      r.heights.resize(n * (size_t)gn_);
      r.j = groundJointBody(X, tau, dt, model, &body, {}, mu, push, joint, lam0, warm_start, tol, min_sweeps, &c, r.normals.data(), r.heights.data());
      return r;
    }

    // ---- body points and the touch mask (smpc_robot_sim_set_body_points and the entries after it) ----
    // point k sits at offsets[k] (metres) in the frame of joint joints[k]; at most 16, shared by the batch; band in metres, 0 stands for 0.02
    struct BodyPoints
    {
      std::vector<int32_t> joints;
      std::vector<double> offsets; // [n][3]
      double band = 0.0;
    };
    // A point whose gap to the ground (the robot's plane, or the terrain below the point) is under `band` takes one of the
    // 8 - nfeet * points_per_foot free contact slots of the robot, in ascending k, and enters the contact solve as a foot point does.  With
    // every point outside the band the results equal those without points bit for bit.  Needs setGround first; setGround called
    // afterwards drops the points.  Independent of the terrain, the joint model, the body parameters, the environment and the solver settings.
    void setBodyPoints(const BodyPoints & p)
    {
      const smpc_body_points_settings c = bodyPointsSettings(p);
      check(smpc_robot_sim_set_body_points(h_, &c));
    }
    // the handle launches what it launched before setBodyPoints
    void clearBodyPoints() { check(smpc_robot_sim_set_body_points(h_, nullptr)); }
    struct BodyContacts
    {
      std::vector<int32_t> body_slots;   // [B][8]: k + 1 of the body point in slot s, 0: unused
      std::vector<double> lam_body;      // [B][8][3]: forces on the robot in world axes
      std::vector<double> body_gap;      // [B][16]: phi_k, 0 beyond the points
      std::vector<int32_t> body_dropped; // [B]
      std::vector<uint8_t> body_touch;   // [B]: 1 iff a slot carries a normal force
    };
    // the five read-outs of the last ground step (host copies; zeros while no points are set)
    BodyContacts lastBodyContacts()
    {
      BodyContacts r = bodyContacts((size_t)batch_);
      check(smpc_robot_sim_read_body_points_last(h_, r.body_slots.data(), r.lam_body.data(), r.body_gap.data(), r.body_dropped.data(), r.body_touch.data()));
      return r;
    }
    // the handle-owned device arrays of the same (null while no points are set).  body_touch is the mask layout of
    // smpc_reset_instances_device and resetGroundWarmStartDevice: handed to them on the shared stream it resets the robots that touched down
    struct BodyPointsDevice
    {
      int32_t * body_slots = nullptr;
      double *lam_body = nullptr, *body_gap = nullptr;
      int32_t * body_dropped = nullptr;
      uint8_t * body_touch = nullptr;
    };
    BodyPointsDevice bodyPointsDevicePointers()
    {
      BodyPointsDevice d;
      check(smpc_robot_sim_get_body_points_last(h_, &d.body_slots, &d.lam_body, &d.body_gap, &d.body_dropped, &d.body_touch));
      return d;
    }
    struct GroundPoints
    {
      GroundTerrain t; // (normals and heights are empty on the plane)
      BodyContacts b;  // ([n] in place of [B])
    };
    // groundTerrainDynamics (terrain non-null) or groundBodyDynamics (null: the planes) with explicit body points; the handle's own points
    // are neither read nor changed
    GroundPoints groundPointsDynamics(const std::vector<double> & X, const std::vector<double> & tau, double dt, const BodyPoints & points,
                                      const Terrain * terrain, const JointModel & model, const std::vector<double> & body = {},
                                      const std::vector<double> & planes = {}, const std::vector<double> & mu = {}, const std::vector<double> & push = {},
                                      int joint = 0, const std::vector<double> & lam0 = {}, bool warm_start = true, double tol = 0.0, int min_sweeps = 0)
    {
      const size_t n = X.size() / (size_t)(nq_ + nv_);
      const smpc_body_points_settings pc = bodyPointsSettings(points);
      smpc_terrain_settings c;
      GroundPoints r;
      if (terrain)
      {
        c = terrainSettings(*terrain, n);
        r.t.normals.resize(n * (size_t)gn_ * 3);
        r.t.heights.resize(n * (size_t)gn_);
      }
      r.b = bodyContacts(n);
      r.t.j = groundJointBody(X, tau, dt, model, &body, planes, mu, push, joint, lam0, warm_start, tol, min_sweeps, terrain ? &c : nullptr,
                              terrain ? r.t.normals.data() : nullptr, terrain ? r.t.heights.data() : nullptr, &pc, &r.b);
      return r;
    }

  private:
    static BodyContacts bodyContacts(size_t n)
    {
      BodyContacts r;
      r.body_slots.resize(n * 8);
      r.lam_body.resize(n * 24);
      r.body_gap.resize(n * 16);
      r.body_dropped.resize(n);
      r.body_touch.resize(n);
      return r;
    }
    static smpc_body_points_settings bodyPointsSettings(const BodyPoints & p)
    {
      if (p.offsets.size() != p.joints.size() * 3)
        throw std::runtime_error("joints [n] and offsets [n][3] expected");
      smpc_body_points_settings c = {};
      c.n = (int32_t)(p.joints.size() < 17 ? p.joints.size() : 17); // (a count above 16 is refused by the library, which names it)
      for (size_t k = 0; k < p.joints.size() && k < 16; k++)
      {
        c.joint[k] = p.joints[k];
        for (int i = 0; i < 3; i++)
          c.offset[k][i] = p.offsets[k * 3 + i];
      }
      c.band = p.band;
      return c;
    }
    smpc_terrain_settings terrainSettings(const Terrain & t, size_t rows) const
    {
      if (t.nx < 0 || t.ny < 0 || t.tiles < 0 || t.heights.size() != (size_t)t.tiles * (size_t)t.ny * (size_t)t.nx)
        throw std::runtime_error("heights [tiles][ny][nx] expected");
      if ((!t.tile.empty() && t.tile.size() != rows) || (!t.origin.empty() && t.origin.size() != rows * 2))
        throw std::runtime_error("tile [rows], origin [rows][2] expected (or empty)");
      smpc_terrain_settings c;
      c.nx = t.nx;
      c.ny = t.ny;
      c.tiles = t.tiles;
      c.cell = t.cell;
      c.heights = t.heights.empty() ? nullptr : t.heights.data();
      c.tile = t.tile.empty() ? nullptr : t.tile.data();
      c.origin = t.origin.empty() ? nullptr : t.origin.data();
      return c;
    }
    // `terrain` non-null: smpc_robot_sim_ground_terrain_dynamics; else `body` null: smpc_robot_sim_ground_joint_dynamics; else
    // smpc_robot_sim_ground_body_dynamics
    GroundJoint groundJointBody(const std::vector<double> & X, const std::vector<double> & tau, double dt, const JointModel & model,
                                const std::vector<double> * body, const std::vector<double> & planes, const std::vector<double> & mu,
                                const std::vector<double> & push, int joint, const std::vector<double> & lam0, bool warm_start, double tol, int min_sweeps,
                                const smpc_terrain_settings * terrain = nullptr, double * normals_out = nullptr, double * heights_out = nullptr,
                                const smpc_body_points_settings * points = nullptr, BodyContacts * bc = nullptr)
    {
      const size_t nx = (size_t)(nq_ + nv_), n = X.size() / nx, nr = 3 * (size_t)gn_, na = (size_t)(nv_ - 6);
      if (n == 0 || X.size() != n * nx || tau.size() != n * na)
        throw std::runtime_error("X [n][nq + nv], tau [n][nv - 6] expected");
      if ((!planes.empty() && planes.size() != n * 4) || (!mu.empty() && mu.size() != n) || (!push.empty() && push.size() != n * 6))
        throw std::runtime_error("planes [n][4], mu [n], push [n][6] expected (or empty)");
      if (!lam0.empty() && lam0.size() != n * nr)
        throw std::runtime_error("lam0 [n][3 points] expected (or empty)");
      if (body && !body->empty() && body->size() != n * (size_t)(nq_ - 6) * 10)
        throw std::runtime_error("body [n][njoints][10] expected (or empty)");
      const smpc_ground_solver_settings s = {warm_start && !lam0.empty() ? 1 : 0, tol, min_sweeps};
      std::vector<double> keep[5];
      const smpc_joint_model_settings m = jointModel(model, n, keep);
      GroundJoint r;
      r.s.g.v_next.resize(n * nv_);
      r.s.g.a.resize(n * nv_);
      r.s.g.lambda.resize(n * nr);
      r.s.g.gap.resize(n * (size_t)gn_);
      r.s.g.contact.resize(n);
      r.s.lambda_contact.resize(n * nr);
      r.s.residual.resize(n);
      r.s.sweeps.resize(n);
      r.tau_applied.resize(n * na);
      r.stops.stop_rows.resize(n * SMPC_JOINT_MAX_STOPS);
      r.stops.lam_stop.resize(n * SMPC_JOINT_MAX_STOPS);
      r.stops.dropped.resize(n);
      const double *pl = planes.empty() ? nullptr : planes.data(), *pm = mu.empty() ? nullptr : mu.data(), *pp = push.empty() ? nullptr : push.data(),
                   *l0 = lam0.empty() ? nullptr : lam0.data();
      if (points)
        check(smpc_robot_sim_ground_points_dynamics(h_, (int)n, X.data(), tau.data(), dt, terrain, pl, pm, pp, joint, &s, l0, &m,
                                                    body && !body->empty() ? body->data() : nullptr, points, r.s.g.v_next.data(), r.s.g.a.data(),
                                                    r.s.g.lambda.data(), r.s.lambda_contact.data(), r.s.g.gap.data(), r.s.g.contact.data(), r.s.sweeps.data(),
                                                    r.s.residual.data(), r.tau_applied.data(), r.stops.stop_rows.data(), r.stops.lam_stop.data(),
                                                    r.stops.dropped.data(), normals_out, heights_out, bc->body_slots.data(), bc->lam_body.data(),
                                                    bc->body_gap.data(), bc->body_dropped.data(), bc->body_touch.data()));
      else if (terrain)
        check(smpc_robot_sim_ground_terrain_dynamics(h_, (int)n, X.data(), tau.data(), dt, terrain, pm, pp, joint, &s, l0, &m,
                                                     body && !body->empty() ? body->data() : nullptr, r.s.g.v_next.data(), r.s.g.a.data(), r.s.g.lambda.data(),
                                                     r.s.lambda_contact.data(), r.s.g.gap.data(), r.s.g.contact.data(), r.s.sweeps.data(), r.s.residual.data(),
                                                     r.tau_applied.data(), r.stops.stop_rows.data(), r.stops.lam_stop.data(), r.stops.dropped.data(), normals_out,
                                                     heights_out));
      else if (body)
        check(smpc_robot_sim_ground_body_dynamics(h_, (int)n, X.data(), tau.data(), dt, pl, pm, pp, joint, &s, l0, &m, body->empty() ? nullptr : body->data(),
                                                  r.s.g.v_next.data(), r.s.g.a.data(), r.s.g.lambda.data(), r.s.lambda_contact.data(), r.s.g.gap.data(),
                                                  r.s.g.contact.data(), r.s.sweeps.data(), r.s.residual.data(), r.tau_applied.data(), r.stops.stop_rows.data(),
                                                  r.stops.lam_stop.data(), r.stops.dropped.data()));
      else
        check(smpc_robot_sim_ground_joint_dynamics(h_, (int)n, X.data(), tau.data(), dt, pl, pm, pp, joint, &s, l0, &m, r.s.g.v_next.data(), r.s.g.a.data(),
                                                   r.s.g.lambda.data(), r.s.lambda_contact.data(), r.s.g.gap.data(), r.s.g.contact.data(), r.s.sweeps.data(),
                                                   r.s.residual.data(), r.tau_applied.data(), r.stops.stop_rows.data(), r.stops.lam_stop.data(),
                                                   r.stops.dropped.data()));
      return r;
    }
    // the C struct of a JointModel for `rows` robots; with one per-robot array the broadcast ones are repeated into `keep` (one stride per call)
    smpc_joint_model_settings jointModel(const JointModel & model, size_t rows, std::vector<double> (&keep)[5]) const
    {
      const size_t na = (size_t)(nv_ - 6);
      const std::vector<double> * src[5] = {&model.tau_max, &model.damping, &model.armature, &model.q_lo, &model.q_hi};
      static const char * const names[5] = {"tau_max", "damping", "armature", "q_lo", "q_hi"};
      bool per_robot = false;
      for (int a = 0; a < 5; a++)
      {
        const size_t sz = src[a]->size();
        if (sz != 0 && sz != na && sz != rows * na)
          throw std::runtime_error(std::string(names[a]) + " [na] or [rows][na] expected (or empty)");
        if (sz != 0 && sz != na)
          per_robot = true;
      }
      const double * ptr[5];
      for (int a = 0; a < 5; a++)
      {
        ptr[a] = src[a]->empty() ? nullptr : src[a]->data();
        if (per_robot && src[a]->size() == na && rows != 1)
        {
          keep[a].resize(rows * na);
          for (size_t i = 0; i < rows; i++)
            for (size_t k = 0; k < na; k++)
              keep[a][i * na + k] = (*src[a])[k];
          ptr[a] = keep[a].data();
        }
      }
      smpc_joint_model_settings m = {ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], per_robot ? 1 : 0, model.stops ? 1 : 0, model.activation, model.stop_erp};
      return m;
    }
    static void check(int rc)
    {
      if (rc < 0)
        throw std::runtime_error(smpc_last_error());
    }
    void gains(const std::vector<double> & Kp, const std::vector<double> & Kd) const
    {
      if ((!Kp.empty() && (int)Kp.size() != fs_) || (!Kd.empty() && (int)Kd.size() != fs_))
        throw std::runtime_error("Kp, Kd: force_size Baumgarte gains each (or empty)");
    }
    smpc_robot_sim * h_ = nullptr;
    int batch_ = 0, nq_ = 0, nv_ = 0, nf_ = 0, fs_ = 0, gp_ = 0, gn_ = 0;
  };

  // ---- host helpers for body parameters (plain C++, no GPU) ----
  // the body parameters [njoints][10] of a robot table: mass | com x y z | Ixx Ixy Iyy Ixz Iyz Izz per joint
  inline std::vector<double> body_params(const smpc_robot_model * robot)
  {
    std::vector<double> b((size_t)robot->njoints * 10);
    for (int j = 0; j < robot->njoints; j++)
    {
      b[(size_t)j * 10] = robot->mass[j];
      for (int k = 0; k < 3; k++)
        b[(size_t)j * 10 + 1 + k] = robot->com[j][k];
      for (int k = 0; k < 6; k++)
        b[(size_t)j * 10 + 4 + k] = robot->inertia[j][k];
    }
    return b;
  }
  // body [rows][10] with mass and inertia of row r multiplied by mass_scale[r % mass_scale.size()] (one factor, one per joint, or one per
  // row); the centres of mass are unchanged
  inline std::vector<double> scale_bodies(const std::vector<double> & body, const std::vector<double> & mass_scale)
  {
    if (body.size() % 10 != 0 || mass_scale.empty() || (body.size() / 10) % mass_scale.size() != 0)
      throw std::runtime_error("scale_bodies: body [rows][10] and mass_scale [1], [njoints] or [rows] expected");
    std::vector<double> out = body;
    for (size_t r = 0; r < body.size() / 10; r++)
    {
      const double s = mass_scale[r % mass_scale.size()];
      out[r * 10] *= s;
      for (int k = 4; k < 10; k++)
        out[r * 10 + k] *= s;
    }
    return out;
  }

  // ---- host helper for the body points (plain C++, no GPU): the eight corners of the box centre +- half_extents in the frame of `joint`,
  // corner k at the signs (k & 1, k & 2, k & 4 -> x, y, z; 0 is the negative side) ----
  inline BatchedRobotSim::BodyPoints box_points(int joint, const double centre[3], const double half_extents[3], double band = 0.0)
  {
    BatchedRobotSim::BodyPoints p;
    p.band = band;
    for (int k = 0; k < 8; k++)
    {
      p.joints.push_back(joint);
      for (int i = 0; i < 3; i++)
        p.offsets.push_back(centre[i] + (((k >> i) & 1) ? half_extents[i] : -half_extents[i]));
    }
    return p;
  }

  // ---- host helpers for the terrain (plain C++, no GPU) ----
  // the sampling of DESIGN 3.28 at the world point (x, y) of one tile heights [ny][nx] with node (0, 0) at (ox, oy): the height of the
  // bilinear patch below the point (coordinates clamped to the grid; NaN and +-inf go to node 0) and its unit normal
  struct TerrainSample
  {
    double h, n[3];
  };
  inline TerrainSample terrain_height(const std::vector<double> & heights, int nx, int ny, double cell, double ox, double oy, double x, double y)
  {
    if (nx < 2 || ny < 2 || heights.size() != (size_t)nx * (size_t)ny)
      throw std::runtime_error("terrain_height: heights [ny][nx] with nx, ny >= 2 expected");
    struct Cell
    {
      int i;
      double u;
    };
    // (sim_terrain_cell and sim_terrain_sample of the library's smpc_sim_terrain_dims.h restated: this header ships without its sources)
    auto cell_of = [&](double p, double o, int n) {
      const double hi = (double)(n - 1), im = (double)(n - 2);
      const double c = (p - o) / cell;
      const double lo = c > 0.0 ? c : 0.0;
      const double cl = lo < hi ? lo : hi;
      const double xc = (c < 0.0 ? -c : c) <= 1.7976931348623157e308 ? cl : 0.0;
      const double fl = std::floor(xc);
      const double fi = fl < im ? fl : im;
      return Cell{(int)fi, xc - fi};
    };
    const Cell a = cell_of(x, ox, nx), b = cell_of(y, oy, ny);
    const double * H = heights.data() + (size_t)b.i * nx + a.i;
    const double h00 = H[0], h10 = H[1], h01 = H[nx], h11 = H[nx + 1], u = a.u, v = b.u;
    const double dx0 = h10 - h00, dx1 = h11 - h01, dy0 = h01 - h00;
    const double h0 = h00 + u * dx0, h1 = h01 + u * dx1;
    const double hx = (dx0 + v * (dx1 - dx0)) / cell, hy = (dy0 + u * ((h11 - h10) - dy0)) / cell;
    const double s = 1.0 / std::sqrt(hx * hx + hy * hy + 1.0);
    TerrainSample r;
    r.h = h0 + v * (h1 - h0);
    r.n[0] = (0.0 - hx) * s;
    r.n[1] = (0.0 - hy) * s;
    r.n[2] = s;
    return r;
  }
  // heights [ny][nx] = f(x, y) at the nodes x = i cell, y = j cell
  template <class F>
  inline std::vector<double> terrain_from_function(F f, int nx, int ny, double cell)
  {
    if (nx < 2 || ny < 2 || !(cell > 0.0))
      throw std::runtime_error("terrain_from_function: nx, ny >= 2 and cell > 0 expected");
    std::vector<double> h((size_t)nx * (size_t)ny);
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++)
        h[(size_t)j * nx + i] = f((double)i * cell, (double)j * cell);
    return h;
  }
} // namespace simple_mpc
