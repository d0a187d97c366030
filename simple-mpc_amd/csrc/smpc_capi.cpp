// smpc_capi.cpp -- extern "C" entry points of include/smpc.h.  An smpc_handle holds one MpcEngineBase (smpc_engine_base.h): every MPC entry
// point checks its arguments and makes one call through that interface; the concrete engines are named in the create functions only.
// Compiled by hipcc for gfx950 (kernels are instantiated here); there is no CPU implementation behind these symbols.
#include "../../include/smpc.h"
#include "../../include/smpc_robots_builtin.h"
#include "smpc_cent_engine.h"
#include "smpc_full_engine.h"
#include "smpc_id.h"
#include "smpc_id_rt.h"
#include "smpc_sim_rt.h"
#include "smpc_sim_ground_rt.h"
#include "smpc_sim_ground_env_rt.h"
#include "smpc_sim_ground_ws_rt.h"
#include "smpc_sim_ground_joint_rt.h"
#include "smpc_robot_check.h"
#include <atomic>
#include <cstring>
#include <memory>
#include <string>

using namespace smpc;

typedef Dims<13, 4> DimsGo2; // free-flyer + 12 revolute joints, 4 point feet

typedef CentDims<4> CentGo2;
typedef CentEngine<DimsGo2, CentGo2> CentEngineGo2;
typedef CentDims<2, 6> CentTalos; // centroidal OCP of the Talos-class biped: 6-D feet, wrench cones (CentroidalOCP with force_size 6)
typedef FullDims<13, 4, 3> FullGo2;   // full dynamics: 12 joint torques, 3-D contacts
typedef FullDims<13, 4, 3, 5> FullGo2Cone; // the same with force_cone: 5 friction-pyramid rows per foot in contact
typedef FullDims<13, 4, 3, 0, 4> FullGo2Land; // land_cstr: 4 rows per landing foot
typedef FullDims<13, 4, 3, 5, 4> FullGo2ConeLand; // force_cone and land_cstr: the land rows behind the pyramid rows
typedef FullDims<23, 2, 6> FullTalos; // Talos-class humanoid: 22 joint torques, two 6-D feet with wrench cones
typedef FullDims<23, 2, 6, 0, 6> FullTalosLand; // land_cstr: 6 frame-velocity rows per landing foot
typedef FullDims<23, 2, 6, 0, 0, 1> KinoTalos;  // KINODYNAMICS OCP of the Talos-class biped: 6-D feet, wrench cones (KinodynamicsOCP with force_size 6)

struct smpc_robot_sim // stand-alone simulator handle: a robot table and nothing else (smpc_sim_rt.h)
{
  std::unique_ptr<RobotSimRt> e;
  std::unique_ptr<RobotSimGround> g; // the ground plane, once smpc_robot_sim_set_ground has been called (destroyed before the engine it refers to)
  std::unique_ptr<RobotSimGroundEnv> ge; // its per-robot environment and the staging of the host-buffer solve (destroyed before the ground it refers to)
  std::unique_ptr<RobotSimGroundWs> gw;  // its solver settings, warm buffer and read-outs (destroyed before the ground it refers to)
  std::unique_ptr<RobotSimGroundJoint> gj; // its joint model and read-outs (destroyed before the ground it refers to)
  std::unique_ptr<RobotSimGroundBody> gb;  // its per-robot body parameters (destroyed before the ground it refers to)
  std::unique_ptr<RobotSimGroundTerrain> gt; // its per-robot height-field terrain (destroyed before the ground it refers to)
  std::unique_ptr<RobotSimGroundPoints> gp;  // its body points and their read-outs (destroyed before the ground it refers to)
  std::vector<double> q_lo, q_hi;        // the robot table's joint limits [nv - 6]: the joint model's defaults
  std::vector<double> body_tab;          // the robot table's mass | com | inertia rows [njoints][10]: what is read while no body parameters are set
};

struct smpc_handle
{
  std::unique_ptr<MpcEngineBase> e; // kinodynamics (smpc_create), centroidal (smpc_create_centroidal) or full dynamics (smpc_create_fulldynamics)
  // state derivatives of every stage (smpc_set_retain_state_derivatives): [B][H][dim] on the handle's device, allocated on the first enable
  double * xdot_all = nullptr;
  bool retain_xdot = false;
  enum
  {
    XDOT_NONE,  // no iterate since the switch was enabled
    XDOT_VALID, // filled by the last iterate
    XDOT_STALE, // smpc_load_state since the last iterate (the buffer is not part of the checkpoint)
    XDOT_RESET  // smpc_reset_instances since the last iterate (the buffer still holds the derivatives of the iterate before the reset)
  } xdot_state = XDOT_NONE;
  ~smpc_handle()
  {
    if (xdot_all)
    {
      set_device(e->device_id);
      dev_free(xdot_all);
    }
  }
};

namespace
{
  thread_local std::string g_err;
  int fail(int code, const std::string & msg)
  {
    g_err = msg;
    return code;
  }
  template <class F>
  int guarded(F && f)
  {
    try
    {
      f();
      return SMPC_OK;
    }
    catch (const InvalidCall & e) // (not on this handle kind, or an index out of its range: smpc_engine_base.h)
    {
      return fail(SMPC_ERR_INVALID, e.what());
    }
    catch (const std::exception & e)
    {
      return fail(SMPC_ERR_RUNTIME, e.what());
    }
  }
  // the engine of a freshly built handle -> *out
  template <class F>
  int create_handle(smpc_handle ** out, F && make)
  {
    return guarded([&] {
      std::unique_ptr<smpc_handle> h(new smpc_handle());
      h->e.reset(make());
      *out = h.release();
    });
  }
  HostMpcSettings host_mpc(const smpc_mpc_settings * mpc)
  {
    HostMpcSettings ms;
    ms.swing_apex = mpc->swing_apex;
    ms.support_force = mpc->support_force;
    ms.TOL = mpc->TOL;
    ms.mu_init = mpc->mu_init;
    ms.timestep = mpc->timestep;
    ms.max_iters = mpc->max_iters;
    ms.num_threads = mpc->num_threads;
    ms.T_fly = mpc->T_fly;
    ms.T_contact = mpc->T_contact;
    ms.T = mpc->T;
    return ms;
  }
  // the weights enter the Gauss-Newton Hessian as they are: they must be symmetric
  bool symmetric(const std::vector<double> & w, int n)
  {
    for (int i = 0; i < n; i++)
      for (int j = 0; j < i; j++)
        if (std::fabs(w[(size_t)i * n + j] - w[(size_t)j * n + i]) > 1e-12 * (1.0 + std::fabs(w[(size_t)i * n + j])))
          return false;
    return true;
  }
  // what the settings of the dense engine's two problems (full dynamics; kinodynamics with 6-D feet) share; nu = size of the control,
  // na = number of actuated joints
  template <class S>
  HostFullSettings host_full(const S * ocp, int ndx, int nu, int na, int fs)
  {
    HostFullSettings s;
    s.timestep = ocp->timestep;
    s.w_x.assign(ocp->w_x, ocp->w_x + (size_t)ndx * ndx);
    s.w_u.assign(ocp->w_u, ocp->w_u + (size_t)nu * nu);
    s.w_cent.assign(ocp->w_cent, ocp->w_cent + 36);
    s.w_frame.assign(ocp->w_frame, ocp->w_frame + fs * fs);
    s.qmin.assign(ocp->qmin, ocp->qmin + na);
    s.qmax.assign(ocp->qmax, ocp->qmax + na);
    for (int i = 0; i < 3; i++)
      s.gravity[i] = ocp->gravity[i];
    s.mu = ocp->mu;
    s.Lfoot = ocp->Lfoot;
    s.Wfoot = ocp->Wfoot;
    s.force_size = fs;
    s.kinematics_limits = ocp->kinematics_limits;
    s.force_cone = ocp->force_cone;
    s.terminal_constraint = ocp->terminal_constraint;
    return s;
  }
  unsigned contact_bits(const uint8_t * contact, int nf)
  {
    unsigned mask = 0;
    for (int k = 0; k < nf; k++)
      mask |= contact[k] ? (1u << k) : 0u;
    return mask;
  }
  int get_output(smpc_handle * h, Output what, double * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->get_output(what, out); });
  }
  // one control step has been enqueued: with retention on, the state derivatives of every stage at its iterate (one launch on the stream)
  void retain_after_iterate(smpc_handle * h)
  {
    if (!h->retain_xdot)
      return;
    h->e->state_derivatives(h->xdot_all);
    h->xdot_state = smpc_handle::XDOT_VALID;
  }
  // why the retained state derivatives cannot be read, or null
  const char * xdot_refusal(const smpc_handle * h)
  {
    if (!h->retain_xdot)
      return "state derivatives of stages t >= 2 are not retained: enable smpc_set_retain_state_derivatives(h, 1) (Python: "
             "setRetainStateDerivatives(True)) before iterate";
    if (h->xdot_state == smpc_handle::XDOT_NONE)
      return "no iterate has run since smpc_set_retain_state_derivatives enabled retention: run iterate first";
    if (h->xdot_state == smpc_handle::XDOT_STALE)
      return "smpc_load_state has run since the last iterate: the state derivatives retained by smpc_set_retain_state_derivatives are "
             "not part of the checkpoint; run iterate first";
    if (h->xdot_state == smpc_handle::XDOT_RESET)
      return "smpc_reset_instances has run since the last iterate: the state derivatives retained by smpc_set_retain_state_derivatives are "
             "those of the iterate before the reset; run iterate first";
    return nullptr;
  }
  // the host-buffer solve behind smpc_robot_sim_ground_joint_dynamics (body null) and smpc_robot_sim_ground_body_dynamics
  int ground_joint_body_dynamics(const char * who, smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane,
                                 const double * mu, const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                 const smpc_joint_model_settings * model, const double * body, double * v_next_out, double * a_out, double * lambda_out,
                                 double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out, double * residual_out,
                                 double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out,
                                 const smpc_terrain_settings * terrain = nullptr, double * normals_out = nullptr, double * heights_out = nullptr,
                                 const smpc_body_points_settings * points = nullptr, int32_t * body_slots_out = nullptr, double * lam_body_out = nullptr,
                                 double * body_gap_out = nullptr, int32_t * body_dropped_out = nullptr, uint8_t * body_touch_out = nullptr);
  // zeros in the five body-point read-outs of n robots (no points: nothing was launched for them)
  void zero_body_points_outputs(int n, int32_t * body_slots_out, double * lam_body_out, double * body_gap_out, int32_t * body_dropped_out,
                                uint8_t * body_touch_out)
  {
    if (body_slots_out)
      std::memset(body_slots_out, 0, sim_points_slots_bytes(n));
    if (lam_body_out)
      std::memset(lam_body_out, 0, sim_points_lam_bytes(n));
    if (body_gap_out)
      std::memset(body_gap_out, 0, sim_points_gap_bytes(n));
    if (body_dropped_out)
      std::memset(body_dropped_out, 0, sim_points_dropped_bytes(n));
    if (body_touch_out)
      std::memset(body_touch_out, 0, sim_points_touch_bytes(n));
  }
} // namespace

extern "C"
{
  const smpc_robot_model * smpc_builtin_robot(const char * name)
  {
    if (!name)
      return nullptr;
    if (!std::strcmp(name, "go2_like"))
      return &SMPC_ROBOT_GO2_LIKE;
    if (!std::strcmp(name, "biped_like"))
      return &SMPC_ROBOT_BIPED_LIKE;
    if (!std::strcmp(name, "talos_like"))
      return &SMPC_ROBOT_TALOS_LIKE;
    return nullptr;
  }
  const char * smpc_last_error(void) { return g_err.c_str(); }
  int smpc_device_count(void) { return device_count(); }

  int smpc_create(
    const smpc_robot_model * robot, const smpc_kinodynamics_settings * ocp, const smpc_mpc_settings * mpc, int batch,
    double gravity_arg, int device_id, smpc_handle ** out)
  {
    if (!robot || !ocp || !mpc || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the MPC engine has no CPU path");
    if (ocp->force_size != 3 && ocp->force_size != 6)
      return fail(SMPC_ERR_INVALID, "force size in settings does not match reference force size");
    if (mpc->T < 2)
      return fail(SMPC_ERR_INVALID, "horizon must have at least 2 stages");
    const HostMpcSettings ms = host_mpc(mpc);
    if (ocp->force_size == 6)
    {
      // 6-D (flat) feet: the kinodynamics variant of the dense stage / solver kernels (FullDims<..., KIN = 1>, smpc_full_model.h)
      if (robot->njoints != KinoTalos::NJ || robot->nfeet != KinoTalos::NF)
        return fail(SMPC_ERR_INVALID, "robot shape (njoints, nfeet, force_size) does not match a built kernel instantiation");
      const int nv = robot->nv, ndx = 2 * nv, na = nv - 6, nu = na + 6 * robot->nfeet;
      HostFullSettings s = host_full(ocp, ndx, nu, na, 6);
      s.w_centder.assign(ocp->w_centder, ocp->w_centder + 36);
      s.w_forces.assign(36, 0.0);
      s.umin.assign(nu, 0.0); // (no torque box in this OCP)
      s.umax.assign(nu, 0.0);
      s.Kp.assign(6, 0.0);
      s.Kd.assign(6, 0.0);
      s.torque_limits = 0;
      s.land_cstr = 0; // (src/kinodynamics.cpp:134-146: land rows exist for 3-D feet only)
      for (int i = 0; i < na; i++)
        if (!(s.qmin[i] <= s.qmax[i]))
          return fail(SMPC_ERR_INVALID, "qmin must not exceed qmax (joint limits are indexed by actuated joint, 0 .. nv - 7)");
      if (!symmetric(s.w_x, ndx) || !symmetric(s.w_u, nu) || !symmetric(s.w_cent, 6) || !symmetric(s.w_centder, 6) || !symmetric(s.w_frame, 6))
        return fail(SMPC_ERR_INVALID, "weight matrices must be symmetric");
      return create_handle(out, [&]() -> MpcEngineBase * {
#if !defined(SMPC_KINO_ONLY) || defined(SMPC_TALOS_TOO) // (experiment builds: -DSMPC_KINO_ONLY -DSMPC_TALOS_TOO = Go2 kinodynamics + the biped's two dense engines)
        return new FullEngine<KinoTalos>(robot, s, ms, batch, gravity_arg, device_id);
#else
        throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#endif
      });
    }
    const int nv = robot->nv, ndx = 2 * nv, nu = nv - 6 + 3 * robot->nfeet;
    HostKinoSettings ks;
    ks.timestep = ocp->timestep;
    ks.w_x.assign(ocp->w_x, ocp->w_x + (size_t)ndx * ndx);
    ks.w_u.assign(ocp->w_u, ocp->w_u + (size_t)nu * nu);
    ks.w_frame.assign(ocp->w_frame, ocp->w_frame + 9);
    ks.w_cent.assign(ocp->w_cent, ocp->w_cent + 36);
    ks.w_centder.assign(ocp->w_centder, ocp->w_centder + 36);
    ks.qmin.assign(ocp->qmin, ocp->qmin + nv - 6);
    ks.qmax.assign(ocp->qmax, ocp->qmax + nv - 6);
    for (int i = 0; i < 3; i++)
      ks.gravity[i] = ocp->gravity[i];
    ks.kinematics_limits = ocp->kinematics_limits;
    ks.terminal_constraint = ocp->terminal_constraint;
    ks.force_cone = ocp->force_cone;
    ks.mu = ocp->mu;
    ks.land_cstr = ocp->land_cstr;
    for (int i = 0; i < nv - 6; i++)
      if (!(ks.qmin[i] <= ks.qmax[i]))
        return fail(SMPC_ERR_INVALID, "qmin must not exceed qmax (joint limits are indexed by actuated joint, 0 .. nv - 7)");
    if (!symmetric(ks.w_x, ndx))
      return fail(SMPC_ERR_INVALID, "w_x must be symmetric");
    if (!symmetric(ks.w_u, nu))
      return fail(SMPC_ERR_INVALID, "w_u must be symmetric");
    return create_handle(out, [&]() -> MpcEngineBase * {
#ifdef SMPC_CENT_ONLY
      throw std::runtime_error("SMPC_CENT_ONLY experiment build");
#else
      return new KinoEngine<DimsGo2>(robot, ks, ms, batch, gravity_arg, device_id);
#endif
    });
  }
  int smpc_create_centroidal(
    const smpc_robot_model * robot, const smpc_centroidal_settings * ocp, const smpc_mpc_settings * mpc, int batch, double gravity_arg,
    int device_id, smpc_handle ** out)
  {
    if (!robot || !ocp || !mpc || !out || !ocp->w_u || !ocp->w_com || !ocp->w_linear_mom || !ocp->w_angular_mom || !ocp->w_linear_acc
        || !ocp->w_angular_acc)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the MPC engine has no CPU path");
    if (ocp->force_size != 3 && ocp->force_size != 6)
      return fail(SMPC_ERR_INVALID, "force size in settings does not match reference force size");
    const bool quad = ocp->force_size == 6;
    if (robot->nfeet != (quad ? CentTalos::NF : CentGo2::NF))
      return fail(SMPC_ERR_INVALID, "robot shape (njoints, nfeet, force_size) does not match a built kernel instantiation");
    // the two built shapes keep the front end of their stage-kernel family; every other robot with these feet: the front end on the run-time
    // joint tree (smpc_frontend_rt.h), on a table that is checked before anything is allocated for it
    const bool built = robot->njoints == (quad ? FullTalos::NJ : DimsGo2::NJ);
    if (!built)
    {
      const std::string why = robot_table_error(robot);
      if (!why.empty())
        return fail(SMPC_ERR_INVALID, why);
    }
    if (mpc->T < 2)
      return fail(SMPC_ERR_INVALID, "horizon must have at least 2 stages");
    const int nu = ocp->force_size * robot->nfeet;
    HostCentSettings cs;
    cs.timestep = ocp->timestep;
    cs.w_u.assign(ocp->w_u, ocp->w_u + (size_t)nu * nu);
    cs.w_com.assign(ocp->w_com, ocp->w_com + 9);
    cs.w_linear_mom.assign(ocp->w_linear_mom, ocp->w_linear_mom + 9);
    cs.w_angular_mom.assign(ocp->w_angular_mom, ocp->w_angular_mom + 9);
    cs.w_linear_acc.assign(ocp->w_linear_acc, ocp->w_linear_acc + 9);
    cs.w_angular_acc.assign(ocp->w_angular_acc, ocp->w_angular_acc + 9);
    for (int i = 0; i < 3; i++)
      cs.gravity[i] = ocp->gravity[i];
    cs.mu = ocp->mu;
    cs.Lfoot = ocp->Lfoot;
    cs.Wfoot = ocp->Wfoot;
    cs.force_size = ocp->force_size;
    if (!symmetric(cs.w_u, nu) || !symmetric(cs.w_com, 3) || !symmetric(cs.w_linear_mom, 3) || !symmetric(cs.w_angular_mom, 3)
        || !symmetric(cs.w_linear_acc, 3) || !symmetric(cs.w_angular_acc, 3))
      return fail(SMPC_ERR_INVALID, "weight matrices must be symmetric");
    const HostMpcSettings ms = host_mpc(mpc);
    return create_handle(out, [&]() -> MpcEngineBase * {
#if !defined(SMPC_KINO_ONLY) || defined(SMPC_XCHECK_SUBSET) // (the cross-check HIP build: Go2 kinodynamics + both centroidal engines)
      if (!built && quad)
        return new CentEngine<RtDims, CentTalos>(robot, cs, ms, batch, gravity_arg, device_id);
      if (!built)
        return new CentEngine<RtDims, CentGo2>(robot, cs, ms, batch, gravity_arg, device_id);
      if (quad)
        return new CentEngine<FullTalos, CentTalos>(robot, cs, ms, batch, gravity_arg, device_id);
      return new CentEngineGo2(robot, cs, ms, batch, gravity_arg, device_id);
#elif defined(SMPC_CENT_ONLY)
      if (quad || !built)
        throw std::runtime_error("SMPC_CENT_ONLY experiment build");
      return new CentEngineGo2(robot, cs, ms, batch, gravity_arg, device_id);
#else
      (void)quad;
      (void)built;
      throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#endif
    });
  }
  int smpc_create_fulldynamics(
    const smpc_robot_model * robot, const smpc_fulldynamics_settings * ocp, const smpc_mpc_settings * mpc, int batch, double gravity_arg,
    int device_id, smpc_handle ** out)
  {
    if (!robot || !ocp || !mpc || !out || !ocp->w_x || !ocp->w_u || !ocp->w_cent || !ocp->w_forces || !ocp->w_frame || !ocp->umin || !ocp->umax
        || !ocp->qmin || !ocp->qmax || !ocp->Kp_correction || !ocp->Kd_correction)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the MPC engine has no CPU path");
    if (ocp->force_size != 3 && ocp->force_size != 6)
      return fail(SMPC_ERR_INVALID, "force size in settings does not match reference force size");
    if (mpc->T < 2)
      return fail(SMPC_ERR_INVALID, "horizon must have at least 2 stages");
    const int nv = robot->nv, ndx = 2 * nv, nu = nv - 6, fs = ocp->force_size;
    HostFullSettings s = host_full(ocp, ndx, nu, nu, fs);
    s.w_forces.assign(ocp->w_forces, ocp->w_forces + fs * fs);
    s.umin.assign(ocp->umin, ocp->umin + nu);
    s.umax.assign(ocp->umax, ocp->umax + nu);
    s.Kp.assign(ocp->Kp_correction, ocp->Kp_correction + fs);
    s.Kd.assign(ocp->Kd_correction, ocp->Kd_correction + fs);
    s.torque_limits = ocp->torque_limits;
    s.land_cstr = ocp->land_cstr;
    for (int i = 0; i < nu; i++)
      if (!(s.qmin[i] <= s.qmax[i]) || !(s.umin[i] <= s.umax[i]))
        return fail(SMPC_ERR_INVALID, "lower limits must not exceed upper limits (indexed by actuated joint, 0 .. nv - 7)");
    if (!symmetric(s.w_x, ndx) || !symmetric(s.w_u, nu) || !symmetric(s.w_cent, 6) || !symmetric(s.w_forces, fs) || !symmetric(s.w_frame, fs))
      return fail(SMPC_ERR_INVALID, "weight matrices must be symmetric");
    const HostMpcSettings ms = host_mpc(mpc);
    return create_handle(out, [&]() -> MpcEngineBase * {
#if defined(SMPC_KINO_ONLY) && defined(SMPC_TALOS_TOO)
      if (robot->njoints == FullTalos::NJ && robot->nfeet == FullTalos::NF && fs == FullTalos::FS && !s.land_cstr)
        return new FullEngine<FullTalos>(robot, s, ms, batch, gravity_arg, device_id);
      throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#elif defined(SMPC_KINO_ONLY) && defined(SMPC_GO2FULL_TOO)
      if (robot->njoints == FullGo2::NJ && robot->nfeet == FullGo2::NF && fs == FullGo2::FS && !s.land_cstr && !s.force_cone)
        return new FullEngine<FullGo2>(robot, s, ms, batch, gravity_arg, device_id);
      throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#elif defined(SMPC_KINO_ONLY)
      throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#else
      if (robot->njoints == FullGo2::NJ && robot->nfeet == FullGo2::NF && fs == FullGo2::FS && s.land_cstr && s.force_cone)
        return new FullEngine<FullGo2ConeLand>(robot, s, ms, batch, gravity_arg, device_id);
      if (robot->njoints == FullGo2::NJ && robot->nfeet == FullGo2::NF && fs == FullGo2::FS && s.land_cstr)
        return new FullEngine<FullGo2Land>(robot, s, ms, batch, gravity_arg, device_id);
      if (robot->njoints == FullTalos::NJ && robot->nfeet == FullTalos::NF && fs == FullTalos::FS && s.land_cstr)
        return new FullEngine<FullTalosLand>(robot, s, ms, batch, gravity_arg, device_id);
      if (robot->njoints == FullGo2::NJ && robot->nfeet == FullGo2::NF && fs == FullGo2::FS && s.force_cone)
        return new FullEngine<FullGo2Cone>(robot, s, ms, batch, gravity_arg, device_id);
      if (robot->njoints == FullGo2::NJ && robot->nfeet == FullGo2::NF && fs == FullGo2::FS)
        return new FullEngine<FullGo2>(robot, s, ms, batch, gravity_arg, device_id);
      if (robot->njoints == FullTalos::NJ && robot->nfeet == FullTalos::NF && fs == FullTalos::FS)
        return new FullEngine<FullTalos>(robot, s, ms, batch, gravity_arg, device_id);
      throw std::runtime_error("robot shape (njoints, nfeet, force_size) does not match a built kernel instantiation");
#endif
    });
  }
  int smpc_destroy(smpc_handle * h)
  {
    delete h;
    return SMPC_OK;
  }
  int smpc_get_dims(const smpc_handle * h, int * d)
  {
    if (!h || !d)
      return fail(SMPC_ERR_INVALID, "null argument");
    std::copy(h->e->dims, h->e->dims + 8, d);
    return SMPC_OK;
  }
  int smpc_generate_cycle_horizon(smpc_handle * h, const uint8_t * cs, int n)
  {
    if (!h || !cs)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->generate_cycle_horizon(cs, n); });
  }
  int smpc_switch_to_walk(smpc_handle * h, const double * v6)
  {
    if (!h || !v6)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->switch_to_walk(v6); });
  }
  int smpc_switch_to_stand(smpc_handle * h)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->switch_to_stand(); });
  }
  int smpc_set_velocity_base_batched(smpc_handle * h, const double * V)
  {
    if (!h || !V)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->set_velocity_base_batched(V); });
  }
  int smpc_set_stage_reference(smpc_handle * h, int t, int what, const double * v, int n)
  {
    if (!h || !v)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->set_stage_reference(t, what, v, n); });
  }
  int smpc_get_stage_reference(smpc_handle * h, int t, int what, double * v, int n)
  {
    if (!h || !v)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->get_stage_reference(t, what, v, n); });
  }
  int smpc_set_reference_pose(smpc_handle * h, int t, int foot, const double * p3)
  {
    if (!h || !p3)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->set_reference_pose(t, foot, p3); });
  }
  int smpc_get_reference_pose(smpc_handle * h, int t, int foot, int instance, double * p3)
  {
    if (!h || !p3)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->get_reference_pose(t, foot, instance, p3); });
  }
  int smpc_set_reference_pose_se3(smpc_handle * h, int t, int foot, const double * p3, const double * R9)
  {
    if (!h || !p3 || !R9)
      return fail(SMPC_ERR_INVALID, "null argument");
    const int rc = smpc_set_reference_pose(h, t, foot, p3);
    if (rc != SMPC_OK)
      return rc;
    return guarded([&] { h->e->set_reference_rotation(t, foot, R9); });
  }
  int smpc_get_reference_pose_se3(smpc_handle * h, int t, int foot, int instance, double * p3, double * R9)
  {
    if (!h || !p3 || !R9)
      return fail(SMPC_ERR_INVALID, "null argument");
    const int rc = smpc_get_reference_pose(h, t, foot, instance, p3);
    if (rc != SMPC_OK)
      return rc;
    return guarded([&] { h->e->get_reference_rotation(t, foot, R9); });
  }
  int smpc_get_contact_state(smpc_handle * h, int t, uint8_t * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      const unsigned m = h->e->contact_mask(t);
      for (int f = 0; f < h->e->dims[6]; f++)
        out[f] = (m >> f) & 1u;
    });
  }
  int smpc_get_cycling_contact_state(smpc_handle * h, int t, uint8_t * out)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    const GaitTimer & tm = h->e->timer;
    const int n = (int)tm.states.size();
    if (!out)
      return n;
    if (n == 0)
      return fail(SMPC_ERR_INVALID, "generateCycleHorizon has not been called");
    if (t < 0 || t >= n)
      return fail(SMPC_ERR_INVALID, "Stage index exceeds the cycle length");
    for (int f = 0; f < tm.nf; f++)
      out[f] = tm.states[t][f];
    return n;
  }
  int smpc_set_x_reference(smpc_handle * h, const double * x)
  {
    if (!h || !x)
      return fail(SMPC_ERR_INVALID, "null argument");
    h->e->x_reference.assign(x, x + h->e->dims[2]);
    return SMPC_OK;
  }
  int smpc_iterate(smpc_handle * h, const double * X)
  {
    if (!h || !X)
      return fail(SMPC_ERR_INVALID, "null argument");
    h->xdot_state = smpc_handle::XDOT_NONE;
    return guarded([&] {
      h->e->iterate_host(X);
      if (h->retain_xdot)
      {
        retain_after_iterate(h);
        h->e->sync();
      }
    });
  }
  int smpc_iterate_async(smpc_handle * h, const double * X)
  {
    if (!h || !X)
      return fail(SMPC_ERR_INVALID, "null argument");
    h->xdot_state = smpc_handle::XDOT_NONE;
    return guarded([&] {
      h->e->iterate_host_async(X); // (synchronous on full-dynamics and centroidal handles)
      retain_after_iterate(h);
    });
  }
  int smpc_gather_outputs(smpc_handle * h, double * out, size_t row_doubles)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->gather_outputs_async(out, row_doubles); });
  }
  int smpc_gather_outputs_device(smpc_handle * h, double * out_device, size_t row_doubles)
  {
    if (!h || !out_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->gather_outputs_device(out_device, row_doubles); });
  }
  int smpc_gather_outputs_peer(smpc_handle * h, double * out_peer, int dst_device)
  {
    if (!h || !out_peer)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->gather_outputs_peer(out_peer, dst_device); });
  }
  int smpc_iterate_device(smpc_handle * h, const double * Xd)
  {
    if (!h || !Xd)
      return fail(SMPC_ERR_INVALID, "null argument");
    h->xdot_state = smpc_handle::XDOT_NONE;
    return guarded([&] {
      h->e->iterate_device(Xd);
      retain_after_iterate(h);
    });
  }
  int smpc_wait(smpc_handle * h)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->sync(); });
  }
  void * smpc_get_stream(smpc_handle * h) { return h ? stream_native(h->e->stream) : nullptr; }
  static size_t state_pass(smpc_handle * h, StateIO::Mode mode, void * buf, size_t cap)
  {
    StateIO io(mode, buf, cap, h->e->stream);
    return h->e->state_io(io);
  }
  int smpc_state_size(smpc_handle * h, size_t * bytes)
  {
    if (!h || !bytes)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { *bytes = state_pass(h, StateIO::COUNT, nullptr, 0); });
  }
  int smpc_save_state(smpc_handle * h, void * buffer, size_t capacity, size_t * written)
  {
    if (!h || !buffer)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      const size_t n = state_pass(h, StateIO::SAVE, buffer, capacity);
      if (written)
        *written = n;
    });
  }
  int smpc_load_state(smpc_handle * h, const void * buffer, size_t size)
  {
    if (!h || !buffer)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (h->xdot_state == smpc_handle::XDOT_VALID)
      h->xdot_state = smpc_handle::XDOT_STALE;
    return guarded([&] { state_pass(h, StateIO::LOAD, const_cast<void *>(buffer), size); });
  }
  // (both forms re-apply the constructor's cold start, reference src/mpc.cpp:72-89, to the chosen instances)
  int smpc_reset_instances(smpc_handle * h, const int * instances, int n)
  {
    if (!h || (!instances && n > 0))
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      h->e->reset_instances(instances, n);
      if (n > 0 && h->xdot_state == smpc_handle::XDOT_VALID)
        h->xdot_state = smpc_handle::XDOT_RESET;
    });
  }
  int smpc_reset_instances_device(smpc_handle * h, const uint8_t * mask_device)
  {
    if (!h || !mask_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      h->e->reset_instances_device(mask_device);
      if (h->xdot_state == smpc_handle::XDOT_VALID)
        h->xdot_state = smpc_handle::XDOT_RESET;
    });
  }
  int smpc_get_x_device(smpc_handle * h, int t, double * out_device)
  {
    if (!h || !out_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->gather_x_device(t, out_device); });
  }
  int smpc_get_xs(smpc_handle * h, double * out) { return get_output(h, OUT_XS, out); }
  int smpc_get_us(smpc_handle * h, double * out) { return get_output(h, OUT_US, out); }
  int smpc_get_vs(smpc_handle * h, double * out) { return get_output(h, OUT_VS, out); }
  int smpc_get_lams(smpc_handle * h, double * out) { return get_output(h, OUT_LAMS, out); }
  int smpc_get_K0(smpc_handle * h, double * out) { return get_output(h, OUT_K0, out); }
  int smpc_get_Ks(smpc_handle * h, double * out) { return get_output(h, OUT_KS, out); }
  int smpc_get_state_derivative01(smpc_handle * h, double * out) { return get_output(h, OUT_XDOT01, out); }
  int smpc_get_reference_poses(smpc_handle * h, double * out) { return get_output(h, OUT_FOOT_REFS, out); }
  int smpc_get_info(smpc_handle * h, double * out) { return get_output(h, OUT_INFO, out); }
  int smpc_get_contact_forces(smpc_handle * h, double * out) { return get_output(h, OUT_CONTACT_FORCES, out); }
  int smpc_debug_get_extra_multipliers(smpc_handle * h, int which, double * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->get_extra_multipliers(which, out); });
  }
  int smpc_set_retain_state_derivatives(smpc_handle * h, int on)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!on)
    {
      h->retain_xdot = false;
      h->xdot_state = smpc_handle::XDOT_NONE;
      return SMPC_OK;
    }
    if (h->retain_xdot)
      return SMPC_OK;
    if (!h->xdot_all)
    {
      try
      {
        set_device(h->e->device_id);
        h->xdot_all = (double *)dev_alloc(h->e->xdot_doubles() * sizeof(double));
      }
      catch (const std::exception & e)
      {
        dev_clear_error(); // (the handle stays usable, retention stays off)
        return fail(SMPC_ERR_RUNTIME, std::string("smpc_set_retain_state_derivatives: ") + e.what());
      }
    }
    h->retain_xdot = true;
    h->xdot_state = smpc_handle::XDOT_NONE;
    return SMPC_OK;
  }
  int smpc_get_state_derivatives(smpc_handle * h, double * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (const char * why = xdot_refusal(h))
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      const stream_t st = h->e->stream;
      set_device(h->e->device_id);
      stream_sync(st);
      d2h(out, h->xdot_all, h->e->xdot_doubles() * sizeof(double), st);
      stream_sync(st);
    });
  }
  int smpc_get_state_derivatives_device(smpc_handle * h, double * out_device)
  {
    if (!h || !out_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (const char * why = xdot_refusal(h))
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      set_device(h->e->device_id);
      d2d(out_device, h->xdot_all, h->e->xdot_doubles() * sizeof(double), h->e->stream);
    });
  }
  int smpc_get_foot_timing(smpc_handle * h, int foot, int which, int * out, int cap)
  {
    const GaitTimer * tm = h ? &h->e->timer : nullptr;
    if (!tm || foot < 0 || foot >= tm->nf || tm->nf == 0)
    {
      fail(SMPC_ERR_INVALID, "invalid foot index or cycle horizon not generated");
      return SMPC_ERR_INVALID;
    }
    const std::vector<int> & v = which ? tm->land[foot] : tm->takeoff[foot];
    for (int i = 0; i < (int)v.size() && i < cap; i++)
      out[i] = v[i];
    return (int)v.size();
  }
  int smpc_get_status(smpc_handle * h, int * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    const int B = h->e->B;
    std::vector<double> info((size_t)B * SC_N);
    const int rc = smpc_get_info(h, info.data());
    if (rc < 0)
      return rc;
    int bad = 0;
    for (int b = 0; b < B; b++)
    {
      const double * s = &info[(size_t)b * SC_N];
      int w = 0;
      for (int i = 0; i < 12; i++)
        if (!std::isfinite(s[i]))
          w |= SMPC_STATUS_NONFINITE;
      if (s[SC_LS_FAILED] != 0.0)
        w |= SMPC_STATUS_LS_FAILED;
      if (s[SC_PREG] >= 1e9)
        w |= SMPC_STATUS_REG_SATURATED;
      out[b] = w;
      bad += w != 0;
    }
    return bad;
  }
  int smpc_get_cold_trace(smpc_handle * h, double * out, int cap)
  {
    if (!h || (!out && cap > 0))
      return fail(SMPC_ERR_INVALID, "null argument");
    const int n = h->e->cold_iters;
    for (int i = 0; i < n && i < cap; i++)
      for (int k = 0; k < 4; k++)
        out[i * 4 + k] = h->e->cold_trace[(size_t)i * 4 + k];
    return n;
  }
  // (size of what smpc_debug_get_lq returns.  A null handle reports the row-major form of a Go2 kinodynamics knot, as this entry point
  // always has.)
  int smpc_lq_size(const smpc_handle * h)
  {
    const int n = h ? h->e->lq_size() : 0;
    return n ? n : kino_lq_size<DimsGo2>();
  }
  int smpc_set_early_exit_on_tol(smpc_handle * h, int on)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null handle");
    return guarded([&] { h->e->set_early_exit(on != 0); });
  }
  int smpc_debug_get_lq(smpc_handle * h, int inst, int t, double * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->debug_lq(inst, t, out); });
  }
  int smpc_debug_get_steps(smpc_handle * h, double * dxs, double * dus)
  {
    if (!h || !dxs || !dus)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->debug_steps(dxs, dus); });
  }
  int smpc_debug_get_terminal(smpc_handle * h, int inst, double * QN, double * qN)
  {
    if (!h || !QN || !qN)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->debug_terminal(inst, QN, qN); });
  }
  int smpc_debug_get_dual_steps(smpc_handle * h, double * dvs, double * dlams)
  {
    if (!h || !dvs || !dlams)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->debug_dual_steps(dvs, dlams); });
  }
  int smpc_debug_get_phase_cycles(smpc_handle * h, double * out64)
  {
    if (!h || !out64)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->phase_cycles(out64); });
  }
  int smpc_set_profiling(smpc_handle * h, int en)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    h->e->profiling = en != 0;
    return SMPC_OK;
  }
  int smpc_kernel_time_slots(void) { return KID_N; }
  // centroidal handle: slot 0 = front-end kernel, slot 1 = the fused control-step kernel (6-D feet: recede, then deriv / riccati / forward /
  // line search in slots 2 .. 5), 0 in the slots behind its CentKernelId
  int smpc_get_kernel_times_n(smpc_handle * h, double * ms, long * calls, int n)
  {
    if (!h || !ms || !calls || n < 0)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      h->e->collect_profile();
      for (int i = 0; i < n && i < KID_N; i++)
      {
        ms[i] = h->e->kernel_ms[i];
        calls[i] = h->e->kernel_calls[i];
      }
    });
  }
  // (kept for callers of the first form: it writes smpc_kernel_time_slots() entries -- use smpc_get_kernel_times_n with the capacity of your arrays)
  int smpc_get_kernel_times(smpc_handle * h, double * ms, long * calls) { return smpc_get_kernel_times_n(h, ms, calls, KID_N); }
  int smpc_reset_kernel_times(smpc_handle * h)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->reset_profile(); });
  }
  int smpc_update_internal_data(smpc_handle * h, const double * X, double * feet, double * com, double * hg, double * centroidal_state)
  {
    if (!h || !X)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->update_internal_data(X, feet, com, hg, centroidal_state); });
  }
  int smpc_debug_frontend_rt(smpc_handle * h, const double * X, double * feet, double * com, double * hg, double * centroidal_state)
  {
    if (!h || !X)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->debug_frontend_rt(X, feet, com, hg, centroidal_state); });
  }
  // (a full-dynamics handle: its own robot, 3-D or 6-D contacts, Kp / Kd of force_size entries)
  int smpc_full_forward_dynamics(
    smpc_handle * h, int n, const double * X, const double * tau, const unsigned * contact_mask, const double * Kp,
    const double * Kd, double prox_accuracy, double prox_mu, int prox_max_iter, double * a_out, double * lambda_out,
    int * iters_out, double * kernel_ms)
  {
    if (!h || !X || !tau || !contact_mask || !a_out || !lambda_out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] {
      h->e->full_forward_dynamics(n, X, tau, contact_mask, Kp, Kd, prox_accuracy, prox_mu, prox_max_iter, a_out, lambda_out, iters_out, kernel_ms);
    });
  }
  int smpc_riccati_feedback(smpc_handle * h, double delay, const double * X_meas, double * u_out)
  {
    if (!h || !X_meas || !u_out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->riccati_feedback(delay, X_meas, u_out); });
  }
  // full-dynamics handle: force_out [B][nfeet][force_size] = interpolated MPC::getContactForces; centroidal handle: x_out [B][9], acc_out = state
  // derivative [B][9], force_out [B][3 nfeet]
  int smpc_interpolate(smpc_handle * h, double delay, int knots, double * x_out, double * acc_out, double * force_out)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { h->e->interpolate(delay, knots, x_out, acc_out, force_out); });
  }
  int smpc_interpolate_knots(int kind, double delay, double timestep, const double * knots, int n, int dim, double * out, int device_id)
  {
    if (!knots || !out || n < 1 || dim < 1 || kind < 0 || kind > 2 || !(timestep > 0.0) || !(delay >= 0.0))
      return fail(SMPC_ERR_INVALID, "invalid argument");
    // the robot is told by the size of the knots: the two topologies the engines are instantiated for (free-flyer + nv - 6 joints)
    const bool biped = (kind == 0 && dim == FullTalos::NX) || (kind == 1 && dim == FullTalos::NQ);
    if (kind == 0 && dim != DimsGo2::NX && !biped)
      return fail(SMPC_ERR_INVALID, "State is not of the right size");
    if (kind == 1 && dim != DimsGo2::NQ && !biped)
      return fail(SMPC_ERR_INVALID, "Configuration is not of the right size");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the interpolator has no CPU path");
    return guarded([&] {
      set_device(device_id);
      stream_t st = stream_create();
      double * dk = (double *)dev_alloc(((size_t)n * dim + dim) * sizeof(double));
      h2d(dk, knots, (size_t)n * dim * sizeof(double), st);
      auto run = [&](auto dims) {
        typedef decltype(dims) DD;
        InterpKnotsArgs<DD> ia;
        ia.kind = kind;
        ia.n = n;
        ia.dim = dim;
        ia.delay = delay;
        ia.timestep = timestep;
        ia.knots = dk;
        ia.out = dk + (size_t)n * dim;
        launch<InterpKnotsArgs<DD>, interp_knots_body<DD>, 64>(1, st, ia);
      };
#ifndef SMPC_KINO_ONLY
      if (biped)
        run(FullTalos());
      else
#endif
        run(DimsGo2());
      d2h(out, dk + (size_t)n * dim, (size_t)dim * sizeof(double), st);
      stream_sync(st);
      dev_free(dk);
      stream_destroy(st);
    });
  }
  int smpc_friction_compensation(
    const double * dry, const double * viscous, int nu, const double * velocity, int velocity_size, double * torque, int torque_size,
    int batch, int device_id)
  {
    if (!dry || !viscous || !velocity || !torque || nu < 1 || batch < 1)
      return fail(SMPC_ERR_INVALID, "invalid argument");
    if (velocity_size != nu)
      return fail(SMPC_ERR_INVALID, "Velocity has wrong size");
    if (torque_size != nu)
      return fail(SMPC_ERR_INVALID, "Torque has wrong size");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the friction compensation has no CPU path");
    return guarded([&] {
      set_device(device_id);
      stream_t st = stream_create();
      const size_t total = (size_t)batch * nu;
      double * d = (double *)dev_alloc((2 * (size_t)nu + 2 * total) * sizeof(double));
      h2d(d, dry, (size_t)nu * sizeof(double), st);
      h2d(d + nu, viscous, (size_t)nu * sizeof(double), st);
      h2d(d + 2 * nu, velocity, total * sizeof(double), st);
      h2d(d + 2 * nu + total, torque, total * sizeof(double), st);
      FrictionArgs fa;
      fa.dry = d;
      fa.viscous = d + nu;
      fa.velocity = d + 2 * nu;
      fa.torque = d + 2 * nu + total;
      fa.nu = nu;
      fa.total = total;
      launch<FrictionArgs, friction_body, 256>((int)((total + 255) / 256), st, fa);
      d2h(torque, fa.torque, total * sizeof(double), st);
      stream_sync(st);
      dev_free(d);
      stream_destroy(st);
    });
  }
  int smpc_centroidal_dynamics(
    double mass, const double * gravity, double timestep, int nfeet, const double * X, const double * U, const unsigned char * contact,
    const double * contact_pos, int batch, double * Xnext, double * A, double * B, int device_id)
  {
    if (!gravity || !X || !U || !contact || !contact_pos || !Xnext || nfeet < 1 || batch < 1 || !(mass > 0.0) || !(timestep > 0.0))
      return fail(SMPC_ERR_INVALID, "invalid argument");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the centroidal dynamics has no CPU path");
    return guarded([&] {
      set_device(device_id);
      stream_t st = stream_create();
      const size_t nu = 3 * (size_t)nfeet, nb = (size_t)batch;
      const size_t n_in = nb * 9 + nb * nu + nb * nfeet * 3, n_out = nb * 9 + nb * 81 + nb * 9 * nu;
      double * d = (double *)dev_alloc((n_in + n_out) * sizeof(double) + nb * nfeet);
      double *dX = d, *dU = dX + nb * 9, *dP = dU + nb * nu, *dXn = dP + nb * nfeet * 3, *dA = dXn + nb * 9, *dB = dA + nb * 81;
      unsigned char * dC = reinterpret_cast<unsigned char *>(dB + nb * 9 * nu);
      h2d(dX, X, nb * 9 * sizeof(double), st);
      h2d(dU, U, nb * nu * sizeof(double), st);
      h2d(dP, contact_pos, nb * nfeet * 3 * sizeof(double), st);
      h2d(dC, contact, nb * nfeet, st);
      CentroidalArgs ca;
      ca.mass = mass;
      ca.dt = timestep;
      for (int i = 0; i < 3; i++)
        ca.g[i] = gravity[i];
      ca.nf = nfeet;
      ca.batch = batch;
      ca.X = dX;
      ca.U = dU;
      ca.pos = dP;
      ca.contact = dC;
      ca.Xn = dXn;
      ca.A = A ? dA : nullptr;
      ca.Bm = B ? dB : nullptr;
      launch<CentroidalArgs, centroidal_body, 64>((batch + 63) / 64, st, ca);
      d2h(Xnext, dXn, nb * 9 * sizeof(double), st);
      if (A)
        d2h(A, dA, nb * 81 * sizeof(double), st);
      if (B)
        d2h(B, dB, nb * 9 * nu * sizeof(double), st);
      stream_sync(st);
      dev_free(d);
      stream_destroy(st);
    });
  }

  // ---- whole-body inverse-dynamics QP (smpc_id.h, smpc_id_rt.h) ----
  static std::atomic<int> g_id_force_rt{0}; // (process-wide; read once per smpc_id_create)
  // the one body of smpc_id_create and smpc_id_create_any: only the routing call differs
  static int id_create_routed(const smpc_robot_model * robot, const smpc_id_settings * c, int batch, int device_id, smpc_id_handle ** out, bool any)
  {
    if (!robot || !c || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the inverse-dynamics engine has no CPU path");
    if (!c->effort_limit || !c->velocity_limit || !c->q_min || !c->q_max)
      return fail(SMPC_ERR_INVALID, "effort, velocity and position limits of the actuated joints are required");
    HostIdSettings hs;
    hs.dev.friction_coefficient = c->friction_coefficient;
    hs.dev.ratio_max = c->contact_weight_ratio_max;
    hs.dev.ratio_min = c->contact_weight_ratio_min;
    hs.dev.kp_base = c->kp_base;
    hs.dev.kp_posture = c->kp_posture;
    hs.dev.kp_contact = c->kp_contact;
    hs.dev.w_base = c->w_base;
    hs.dev.w_posture = c->w_posture;
    hs.dev.w_contact_motion = c->w_contact_motion;
    hs.dev.w_contact_force = c->w_contact_force;
    hs.dev.contact_motion_equality = c->contact_motion_equality;
    hs.dev.control_dt = c->control_dt;
    hs.dev.admm_iters = c->admm_iters > 0 ? c->admm_iters : 400;
    hs.dev.rho = c->admm_rho > 0 ? c->admm_rho : 0.1;
    hs.dev.sigma = c->admm_sigma > 0 ? c->admm_sigma : 1e-6;
    hs.dev.alpha = c->admm_alpha > 0 ? c->admm_alpha : 1.6;
    hs.dev.admm_tol = c->admm_tol == 0.0 ? 1e-7 : c->admm_tol;
    hs.dev.centroidal = c->centroidal != 0;
    hs.dev.pad_ = 0;
    hs.dev.base_as_coded = c->base_reference_as_coded != 0;
    hs.dev.tsid_bounds = c->tsid_joint_bounds != 0;
    hs.dev.kp_com = c->kp_com;
    hs.dev.kp_feet_tracking = c->kp_feet_tracking;
    hs.dev.w_com = c->w_com;
    hs.dev.w_feet_tracking = c->w_feet_tracking;
    if (c->centroidal && !(c->kp_com >= 0.0 && c->kp_feet_tracking >= 0.0))
      return fail(SMPC_ERR_INVALID, "task gains must not be negative");
    if (!(c->kp_base >= 0.0 && c->kp_posture >= 0.0 && c->kp_contact >= 0.0))
      return fail(SMPC_ERR_INVALID, "task gains must not be negative");
    const bool quad = c->force_size == 6;
    if (c->force_size != 0 && c->force_size != 3 && c->force_size != 6)
      return fail(SMPC_ERR_INVALID, "force size must be 3 (point feet) or 6 (flat feet)");
    // the two built shapes keep their templated engines and kernel symbols; every other table with 4 point feet: the engine on the run-time
    // joint tree (smpc_id_rt.h), on a table that is checked before anything is allocated for it
    std::string why;
    const bool force_rt = g_id_force_rt.load() != 0;
    const IdRoute route = any ? id_route_any(robot, quad, FullGo2::NJ, FullGo2::NF, FullTalos::NJ, FullTalos::NF, force_rt, why)
                              : id_route(robot, quad, FullGo2::NJ, FullGo2::NF, FullTalos::NJ, FullTalos::NF, force_rt, why);
    if (route == ID_ROUTE_REFUSED)
      return fail(SMPC_ERR_INVALID, why);
    const int na = robot->nv - 6;
    hs.tau_max.assign(c->effort_limit, c->effort_limit + na);
    hs.v_max.assign(c->velocity_limit, c->velocity_limit + na);
    hs.q_min.assign(c->q_min, c->q_min + na);
    hs.q_max.assign(c->q_max, c->q_max + na);
    if (quad)
    {
      if (!c->quad_contact_points)
        return fail(SMPC_ERR_INVALID, "flat feet need the four corners of every sole (quad_contact_points, [nfeet][4][3])");
      hs.quad_points.assign(c->quad_contact_points, c->quad_contact_points + (size_t)robot->nfeet * 12);
    }
    return guarded([&] {
#if defined(SMPC_KINO_ONLY) && !defined(SMPC_WITH_ID) // (tools/variant_build.sh <name> -DSMPC_WITH_ID: the ID engines too)
      throw std::runtime_error("SMPC_KINO_ONLY experiment build");
#endif
      if (route == ID_ROUTE_GO2)
        *out = reinterpret_cast<smpc_id_handle *>(static_cast<IdEngineBase *>(new IdEngine<FullGo2>(robot, hs, batch, device_id)));
      else if (route == ID_ROUTE_TALOS)
        *out = reinterpret_cast<smpc_id_handle *>(static_cast<IdEngineBase *>(new IdEngine<FullTalos>(robot, hs, batch, device_id)));
      else
        *out = reinterpret_cast<smpc_id_handle *>(static_cast<IdEngineBase *>(new IdEngineRt(robot, hs, batch, device_id, route == ID_ROUTE_RT6)));
    });
  }
  int smpc_id_create(const smpc_robot_model * robot, const smpc_id_settings * c, int batch, int device_id, smpc_id_handle ** out)
  {
    return id_create_routed(robot, c, batch, device_id, out, false);
  }
  int smpc_id_create_any(const smpc_robot_model * robot, const smpc_id_settings * c, int batch, int device_id, smpc_id_handle ** out)
  {
    return id_create_routed(robot, c, batch, device_id, out, true);
  }
  // debug: send the built point-foot shape (13 joints / 4 point feet) through the run-time engine too, so that the two can be compared; under
  // smpc_id_create_any also the built flat-foot shape (23 joints / 2 flat feet)
  int smpc_debug_id_force_rt(int on)
  {
    return g_id_force_rt.exchange(on != 0 ? 1 : 0);
  }
  int smpc_id_get_dims(smpc_id_handle * h, int * dims)
  {
    if (!h || !dims)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(h);
    const int d[10] = {e->B, e->nq, e->nv, e->nf, e->nfw, e->n, e->m, e->np, e->mp, e->nmot};
    for (int i = 0; i < 10; i++)
      dims[i] = d[i];
    return SMPC_OK;
  }
  void smpc_id_destroy(smpc_id_handle * h) { delete reinterpret_cast<IdEngineBase *>(h); }
  int smpc_id_set_target(smpc_id_handle * h, int instance, const double * q, const double * v, const double * a, const uint8_t * contact, const double * f)
  {
    if (!h || !q || !v || !a || !contact || !f)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(h);
    const unsigned mask = contact_bits(contact, e->nf);
    return guarded([&] { e->set_target(instance, q, v, a, mask, f); });
  }
  int smpc_id_set_targets(smpc_id_handle * h, const double * Q, const double * V, const double * A, const uint8_t * contact, const double * F)
  {
    if (!h || !Q || !V || !A || !contact || !F)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->set_targets(Q, V, A, contact, F); });
  }
  int smpc_id_set_target_centroidal(smpc_id_handle * h, int instance, const double * com, const double * vcom, const double * feet_p,
                                    const double * feet_v, const uint8_t * contact, const double * f)
  {
    if (!h || !com || !vcom || !feet_p || !feet_v || !contact || !f)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(h);
    const unsigned mask = contact_bits(contact, e->nf);
    return guarded([&] { e->set_target_centroidal(instance, com, vcom, feet_p, feet_v, mask, f); });
  }
  int smpc_id_set_targets_centroidal(smpc_id_handle * h, const double * COM, const double * VCOM, const double * FEET_P, const double * FEET_V,
                                     const uint8_t * contact, const double * F)
  {
    if (!h || !COM || !VCOM || !FEET_P || !FEET_V || !contact || !F)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->set_targets_centroidal(COM, VCOM, FEET_P, FEET_V, contact, F); });
  }
  int smpc_id_solve(smpc_id_handle * h, const double * X, double * tau, double * a, double * f, double * resid)
  {
    if (!h || !X || !tau)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(h);
    return guarded([&] {
      std::vector<double> ta, tf;
      if (!a)
        ta.resize((size_t)e->B * e->nv);
      if (!f)
        tf.resize((size_t)e->B * e->nfw * e->nf);
      e->solve(X, tau, a ? a : ta.data(), f ? f : tf.data(), resid);
    });
  }
  int smpc_id_solve_device(smpc_id_handle * h, const double * X_device, double * tau_device)
  {
    if (!h || !X_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->solve_device(X_device, tau_device); });
  }
  int smpc_id_wait(smpc_id_handle * h)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->wait(); });
  }
  int smpc_id_get_resid(smpc_id_handle * h, double * resid)
  {
    if (!h || !resid)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->get_resid(resid); });
  }
  int smpc_id_reset(smpc_id_handle * h, int instance)
  {
    if (!h)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->reset(instance); });
  }
  const double * smpc_id_get_tau_device(smpc_id_handle * h) { return h ? reinterpret_cast<IdEngineBase *>(h)->tau_device() : nullptr; }
  int smpc_id_set_targets_from_mpc(smpc_id_handle * id, smpc_handle * mpc, double delay, int knots)
  {
    if (!id || !mpc)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(id);
    MpcEngineBase & m = *mpc->e;
    double *com, *vcom, *fp, *fv;
    e->centroidal_target_buffers(&com, &vcom, &fp, &fv);
    // centroidal MPC -> CentroidalID (examples/talos_centroidal.py:218-243); kinodynamics OCP (either engine) or full-dynamics OCP ->
    // KinodynamicsID: states, accelerations, contact forces
    if (m.centroidal() && !com)
      return fail(SMPC_ERR_INVALID, "a centroidal MPC handle feeds a CentroidalID controller");
    if (!m.centroidal() && com)
      return fail(SMPC_ERR_INVALID, "a kinodynamics MPC handle feeds a KinodynamicsID controller");
    if (e->B != m.B || e->nv != m.dims[1] || e->nf != m.dims[6]
        || (m.centroidal() ? e->nfw * e->nf != m.dims[4] : (e->nq != m.dims[0] || e->nfw != m.force_size)))
      return fail(SMPC_ERR_INVALID, "the controller and the MPC must hold the same batch of the same robot");
    return guarded([&] {
      double *x, *a, *f;
      e->target_buffers(&x, &a, &f);
      e->set_mask_all(m.contact_mask(0));
      const bool shared = e->solve_stream() == m.stream; // (one in-order queue: nothing to order)
      if (!shared)
        e->wait(); // (the previous solve has read its targets)
      if (m.centroidal())
        m.interpolate_device_id(delay, knots, com, vcom, fp, fv, f);
      else
        m.interpolate_device(delay, knots, x, a, f);
      if (!shared)
        m.wait_stream(e->solve_stream()); // the next solve starts after the targets are written
    });
  }
  int smpc_id_share_stream(smpc_id_handle * id, smpc_handle * mpc)
  {
    if (!id)
      return fail(SMPC_ERR_INVALID, "null argument");
    IdEngineBase * e = reinterpret_cast<IdEngineBase *>(id);
    if (!mpc)
      return guarded([&] { e->adopt_stream(e->solve_stream(), true); });
    if (mpc->e->device_id != e->device())
      return fail(SMPC_ERR_INVALID, "smpc_id_share_stream: the controller and the MPC handle live on different devices");
    return guarded([&] { e->adopt_stream(mpc->e->stream, false); });
  }
  // (a full-dynamics handle: its own robot and contact model, Kp / Kd of force_size entries)
  int smpc_sim_step_device(smpc_handle * h, double * X_device, const double * tau_device, const uint8_t * contact, const double * Kp, const double * Kd, double dt)
  {
    if (!h || !X_device || !tau_device || !contact)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!(dt > 0.0))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    return guarded([&] { h->e->sim_step_device(X_device, tau_device, contact_bits(contact, h->e->dims[6]), Kp, Kd, dt); });
  }
  double * smpc_id_get_x_device(smpc_id_handle * h) { return h ? reinterpret_cast<IdEngineBase *>(h)->x_device() : nullptr; }
  int smpc_id_debug_get(smpc_id_handle * h, int what, double * out)
  {
    if (!h || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { reinterpret_cast<IdEngineBase *>(h)->debug_get(what, out); });
  }

  // ---- batched rigid-body simulator on a run-time joint tree (smpc_sim_rt.h) ----
  int smpc_robot_sim_create(const smpc_robot_model * robot, int force_size, int batch, const double * gravity, int device_id, smpc_robot_sim ** out)
  {
    if (!robot || !out)
      return fail(SMPC_ERR_INVALID, "null argument");
    *out = nullptr;
    // admission before anything else: nothing is allocated for a table, a contact size or a batch the simulator is not built for
    const std::string why = sim_rt_admission_error(robot, force_size, batch);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    if (gravity && !(std::isfinite(gravity[0]) && std::isfinite(gravity[1]) && std::isfinite(gravity[2])))
      return fail(SMPC_ERR_INVALID, "gravity is not finite");
    if (device_count() <= 0)
      return fail(SMPC_ERR_NO_DEVICE, "no HIP device visible: the simulator has no CPU path");
    return guarded([&] {
      std::unique_ptr<smpc_robot_sim> h(new smpc_robot_sim());
      h->e.reset(new RobotSimRt(robot, force_size, batch, gravity, device_id));
      h->q_lo.assign(robot->q_lo, robot->q_lo + h->e->sz.na);
      h->q_hi.assign(robot->q_hi, robot->q_hi + h->e->sz.na);
      h->body_tab.resize((size_t)robot->njoints * SIM_BODY_ROW);
      sim_body_table_rows(robot, h->body_tab.data());
      *out = h.release();
    });
  }
  void smpc_robot_sim_destroy(smpc_robot_sim * sim) { delete sim; }
  int smpc_robot_sim_get_dims(smpc_robot_sim * sim, int * dims)
  {
    if (!sim || !dims)
      return fail(SMPC_ERR_INVALID, "null argument");
    const RobotSimRt & e = *sim->e;
    const int d[5] = {e.B, e.sz.nq, e.sz.nv, e.sz.nfeet, e.sz.fs};
    for (int i = 0; i < 5; i++)
      dims[i] = d[i];
    return SMPC_OK;
  }
  int smpc_robot_sim_wait(smpc_robot_sim * sim)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { sim->e->wait(); });
  }
  void * smpc_robot_sim_get_stream(smpc_robot_sim * sim) { return sim ? stream_native(sim->e->stream) : nullptr; }
  int smpc_robot_sim_share_stream(smpc_robot_sim * sim, smpc_handle * mpc)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!mpc)
      return guarded([&] { sim->e->adopt_stream(sim->e->stream, true); });
    if (mpc->e->device_id != sim->e->device_id)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_share_stream: the simulator and the MPC handle live on different devices");
    return guarded([&] { sim->e->adopt_stream(mpc->e->stream, false); });
  }
  int smpc_robot_sim_forward_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, const unsigned * contact_mask, const double * Kp,
                                      const double * Kd, double prox_accuracy, double prox_mu, int prox_max_iter, double * a_out, double * lambda_out,
                                      int * iters_out)
  {
    if (!sim || !X || !tau || !contact_mask || !a_out || !lambda_out)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (n < 1)
      return fail(SMPC_ERR_INVALID, "n must be positive");
    return guarded([&] { sim->e->forward_dynamics(n, X, tau, contact_mask, Kp, Kd, prox_accuracy, prox_mu, prox_max_iter, a_out, lambda_out, iters_out); });
  }
  int smpc_robot_sim_step_device(smpc_robot_sim * sim, double * X_device, const double * tau_device, const uint8_t * contact, const uint32_t * mask_device,
                                 const double * Kp, const double * Kd, double dt)
  {
    if (!sim || !X_device || !tau_device || (!contact && !mask_device))
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!(dt > 0.0))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    const unsigned mask_all = contact ? contact_bits(contact, sim->e->sz.nfeet) : 0u;
    return guarded([&] { sim->e->step_device(X_device, tau_device, mask_all, mask_device, Kp, Kd, dt); });
  }
  int smpc_robot_sim_get_last(smpc_robot_sim * sim, double ** a_device, double ** lambda_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (a_device)
      *a_device = sim->e->a;
    if (lambda_device)
      *lambda_device = sim->e->lam;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_last(smpc_robot_sim * sim, double * a_out, double * lambda_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    return guarded([&] { sim->e->read_last(a_out, lambda_out); });
  }

  // ---- ground plane with unilateral frictional contact (smpc_sim_ground_rt.h) ----
  int smpc_robot_sim_set_ground(smpc_robot_sim * sim, const smpc_ground_settings * settings)
  {
    if (!sim || !settings)
      return fail(SMPC_ERR_INVALID, "null argument");
    // admission before anything else: nothing is allocated, and the previous settings stay, for settings the kernel is not built for
    const std::string why = sim_ground_admission_error(sim->e->sz.nfeet, settings);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      sim->e->wait(); // (a step in flight still writes the buffers that are replaced below)
      std::unique_ptr<RobotSimGround> g(new RobotSimGround(*sim->e, settings));
      sim->ge.reset(); // (the per-robot environment and the push go with the ground they were set on)
      sim->gw.reset(); // (and so do the solver settings and the warm buffer)
      sim->gj.reset(); // (and the joint model)
      sim->gb.reset(); // (and the body parameters)
      sim->gt.reset(); // (and the terrain)
      sim->gp.reset(); // (and the body points)
      sim->g = std::move(g);
    });
  }
  int smpc_robot_sim_get_ground_dims(smpc_robot_sim * sim, int * dims)
  {
    if (!sim || !dims)
      return fail(SMPC_ERR_INVALID, "null argument");
    dims[0] = sim->g ? sim->g->gz.P : 0;
    dims[1] = sim->g ? sim->g->gz.npts : 0;
    return SMPC_OK;
  }
  int smpc_robot_sim_step_ground_device(smpc_robot_sim * sim, double * X_device, const double * tau_device, double dt)
  {
    if (!sim || !X_device || !tau_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_step_ground_device: no ground yet, call smpc_robot_sim_set_ground first");
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    if (sim->gp && sim->gp->active) // (body points have been set: a body-point kernel at 32 rows, on the terrain if there is one, with the joint model and the bodies if there are any)
      return guarded([&] {
        if (!sim->gj)
          sim->gj.reset(new RobotSimGroundJoint(*sim->g)); // (its arrays stay null: nothing is allocated)
        const bool terr = sim->gt && sim->gt->active;
        SimTerrainDev view;
        if (terr)
          view = sim->gt->view();
        const SimPointsDev pts = sim->gp->view();
        sim->gj->step_device(X_device, tau_device, dt, sim->ge.get(), sim->gw.get(), sim->gb && sim->gb->active ? sim->gb->body : nullptr, terr ? &view : nullptr,
                             &pts);
      });
    if (sim->gt && sim->gt->active) // (a terrain has been set: sim_ground_terrain_rt_body with the joint model and the bodies if there are any, else the inert model and a null body)
      return guarded([&] {
        if (!sim->gj)
          sim->gj.reset(new RobotSimGroundJoint(*sim->g)); // (its arrays stay null: nothing is allocated)
        const SimTerrainDev view = sim->gt->view();
        sim->gj->step_device(X_device, tau_device, dt, sim->ge.get(), sim->gw.get(), sim->gb && sim->gb->active ? sim->gb->body : nullptr, &view);
      });
    if (sim->gb && sim->gb->active) // (body parameters have been set: sim_ground_body_rt_body with the joint model if there is one, else the inert one)
      return guarded([&] {
        if (!sim->gj)
          sim->gj.reset(new RobotSimGroundJoint(*sim->g)); // (its arrays stay null: nothing is allocated)
        sim->gj->step_device(X_device, tau_device, dt, sim->ge.get(), sim->gw.get(), sim->gb->body);
      });
    if (sim->gj && sim->gj->active) // (a joint model has been set: sim_ground_joint_rt_body, which reads the environment and the solver settings if there are any)
      return guarded([&] { sim->gj->step_device(X_device, tau_device, dt, sim->ge.get(), sim->gw.get()); });
    if (sim->gw && sim->gw->active) // (solver settings have been set: sim_ground_ws_rt_body, which reads the environment if there is one)
      return guarded([&] { sim->gw->step_device(X_device, tau_device, dt, sim->ge.get()); });
    if (sim->ge && sim->ge->active) // (a per-robot environment or a push has been set: sim_ground_env_rt_body)
      return guarded([&] { sim->ge->step_device(X_device, tau_device, dt); });
    return guarded([&] { sim->g->step_device(X_device, tau_device, dt); });
  }
  int smpc_robot_sim_ground_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, double * v_next_out, double * a_out,
                                     double * lambda_out, double * gap_out, uint32_t * contact_out)
  {
    if (!sim || !X || !tau)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_ground_dynamics: no ground yet, call smpc_robot_sim_set_ground first");
    if (n < 1)
      return fail(SMPC_ERR_INVALID, "n must be positive");
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    return guarded([&] { sim->g->dynamics(n, X, tau, dt, v_next_out, a_out, lambda_out, gap_out, contact_out); });
  }
  int smpc_robot_sim_get_ground_last(smpc_robot_sim * sim, double ** lambda_device, uint32_t ** contact_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_get_ground_last: no ground yet, call smpc_robot_sim_set_ground first");
    if (lambda_device)
      *lambda_device = sim->g->lam;
    if (contact_device)
      *contact_device = sim->g->contact;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_ground_last(smpc_robot_sim * sim, double * lambda_out, uint32_t * contact_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_read_ground_last: no ground yet, call smpc_robot_sim_set_ground first");
    return guarded([&] { sim->g->read_last(lambda_out, contact_out); });
  }

  // ---- per-robot planes, friction and pushes on the ground (smpc_sim_ground_env_rt.h) ----
  int smpc_robot_sim_set_ground_env(smpc_robot_sim * sim, const double * plane, const double * mu)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_ground_env: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous environment stays, for values the model does not admit
    const std::string why = sim_ground_env_admission_error(sim->e->B, plane, mu);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->ge)
        sim->ge.reset(new RobotSimGroundEnv(*sim->g));
      sim->ge->set_env(plane, mu);
    });
  }
  int smpc_robot_sim_set_ground_push(smpc_robot_sim * sim, int push_joint, const double * push)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_ground_push: no ground yet, call smpc_robot_sim_set_ground first");
    const std::string why = sim_ground_push_admission_error(sim->e->B, sim->e->sz.nq - 6, push_joint, push);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->ge)
        sim->ge.reset(new RobotSimGroundEnv(*sim->g));
      sim->ge->set_push(push_joint, push);
    });
  }
  int smpc_robot_sim_get_ground_push(smpc_robot_sim * sim, double ** push_device)
  {
    if (!sim || !push_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_get_ground_push: no ground yet, call smpc_robot_sim_set_ground first");
    *push_device = sim->ge ? sim->ge->push : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_ground_env_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                         const double * push, int push_joint, double * v_next_out, double * a_out, double * lambda_out, double * gap_out,
                                         uint32_t * contact_out)
  {
    if (!sim || !X || !tau)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_ground_env_dynamics: no ground yet, call smpc_robot_sim_set_ground first");
    if (n < 1)
      return fail(SMPC_ERR_INVALID, "n must be positive");
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    std::string why = sim_ground_env_admission_error(n, plane, mu);
    if (why.empty())
      why = sim_ground_push_admission_error(n, sim->e->sz.nq - 6, push_joint, push);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->ge)
        sim->ge.reset(new RobotSimGroundEnv(*sim->g)); // (staging only: the handle's ground steps stay on sim_ground_rt_body until a setter is called)
      sim->ge->dynamics(n, X, tau, dt, plane, mu, push, push_joint, v_next_out, a_out, lambda_out, gap_out, contact_out);
    });
  }

  // ---- warm-started contact solve with a stopping rule (smpc_sim_ground_ws_rt.h) ----
  int smpc_robot_sim_set_ground_solver(smpc_robot_sim * sim, const smpc_ground_solver_settings * settings)
  {
    if (!sim || !settings)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_ground_solver: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous settings and the warm buffer stay, for settings the model does not admit
    const std::string why = sim_ground_ws_admission_error(sim->g->gs.sweeps, settings);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gw)
        sim->gw.reset(new RobotSimGroundWs(*sim->g));
      sim->gw->set_solver(settings);
    });
  }
  int smpc_robot_sim_reset_ground_warm_start(smpc_robot_sim * sim, const int * indices, int n)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_reset_ground_warm_start: no ground yet, call smpc_robot_sim_set_ground first");
    std::vector<unsigned char> m((size_t)sim->e->B);
    const std::string why = sim_ground_ws_reset_error(indices, n, sim->e->B, m.data());
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    if (!sim->gw) // (no warm buffer before the setter: nothing to zero, nothing allocated)
      return SMPC_OK;
    return guarded([&] { sim->gw->reset_list(m); });
  }
  int smpc_robot_sim_reset_ground_warm_start_device(smpc_robot_sim * sim, const uint8_t * mask_device)
  {
    if (!sim || !mask_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_reset_ground_warm_start_device: no ground yet, call smpc_robot_sim_set_ground first");
    if (!sim->gw)
      return SMPC_OK;
    return guarded([&] { sim->gw->reset_device(mask_device); });
  }
  int smpc_robot_sim_get_ground_solver_last(smpc_robot_sim * sim, int32_t ** sweeps_device, double ** residual_device, double ** warm_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_get_ground_solver_last: no ground yet, call smpc_robot_sim_set_ground first");
    // (null pointers before the setter or the first host-buffer solve: a getter allocates nothing)
    if (sweeps_device)
      *sweeps_device = sim->gw ? sim->gw->sweeps : nullptr;
    if (residual_device)
      *residual_device = sim->gw ? sim->gw->resid : nullptr;
    if (warm_device)
      *warm_device = sim->gw ? sim->gw->warm : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_ground_solver_last(smpc_robot_sim * sim, int32_t * sweeps_out, double * residual_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_read_ground_solver_last: no ground yet, call smpc_robot_sim_set_ground first");
    if (!sim->gw) // (zeros before the setter, without allocating or joining the stream)
    {
      for (int i = 0; i < sim->e->B; i++)
      {
        if (sweeps_out)
          sweeps_out[i] = 0;
        if (residual_out)
          residual_out[i] = 0.0;
      }
      return SMPC_OK;
    }
    return guarded([&] { sim->gw->read_last(sweeps_out, residual_out); });
  }
  int smpc_robot_sim_ground_solve_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                           const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                           double * v_next_out, double * a_out, double * lambda_out, double * lambda_contact_out, double * gap_out,
                                           uint32_t * contact_out, int32_t * sweeps_out, double * residual_out)
  {
    if (!sim || !X || !tau)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_ground_solve_dynamics: no ground yet, call smpc_robot_sim_set_ground first");
    if (n < 1)
      return fail(SMPC_ERR_INVALID, "n must be positive");
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    const smpc_ground_solver_settings inert = {0, 0.0, 0};
    const smpc_ground_solver_settings * st = settings ? settings : &inert;
    std::string why = sim_ground_ws_admission_error(sim->g->gs.sweeps, st);
    if (why.empty())
      why = sim_ground_env_admission_error(n, plane, mu);
    if (why.empty())
      why = sim_ground_push_admission_error(n, sim->e->sz.nq - 6, push_joint, push);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gw)
        sim->gw.reset(new RobotSimGroundWs(*sim->g)); // (staging only: the handle's ground steps keep their kernel until the setter is called)
      sim->gw->dynamics(n, X, tau, dt, plane, mu, push, push_joint, sim_ground_ws_resolve(st), lambda0, v_next_out, a_out, lambda_out, lambda_contact_out,
                        gap_out, contact_out, sweeps_out, residual_out);
    });
  }

  // ---- effort limits, joint damping, armature and joint-limit stops (smpc_sim_ground_joint_rt.h) ----
  int smpc_robot_sim_set_joint_model(smpc_robot_sim * sim, const smpc_joint_model_settings * model)
  {
    if (!sim || !model)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_joint_model: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous model stays, for values the model does not admit
    const std::string why = sim_joint_admission_error(sim->e->B, sim->e->sz.na, sim->q_lo.data(), sim->q_hi.data(), model);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gj)
        sim->gj.reset(new RobotSimGroundJoint(*sim->g));
      sim->gj->set_model(model, sim->q_lo.data(), sim->q_hi.data());
    });
  }
  int smpc_robot_sim_get_joint_last(smpc_robot_sim * sim, double ** tau_applied_device, int32_t ** stop_rows_device, double ** lam_stop_device,
                                    int32_t ** dropped_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_get_joint_last: no ground yet, call smpc_robot_sim_set_ground first");
    // (null pointers before the setter: a getter allocates nothing)
    const bool have = sim->gj && sim->gj->active;
    if (tau_applied_device)
      *tau_applied_device = have ? sim->gj->tau_applied : nullptr;
    if (stop_rows_device)
      *stop_rows_device = have ? sim->gj->rows : nullptr;
    if (lam_stop_device)
      *lam_stop_device = have ? sim->gj->lams : nullptr;
    if (dropped_device)
      *dropped_device = have ? sim->gj->dropped : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_joint_last(smpc_robot_sim * sim, double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_read_joint_last: no ground yet, call smpc_robot_sim_set_ground first");
    if (!(sim->gj && sim->gj->active)) // (zeros before the setter, without allocating or joining the stream)
    {
      const int B = sim->e->B, na = sim->e->sz.na;
      for (int i = 0; i < B; i++)
      {
        for (int k = 0; k < na && tau_applied_out; k++)
          tau_applied_out[(size_t)i * na + k] = 0.0;
        for (int r = 0; r < SIM_JOINT_MAX_STOPS; r++)
        {
          if (stop_rows_out)
            stop_rows_out[(size_t)i * SIM_JOINT_MAX_STOPS + r] = 0;
          if (lam_stop_out)
            lam_stop_out[(size_t)i * SIM_JOINT_MAX_STOPS + r] = 0.0;
        }
        if (dropped_out)
          dropped_out[i] = 0;
      }
      return SMPC_OK;
    }
    return guarded([&] { sim->gj->read_last(tau_applied_out, stop_rows_out, lam_stop_out, dropped_out); });
  }
  int smpc_robot_sim_ground_joint_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                           const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                           const smpc_joint_model_settings * model, double * v_next_out, double * a_out, double * lambda_out,
                                           double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out, double * residual_out,
                                           double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out)
  {
    return ground_joint_body_dynamics("smpc_robot_sim_ground_joint_dynamics", sim, n, X, tau, dt, plane, mu, push, push_joint, settings, lambda0, model, nullptr,
                                      v_next_out, a_out, lambda_out, lambda_contact_out, gap_out, contact_out, sweeps_out, residual_out, tau_applied_out,
                                      stop_rows_out, lam_stop_out, dropped_out);
  }

  // ---- per-robot link masses, centres of mass and inertias (smpc_sim_ground_joint_rt.h: sim_ground_body_rt_body) ----
  int smpc_robot_sim_set_body_params(smpc_robot_sim * sim, const double * body)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_body_params: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous parameters stay, for rows a robot table could not carry
    const std::string why = sim_body_admission_error(sim->e->B, sim->e->sz.nq - 6, body);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gb)
      {
        if (!body) // (nothing to clear, nothing allocated)
          return;
        sim->gb.reset(new RobotSimGroundBody(*sim->g));
      }
      sim->gb->set(body);
    });
  }
  int smpc_robot_sim_read_body_params(smpc_robot_sim * sim, double * body_out)
  {
    if (!sim || !body_out)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (sim->gb && sim->gb->active)
      return guarded([&] { sim->gb->read(body_out); });
    for (int i = 0; i < sim->e->B; i++) // (the table's rows, without allocating or joining the stream)
      std::memcpy(body_out + (size_t)i * sim->body_tab.size(), sim->body_tab.data(), sim->body_tab.size() * sizeof(double));
    return SMPC_OK;
  }
  int smpc_robot_sim_get_body_params(smpc_robot_sim * sim, double ** body_device)
  {
    if (!sim || !body_device)
      return fail(SMPC_ERR_INVALID, "null argument");
    *body_device = sim->gb && sim->gb->active ? sim->gb->body : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_ground_body_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane, const double * mu,
                                          const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                          const smpc_joint_model_settings * model, const double * body, double * v_next_out, double * a_out, double * lambda_out,
                                          double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out, double * residual_out,
                                          double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out)
  {
    return ground_joint_body_dynamics("smpc_robot_sim_ground_body_dynamics", sim, n, X, tau, dt, plane, mu, push, push_joint, settings, lambda0, model, body,
                                      v_next_out, a_out, lambda_out, lambda_contact_out, gap_out, contact_out, sweeps_out, residual_out, tau_applied_out,
                                      stop_rows_out, lam_stop_out, dropped_out);
  }

  // ---- per-robot height-field terrain (smpc_sim_ground_joint_rt.h: sim_ground_terrain_rt_body) ----
  int smpc_robot_sim_set_terrain(smpc_robot_sim * sim, const smpc_terrain_settings * terrain)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_terrain: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous terrain stays
    const std::string why = sim_terrain_admission_error(sim->e->B, terrain);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gt)
      {
        if (!terrain) // (nothing to clear, nothing allocated)
          return;
        sim->gt.reset(new RobotSimGroundTerrain(*sim->g));
      }
      sim->gt->set(terrain);
    });
  }
  int smpc_robot_sim_get_terrain(smpc_robot_sim * sim, double ** heights_device, int32_t ** tile_device, double ** origin_device, int32_t * nx, int32_t * ny,
                                 int32_t * tiles, double * cell)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    const bool on = sim->gt && sim->gt->active;
    if (heights_device)
      *heights_device = on ? sim->gt->heights : nullptr;
    if (tile_device)
      *tile_device = on ? sim->gt->tile : nullptr;
    if (origin_device)
      *origin_device = on ? sim->gt->origin : nullptr;
    if (nx)
      *nx = on ? sim->gt->nx : 0;
    if (ny)
      *ny = on ? sim->gt->ny : 0;
    if (tiles)
      *tiles = on ? sim->gt->tiles : 0;
    if (cell)
      *cell = on ? sim->gt->cell : 0.0;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_terrain_last(smpc_robot_sim * sim, double * normals_out, double * heights_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->gt || !sim->gt->active)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_read_terrain_last: no terrain, call smpc_robot_sim_set_terrain first");
    return guarded([&] { sim->gt->read_last(normals_out, heights_out); });
  }
  int smpc_robot_sim_get_terrain_last(smpc_robot_sim * sim, double ** normals_device, double ** heights_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    const bool on = sim->gt && sim->gt->active;
    if (normals_device)
      *normals_device = on ? sim->gt->n_last : nullptr;
    if (heights_device)
      *heights_device = on ? sim->gt->h_last : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_ground_terrain_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const smpc_terrain_settings * terrain,
                                             const double * mu, const double * push, int push_joint, const smpc_ground_solver_settings * settings,
                                             const double * lambda0, const smpc_joint_model_settings * model, const double * body, double * v_next_out,
                                             double * a_out, double * lambda_out, double * lambda_contact_out, double * gap_out, uint32_t * contact_out,
                                             int32_t * sweeps_out, double * residual_out, double * tau_applied_out, int32_t * stop_rows_out,
                                             double * lam_stop_out, int32_t * dropped_out, double * normals_out, double * heights_out)
  {
    if (!terrain)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_ground_terrain_dynamics: terrain is null");
    return ground_joint_body_dynamics("smpc_robot_sim_ground_terrain_dynamics", sim, n, X, tau, dt, nullptr, mu, push, push_joint, settings, lambda0, model, body,
                                      v_next_out, a_out, lambda_out, lambda_contact_out, gap_out, contact_out, sweeps_out, residual_out, tau_applied_out,
                                      stop_rows_out, lam_stop_out, dropped_out, terrain, normals_out, heights_out);
  }

  // ---- body points and the touch mask (smpc_sim_ground_joint_rt.h: sim_ground_points_rt_body / sim_ground_points_terrain_rt_body) ----
  int smpc_robot_sim_set_body_points(smpc_robot_sim * sim, const smpc_body_points_settings * points)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_set_body_points: no ground yet, call smpc_robot_sim_set_ground first");
    // admission before anything else: nothing is allocated, and the previous points stay
    const std::string why = sim_points_admission_error(sim->e->sz.nfeet, sim->g->gz.P, sim->e->sz.nq - 6, points);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    return guarded([&] {
      if (!sim->gp)
      {
        if (!points || points->n == 0) // (nothing to clear, nothing allocated)
          return;
        sim->gp.reset(new RobotSimGroundPoints(*sim->g));
      }
      sim->gp->set(points);
    });
  }
  int smpc_robot_sim_get_body_points_last(smpc_robot_sim * sim, int32_t ** body_slots_device, double ** lam_body_device, double ** body_gap_device,
                                          int32_t ** body_dropped_device, uint8_t ** body_touch_device)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    const bool on = sim->gp && sim->gp->active;
    if (body_slots_device)
      *body_slots_device = on ? sim->gp->own.slots : nullptr;
    if (lam_body_device)
      *lam_body_device = on ? sim->gp->own.lam : nullptr;
    if (body_gap_device)
      *body_gap_device = on ? sim->gp->own.gap : nullptr;
    if (body_dropped_device)
      *body_dropped_device = on ? sim->gp->own.dropped : nullptr;
    if (body_touch_device)
      *body_touch_device = on ? sim->gp->own.touch : nullptr;
    return SMPC_OK;
  }
  int smpc_robot_sim_read_body_points_last(smpc_robot_sim * sim, int32_t * body_slots_out, double * lam_body_out, double * body_gap_out,
                                           int32_t * body_dropped_out, uint8_t * body_touch_out)
  {
    if (!sim)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, "smpc_robot_sim_read_body_points_last: no ground yet, call smpc_robot_sim_set_ground first");
    if (!(sim->gp && sim->gp->active)) // (zeros while no points are set, without allocating)
      return guarded([&] {
        sim->e->wait();
        zero_body_points_outputs(sim->e->B, body_slots_out, lam_body_out, body_gap_out, body_dropped_out, body_touch_out);
      });
    return guarded([&] { sim->gp->read_last(body_slots_out, lam_body_out, body_gap_out, body_dropped_out, body_touch_out); });
  }
  int smpc_robot_sim_ground_points_dynamics(smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const smpc_terrain_settings * terrain,
                                            const double * plane, const double * mu, const double * push, int push_joint,
                                            const smpc_ground_solver_settings * settings, const double * lambda0, const smpc_joint_model_settings * model,
                                            const double * body, const smpc_body_points_settings * points, double * v_next_out, double * a_out,
                                            double * lambda_out, double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out,
                                            double * residual_out, double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out,
                                            int32_t * dropped_out, double * normals_out, double * heights_out, int32_t * body_slots_out,
                                            double * lam_body_out, double * body_gap_out, int32_t * body_dropped_out, uint8_t * body_touch_out)
  {
    return ground_joint_body_dynamics("smpc_robot_sim_ground_points_dynamics", sim, n, X, tau, dt, terrain ? nullptr : plane, mu, push, push_joint, settings,
                                      lambda0, model, body, v_next_out, a_out, lambda_out, lambda_contact_out, gap_out, contact_out, sweeps_out, residual_out,
                                      tau_applied_out, stop_rows_out, lam_stop_out, dropped_out, terrain, normals_out, heights_out, points, body_slots_out,
                                      lam_body_out, body_gap_out, body_dropped_out, body_touch_out);
  }
}

namespace
{
  int ground_joint_body_dynamics(const char * who, smpc_robot_sim * sim, int n, const double * X, const double * tau, double dt, const double * plane,
                                 const double * mu, const double * push, int push_joint, const smpc_ground_solver_settings * settings, const double * lambda0,
                                 const smpc_joint_model_settings * model, const double * body, double * v_next_out, double * a_out, double * lambda_out,
                                 double * lambda_contact_out, double * gap_out, uint32_t * contact_out, int32_t * sweeps_out, double * residual_out,
                                 double * tau_applied_out, int32_t * stop_rows_out, double * lam_stop_out, int32_t * dropped_out,
                                 const smpc_terrain_settings * terrain, double * normals_out, double * heights_out,
                                 const smpc_body_points_settings * points, int32_t * body_slots_out, double * lam_body_out, double * body_gap_out,
                                 int32_t * body_dropped_out, uint8_t * body_touch_out)
  {
    if (!sim || !X || !tau)
      return fail(SMPC_ERR_INVALID, "null argument");
    if (!sim->g)
      return fail(SMPC_ERR_INVALID, std::string(who) + ": no ground yet, call smpc_robot_sim_set_ground first");
    if (n < 1)
      return fail(SMPC_ERR_INVALID, "n must be positive");
    if (!(dt > 0.0) || !std::isfinite(dt))
      return fail(SMPC_ERR_INVALID, "dt must be positive");
    const smpc_ground_solver_settings inert = {0, 0.0, 0};
    const smpc_ground_solver_settings * st = settings ? settings : &inert;
    std::string why = sim_ground_ws_admission_error(sim->g->gs.sweeps, st);
    if (why.empty())
      why = sim_ground_env_admission_error(n, plane, mu);
    if (why.empty())
      why = sim_ground_push_admission_error(n, sim->e->sz.nq - 6, push_joint, push);
    if (why.empty())
      why = sim_joint_admission_error(n, sim->e->sz.na, sim->q_lo.data(), sim->q_hi.data(), model);
    if (why.empty())
      why = sim_body_admission_error(n, sim->e->sz.nq - 6, body);
    if (why.empty())
      why = sim_terrain_admission_error(n, terrain);
    if (why.empty())
      why = sim_points_admission_error(sim->e->sz.nfeet, sim->g->gz.P, sim->e->sz.nq - 6, points);
    if (!why.empty())
      return fail(SMPC_ERR_INVALID, why);
    const bool with_points = points != nullptr && points->n > 0;
    return guarded([&] {
      if (!sim->gj)
        sim->gj.reset(new RobotSimGroundJoint(*sim->g)); // (staging only: the handle's ground steps keep their kernel until the setter is called)
      SimTerrainDev view;
      if (terrain)
      {
        if (!sim->gt)
          sim->gt.reset(new RobotSimGroundTerrain(*sim->g)); // (staging only, likewise: the handle's own terrain is neither read nor changed)
        view = sim->gt->stage(n, terrain);
      }
      const double * body_dev = nullptr;
      if (body)
      {
        if (!sim->gb)
          sim->gb.reset(new RobotSimGroundBody(*sim->g)); // (staging only, likewise)
        body_dev = sim->gb->stage(n, body);
      }
      SimPointsDev pview;
      if (with_points)
      {
        if (!sim->gp)
          sim->gp.reset(new RobotSimGroundPoints(*sim->g)); // (staging only, likewise: the handle's own points are neither read nor changed)
        pview = sim->gp->stage(n, points);
      }
      sim->gj->dynamics(n, X, tau, dt, plane, mu, push, push_joint, sim_ground_ws_resolve(st), lambda0, model, sim->q_lo.data(), sim->q_hi.data(),
                        v_next_out, a_out, lambda_out, lambda_contact_out, gap_out, contact_out, sweeps_out, residual_out, tau_applied_out, stop_rows_out,
                        lam_stop_out, dropped_out, body_dev, terrain ? &view : nullptr, with_points ? &pview : nullptr);
      if (terrain)
        sim->gt->read_staged(n, normals_out, heights_out);
      if (with_points)
        sim->gp->read_staged(n, body_slots_out, lam_body_out, body_gap_out, body_dropped_out, body_touch_out);
      else
        zero_body_points_outputs(n, body_slots_out, lam_body_out, body_gap_out, body_dropped_out, body_touch_out);
    });
  }
} // namespace
