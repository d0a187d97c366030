// smpc_sim_joint_dims.h -- host-side admission, defaults and sizes of the simulator's joint model (smpc_sim_ground_joint_rt.h):
// which smpc_joint_model_settings a handle accepts, the scalars as the kernel reads them, and the sizes of the model's arrays and of the
// per-robot read-outs.  Plain C++ with no backend behind it, so that a stand-alone host program can exercise it
// (tests/cpp/sim_joint_dims_check.cpp).
#pragma once
#include "smpc_sim_ground_dims.h"

namespace smpc
{
  constexpr int SIM_JOINT_MAX_STOPS = SMPC_JOINT_MAX_STOPS; // NJ: stop rows per robot and step
  constexpr double SIM_JOINT_DEFAULT_ACTIVATION = 0.1;     // rad
  constexpr double SIM_JOINT_DEFAULT_STOP_ERP = 0.2;

  // the scalars as the kernel reads them (admitted model: stops 0 / 1, activation > 0, stop_erp in (0, 1])
  struct SimJointScalars
  {
    int stops;
    double activation, stop_erp;
  };
  // (a null model is the inert one)
  inline SimJointScalars sim_joint_resolve(const smpc_joint_model_settings * m)
  {
    SimJointScalars r;
    r.stops = m && m->stops != 0 ? 1 : 0;
    r.activation = m && m->activation > 0.0 ? m->activation : SIM_JOINT_DEFAULT_ACTIVATION;
    r.stop_erp = m && m->stop_erp > 0.0 ? m->stop_erp : SIM_JOINT_DEFAULT_STOP_ERP;
    return r;
  }

  // bytes of the buffers of n robots with na actuated joints: one array of the model [n][na] doubles, tau_applied [n][na] doubles,
  // stop_rows [n][NJ] int32, lam_stop [n][NJ] doubles, dropped [n] int32
  struct SimJointSizes
  {
    size_t array_bytes, tau_bytes, rows_bytes, lam_bytes, dropped_bytes;
  };
  inline SimJointSizes sim_joint_sizes(int n, int na)
  {
    SimJointSizes z;
    z.array_bytes = (size_t)n * (size_t)na * sizeof(double);
    z.tau_bytes = (size_t)n * (size_t)na * sizeof(double);
    z.rows_bytes = (size_t)n * SIM_JOINT_MAX_STOPS * sizeof(int);
    z.lam_bytes = (size_t)n * SIM_JOINT_MAX_STOPS * sizeof(double);
    z.dropped_bytes = (size_t)n * sizeof(int);
    return z;
  }

  // "" if this joint model is accepted for n robots with na actuated joints whose table limits are tab_lo / tab_hi [na] (they stand in
  // for a null q_lo / q_hi), else one sentence that names the field and the first offending index (robot, joint; robot 0 for broadcast
  // arrays).  Nothing is allocated before this has answered; a refused call leaves the previous model in force.
  inline std::string sim_joint_admission_error(int n, int na, const double * tab_lo, const double * tab_hi, const smpc_joint_model_settings * m)
  {
    char b[240];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("joint model: ") + b;
    };
    if (!m)
      return std::string();
    if (m->stops != 0 && m->stops != 1)
      return say("stops = %d is neither 0 nor 1", m->stops);
    if (!(m->activation >= 0.0) || !std::isfinite(m->activation))
      return say("activation = %g is negative or not finite (rad, > 0; 0 stands for %g)", m->activation, SIM_JOINT_DEFAULT_ACTIVATION);
    if (!(m->stop_erp >= 0.0 && m->stop_erp <= 1.0))
      return say("stop_erp = %g is outside [0, 1] (0 stands for %g)", m->stop_erp, SIM_JOINT_DEFAULT_STOP_ERP);
    if (m->per_robot != 0 && m->per_robot != 1)
      return say("per_robot = %d is neither 0 nor 1", m->per_robot);
    const int rows = m->per_robot ? n : 1;
    for (int i = 0; i < rows; i++)
      for (int k = 0; k < na; k++)
      {
        const size_t at = (size_t)i * na + k;
        if (m->tau_max && !(m->tau_max[at] >= 0.0))
          return say("tau_max[%d][%d] = %g is negative or NaN (>= 0, +inf allowed)", i, k, m->tau_max[at]);
        if (m->damping && !(m->damping[at] >= 0.0 && std::isfinite(m->damping[at])))
          return say("damping[%d][%d] = %g is negative or not finite", i, k, m->damping[at]);
        if (m->armature && !(m->armature[at] >= 0.0 && std::isfinite(m->armature[at])))
          return say("armature[%d][%d] = %g is negative or not finite", i, k, m->armature[at]);
        const double lo = m->q_lo ? m->q_lo[at] : (tab_lo ? tab_lo[k] : -INFINITY);
        const double hi = m->q_hi ? m->q_hi[at] : (tab_hi ? tab_hi[k] : INFINITY);
        if (lo != lo)
          return say("q_lo[%d][%d] is NaN", i, k);
        if (hi != hi)
          return say("q_hi[%d][%d] is NaN", i, k);
        if (lo > hi)
          return say("q_lo[%d][%d] = %g exceeds q_hi[%d][%d] = %g", i, k, lo, i, k, hi);
      }
    return std::string();
  }
} // namespace smpc
