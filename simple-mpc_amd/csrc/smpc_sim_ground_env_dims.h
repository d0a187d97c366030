// smpc_sim_ground_env_dims.h -- host-side admission of the per-robot environment of the simulator's ground (smpc_sim_ground_env_rt.h): which
// planes [n][4] = (n, d), friction coefficients [n], pushes [n][6] = (f, o) and push joint a handle accepts from the host, and the contact
// frame of a plane as the kernel builds it.  Plain C++ with no backend behind it, so that a stand-alone host program can exercise it
// (tests/cpp/sim_ground_env_dims_check.cpp).
#pragma once
#include "smpc_sim_ground_dims.h"

namespace smpc
{
  constexpr int SIM_GROUND_ENV_DOUBLES = 11;      // per robot: plane 4, mu 1, push 6
  constexpr double SIM_GROUND_ENV_UNIT_TOL = 1e-9; // | |n| - 1 | of an admitted normal
  constexpr double SIM_GROUND_ENV_MIN_NZ = 0.5;    // n.z of an admitted normal (the frame divides by |e_y x n| = sqrt(n.x^2 + n.z^2) >= 0.5)

  // the contact frame of the unit normal n: t1 = (e_y x n) / |e_y x n|, t2 = n x t1, Rc = [t1 t2 n]; the identity for n = e_z
  inline void sim_ground_env_frame(const double * n, double * t1, double * t2)
  {
    const double cx = n[2], cz = -n[0]; // e_y x n = (n.z, 0, -n.x)
    const double inv = 1.0 / std::sqrt(cx * cx + cz * cz);
    t1[0] = cx * inv;
    t1[1] = 0.0;
    t1[2] = cz * inv;
    t2[0] = n[1] * t1[2] - n[2] * t1[1];
    t2[1] = n[2] * t1[0] - n[0] * t1[2];
    t2[2] = n[0] * t1[1] - n[1] * t1[0];
  }

  // "" if the host arrays plane [n][4] and mu [n] (either may be null: uniform) are admitted, else one sentence that names the field and the
  // robot.  Nothing is allocated before this has answered.
  inline std::string sim_ground_env_admission_error(int n, const double * plane, const double * mu)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("ground environment: ") + b;
    };
    if (n < 1)
      return say("n = %d robots (n >= 1)", n);
    if (plane)
      for (int i = 0; i < n; i++)
      {
        const double * p = plane + (size_t)i * 4;
        for (int k = 0; k < 4; k++)
          if (!std::isfinite(p[k]))
            return say("plane[%d][%d] of robot %d is not finite", i, k, i);
        const double len = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (!(std::fabs(len - 1.0) <= SIM_GROUND_ENV_UNIT_TOL))
          return say("plane[%d]: the normal of robot %d has length %.12g (a unit normal: | |n| - 1 | <= 1e-9)", i, i, len);
        if (!(p[2] >= SIM_GROUND_ENV_MIN_NZ))
          return say("plane[%d]: the normal of robot %d has n.z = %g (n.z >= 0.5)", i, i, p[2]);
      }
    if (mu)
      for (int i = 0; i < n; i++)
      {
        if (!std::isfinite(mu[i]))
          return say("mu[%d] of robot %d is not finite", i, i);
        if (!(mu[i] > 0.0))
          return say("mu[%d] = %g of robot %d is not positive", i, mu[i], i);
      }
    return std::string();
  }

  // the same for a push: push_joint in 0 .. njoints - 1 whether or not an array is given; push [n][6] (may be null: no push) finite
  inline std::string sim_ground_push_admission_error(int n, int njoints, int push_joint, const double * push)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("ground environment: ") + b;
    };
    if (n < 1)
      return say("n = %d robots (n >= 1)", n);
    if (push_joint < 0 || push_joint >= njoints)
      return say("push_joint = %d is outside [0, %d]", push_joint, njoints - 1);
    if (push)
      for (int i = 0; i < n; i++)
        for (int k = 0; k < 6; k++)
          if (!std::isfinite(push[(size_t)i * 6 + k]))
            return say("push[%d][%d] of robot %d is not finite", i, k, i);
    return std::string();
  }
} // namespace smpc
