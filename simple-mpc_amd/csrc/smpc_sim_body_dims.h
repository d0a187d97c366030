// smpc_sim_body_dims.h -- host-side admission, layout and sizes of the simulator's per-robot body parameters (smpc_sim_ground_joint_rt.h:
// sim_ground_body_rt_body): which body[n][njoints][10] a handle accepts, the rows of a robot table in that layout, and the
// size of the array.  Plain C++ with no backend behind it, so that a stand-alone host program can exercise it
// (tests/cpp/sim_body_dims_check.cpp).
#pragma once
#include "../../include/smpc_robot.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>

namespace smpc
{
  constexpr int SIM_BODY_ROW = 10; // mass | com x y z | Ixx Ixy Iyy Ixz Iyz Izz: mass[j], com[j], inertia[j] of smpc_robot.h in that order

  inline size_t sim_body_bytes(int n, int njoints) { return (size_t)n * (size_t)njoints * SIM_BODY_ROW * sizeof(double); }

  // the rows [njoints][10] of a robot table
  inline void sim_body_table_rows(const smpc_robot_model * rm, double * out)
  {
    for (int j = 0; j < rm->njoints; j++)
    {
      double * r = out + (size_t)j * SIM_BODY_ROW;
      r[0] = rm->mass[j];
      for (int i = 0; i < 3; i++)
        r[1 + i] = rm->com[j][i];
      for (int i = 0; i < 6; i++)
        r[4 + i] = rm->inertia[j][i];
    }
  }

  // "" if body[n][njoints][10] is accepted, else one sentence that names the field and the first offending [robot][joint].  A row is
  // admitted exactly when a robot table carrying it would pass smpc_robot_check.h: mass finite and > 0, com finite, inertia finite.  A null
  // array (no body parameters: the table's) is accepted.  Nothing is allocated before this has answered; a refused call leaves the
  // previous parameters in force.
  inline std::string sim_body_admission_error(int n, int njoints, const double * body)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("body parameters: ") + b;
    };
    if (!body)
      return std::string();
    for (int i = 0; i < n; i++)
      for (int j = 0; j < njoints; j++)
      {
        const double * r = body + ((size_t)i * njoints + j) * SIM_BODY_ROW;
        if (!std::isfinite(r[0]) || !(r[0] > 0.0))
          return say("mass[%d][%d] = %g is not a positive finite number", i, j, r[0]);
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(r[1 + k]))
            return say("com[%d][%d] is not finite", i, j);
        for (int k = 0; k < 6; k++)
          if (!std::isfinite(r[4 + k]))
            return say("inertia[%d][%d] is not finite", i, j);
      }
    return std::string();
  }
} // namespace smpc
