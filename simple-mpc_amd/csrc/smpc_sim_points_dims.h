// smpc_sim_points_dims.h -- host-side admission, defaults and sizes of the simulator's body points (smpc_sim_ground_joint_rt.h:
// sim_ground_points_rt_body / sim_ground_points_terrain_rt_body): which smpc_body_points_settings a handle accepts, the free
// slots beside the foot points, the band with its default, and the sizes of the device copy and of the five read-outs.  Plain C++ with no
// backend behind it, so that a stand-alone host program can exercise it (tests/cpp/sim_points_dims_check.cpp).
#pragma once
#include "smpc_sim_ground_dims.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>

namespace smpc
{
  constexpr int SIM_POINTS_MAX = 16;                      // body points of a handle (shared by the batch)
  constexpr int SIM_POINTS_SLOTS = SIM_GROUND_MAX_POINTS; // the length of the per-robot slot read-outs: 8, whatever S is
  constexpr double SIM_POINTS_DEFAULT_BAND = 0.02;        // metres

  // S: the slots free beside the foot points (arguments as admitted by smpc_sim_ground_dims.h)
  inline int sim_points_free_slots(int nfeet, int P) { return SIM_GROUND_MAX_POINTS - nfeet * P; }
  inline double sim_points_band(double band) { return band > 0.0 ? band : SIM_POINTS_DEFAULT_BAND; }

  inline size_t sim_points_joint_bytes() { return (size_t)SIM_POINTS_MAX * sizeof(int); }
  inline size_t sim_points_offset_bytes() { return (size_t)SIM_POINTS_MAX * 3 * sizeof(double); }
  inline size_t sim_points_slots_bytes(int n) { return (size_t)n * SIM_POINTS_SLOTS * sizeof(int); }
  inline size_t sim_points_lam_bytes(int n) { return (size_t)n * SIM_POINTS_SLOTS * 3 * sizeof(double); }
  inline size_t sim_points_gap_bytes(int n) { return (size_t)n * SIM_POINTS_MAX * sizeof(double); }
  inline size_t sim_points_dropped_bytes(int n) { return (size_t)n * sizeof(int); }
  inline size_t sim_points_touch_bytes(int n) { return (size_t)n; }

  // "" if these body points are accepted on a handle of `nfeet` feet with P points per foot and `nj` joints, else one sentence that names
  // the field and the first offending index.  Null settings or n = 0 (no body points) are accepted.  Nothing is allocated before this has
  // answered; a refused call leaves the previous points in force.
  //   n in [0, 16]; S = 8 - nfeet P >= 1 free slots; joint[k] in [0, nj); offset[k] finite; band finite and >= 0 (0 stands for 0.02)
  inline std::string sim_points_admission_error(int nfeet, int P, int nj, const smpc_body_points_settings * s)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("body points: ") + b;
    };
    if (!s)
      return std::string();
    if (s->n < 0 || s->n > SIM_POINTS_MAX)
      return say("n = %d is outside [0, %d]", (int)s->n, SIM_POINTS_MAX);
    if (s->n == 0)
      return std::string();
    if (sim_points_free_slots(nfeet, P) < 1)
      return say("nfeet * points_per_foot = %d * %d = %d leaves no free slot of the %d contact points", nfeet, P, nfeet * P, SIM_GROUND_MAX_POINTS);
    if (!std::isfinite(s->band) || s->band < 0.0)
      return say("band = %g is not a finite number >= 0 (0 stands for the default %g)", s->band, SIM_POINTS_DEFAULT_BAND);
    for (int k = 0; k < s->n; k++)
    {
      if (s->joint[k] < 0 || s->joint[k] >= nj)
        return say("joint[%d] = %d is outside [0, %d)", k, (int)s->joint[k], nj);
      for (int i = 0; i < 3; i++)
        if (!std::isfinite(s->offset[k][i]))
          return say("offset[%d][%d] is not finite", k, i);
    }
    return std::string();
  }
} // namespace smpc
