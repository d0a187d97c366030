// smpc_sim_ground_dims.h -- host-side admission, defaults and sizes of the ground plane of the rigid-body simulator (smpc_sim_ground_rt.h):
// which smpc_ground_settings a simulator handle of `nfeet` feet accepts, the settings with their defaults filled in, the number of contact
// points and rows and the kernel instantiation they select.  Plain C++ with no backend behind it, so that a stand-alone host program can
// exercise it (tests/cpp/sim_ground_dims_check.cpp).
#pragma once
#include "../../include/smpc.h"
#include <cmath>
#include <cstdio>
#include <string>

namespace smpc
{
  constexpr int SIM_GROUND_MAX_POINTS = 8;                      // contact points of one robot: nfeet * points_per_foot
  constexpr int SIM_GROUND_MAX_ROWS = 3 * SIM_GROUND_MAX_POINTS; // 24
  constexpr int SIM_GROUND_MAX_PPF = 4;                          // points per foot

  struct SimGroundSizes
  {
    int P, npts, nrows, inst; // points per foot, nfeet P points, 3 rows each, kernel instantiation (12 or 24 rows)
  };
  // (arguments as admitted: 1 <= P <= 4, nfeet P <= 8)
  inline SimGroundSizes sim_ground_sizes(int nfeet, int P)
  {
    SimGroundSizes s;
    s.P = P;
    s.npts = nfeet * P;
    s.nrows = 3 * s.npts;
    s.inst = s.nrows <= 12 ? 12 : 24;
    return s;
  }

  // the settings as the kernel reads them: the defaults of include/smpc.h for arguments that are 0 (admitted settings have none below 0)
  struct SimGroundSettings
  {
    double ground_z, mu, erp, compliance;
    int sweeps, P;
    double points[SIM_GROUND_MAX_PPF][3];
  };
  inline SimGroundSettings sim_ground_resolve(const smpc_ground_settings * g)
  {
    SimGroundSettings s;
    s.ground_z = g->ground_z;
    s.mu = g->mu > 0.0 ? g->mu : 0.7;
    s.erp = g->erp > 0.0 ? g->erp : 0.2;
    s.compliance = g->compliance > 0.0 ? g->compliance : 1e-8;
    s.sweeps = g->sweeps > 0 ? g->sweeps : 30;
    const bool dflt = g->points_per_foot <= 0; // one point at the foot frame's origin
    s.P = dflt ? 1 : g->points_per_foot;
    for (int k = 0; k < SIM_GROUND_MAX_PPF; k++)
      for (int i = 0; i < 3; i++)
        s.points[k][i] = !dflt && k < s.P ? g->points[k][i] : 0.0;
    return s;
  }

  // "" if smpc_robot_sim_set_ground accepts these settings on a handle of `nfeet` feet, else one sentence that names the offending field.
  // Nothing is allocated before this has answered.  An argument that is 0 stands for its default (mu, erp, compliance, sweeps,
  // points_per_foot); a negative one is refused, so that what the kernel reads obeys mu > 0, 0 < erp <= 1, compliance > 0, sweeps >= 1,
  // 1 <= points_per_foot <= 4 and nfeet * points_per_foot <= 8 contact points (24 rows), every number finite.
  inline std::string sim_ground_admission_error(int nfeet, const smpc_ground_settings * g)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("ground settings: ") + b;
    };
    if (!std::isfinite(g->ground_z))
      return say("%s", "ground_z is not finite");
    if (!std::isfinite(g->mu))
      return say("%s", "mu is not finite (mu >= 0; 0 stands for the default 0.7)");
    if (g->mu < 0.0)
      return say("mu = %g is negative", g->mu);
    if (!std::isfinite(g->erp) || g->erp < 0.0 || g->erp > 1.0)
      return say("erp = %g is outside [0, 1]", g->erp);
    if (!std::isfinite(g->compliance))
      return say("%s", "compliance is not finite (compliance > 0; 0 stands for the default 1e-8)");
    if (g->compliance < 0.0)
      return say("compliance = %g is negative", g->compliance);
    if (g->sweeps < 0)
      return say("sweeps = %d is negative (sweeps >= 1; 0 stands for the default 30)", g->sweeps);
    if (g->points_per_foot < 0 || g->points_per_foot > SIM_GROUND_MAX_PPF)
      return say("points_per_foot = %d is outside [1, %d] (0 stands for one point at the foot frame's origin)", g->points_per_foot, SIM_GROUND_MAX_PPF);
    const int P = g->points_per_foot > 0 ? g->points_per_foot : 1;
    if (nfeet < 1 || nfeet * P > SIM_GROUND_MAX_POINTS)
      return say("nfeet * points_per_foot = %d * %d = %d is outside [1, %d] contact points", nfeet, P, nfeet * P, SIM_GROUND_MAX_POINTS);
    if (g->points_per_foot > 0)
      for (int k = 0; k < P; k++)
        for (int i = 0; i < 3; i++)
          if (!std::isfinite(g->points[k][i]))
            return say("points[%d][%d] is not finite", k, i);
    return std::string();
  }
} // namespace smpc
