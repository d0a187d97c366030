// smpc_robot_check.h -- validation of a caller-filled robot table (include/smpc_robot.h) before an engine with a run-time joint tree
// (smpc_frontend_rt.h) allocates anything for it.  Plain C++ with no backend behind it, so that a stand-alone host program can exercise
// it (tests/cpp/robot_table_check.cpp).
#pragma once
#include "../../include/smpc_robot.h"
#include <cmath>
#include <cstdio>
#include <string>

namespace smpc
{
  // "" if the table describes a robot the run-time front end can evaluate, else one sentence that names the offending field.  Checked
  // in the order of the struct; nothing past njoints / nfeet entries is read.
  inline std::string robot_table_error(const smpc_robot_model * rm)
  {
    char b[160];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("robot table: ") + b;
    };
    if (rm->njoints < 2 || rm->njoints > SMPC_MAX_JOINTS)
      return say("njoints = %d is outside [2, %d]", rm->njoints, SMPC_MAX_JOINTS);
    const int nj = rm->njoints;
    if (rm->nq != nj + 6)
      return say("nq = %d, expected njoints + 6 = %d", rm->nq, nj + 6);
    if (rm->nv != nj + 5)
      return say("nv = %d, expected njoints + 5 = %d", rm->nv, nj + 5);
    if (rm->parent[0] != -1)
      return say("parent[0] = %d, expected -1 (joint 0 is the free-flyer)", rm->parent[0]);
    if (rm->jtype[0] != 0)
      return say("jtype[0] = %d, expected 0 (joint 0 is the free-flyer)", rm->jtype[0]);
    for (int j = 1; j < nj; j++)
    {
      if (rm->parent[j] < 0 || rm->parent[j] >= j)
        return say("parent[%d] = %d is outside [0, %d) (joints must be topologically ordered)", j, rm->parent[j], j);
      if (rm->jtype[j] < 1 || rm->jtype[j] > 3)
        return say("jtype[%d] = %d, expected 1, 2 or 3 (revolute X / Y / Z)", j, rm->jtype[j]);
    }
    auto finite = [](const double * v, int n) {
      for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i]))
          return false;
      return true;
    };
    double msum = 0.0;
    for (int j = 0; j < nj; j++)
    {
      if (!finite(rm->jp_R[j], 9))
        return say("jp_R[%d] is not finite", j);
      {
        // a placement is a rotation: R^T R = I (1e-9, the tolerance of total_mass below) and det R > 0
        const double * R = rm->jp_R[j];
        double dev = 0.0;
        for (int a = 0; a < 3; a++)
          for (int c = 0; c < 3; c++)
            dev = std::fmax(dev, std::fabs(R[a] * R[c] + R[3 + a] * R[3 + c] + R[6 + a] * R[6 + c] - (a == c ? 1.0 : 0.0)));
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(dev <= 1e-9) || !(det > 0.0))
          return say("jp_R[%d] is not a rotation (max |R^T R - I| = %.3g, det = %.3g)", j, dev, det);
      }
      if (!finite(rm->jp_p[j], 3))
        return say("jp_p[%d] is not finite", j);
      if (!std::isfinite(rm->mass[j]) || !(rm->mass[j] > 0.0))
        return say("mass[%d] is not a positive finite number", j);
      if (!finite(rm->com[j], 3))
        return say("com[%d] is not finite", j);
      if (!finite(rm->inertia[j], 6))
        return say("inertia[%d] is not finite", j);
      msum += rm->mass[j];
    }
    if (rm->nfeet < 1 || rm->nfeet > SMPC_MAX_FEET)
      return say("nfeet = %d is outside [1, %d]", rm->nfeet, SMPC_MAX_FEET);
    for (int f = 0; f < rm->nfeet; f++)
    {
      if (rm->foot_joint[f] < 0 || rm->foot_joint[f] >= nj)
        return say("foot_joint[%d] = %d is outside [0, %d)", f, rm->foot_joint[f], nj);
      if (!finite(rm->foot_p[f], 3))
        return say("foot_p[%d] is not finite", f);
      if (!finite(rm->foot_ref_p[f], 3))
        return say("foot_ref_p[%d] is not finite", f);
    }
    if (!finite(rm->q_ref, rm->nq))
      return say("q_ref is not finite");
    if (!finite(rm->q_lo, nj - 1))
      return say("q_lo is not finite");
    if (!finite(rm->q_hi, nj - 1))
      return say("q_hi is not finite");
    if (!std::isfinite(rm->total_mass) || !(std::fabs(rm->total_mass - msum) <= 1e-9 * msum))
      return say("total_mass = %.17g is not the sum of the masses %.17g (1e-9 relative)", rm->total_mass, msum);
    return std::string();
  }
} // namespace smpc
