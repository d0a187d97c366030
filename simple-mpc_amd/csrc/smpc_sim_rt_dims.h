// smpc_sim_rt_dims.h -- host-side sizes and admission of the stand-alone rigid-body simulator on a RUN-TIME joint tree (smpc_sim_rt.h):
// which (robot table, contact size, batch) a simulator handle is built for, and the sizes of its buffers.  Plain C++ with no backend behind
// it, so that a stand-alone host program can exercise it (tests/cpp/sim_rt_dims_check.cpp).
#pragma once
#include "smpc_robot_check.h"

namespace smpc
{
  constexpr int SIM_RT_MAX_NV = SMPC_MAX_JOINTS + 5; // 37
  constexpr int SIM_RT_MAX_ROWS = 12;                // contact rows of one robot: 4 point contacts or 2 flat ones

  struct SimRtSizes
  {
    int nq, nv, nx, na, nfeet, fs, nlam; // nx = nq + nv ; na = nv - 6 joint torques ; nlam = fs nfeet entries of lambda per robot
  };
  inline SimRtSizes sim_rt_sizes(int njoints, int nfeet, int force_size)
  {
    SimRtSizes s;
    s.nq = njoints + 6;
    s.nv = njoints + 5;
    s.nx = s.nq + s.nv;
    s.na = s.nv - 6;
    s.nfeet = nfeet;
    s.fs = force_size;
    s.nlam = force_size * nfeet;
    return s;
  }

  // "" if smpc_robot_sim_create builds a handle for these arguments, else one sentence that names the offending field.  Nothing is allocated
  // before this has answered.  force_size 3: point contacts (CONTACT_3D, LOCAL), 1 .. SMPC_MAX_FEET feet; force_size 6: flat contacts
  // (CONTACT_6D, LOCAL_WORLD_ALIGNED), 1 .. 2 feet -- a robot never has more than SIM_RT_MAX_ROWS contact rows (four 6-D contacts on a
  // quadruped over-constrain its legs: the Delassus matrix is singular up to the proximal damping).
  inline std::string sim_rt_admission_error(const smpc_robot_model * rm, int force_size, int batch)
  {
    char b[200];
    if (force_size != 3 && force_size != 6)
    {
      std::snprintf(b, sizeof(b), "force_size = %d, the simulator builds contacts of size 3 (point feet) or 6 (flat feet)", force_size);
      return b;
    }
    if (batch < 1)
    {
      std::snprintf(b, sizeof(b), "batch = %d must be positive", batch);
      return b;
    }
    const std::string why = robot_table_error(rm);
    if (!why.empty())
      return why;
    const int maxf = force_size == 6 ? SIM_RT_MAX_ROWS / 6 : SMPC_MAX_FEET;
    if (rm->nfeet < 1 || rm->nfeet > maxf)
    {
      std::snprintf(b, sizeof(b), "robot table: nfeet = %d is outside [1, %d] for force_size %d (at most %d contact rows per robot)", rm->nfeet, maxf,
                    force_size, SIM_RT_MAX_ROWS);
      return b;
    }
    return std::string();
  }
} // namespace smpc
