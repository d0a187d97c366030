// smpc_sim_ground_ws_dims.h -- host-side admission, defaults and sizes of the warm-started ground contact solve with a stopping rule
// (smpc_sim_ground_ws_rt.h): which smpc_ground_solver_settings a handle whose ground runs `sweeps` sweeps accepts, the settings as the
// kernel reads them, the sizes of the warm buffer and of the per-robot read-outs, and the validation of a reset list.  Plain C++ with no
// backend behind it, so that a stand-alone host program can exercise it (tests/cpp/sim_ground_ws_dims_check.cpp).
#pragma once
#include "smpc_sim_ground_dims.h"
#include "smpc_reset_mask.h"

namespace smpc
{
  // the solver settings as the kernel reads them (admitted settings: tol >= 0 finite, 1 <= min_sweeps <= sweeps)
  struct SimGroundWsSettings
  {
    int warm_start; // 0 / 1
    double tol;     // m/s; 0: the stopping test is never made
    int min_sweeps; // 1 .. sweeps
  };
  inline SimGroundWsSettings sim_ground_ws_resolve(const smpc_ground_solver_settings * s)
  {
    SimGroundWsSettings r;
    r.warm_start = s->warm_start != 0 ? 1 : 0;
    r.tol = s->tol;
    r.min_sweeps = s->min_sweeps > 0 ? s->min_sweeps : 1;
    return r;
  }

  // bytes of the handle-owned buffers of B robots with `nrows` contact rows: the warm buffer [B][nrows] doubles, sweeps_used [B] int32,
  // residual [B] doubles
  struct SimGroundWsSizes
  {
    size_t warm_bytes, sweeps_bytes, residual_bytes;
  };
  inline SimGroundWsSizes sim_ground_ws_sizes(int B, int nrows)
  {
    SimGroundWsSizes z;
    z.warm_bytes = (size_t)B * (size_t)nrows * sizeof(double);
    z.sweeps_bytes = (size_t)B * sizeof(int);
    z.residual_bytes = (size_t)B * sizeof(double);
    return z;
  }

  // "" if these solver settings are accepted on a ground of `sweeps` sweeps (the resolved value, >= 1), else one sentence that names the
  // offending field.  Nothing is allocated before this has answered; a refused call leaves the previous settings in force.
  inline std::string sim_ground_ws_admission_error(int sweeps, const smpc_ground_solver_settings * s)
  {
    char b[200];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("ground solver settings: ") + b;
    };
    if (s->warm_start != 0 && s->warm_start != 1)
      return say("warm_start = %d is neither 0 nor 1", s->warm_start);
    if (!std::isfinite(s->tol))
      return say("%s", "tol is not finite (tol >= 0 m/s; 0 switches the stopping test off)");
    if (s->tol < 0.0)
      return say("tol = %g is negative", s->tol);
    if (s->min_sweeps < 0)
      return say("min_sweeps = %d is negative (1 .. sweeps; 0 stands for 1)", s->min_sweeps);
    if (s->min_sweeps > sweeps)
      return say("min_sweeps = %d exceeds the ground's sweeps = %d", s->min_sweeps, sweeps);
    return std::string();
  }

  // "" if the reset list idx[0 .. n) is accepted on a batch of B robots (n = 0: every robot; the list may be unsorted and may repeat an
  // index), else one sentence; on success mask[0 .. B) holds 1 for every robot to reset
  inline std::string sim_ground_ws_reset_error(const int * idx, int n, int B, unsigned char * mask)
  {
    char b[200];
    if (n < 0)
    {
      std::snprintf(b, sizeof(b), "ground warm start reset: n = %d is negative", n);
      return std::string(b);
    }
    if (n == 0)
    {
      for (int i = 0; i < B; i++)
        mask[i] = 1;
      return std::string();
    }
    if (!idx)
      return std::string("ground warm start reset: null index list");
    const int bad = reset_mask_from_list(idx, n, B, mask);
    if (bad >= 0)
    {
      std::snprintf(b, sizeof(b), "ground warm start reset: indices[%d] = %d is outside [0, %d]", bad, idx[bad], B - 1);
      return std::string(b);
    }
    return std::string();
  }
} // namespace smpc
