// smpc_reset.h -- reset of single instances of a batched MPC handle to its cold start (smpc_reset_instances, include/smpc.h).
//
// The constructor of every engine solves the default problem once and gives every instance that solution (reference src/mpc.cpp:72-89;
// StageEngine::cold_solve, CentEngine::cold_solve).  The engine keeps one instance's copy of it on the device (the segments below); a
// reset writes that copy over the solver state of the instances a device mask selects, relative to the current ring head.  Which buffer
// is solver state and which is problem data: DESIGN.md "Resetting single instances".
#pragma once
#include "smpc_model.h"

namespace smpc
{
  enum ResetKind
  {
    RESET_RING = 0, // dst [B][R][n] on the ring, src [R][n] in the order of the horizon (slot t of head 0)
    RESET_STAGE,    // dst [B][H][n] linear in t, src [H][n]
    RESET_INST      // dst [B][n], src [n]
  };
  struct ResetSeg
  {
    const double * src; // retained cold solution of one instance
    double * dst;       // the engine's buffer
    int n, kind;
  };
  constexpr int RESET_MAX_SEGS = 16;
  struct ResetArgs
  {
    const unsigned char * mask; // [B] (device): instances with a non-zero byte are reset
    int B, H, R, head;
    int nseg;
    ResetSeg seg[RESET_MAX_SEGS];
    int * ls_sel; // [B] line-search selection of the stage-wise engines (null: the engine has none)
    int ls_sel0;  // ... as the cold solve left it
  };

  // grid = B * R, 64 lanes: block = (instance, horizon node t).  A block of an instance that is not selected returns at once.  The lanes
  // run along the contiguous doubles of the node, loads first, then the stores; the per-instance segments go with the block of t = 0.
  SMPC_DEV void reset_body(const ResetArgs & ka, int block)
  {
    constexpr int NT = 64, NV = 4;
    const int inst = block / ka.R, t = block - inst * ka.R;
    if (ka.mask[inst] == 0)
      return;
    const int slot = ring_slot(ka.head, t, ka.R);
    for (int s = 0; s < ka.nseg; s++)
    {
      const ResetSeg & sg = ka.seg[s];
      const int n = sg.n;
      const double * src = sg.src + (size_t)t * n;
      double * dst;
      if (sg.kind == RESET_RING)
        dst = sg.dst + ((size_t)inst * ka.R + slot) * n;
      else if (sg.kind == RESET_STAGE)
      {
        if (t >= ka.H)
          continue;
        dst = sg.dst + ((size_t)inst * ka.H + t) * n;
      }
      else
      {
        if (t != 0)
          continue;
        dst = sg.dst + (size_t)inst * n;
      }
      SMPC_LANES(NT)
      for (int i0 = lane; i0 < n; i0 += NT * NV)
      {
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; k++)
          if (i0 + k * NT < n)
            v[k] = src[i0 + k * NT];
#pragma unroll
        for (int k = 0; k < NV; k++)
          if (i0 + k * NT < n)
            dst[i0 + k * NT] = v[k];
      }
      SMPC_LANES_END_WAVE
    }
    if (t == 0 && ka.ls_sel != nullptr)
    {
      SMPC_LANES(NT)
      if (lane == 0)
        ka.ls_sel[inst] = ka.ls_sel0;
      SMPC_LANES_END_WAVE
    }
  }

  // the retained cold solution: one device block, and the plan of the kernel that writes it back
  struct ColdSolution
  {
    double * dev = nullptr; // owned by the engine (released with its buffers)
    size_t doubles = 0, used = 0;
    ResetArgs plan{};
    void begin(int B, int H, int R, size_t total)
    {
      plan = ResetArgs{};
      plan.B = B;
      plan.H = H;
      plan.R = R;
      doubles = total;
      used = 0;
      dev = (double *)dev_alloc(total * sizeof(double));
    }
    // instance 0 of `buf` (null: the problem has no such buffer) as it is now -> the next segment
    void retain(double * buf, int n, ResetKind kind, stream_t st)
    {
      if (buf == nullptr || n == 0)
        return;
      const size_t len = (size_t)n * (kind == RESET_RING ? plan.R : (kind == RESET_STAGE ? plan.H : 1));
      if (plan.nseg >= RESET_MAX_SEGS || used + len > doubles)
        throw std::runtime_error("internal: the retained cold solution does not fit its block");
      d2d(dev + used, buf, len * sizeof(double), st);
      plan.seg[plan.nseg++] = ResetSeg{dev + used, buf, n, (int)kind};
      used += len;
    }
  };
} // namespace smpc
