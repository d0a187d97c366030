// smpc_frontend_rt.h -- the state front end on a RUN-TIME joint tree: what RobotDataHandler::updateInternalData(x, false) +
// getCentroidalState provide for a measured multibody state (reference src/robot-handler.cpp:106-127, 142-149) -- foot positions,
// centre of mass, centroidal momentum, centroidal state [com; h_lin; h_ang] -- for any robot table of include/smpc_robot.h with up to
// SMPC_MAX_JOINTS joints.  Joint count, parents, axis types and feet are DATA of the device table: one code object serves every robot
// (frontend_body<D> / frontend_full_body<DF> are shaped around a compile-time joint count and serve the stage kernels of their engines).
//
// Shape: one wavefront per instance, lane = joint, as the two templated front ends.  The tree pass is a chain of at most `nlevels`
// dependent steps per instance whatever the form; a lane-per-instance kernel would walk all joints serially in every lane with the 18
// doubles of every ancestor placement live per lane, and would read X with a stride of nx doubles between lanes.  Here the joint-local
// work (sincos, jpR Rq) and the body momenta run once for all joints side by side, X is read as one contiguous run, and 64 instances
// are 64 independent blocks for the scheduler.
//   phase 0   global loads: the lane's joint constants and tree entries -> registers, the state -> LDS; joint-local rotation
//   phase 1   root -> leaf, one step per tree level: placement and spatial velocity (about the world origin) from the parent's
//   phase 2   body momentum h_j = I_j v_j, m_j, m_j c_j -> LDS ; feet (lanes 32 .. 32 + nfeet - 1)
//   phase 3   lanes 0 .. 9: sums over the joints in ascending order (the oracle's composite sums, in lane-parallel form)
//   phase 4   com = sum(m c) / sum(m), h_ang about the CoM; stores
// All global loads are issued in phase 0, all global stores in phase 4.  LDS is sized by SMPC_MAX_JOINTS.
#pragma once
#include "../../include/smpc_robot.h"
#include "smpc_math.h"
#include <stdexcept>

namespace smpc
{
  struct RtDims // tag of CentEngine's front-end parameter: the joint tree is data (nq, nv are members of the engine)
  {
  };

  // the robot table as the kernel reads it (device resident, one copy per handle)
  struct RtDevModel
  {
    double jpR[SMPC_MAX_JOINTS][9];
    double jpp[SMPC_MAX_JOINTS][3];
    double mass[SMPC_MAX_JOINTS];
    double com[SMPC_MAX_JOINTS][3];
    double inertia[SMPC_MAX_JOINTS][6];
    double foot_p[SMPC_MAX_FEET][3];
    int parent[SMPC_MAX_JOINTS];
    int jtype[SMPC_MAX_JOINTS];
    int level[SMPC_MAX_JOINTS]; // depth in the tree (joint 0: 0)
    int foot_joint[SMPC_MAX_FEET];
    int njoints, nfeet, nlevels, pad_;
  };

  // robot table -> device table; the table has passed robot_table_error (smpc_robot_check.h)
  inline void fill_rt_model(const smpc_robot_model * rm, RtDevModel & m)
  {
    if (rm->njoints < 1 || rm->njoints > SMPC_MAX_JOINTS || rm->nfeet < 0 || rm->nfeet > SMPC_MAX_FEET)
      throw std::runtime_error("robot table: njoints / nfeet outside the table's bounds");
    std::memset(&m, 0, sizeof(m));
    m.njoints = rm->njoints;
    m.nfeet = rm->nfeet;
    int maxlev = 0;
    for (int j = 0; j < rm->njoints; j++)
    {
      if (j > 0 && (rm->parent[j] < 0 || rm->parent[j] >= j))
        throw std::runtime_error("robot joints must be topologically ordered");
      m.parent[j] = j == 0 ? 0 : rm->parent[j];
      m.jtype[j] = rm->jtype[j];
      m.level[j] = j == 0 ? 0 : m.level[rm->parent[j]] + 1;
      maxlev = m.level[j] > maxlev ? m.level[j] : maxlev;
      for (int i = 0; i < 9; i++)
        m.jpR[j][i] = rm->jp_R[j][i];
      for (int i = 0; i < 3; i++)
      {
        m.jpp[j][i] = rm->jp_p[j][i];
        m.com[j][i] = rm->com[j][i];
      }
      m.mass[j] = rm->mass[j];
      for (int i = 0; i < 6; i++)
        m.inertia[j][i] = rm->inertia[j][i];
    }
    m.nlevels = maxlev + 1;
    for (int f = 0; f < rm->nfeet; f++)
    {
      if (rm->foot_joint[f] < 0 || rm->foot_joint[f] >= rm->njoints)
        throw std::runtime_error("robot table: foot_joint out of range");
      m.foot_joint[f] = rm->foot_joint[f];
      for (int i = 0; i < 3; i++)
        m.foot_p[f][i] = rm->foot_p[f][i];
    }
  }

  struct FrontendRtArgs
  {
    const RtDevModel * model;
    const double * X;                 // [B][nx] measured states (device), nx = nq + nv = 2 njoints + 11
    double *feet, *com, *hg, *cstate; // [B][nfeet*3], [B][3], [B][6], [B][9] (device), any may be null
  };

  struct FrontendRtScratch
  {
    double x[2 * SMPC_MAX_JOINTS + 11];
    double oR[SMPC_MAX_JOINTS * 9]; // world placement of every joint
    double op[SMPC_MAX_JOINTS * 3];
    double vel[SMPC_MAX_JOINTS * 6];  // spatial velocity [linear; angular] about the world origin
    double body[SMPC_MAX_JOINTS * 10]; // m | m c | h_lin | h_ang (about the world origin) of every body
    double sum[10];
    double footp[SMPC_MAX_FEET * 3];
  };

  // grid = B, 64 lanes
  SMPC_DEV void frontend_rt_body(const FrontendRtArgs & ka, int block)
  {
    constexpr int NT = 64, MAXJ = SMPC_MAX_JOINTS, MAXF = SMPC_MAX_FEET;
    static_assert(MAXJ <= 32 && MAXF <= 32, "lane = joint below 32, lane - 32 = foot");
    const int inst = block;
    const RtDevModel & mg = *ka.model;
    // (wave-uniform: scalar loads; clamped so that no table entry can index outside the LDS arrays)
    const int nj = mg.njoints < MAXJ ? mg.njoints : MAXJ;
    const int nf = mg.nfeet < MAXF ? mg.nfeet : MAXF;
    const int nlev = mg.nlevels < MAXJ ? mg.nlevels : MAXJ;
    const int nq = nj + 6, nx = 2 * nj + 11;
    SMPC_LDS(FrontendRtScratch, scs, 1);
    FrontendRtScratch & sc = scs[0];
    SMPC_PLA(double, jg, NT, 22); // jpR 0..8 | jpp 9..11 | mass 12 | com 13..15 | inertia 16..21 of this lane's joint
    SMPC_PLA(double, fp, NT, 3);  // foot_p of this lane's foot (lanes 32 ..)
    SMPC_PL(int, par, NT);
    SMPC_PL(int, jt, NT);
    SMPC_PL(int, lev, NT);
    SMPC_PL(int, fj, NT);
    // ---- phase 0: every global load ----
    SMPC_LANES(NT)
    {
      const int j = lane < nj ? lane : 0;
#pragma unroll
      for (int i = 0; i < 9; i++)
        SMPC_PLV(jg)[i] = mg.jpR[j][i];
#pragma unroll
      for (int i = 0; i < 3; i++)
      {
        SMPC_PLV(jg)[9 + i] = mg.jpp[j][i];
        SMPC_PLV(jg)[13 + i] = mg.com[j][i];
      }
      SMPC_PLV(jg)[12] = mg.mass[j];
#pragma unroll
      for (int i = 0; i < 6; i++)
        SMPC_PLV(jg)[16 + i] = mg.inertia[j][i];
      const int p = mg.parent[j];
      SMPC_PLV(par) = p >= 0 && p < nj ? p : 0;
      SMPC_PLV(jt) = mg.jtype[j];
      SMPC_PLV(lev) = mg.level[j];
      const int f = lane >= 32 && lane < 32 + nf ? lane - 32 : 0;
      const int q = mg.foot_joint[f];
      SMPC_PLV(fj) = q >= 0 && q < nj ? q : 0;
#pragma unroll
      for (int i = 0; i < 3; i++)
        SMPC_PLV(fp)[i] = mg.foot_p[f][i];
      for (int i = lane; i < nx; i += NT)
        sc.x[i] = ka.X[(size_t)inst * nx + i];
    }
    SMPC_LANES_END_WAVE
    const double * vq = &sc.x[nq];
    SMPC_LANES(NT)
    if (lane < nj)
    {
      const int j = lane;
      if (j == 0)
      {
        const M3 R = quat_to_R(Quat{sc.x[3], sc.x[4], sc.x[5], sc.x[6]});
        const V3 p = ld3(sc.x);
        // free-flyer: v[0:6] = [v; w] in the local frame
        const V3 w = R * ld3(vq + 3);
        const V3 v = R * ld3(vq) + cross(p, w);
        stm3(&sc.oR[0], R);
        st3(&sc.op[0], p);
        stsv(&sc.vel[0], SV{v, w});
      }
      else
      {
        double s, c;
        sincos(sc.x[6 + j], &s, &c);
        const int t = SMPC_PLV(jt);
        const M3 Rq = t == 1 ? M3{1, 0, 0, 0, c, -s, 0, s, c} : (t == 2 ? M3{c, 0, s, 0, 1, 0, -s, 0, c} : M3{c, -s, 0, s, c, 0, 0, 0, 1});
        stm3(&sc.oR[j * 9], ldm3(&SMPC_PLV(jg)[0]) * Rq); // (joint-local until the joint's level is reached)
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 1: root -> leaf ----
    for (int lvl = 1; lvl < nlev; lvl++)
    {
      SMPC_LANES(NT)
      if (lane > 0 && lane < nj && SMPC_PLV(lev) == lvl)
      {
        const int j = lane, pj = SMPC_PLV(par);
        const M3 Rp = ldm3(&sc.oR[pj * 9]);
        const M3 R = Rp * ldm3(&sc.oR[j * 9]);
        const V3 p = ld3(&sc.op[pj * 3]) + Rp * ld3(&SMPC_PLV(jg)[9]);
        const int col = SMPC_PLV(jt) - 1;
        const V3 ax = col == 0 ? mk3(R.a00, R.a10, R.a20) : (col == 1 ? mk3(R.a01, R.a11, R.a21) : mk3(R.a02, R.a12, R.a22));
        const SV sk = SV{cross(p, ax), ax};
        stm3(&sc.oR[j * 9], R);
        st3(&sc.op[j * 3], p);
        stsv(&sc.vel[j * 6], ldsv(&sc.vel[pj * 6]) + vq[j + 5] * sk);
      }
      SMPC_LANES_END_WAVE
    }
    // ---- phase 2: body momenta about the world origin; feet ----
    SMPC_LANES(NT)
    if (lane < nj)
    {
      const int j = lane;
      const M3 R = ldm3(&sc.oR[j * 9]);
      const V3 p = ld3(&sc.op[j * 3]);
      const SV v = ldsv(&sc.vel[j * 6]);
      const double m = SMPC_PLV(jg)[12];
      const V3 c = R * ld3(&SMPC_PLV(jg)[13]) + p;
      const double * il = &SMPC_PLV(jg)[16];
      const M3 Il = M3{il[0], il[1], il[3], il[1], il[2], il[4], il[3], il[4], il[5]};
      const M3 Iw = R * Il * transpose(R);
      const double cc = dot(c, c);
      SI I;
      I.m = m;
      I.mc = m * c;
      I.jxx = Iw.a00 + m * (cc - c.x * c.x);
      I.jxy = Iw.a01 - m * c.x * c.y;
      I.jxz = Iw.a02 - m * c.x * c.z;
      I.jyy = Iw.a11 + m * (cc - c.y * c.y);
      I.jyz = Iw.a12 - m * c.y * c.z;
      I.jzz = Iw.a22 + m * (cc - c.z * c.z);
      double * o = &sc.body[j * 10];
      o[0] = m;
      st3(o + 1, I.mc);
      stsv(o + 4, I * v);
    }
    else if (lane >= 32 && lane < 32 + nf)
    {
      const int f = lane - 32, j = SMPC_PLV(fj);
      st3(&sc.footp[f * 3], ldm3(&sc.oR[j * 9]) * ld3(SMPC_PLV(fp)) + ld3(&sc.op[j * 3]));
    }
    SMPC_LANES_END_WAVE
    // ---- phase 3: sums over the joints, one entry per lane ----
    SMPC_LANES(NT)
    if (lane < 10)
    {
      double s = 0.0;
      for (int j = 0; j < nj; j++)
        s += sc.body[j * 10 + lane];
      sc.sum[lane] = s;
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: centroidal quantities; every global store ----
    SMPC_LANES(NT)
    {
      const V3 com = (1.0 / sc.sum[0]) * ld3(&sc.sum[1]);
      const V3 hl = ld3(&sc.sum[4]);
      const V3 ha = ld3(&sc.sum[7]) - cross(com, hl);
      const int k = lane < 9 ? lane : 0;
      const double cst = k < 3 ? v3c(com, k) : (k < 6 ? v3c(hl, k - 3) : v3c(ha, k - 6));
      if (ka.feet != nullptr && lane < nf * 3)
        ka.feet[(size_t)inst * nf * 3 + lane] = sc.footp[lane];
      if (ka.com != nullptr && lane < 3)
        ka.com[(size_t)inst * 3 + lane] = cst;
      if (ka.hg != nullptr && lane < 6)
        ka.hg[(size_t)inst * 6 + lane] = lane < 3 ? v3c(hl, lane) : v3c(ha, lane - 3);
      if (ka.cstate != nullptr && lane < 9)
        ka.cstate[(size_t)inst * 9 + lane] = cst;
    }
    SMPC_LANES_END_WAVE
  }
} // namespace smpc
