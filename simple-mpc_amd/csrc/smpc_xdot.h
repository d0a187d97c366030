// smpc_xdot.h -- retained state derivatives of EVERY stage of the horizon (MPC::getStateDerivative(t), reference src/mpc.cpp:346-352:
// the continuous dynamics xdot_t = f(x_t, u_t) the solver evaluated at the accepted iterate, `Et.ev[t].xdot`).
//
// The solver kernels keep xdot of stages 0 and 1 only (xdot01, written by the accepting line search).  When a handle retains the state
// derivatives (smpc_set_retain_state_derivatives), one launch of xdot_all_body after the solve re-evaluates f at the returned xs[t], us[t] of
// every (instance, stage) pair, with the stage's contact mask and the parameters the solve saw, into out[B][H][dim]:
//   XD_KINO_LANE  kinodynamics, lane = (instance, stage): the tree pass of lane_tree_body (joint placements, velocities, bias accelerations,
//                 world inertias, totals at the root) and the closed-form base acceleration; dim = 2 NV, [v ; a_base, u_joint_acc]
//   XD_KINO_WAVE  the same for robots the lane pass does not take (DevModel::lane_slots = 0): kino_tree_phases, one wavefront per pair
//   XD_FULL       dense engines (full dynamics, and the kinodynamics variant of 6-D feet): full_dynamics_phases -- the constrained forward
//                 dynamics with the stage's contacts, Baumgarte terms and the proximal settings of record -- one wavefront per pair, as
//                 fdyn_trial_body; dim = 2 NV, [v ; a]
//   XD_CENT       centroidal, lane = (instance, stage): [h / m ; m g + sum f ; sum (p - c) x f (+ tau of 6-D feet)]; dim = 9
// Nothing here is shared with the solver's kernels: the tuned stage kernels are untouched, and a handle that does not retain pays nothing.
#pragma once
#include "smpc_cent_kernels.h"
#include "smpc_full_stage.h"
#include "smpc_kino_lane.h"

namespace smpc
{
  enum XdotKind
  {
    XD_KINO_LANE = 0,
    XD_KINO_WAVE = 1,
    XD_FULL = 2,
    XD_CENT = 3
  };
  template <class BUF>
  struct XdotArgs
  {
    BUF b;       // xs, us (rings), stages, model; centroidal: foot (contact positions [B][H][NF][3])
    int head;    // ring head of the solve
    double * out; // [B][H][dim]
  };

  // ---- kinodynamics, lane = instance of a block of 64 at one stage; grid = H * ceil(B / 64) ----
  template <class D, int NSLOT>
  SMPC_DEV void xdot_kino_lane(const XdotArgs<Buffers<D>> & ka, int block)
  {
    typedef LaneStage<D> ST;
    constexpr int NT = 64, NX = D::NX, NU = D::NU, NF = D::NF, NV = D::NV, NJ = D::NJ, NQ = D::NQ, NO = 2 * NV;
    static_assert(NQ == NV + 1 && NX <= NT && NU <= NT && NO <= NT, "one element per lane");
    static_assert(NX + NU >= NO, "the outputs are parked in the rows of the staged inputs");
    const Buffers<D> & b = ka.b;
    const int H = b.H, R = b.R;
    const int t = block % H, g = block / H;
    const int base = g * NT, np = b.B - base < NT ? b.B - base : NT;
    const unsigned mask = b.stages[t].mask;
    const int st = ring_slot(ka.head, t, R);
    const DevModel<D> & mg = *b.model;
    SMPC_LDS(double, stg, (NX + NU) * LANE_PAD); // row f, column p: element f of [x | u] of problem p; then the outputs in rows 0 .. NO-1
    SMPC_LDS(LaneModel<D>, lms, 1);
    LaneModel<D> & lm = lms[0];
    // ---- model constants and the inputs of the 64 problems (lane = element: coalesced runs, transposed into LDS) ----
    SMPC_LANES(NT)
    {
      for (int i = lane; i < NJ * 9; i += NT)
        lm.jpR[i / 9][i % 9] = mg.jpR[i / 9][i % 9];
      for (int i = lane; i < NJ * 6; i += NT)
        lm.inertia[i / 6][i % 6] = mg.inertia[i / 6][i % 6];
      for (int i = lane; i < NJ * 3; i += NT)
      {
        lm.jpp[i / 3][i % 3] = mg.jpp[i / 3][i % 3];
        lm.com[i / 3][i % 3] = mg.com[i / 3][i % 3];
      }
      if (lane < NJ)
      {
        lm.mass[lane] = mg.mass[lane];
        lm.jtype[lane] = mg.jtype[lane];
        lm.par_slot[lane] = mg.par_slot[lane];
        lm.save_slot[lane] = mg.save_slot[lane];
      }
      if (lane < NF * 3)
        lm.foot_p[lane / 3][lane % 3] = mg.foot_p[lane / 3][lane % 3];
      if (lane < NF)
        lm.foot_joint[lane] = mg.foot_joint[lane];
      constexpr int SB = 16; // problems per batch of loads (issued back to back, then committed)
      const int lx = lane < NX ? lane : 0, lu = lane < NU ? lane : 0;
      for (int p0 = 0; p0 < np; p0 += SB)
      {
        double vx[SB], vu[SB];
#pragma unroll
        for (int q = 0; q < SB; q++)
        {
          const int p = p0 + q < np ? p0 + q : np - 1;
          const size_t sl = (size_t)(base + p) * R + st;
          vx[q] = b.xs[sl * NX + lx];
          vu[q] = b.us[sl * NU + lu];
        }
#pragma unroll
        for (int q = 0; q < SB; q++)
          if (p0 + q < np)
          {
            if (lane < NX)
              stg[lane * LANE_PAD + p0 + q] = vx[q];
            if (lane < NU)
              stg[(NX + lane) * LANE_PAD + p0 + q] = vu[q];
          }
      }
    }
    SMPC_LANES_END_WAVE
    const double total_mass = mg.total_mass;
    const V3 gravity = ld3(mg.gravity);
    // ---- lane = problem: the tree pass of lane_tree_body (evaluation mode, no step) down to the base acceleration ----
    SMPC_LANES(NT)
    if (lane < np)
    {
      auto SX = [&](int i) { return stg[i * LANE_PAD + lane]; };
      auto SU = [&](int i) { return stg[(NX + i) * LANE_PAD + lane]; };
      double xb[7], vb[6];
#pragma unroll
      for (int i = 0; i < 7; i++)
        xb[i] = SX(i);
#pragma unroll
      for (int k = 0; k < 6; k++)
        vb[k] = SX(NQ + k);
      LaneJoint cur, slot[NSLOT];
      SI Itot;
      SV Ftot;
      const M3 R0 = quat_to_R(Quat{xb[3], xb[4], xb[5], xb[6]});
      const V3 p0 = mk3(xb[0], xb[1], xb[2]);
      V3 fsum = mk3(0, 0, 0), msum = mk3(0, 0, 0); // sum of the contact forces, sum of p_f x F_f
#pragma unroll 1
      for (int j = 0; j < NJ; j++)
      {
        if (j == 0)
        {
          cur.R = R0;
          cur.p = p0;
          cur.v = sv0();
#pragma unroll
          for (int k = 0; k < 6; k++)
          {
            const V3 ax = m3_col(R0, k % 3);
            const SV sk = k < 3 ? SV{ax, mk3(0, 0, 0)} : SV{cross(p0, ax), ax};
            cur.v = cur.v + vb[k] * sk;
          }
          cur.a = sv0();
        }
        else
        {
          const int ps = lm.par_slot[j];
#pragma unroll
          for (int s = 0; s < NSLOT; s++)
            if (ps == s)
              cur = slot[s];
          double sn_, cs_;
          sincos(SX(7 + j - 1), &sn_, &cs_);
          const int jt = lm.jtype[j];
          const M3 Rq = jt == 1 ? M3{1, 0, 0, 0, cs_, -sn_, 0, sn_, cs_}
                                : (jt == 2 ? M3{cs_, 0, sn_, 0, 1, 0, -sn_, 0, cs_} : M3{cs_, -sn_, 0, sn_, cs_, 0, 0, 0, 1});
          const M3 Rj = cur.R * (ldm3(lm.jpR[j]) * Rq);
          const V3 pj = cur.p + cur.R * ld3(lm.jpp[j]);
          const V3 ax = m3_col(Rj, jt - 1);
          const SV sk = SV{cross(pj, ax), ax};
          const double qd = SX(NQ + 6 + j - 1), aj = SU(3 * NF + j - 1);
          const SV vp = cur.v;
          cur.R = Rj;
          cur.p = pj;
          cur.v = vp + qd * sk;
          cur.a = cur.a + qd * crm(vp, sk) + aj * sk;
        }
        {
          const int ss = lm.save_slot[j];
#pragma unroll
          for (int s = 0; s < NSLOT; s++)
            if (ss == s)
              slot[s] = cur;
        }
        {
          const double m = lm.mass[j];
          const V3 c = cur.R * ld3(lm.com[j]) + cur.p;
          const double * il = lm.inertia[j];
          const M3 Il = M3{il[0], il[1], il[3], il[1], il[2], il[4], il[3], il[4], il[5]};
          const M3 Iw = cur.R * Il * transpose(cur.R);
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
          const SV h = I * cur.v;
          const SV F = I * cur.a + crf(cur.v, h);
          if (j == 0)
          {
            Itot = I;
            Ftot = F;
          }
          else
          {
            Itot = Itot + I;
            Ftot = Ftot + F;
          }
        }
#pragma unroll 1
        for (int f = 0; f < NF; f++)
          if (j == lm.foot_joint[f] && ((mask >> f) & 1u))
          {
            const V3 fp = cur.R * ld3(lm.foot_p[f]) + cur.p;
            const V3 Ff = mk3(SU(3 * f), SU(3 * f + 1), SU(3 * f + 2));
            fsum = fsum + Ff;
            msum = msum + cross(fp, Ff);
          }
      }
      // ---- rate of the centroidal momentum without the base acceleration, target rate, base acceleration (closed form) ----
      const double im = 1.0 / Itot.m;
      const V3 com = im * Itot.mc;
      double rhs[6];
      {
        const V3 fl = total_mass * gravity + fsum;
        const V3 fa = msum - cross(com, fsum);
        const V3 ba = Ftot.a - cross(com, Ftot.l);
        rhs[0] = fl.x - Ftot.l.x;
        rhs[1] = fl.y - Ftot.l.y;
        rhs[2] = fl.z - Ftot.l.z;
        rhs[3] = fa.x - ba.x;
        rhs[4] = fa.y - ba.y;
        rhs[5] = fa.z - ba.z;
      }
      double o[NO];
      {
        const double cc = dot(com, com);
        const double jxx = Itot.jxx - Itot.m * (cc - com.x * com.x), jyy = Itot.jyy - Itot.m * (cc - com.y * com.y),
                     jzz = Itot.jzz - Itot.m * (cc - com.z * com.z);
        const double jxy = Itot.jxy + Itot.m * com.x * com.y, jxz = Itot.jxz + Itot.m * com.x * com.z, jyz = Itot.jyz + Itot.m * com.y * com.z;
        const double a00 = jyy * jzz - jyz * jyz, a01 = jxz * jyz - jxy * jzz, a02 = jxy * jyz - jxz * jyy;
        const double a11 = jxx * jzz - jxz * jxz, a12 = jxy * jxz - jxx * jyz, a22 = jxx * jyy - jxy * jxy;
        const double idet = 1.0 / (jxx * a00 + jxy * a01 + jxz * a02);
        const M3 Ji = M3{a00 * idet, a01 * idet, a02 * idet, a01 * idet, a11 * idet, a12 * idet, a02 * idet, a12 * idet, a22 * idet};
        double Agbi[36];
#pragma unroll
        for (int c = 0; c < 6; c++)
        {
          V3 ml, ma;
          if (c < 3)
          {
            ml = mk3(c == 0 ? im : 0.0, c == 1 ? im : 0.0, c == 2 ? im : 0.0);
            ma = mk3(0, 0, 0);
          }
          else
          {
            ma = m3_col(Ji, c - 3);
            ml = cross(com, ma);
          }
          const V3 top = tmul(R0, ml - cross(p0, ma)), bot = tmul(R0, ma);
          Agbi[0 * 6 + c] = top.x;
          Agbi[1 * 6 + c] = top.y;
          Agbi[2 * 6 + c] = top.z;
          Agbi[3 * 6 + c] = bot.x;
          Agbi[4 * 6 + c] = bot.y;
          Agbi[5 * 6 + c] = bot.z;
        }
#pragma unroll
        for (int r = 0; r < 6; r++)
        {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < 6; m++)
            s += Agbi[r * 6 + m] * rhs[m];
          o[NV + r] = s;
        }
      }
#pragma unroll
      for (int i = 0; i < NV; i++)
        o[i] = SX(NQ + i);
#pragma unroll
      for (int i = 6; i < NV; i++)
        o[NV + i] = SU(3 * NF + i - 6);
      // (the lane's own column only: every input of this lane is read above)
#pragma unroll
      for (int i = 0; i < NO; i++)
        stg[i * LANE_PAD + lane] = o[i];
    }
    SMPC_LANES_END_WAVE
    // ---- lane = element: each problem's row of the output as one coalesced run ----
    SMPC_LANES(NT)
    if (lane < NO)
      for (int p = 0; p < np; p++)
        ka.out[((size_t)(base + p) * H + t) * NO + lane] = stg[lane * LANE_PAD + p];
    SMPC_LANES_END_WAVE
  }

  // ---- kinodynamics, one wavefront per (instance, stage): kino_tree_phases; grid = B * H ----
  template <class D>
  SMPC_DEV void xdot_kino_wave(const XdotArgs<Buffers<D>> & ka, int block)
  {
    typedef KinoScratch<D, false> SC;
    constexpr int NT = 64, NX = D::NX, NU = D::NU, NV = D::NV, NQ = D::NQ;
    const Buffers<D> & b = ka.b;
    const int H = b.H, R = b.R;
    const int inst = block / H, t = block % H;
    const DevModel<D> & mg = *b.model;
    const size_t sl = (size_t)inst * R + ring_slot(ka.head, t, R);
    SMPC_LDS(SC, scs, 1);
    SC & sc = scs[0];
    StageIn<D> in;
    in.md = &mg;
    in.terminal = false;
    in.mask = b.stages[t].mask;
    in.u_ref = b.stages[t].u_ref;
    in.x_tgt = b.stages[t].x_tgt;
    in.foot_ref = b.foot_ref + ((size_t)inst * H + t) * D::NF * 3;
    SMPC_LANES(NT)
    {
      static_assert(NX <= NT && NU <= NT, "one element per lane");
      const double vx = b.xs[sl * NX + (lane < NX ? lane : 0)], vu = b.us[sl * NU + (lane < NU ? lane : 0)];
      const double vxt = in.x_tgt[lane < NX ? lane : 0];
      lanes_load_model<D, NT>(sc, &mg, lane);
      if (lane < NX)
      {
        sc.x[lane] = vx;
        sc.in_x_tgt[lane] = vxt;
      }
      if (lane < NU)
        sc.u[lane] = vu;
    }
    SMPC_LANES_END_WAVE
    kino_tree_phases<D, false>(sc, in);
    SMPC_LANES(NT)
    if (lane < NV)
    {
      double * o = ka.out + ((size_t)inst * H + t) * 2 * NV;
      o[lane] = sc.x[NQ + lane];
      o[NV + lane] = sc.a[lane];
    }
    SMPC_LANES_END_WAVE
  }

  // ---- dense engines, one wavefront per (instance, stage): full_dynamics_phases; grid = B * H ----
  template <class D>
  SMPC_DEV void xdot_full_wave(const XdotArgs<Buffers<D>> & ka, int block)
  {
    typedef FullScratch<D, false> SC;
    constexpr int NT = 64, NX = D::NX, NU = D::NU, NV = D::NV, NQ = D::NQ, NF = D::NF;
    const Buffers<D> & b = ka.b;
    const int H = b.H, R = b.R;
    const int inst = block / H, t = block % H;
    const DevModel<D> & mg = *b.model;
    const unsigned mask = b.stages[t].mask & ((1u << NF) - 1u);
    const size_t sl = (size_t)inst * R + ring_slot(ka.head, t, R);
    SMPC_LDS(SC, scs, 1);
    SC & sc = scs[0];
    SMPC_LANES(NT)
    {
      constexpr int PX = (NX + NT - 1) / NT, PU = (NU + NT - 1) / NT;
      double vx[PX], vu[PU];
#pragma unroll
      for (int n = 0; n < PX; n++)
        vx[n] = b.xs[sl * NX + (lane + n * NT < NX ? lane + n * NT : NX - 1)];
#pragma unroll
      for (int n = 0; n < PU; n++)
        vu[n] = b.us[sl * NU + (lane + n * NT < NU ? lane + n * NT : NU - 1)];
      full_load_head<D, NT>(sc.h, &mg, lane);
#pragma unroll
      for (int n = 0; n < PX; n++)
        if (lane + n * NT < NX)
          sc.x[lane + n * NT] = vx[n];
#pragma unroll
      for (int n = 0; n < PU; n++)
        if (lane + n * NT < NU)
          sc.u[lane + n * NT] = vu[n];
    }
    SMPC_LANES_END_WAVE
    FullProf fp;
    full_dynamics_phases<D, false>(sc, (FullScratchDeriv<D> *)nullptr, mg, mask, true, fp);
    SMPC_LANES(NT)
    {
      double * o = ka.out + ((size_t)inst * H + t) * 2 * NV;
      for (int i = lane; i < NV; i += NT)
      {
        o[i] = sc.x[NQ + i];
        o[NV + i] = sc.a[i];
      }
    }
    SMPC_LANES_END_WAVE
  }

  // ---- centroidal, lane = (instance, stage) item; grid = ceil(B H / 64) ----
  template <class DC>
  SMPC_DEV void xdot_cent_lane(const XdotArgs<CentBuffers<DC>> & ka, int block)
  {
    constexpr int NT = 64, NF = DC::NF, NU = DC::NU, FS = DC::FS;
    const CentBuffers<DC> & b = ka.b;
    const int H = b.H, R = b.R;
    const CentDevModel<DC> & md = *b.model;
    SMPC_LANES(NT)
    {
      const int item = block * NT + lane;
      if (item < b.B * H)
      {
        const int inst = item / H, t = item % H;
        const size_t sl = (size_t)inst * R + ring_slot(ka.head, t, R);
        const double * xg = b.xs + sl * 9;
        const double * u = b.us + sl * NU;
        const double * pf = b.foot + ((size_t)inst * H + t) * (3 * NF);
        const unsigned mask = b.stages[t].mask;
        const V3 c = ld3(xg);
        V3 fs = mk3(0, 0, 0), ts = mk3(0, 0, 0);
#pragma unroll
        for (int f = 0; f < NF; f++)
          if ((mask >> f) & 1u)
          {
            const V3 F = ld3(u + FS * f);
            fs = fs + F;
            ts = ts + cross(ld3(pf + 3 * f) - c, F);
            if (FS == 6)
              ts = ts + ld3(u + FS * f + 3);
          }
        const double imass = 1.0 / md.mass;
        double * o = ka.out + (size_t)item * 9;
        o[0] = xg[3] * imass;
        o[1] = xg[4] * imass;
        o[2] = xg[5] * imass;
        o[3] = md.mass * md.gravity[0] + fs.x;
        o[4] = md.mass * md.gravity[1] + fs.y;
        o[5] = md.mass * md.gravity[2] + fs.z;
        o[6] = ts.x;
        o[7] = ts.y;
        o[8] = ts.z;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // the kernel: one template, instantiated per engine (D: Dims / FullDims / CentDims; BUF: that engine's buffer set)
  template <class D, class BUF, int KIND, int NSLOT = 1>
  SMPC_DEV void xdot_all_body(const XdotArgs<BUF> & ka, int block)
  {
    if constexpr (KIND == XD_KINO_LANE)
      xdot_kino_lane<D, NSLOT>(ka, block);
    else if constexpr (KIND == XD_KINO_WAVE)
      xdot_kino_wave<D>(ka, block);
    else if constexpr (KIND == XD_FULL)
      xdot_full_wave<D>(ka, block);
    else
      xdot_cent_lane<D>(ka, block);
  }
  // grid of a launch over B instances, H stages
  SMPC_HD int xdot_grid(int kind, int B, int H) { return kind == XD_KINO_LANE ? H * ((B + 63) / 64) : (kind == XD_CENT ? (B * H + 63) / 64 : B * H); }
} // namespace smpc
