// smpc_id_rt.h -- the whole-body inverse-dynamics QP of smpc_id.h (KinodynamicsID / CentroidalID of the reference,
// src/inverse-dynamics/kinodynamics-id.cpp:7-237, centroidal-id.cpp:6-147) on a RUN-TIME joint tree: any validated robot table with 4 point
// feet and 2 .. SMPC_MAX_JOINTS joints.  Joint count, parents, axis types and feet are DATA of the device table, as in smpc_frontend_rt.h;
// the problem sizes (nv, n = nv + 12, m = n + 34 + nv - 6, padded to multiples of 16) travel in the kernel arguments.  One wavefront per robot.
//   id_quant_rt_body     M (composite rigid body), h (recursive Newton-Euler at zero acceleration), world-frame linear foot Jacobians, their
//                        drift, foot velocities and positions, CoM -- lane = joint, one step per tree level, world frame about the origin
//   id_assemble_rt_body  H, g, C, l, u: id_assemble_body term by term with run-time strides
//   qp_admm_rt_body<NP>  the ADMM of qp_admm_body (same constants, residual check, rho adaptation, warm start) with K^-1 and the general rows
//                        of C in LDS and two row blocks per lane (up to 65 general rows); instantiated for the padded sizes 32, 48 and 64
// and, for any validated table with 2 flat feet (tsid Contact6d; n = nv + 24, m = n + 52 + nv - 6), id6_quant_rt_body / id6_assemble_rt_body /
// qp6_admm_rt_body<NP>: the flat-foot kernels of smpc_id.h with run-time sizes.
// Rules of DESIGN 3: every global load of id_quant_rt_body is issued in its first phase and every global store in its last one; vector
// stores only; wave-level ordering points (SMPC_LANES_END_WAVE); every index that comes from the device table is clamped before it
// addresses LDS.
#pragma once
#include "smpc_id.h"
#include "smpc_frontend_rt.h"
#include "smpc_id_rt_dims.h"

namespace smpc
{
  struct IdRtDevModel
  {
    RtDevModel t;
    unsigned anc[SMPC_MAX_JOINTS]; // bit k of anc[j]: joint k is j or an ancestor of j
    double total_mass;
  };

  struct IdRtBuffers
  {
    int B = 0, nv = 0, n = 0, m = 0, np = 0, mp = 0;
    const IdRtDevModel * model = nullptr;
    const double * X = nullptr;                                                              // [B][2 nv + 1]
    double *Mq = nullptr, *nle = nullptr, *J = nullptr, *Jdv = nullptr, *vfoot = nullptr;  // [B][nv nv], [nv], [12][nv], [12], [12]
    double *com = nullptr, *footp = nullptr;                                                 // [B][3], [12]
    double *H = nullptr, *g = nullptr, *C = nullptr, *l = nullptr, *u = nullptr;             // [B][np np], [np], [mp][np], [mp], [mp]
    double *x = nullptr, *z = nullptr, *lam = nullptr, *rho = nullptr;
    int * warm = nullptr;
    double *tx = nullptr, *ta = nullptr, *tf = nullptr;                                      // [B][2 nv + 1], [nv], [12]
    unsigned * tmask = nullptr;
    double *tcom = nullptr, *tvcom = nullptr, *tfp = nullptr, *tfv = nullptr;
    double *tau = nullptr, *a = nullptr, *f = nullptr, *resid = nullptr;                     // [B][nv - 6], [nv], [12], [B]
    double *tau_max = nullptr, *v_max = nullptr, *q_min = nullptr, *q_max = nullptr;         // [nv - 6]
    IdSettingsDev s;
  };

  struct IdQuantRtScratch
  {
    static constexpr int MAXJ = SMPC_MAX_JOINTS, MAXV = ID_RT_MAX_NV, NF = ID_RT_NFEET;
    double x[2 * MAXJ + 11];
    double oR[MAXJ * 9], op[MAXJ * 3];
    double vel[MAXJ * 6], acc[MAXJ * 6]; // spatial velocity / acceleration at zero joint accelerations (no gravity), [linear; angular] about the world origin
    double S[MAXV * 6];                  // motion subspace of every degree of freedom (world frame, about the origin)
    double body[MAXJ * 10];              // spatial inertia of every body about the world origin
    double fb[MAXJ * 6];                 // body forces of the Newton-Euler pass [force; moment]
    double Ic[MAXJ * 10], fs[MAXJ * 6];  // sums over the subtree of every joint
    double F[MAXV * 6], h[MAXV];
    double footp[NF * 3];
    unsigned anc[MAXJ];
    int fj[NF];
  };

  SMPC_HD double id_rt_dot6(const double * s, const double * f) { return s[0] * f[0] + s[1] * f[1] + s[2] * f[2] + s[3] * f[3] + s[4] * f[4] + s[5] * f[5]; }

  // ---- the tree walk both kernels on a run-time tree share (id_quant_rt_body here, sim_rt_body of smpc_sim_rt.h) ----
  // From one state `x` ([2 nj + 11], device) into `sc`: placements, motion-subspace columns, spatial velocities and bias accelerations of every
  // joint (one step per tree level), body inertias and forces f = I (a - g) + v x* (I v) under the gravity field g, foot positions, the
  // sums over the subtree of every joint through the ancestor bit sets, F_d = Ic S_d and h_d = S_d . f (the bias forces).  Its first phase
  // issues every global load it makes; it stores nothing outside `sc`.
  // BODY: lane j takes mass, com and inertia of its body from `rows` + 10 j (device, [nj][10] doubles of ONE robot in the
  // order mass | com | Ixx Ixy Iyy Ixz Iyz Izz: 80 contiguous bytes per lane) instead of from the device table; a null `rows` (wave-uniform)
  // reads the table.  The values enter arithmetic only, never an index.  BODY = false is the walk every other kernel uses.
  template <bool BODY>
  SMPC_DEV void rt_tree_phases_impl(IdQuantRtScratch & sc, const IdRtDevModel & mi, const double * x, const V3 g, const double * rows)
  {
    typedef IdQuantRtScratch SC;
    constexpr int NT = 64, MAXJ = SC::MAXJ, MAXV = SC::MAXV, NF = SC::NF;
    static_assert(MAXJ <= 32 && MAXV <= NT, "lane = joint below 32, lane - 32 = foot, lane = degree of freedom");
    const RtDevModel & mg = mi.t;
    const int nj = mg.njoints < MAXJ ? (mg.njoints > 1 ? mg.njoints : 1) : MAXJ;
    const int nlev = mg.nlevels < MAXJ ? mg.nlevels : MAXJ;
    const int nv = nj + 5, nq = nj + 6, nx = 2 * nj + 11;
    SMPC_PLA(double, jg, NT, 22); // jpR 0..8 | jpp 9..11 | mass 12 | com 13..15 | inertia 16..21 of this lane's joint
    SMPC_PLA(double, fp, NT, 3);
    SMPC_PL(int, par, NT);
    SMPC_PL(int, jt, NT);
    SMPC_PL(int, lev, NT);
    // ---- phase 0: every global load ----
    SMPC_LANES(NT)
    {
      const int j = lane < nj ? lane : 0;
#pragma unroll
      for (int i = 0; i < 9; i++)
        SMPC_PLV(jg)[i] = mg.jpR[j][i];
      if (BODY && rows != nullptr)
      {
#pragma unroll
        for (int i = 0; i < 3; i++)
          SMPC_PLV(jg)[9 + i] = mg.jpp[j][i];
#pragma unroll
        for (int i = 0; i < 10; i++)
          SMPC_PLV(jg)[12 + i] = rows[(size_t)j * 10 + i];
      }
      else
      {
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
      }
      const int p = mg.parent[j];
      SMPC_PLV(par) = p >= 0 && p < nj ? p : 0;
      SMPC_PLV(jt) = mg.jtype[j];
      SMPC_PLV(lev) = mg.level[j];
      const unsigned an = mi.anc[j];
      const int f = lane >= 32 && lane < 32 + NF ? lane - 32 : 0;
      const int q = mg.foot_joint[f];
#pragma unroll
      for (int i = 0; i < 3; i++)
        SMPC_PLV(fp)[i] = mg.foot_p[f][i];
      for (int i = lane; i < nx; i += NT)
        sc.x[i] = x[i];
      if (lane < MAXJ)
        sc.anc[lane] = lane < nj ? an : 0u;
      if (lane >= 32 && lane < 32 + NF)
        sc.fj[f] = q >= 0 && q < nj ? q : 0;
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
        // free-flyer: v[0:6] = [v; w] in the local frame; its six columns: translations along / rotations about the base axes
        const V3 w = R * ld3(vq + 3);
        const V3 v = R * ld3(vq) + cross(p, w);
        stm3(&sc.oR[0], R);
        st3(&sc.op[0], p);
        stsv(&sc.vel[0], SV{v, w});
        stsv(&sc.acc[0], sv0()); // (d/dt of the columns times the local velocity: v x v = 0)
        for (int k = 0; k < 3; k++)
        {
          const V3 e = k == 0 ? mk3(R.a00, R.a10, R.a20) : (k == 1 ? mk3(R.a01, R.a11, R.a21) : mk3(R.a02, R.a12, R.a22));
          stsv(&sc.S[k * 6], SV{e, mk3(0, 0, 0)});
          stsv(&sc.S[(3 + k) * 6], SV{cross(p, e), e});
        }
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
    // ---- phase 1: root -> leaf, one step per tree level ----
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
        const SV vp = ldsv(&sc.vel[pj * 6]);
        const SV vj = vq[j + 5] * sk;
        stm3(&sc.oR[j * 9], R);
        st3(&sc.op[j * 3], p);
        stsv(&sc.S[(5 + j) * 6], sk);
        stsv(&sc.vel[j * 6], vp + vj);
        stsv(&sc.acc[j * 6], ldsv(&sc.acc[pj * 6]) + crm(vp, vj)); // (v_j x S qd = v_parent x S qd)
      }
      SMPC_LANES_END_WAVE
    }
    // ---- phase 2: body inertias about the world origin, body forces f = I (a - g) + v x* (I v); feet ----
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
      stsi(&sc.body[j * 10], I);
      SV a = ldsv(&sc.acc[j * 6]);
      a.l = a.l - g; // the gravity field as an acceleration of the world
      stsv(&sc.fb[j * 6], I * a + crf(v, I * v));
    }
    else if (lane >= 32 && lane < 32 + NF)
    {
      const int f = lane - 32, j = sc.fj[f];
      st3(&sc.footp[f * 3], ldm3(&sc.oR[j * 9]) * ld3(SMPC_PLV(fp)) + ld3(&sc.op[j * 3]));
    }
    SMPC_LANES_END_WAVE
    // ---- phase 3: sums over the subtree of every joint, joints in ascending order ----
    SMPC_LANES(NT)
    if (lane < nj)
    {
      const int j = lane;
      SI I = ldsi(&sc.body[j * 10]);
      SV f = ldsv(&sc.fb[j * 6]);
      for (int k = j + 1; k < nj; k++)
        if ((sc.anc[k] >> j) & 1u)
        {
          I = I + ldsi(&sc.body[k * 10]);
          f = f + ldsv(&sc.fb[k * 6]);
        }
      stsi(&sc.Ic[j * 10], I);
      stsv(&sc.fs[j * 6], f);
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: F_d = Ic S_d, h_d = S_d . f of the subtree ----
    SMPC_LANES(NT)
    if (lane < nv)
    {
      const int d = lane, jd = d < 6 ? 0 : d - 5;
      stsv(&sc.F[d * 6], ldsi(&sc.Ic[jd * 10]) * ldsv(&sc.S[d * 6]));
      sc.h[d] = id_rt_dot6(&sc.S[d * 6], &sc.fs[jd * 6]);
    }
    SMPC_LANES_END_WAVE
  }
  SMPC_DEV void rt_tree_phases(IdQuantRtScratch & sc, const IdRtDevModel & mi, const double * x, const V3 g)
  {
    rt_tree_phases_impl<false>(sc, mi, x, g, nullptr);
  }

  // ---- kernel 1: rigid-body quantities on the run-time tree ----   grid = B, 64 lanes
  SMPC_DEV void id_quant_rt_body(const IdRtBuffers & b, int block)
  {
    typedef IdQuantRtScratch SC;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF;
    const int inst = block;
    const IdRtDevModel & mi = *b.model;
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nx = 2 * nj + 11;
    SMPC_LDS(SC, scs, 1);
    SC & sc = scs[0];
    // ---- phases 0 .. 4 ----
    rt_tree_phases(sc, mi, b.X + (size_t)inst * nx, mk3(0.0, 0.0, -9.81));
    // ---- phase 5: every global store ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < nv * nv; idx += NT)
      {
        const int r = idx / nv, c = idx % nv;
        const int lo = r < c ? r : c, hi = r < c ? c : r; // (one expression for both triangles: M is symmetric bit for bit)
        const int jl = lo < 6 ? 0 : lo - 5, jh = hi < 6 ? 0 : hi - 5;
        b.Mq[(size_t)inst * nv * nv + idx] = ((sc.anc[jh] >> jl) & 1u) ? id_rt_dot6(&sc.S[lo * 6], &sc.F[hi * 6]) : 0.0;
      }
      if (lane < nv)
        b.nle[(size_t)inst * nv + lane] = sc.h[lane];
      for (int idx = lane; idx < 3 * NF * nv; idx += NT)
      {
        const int r = idx / nv, k = idx % nv, f = r / 3, i = r % 3;
        const int jk = k < 6 ? 0 : k - 5;
        double val = 0.0;
        if ((sc.anc[sc.fj[f]] >> jk) & 1u)
        { // velocity of the foot point under the unit twist of column k
          const SV s = ldsv(&sc.S[k * 6]);
          val = v3c(s.l + cross(s.a, ld3(&sc.footp[f * 3])), i);
        }
        b.J[(size_t)inst * 3 * NF * nv + idx] = val;
      }
      if (lane < 3 * NF)
      {
        const int f = lane / 3, i = lane % 3, jf = sc.fj[f];
        const V3 p = ld3(&sc.footp[f * 3]);
        const SV v = ldsv(&sc.vel[jf * 6]), a = ldsv(&sc.acc[jf * 6]);
        const V3 vp = v.l + cross(v.a, p);
        // classical acceleration of the point at zero joint accelerations
        const V3 ap = a.l + cross(a.a, p) + cross(v.a, vp);
        b.Jdv[(size_t)inst * 3 * NF + lane] = v3c(ap, i);
        b.vfoot[(size_t)inst * 3 * NF + lane] = v3c(vp, i);
        b.footp[(size_t)inst * 3 * NF + lane] = sc.footp[lane];
      }
      if (lane < 3)
        b.com[(size_t)inst * 3 + lane] = sc.Ic[1 + lane] / sc.Ic[0];
    }
    SMPC_LANES_END_WAVE
  }

  // ---- kernel 2: QP data (id_assemble_body with run-time sizes) ----
  SMPC_DEV void id_assemble_rt_body(const IdRtBuffers & b, int block)
  {
    constexpr int NT = 64, NF = ID_RT_NFEET, MAXV = ID_RT_MAX_NV;
    const int inst = block;
    const IdSettingsDev & s = b.s;
    const int NV = b.nv < MAXV ? (b.nv > 7 ? b.nv : 7) : MAXV, NQ = NV + 1, NX = 2 * NV + 1, NA = NV - 6;
    const int N = NV + 3 * NF, M = N + 6 + 7 * NF + NA, NP = ((N + 15) / 16) * 16, MP = ((M + 15) / 16) * 16;
    const int R_DYN = N, R_MOT = N + 6, R_FRI = R_MOT + 3 * NF, R_ACT = R_FRI + 4 * NF;
    const double * x = b.X + (size_t)inst * NX;
    const double * q = x;
    const double * v = x + NQ;
    SMPC_LDS(double, sM, MAXV * MAXV);
    SMPC_LDS(double, sJ, 3 * NF * MAXV);
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NV * NV; idx += NT)
        sM[idx] = b.Mq[(size_t)inst * NV * NV + idx];
      for (int idx = lane; idx < 3 * NF * NV; idx += NT)
        sJ[idx] = b.J[(size_t)inst * 3 * NF * NV + idx];
    }
    SMPC_LANES_END_WAVE
    const double * Mq = sM;
    const double * nle = b.nle + (size_t)inst * NV;
    const double * J = sJ;
    const double * Jdv = b.Jdv + (size_t)inst * 3 * NF;
    const double * vf = b.vfoot + (size_t)inst * 3 * NF;
    const double *tq = b.tx + (size_t)inst * NX, *tv = tq + NQ, *ta = b.ta + (size_t)inst * NV, *tf = b.tf + (size_t)inst * 3 * NF;
    const unsigned mask = b.tmask[inst];
    double * H = b.H + (size_t)inst * NP * NP;
    double * g = b.g + (size_t)inst * NP;
    double * C = b.C + (size_t)inst * MP * NP;
    double * l = b.l + (size_t)inst * MP;
    double * u = b.u + (size_t)inst * MP;
    const double total_mass = b.model->total_mass;
    const double kdp = 2.0 * sqrt(s.kp_posture), kdb = 2.0 * sqrt(s.kp_base), kdc = 2.0 * sqrt(s.kp_contact);
    const double kdm = 2.0 * sqrt(s.kp_com), kdt = 2.0 * sqrt(s.kp_feet_tracking);
    const bool com_task = s.centroidal && s.w_com > 0, track_task = s.centroidal && s.w_feet_tracking > 0;
    const int base0 = s.centroidal ? 3 : 0; // (CentroidalID: orientation rows only, centroidal-id.cpp:10-20)
    SMPC_LDS(double, e6, 6);
    SMPC_LDS(double, Jc, 3 * MAXV); // CoM Jacobian R_b M_lin / m
    SMPC_LDS(double, bc, 3);        // right-hand side of the CoM task
    SMPC_LDS(double, bt, 3 * NF);   // right-hand sides of the foot-tracking tasks
    SMPC_LANES(NT)
    if (com_task)
      for (int idx = lane; idx < 3 * NV; idx += NT)
      {
        const int i = idx / NV, k = idx % NV;
        const M3 Rb = quat_to_R(Quat{q[3], q[4], q[5], q[6]});
        const double im = 1.0 / total_mass;
        const double r0 = i == 0 ? Rb.a00 : (i == 1 ? Rb.a10 : Rb.a20), r1 = i == 0 ? Rb.a01 : (i == 1 ? Rb.a11 : Rb.a21),
                     r2 = i == 0 ? Rb.a02 : (i == 1 ? Rb.a12 : Rb.a22);
        Jc[idx] = im * (r0 * Mq[k] + r1 * Mq[NV + k] + r2 * Mq[2 * NV + k]);
      }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      if (com_task && lane < 3)
      { // a_com = J_com a + drift, drift = R_b nle_lin / m + g (TaskComEquality, centroidal-id.cpp:22-27)
        const int i = lane;
        const M3 Rb = quat_to_R(Quat{q[3], q[4], q[5], q[6]});
        const double im = 1.0 / total_mass;
        const double r0 = i == 0 ? Rb.a00 : (i == 1 ? Rb.a10 : Rb.a20), r1 = i == 0 ? Rb.a01 : (i == 1 ? Rb.a11 : Rb.a21),
                     r2 = i == 0 ? Rb.a02 : (i == 1 ? Rb.a12 : Rb.a22);
        double vc = 0.0;
        for (int k = 0; k < NV; k++)
          vc += Jc[i * NV + k] * v[k];
        const double dr = im * (r0 * nle[0] + r1 * nle[1] + r2 * nle[2]) + (i == 2 ? -9.81 : 0.0);
        bc[i] = s.kp_com * (b.tcom[(size_t)inst * 3 + i] - b.com[(size_t)inst * 3 + i]) + kdm * (b.tvcom[(size_t)inst * 3 + i] - vc) - dr;
      }
      if (track_task && lane >= 32 && lane < 32 + 3 * NF)
      { // position tracking of the feet out of contact (centroidal-id.cpp:101-129; point feet: linear part)
        const int r = lane - 32;
        const size_t o = (size_t)inst * 3 * NF + r;
        bt[r] = s.kp_feet_tracking * (b.tfp[o] - b.footp[o]) + kdt * (b.tfv[o] - vf[r]) - Jdv[r];
      }
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    if (lane == 0)
    { // base error log6(M_b^-1 M_t), local frame
      const SE3 Mb{quat_to_R(Quat{q[3], q[4], q[5], q[6]}), mk3(q[0], q[1], q[2])};
      const SE3 Mt{quat_to_R(Quat{tq[3], tq[4], tq[5], tq[6]}), mk3(tq[0], tq[1], tq[2])};
      V3 ev, ew;
      log6(se3_mul(se3_inv(Mb), Mt), ev, ew);
      st3(e6, ev);
      st3(e6 + 3, ew);
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      // ---- H (N x N, padded with unit diagonal) and g ----
      for (int idx = lane; idx < NP * NP; idx += NT)
      {
        const int i = idx / NP, j = idx % NP;
        double h = 0.0;
        if (i >= N || j >= N)
          h = (i == j) ? 1.0 : 0.0; // padding variables: pinned by their own unit curvature and zero gradient
        else
        {
          if (i == j && i >= 6 && i < NV && s.w_posture > 0)
            h += s.w_posture;
          if (i == j && i >= base0 && i < 6 && s.w_base > 0)
            h += s.w_base;
          if (i < NV && j < NV && com_task)
            for (int r = 0; r < 3; r++)
              h += s.w_com * Jc[r * NV + i] * Jc[r * NV + j];
          if (i < NV && j < NV && track_task)
            for (int r = 0; r < 3 * NF; r++)
              if (!((mask >> (r / 3)) & 1u))
                h += s.w_feet_tracking * J[r * NV + i] * J[r * NV + j];
          if (i < NV && j < NV && !s.contact_motion_equality && s.w_contact_motion > 0)
            for (int r = 0; r < 3 * NF; r++)
              if ((mask >> (r / 3)) & 1u)
                h += s.w_contact_motion * J[r * NV + i] * J[r * NV + j];
          if (i == j && i >= NV && s.w_contact_force > 0 && ((mask >> ((i - NV) / 3)) & 1u))
            h += s.w_contact_force;
        }
        H[idx] = h;
      }
      for (int i = lane; i < NP; i += NT)
      {
        double gi = 0.0;
        if (i < N)
        {
          if (i >= 6 && i < NV && s.w_posture > 0)
            gi -= s.w_posture * (ta[i] + s.kp_posture * (tq[i + 1] - q[i + 1]) + kdp * (tv[i] - v[i]));
          if (i >= base0 && i < 6 && s.w_base > 0)
          {
            const V3 dr = cross(mk3(v[3], v[4], v[5]), mk3(v[0], v[1], v[2]));
            // (velocity / acceleration references: DESIGN 3.12; base_as_coded: the reference literally, kinodynamics-id.cpp:222-223)
            const double ades = s.base_as_coded ? s.kp_base * e6[i] + kdb * (ta[i] - v[i]) : s.kp_base * e6[i] + kdb * (tv[i] - v[i]) + ta[i];
            gi -= s.w_base * (ades - (i == 0 ? dr.x : (i == 1 ? dr.y : (i == 2 ? dr.z : 0.0))));
          }
          if (i < NV && com_task)
            for (int r = 0; r < 3; r++)
              gi -= s.w_com * Jc[r * NV + i] * bc[r];
          if (i < NV && track_task)
            for (int r = 0; r < 3 * NF; r++)
              if (!((mask >> (r / 3)) & 1u))
                gi -= s.w_feet_tracking * J[r * NV + i] * bt[r];
          if (i < NV && !s.contact_motion_equality && s.w_contact_motion > 0)
            for (int r = 0; r < 3 * NF; r++)
              if ((mask >> (r / 3)) & 1u)
                gi -= s.w_contact_motion * J[r * NV + i] * (-Jdv[r] - kdc * vf[r]);
          if (i >= NV && s.w_contact_force > 0 && ((mask >> ((i - NV) / 3)) & 1u))
            gi -= s.w_contact_force * tf[i - NV];
        }
        g[i] = gi;
      }
      // ---- C, l, u ----  (rows 0 .. N-1, the box on y, are the identity and the padding rows are zero: written once when the engine
      //                     is created; only the general rows change with the state)
      for (int idx = N * NP + lane; idx < M * NP; idx += NT)
      {
        const int r = idx / NP, c = idx % NP;
        double val = 0.0;
        if (c < N && r < R_MOT)
        { // dynamics rows: [M_b | -J_b^T]
          const int i = r - R_DYN;
          val = c < NV ? Mq[i * NV + c] : -J[(c - NV) * NV + i];
        }
        else if (c < N && r < R_FRI)
        { // contact motion rows (equality variant, feet in contact)
          const int rr = r - R_MOT;
          if (s.contact_motion_equality && ((mask >> (rr / 3)) & 1u) && c < NV)
            val = J[rr * NV + c];
        }
        else if (c < N && r < R_ACT)
        { // friction pyramid: +-f_x - mu f_z, +-f_y - mu f_z
          const int rr = r - R_FRI, f = rr / 4, k = rr % 4;
          if ((mask >> f) & 1u)
          {
            if (c == NV + 3 * f + k / 2)
              val = (k % 2 == 0) ? 1.0 : -1.0;
            else if (c == NV + 3 * f + 2)
              val = -s.friction_coefficient;
          }
        }
        else if (c < N && r < M)
        { // actuation rows: [M_a | -J_a^T]
          const int j = r - R_ACT;
          val = c < NV ? Mq[(6 + j) * NV + c] : -J[(c - NV) * NV + 6 + j];
        }
        C[idx] = val;
      }
      for (int r = lane; r < MP; r += NT)
      {
        double lo = -ID_INF, hi = ID_INF;
        const double W = total_mass * 9.81, dt = s.control_dt;
        if (r >= 6 && r < NV)
        { // joint limits as acceleration bounds over one control period
          const int j = r - 6;
          const double qa = q[7 + j], va = v[6 + j];
          lo = fmax((-b.v_max[j] - va) / dt, 2.0 * (b.q_min[j] - qa - va * dt) / (dt * dt));
          hi = fmin((b.v_max[j] - va) / dt, 2.0 * (b.q_max[j] - qa - va * dt) / (dt * dt));
          if (lo > hi)
            lo = hi = fmin(lo, hi);
          if (s.tsid_bounds)
            id_tsid_acc_limits(qa, va, b.q_min[j], b.q_max[j], b.v_max[j], dt, lo, hi);
        }
        else if (r >= NV && r < N)
        {
          const int f = (r - NV) / 3, i = (r - NV) % 3;
          if (!((mask >> f) & 1u))
            lo = hi = 0.0;
          else if (i == 2)
          {
            lo = s.ratio_min * W;
            hi = s.ratio_max * W;
          }
        }
        else if (r >= N && r < R_MOT)
          lo = hi = -nle[r - R_DYN];
        else if (r >= R_MOT && r < R_FRI)
        {
          const int rr = r - R_MOT;
          if (s.contact_motion_equality && ((mask >> (rr / 3)) & 1u))
            lo = hi = -Jdv[rr] - kdc * vf[rr];
        }
        else if (r >= R_FRI && r < R_ACT)
        {
          if ((mask >> ((r - R_FRI) / 4)) & 1u)
            hi = 0.0;
        }
        else if (r >= R_ACT && r < M)
        {
          const int j = r - R_ACT;
          lo = -b.tau_max[j] - nle[6 + j];
          hi = b.tau_max[j] - nle[6 + j];
        }
        l[r] = lo;
        u[r] = hi;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // ---- kernel 3: ADMM ----
  // Layout: K^-1 (NP x NP) and the general rows of C (row stride NP + 1) stay in LDS; lane i < n owns variable i and box row i, lane k owns
  // the general rows k and k + 64 (the second block exists only when the robot has more than 64 general rows: 32 joints).  The vectors
  // live one element per lane and are broadcast with v_readlane.  Every dot product is ONE accumulator summed in ascending index
  // order (rows of the first block, then of the second), the order of qp_admm_body and of the oracle's loops.
  template <int NP>
  struct QpRtLds
  {
    static constexpr int GRMAX = NP + 16 < ID_RT_MAX_GR ? NP + 16 : ID_RT_MAX_GR; // n <= NP  =>  nv <= NP - 12  =>  general rows nv + 28 <= NP + 16
    static constexpr int GRK = ((GRMAX + 3) / 4) * 4, LDC = NP + 1;
    double K[NP * NP];
    double C[GRK * LDC];
    double rg[GRK];
    double swp[2 * 4 * 16 * ((2 * NP + 15) / 16)];
    double red[256], red4[4];
  };

  template <int NP>
  SMPC_DEV void qp_admm_rt_body(const IdRtBuffers & b, int block)
  {
    typedef QpRtLds<NP> L;
    constexpr int NT = 64, NF = ID_RT_NFEET, LDC = L::LDC, GRMAX = L::GRMAX, GRK = L::GRK;
    static_assert(NP <= NT && GRMAX <= 2 * NT, "one variable per lane, two general rows per lane");
    const int inst = block;
    const IdSettingsDev & st = b.s;
    const double sigma = st.sigma, alpha = st.alpha;
    // (sizes: kernel arguments, clamped to what this instantiation holds)
    const int NVmax = NP - 3 * NF < ID_RT_MAX_NV ? NP - 3 * NF : ID_RT_MAX_NV;
    const int NV = b.nv < NVmax ? (b.nv > 7 ? b.nv : 7) : NVmax, NA = NV - 6, N = NV + 3 * NF, GR = 6 + 7 * NF + NA;
    const int MP = ((N + GR + 15) / 16) * 16;
    const int GR0 = GR < NT ? GR : NT; // rows of the first block
    SMPC_LDS(L, ls, 1);
    L & s = ls[0];
    const double * Hg = b.H + (size_t)inst * NP * NP;
    const double * Cg = b.C + (size_t)inst * MP * NP + (size_t)N * NP; // general rows
    const bool warm = b.warm[inst] != 0;
    double rho = warm ? b.rho[inst] : st.rho;
    SMPC_PL(double, x, NT);
    SMPC_PL(double, g, NT);
    SMPC_PL(double, rhs, NT);
    SMPC_PL(double, xt, NT);
    SMPC_PL(double, zb, NT);
    SMPC_PL(double, lamb, NT);
    SMPC_PL(double, lb, NT);
    SMPC_PL(double, ub, NT);
    SMPC_PL(double, rb, NT);
    SMPC_PL(double, zg0, NT);
    SMPC_PL(double, lamg0, NT);
    SMPC_PL(double, lg0, NT);
    SMPC_PL(double, ug0, NT);
    SMPC_PL(double, rg0, NT);
    SMPC_PL(double, wg0, NT);
    SMPC_PL(double, zg1, NT);
    SMPC_PL(double, lamg1, NT);
    SMPC_PL(double, lg1, NT);
    SMPC_PL(double, ug1, NT);
    SMPC_PL(double, rg1, NT);
    SMPC_PL(double, wg1, NT);
    SMPC_LANES(NT)
    {
      // general rows of C -> LDS (rows GR .. GRK - 1: zero, they are K-steps of the matrix product below)
      for (int idx = lane; idx < GRK * NP; idx += NT)
      {
        const int k = idx / NP, i = idx % NP;
        s.C[k * LDC + i] = k < GR ? Cg[(size_t)k * NP + i] : 0.0;
      }
      const int i = lane < NP ? lane : 0, kb = lane < N ? lane : 0;
      const int k0 = N + (lane < GR ? lane : 0), k1 = N + (lane + NT < GR ? lane + NT : 0);
      SMPC_PLV(g) = b.g[(size_t)inst * NP + i];
      SMPC_PLV(x) = warm ? b.x[(size_t)inst * NP + i] : 0.0;
      SMPC_PLV(rhs) = SMPC_PLV(xt) = 0.0;
      {
        const double lo = b.l[(size_t)inst * MP + kb], hi = b.u[(size_t)inst * MP + kb];
        SMPC_PLV(lb) = lo;
        SMPC_PLV(ub) = hi;
        SMPC_PLV(zb) = warm ? b.z[(size_t)inst * MP + kb] : fmin(fmax(0.0, lo), hi);
        SMPC_PLV(lamb) = warm ? b.lam[(size_t)inst * MP + kb] : 0.0;
      }
      {
        const double lo = b.l[(size_t)inst * MP + k0], hi = b.u[(size_t)inst * MP + k0];
        SMPC_PLV(lg0) = lo;
        SMPC_PLV(ug0) = hi;
        SMPC_PLV(zg0) = warm ? b.z[(size_t)inst * MP + k0] : fmin(fmax(0.0, lo), hi);
        SMPC_PLV(lamg0) = warm ? b.lam[(size_t)inst * MP + k0] : 0.0;
      }
      {
        const double lo = b.l[(size_t)inst * MP + k1], hi = b.u[(size_t)inst * MP + k1];
        SMPC_PLV(lg1) = lo;
        SMPC_PLV(ug1) = hi;
        SMPC_PLV(zg1) = warm ? b.z[(size_t)inst * MP + k1] : fmin(fmax(0.0, lo), hi);
        SMPC_PLV(lamg1) = warm ? b.lam[(size_t)inst * MP + k1] : 0.0;
      }
      SMPC_PLV(wg0) = SMPC_PLV(wg1) = 0.0;
      SMPC_PLV(rb) = SMPC_PLV(rg0) = SMPC_PLV(rg1) = 1.0;
    }
    SMPC_LANES_END_WAVE
    // row weights r = rho (1e3 rho on equality rows, 1e-6 rho on free rows) ; K = H + sigma I + C^T diag(r) C -> its inverse in LDS
    auto factor = [&]() {
      SMPC_LANES(NT)
      {
        auto weight = [&](double lo, double hi) { return (hi - lo < 1e-12) ? 1e3 * rho : ((lo <= -ID_INF && hi >= ID_INF) ? 1e-6 * rho : rho); };
        SMPC_PLV(rb) = weight(SMPC_PLV(lb), SMPC_PLV(ub));
        SMPC_PLV(rg0) = weight(SMPC_PLV(lg0), SMPC_PLV(ug0));
        SMPC_PLV(rg1) = weight(SMPC_PLV(lg1), SMPC_PLV(ug1));
        if (lane < GR)
          s.rg[lane] = SMPC_PLV(rg0);
        if (lane + NT < GRK)
          s.rg[lane + NT] = lane + NT < GR ? SMPC_PLV(rg1) : 0.0;
        if (lane >= GR && lane < GRK)
          s.rg[lane] = 0.0;
        if (lane < NP)
          s.red[lane] = lane < N ? SMPC_PLV(rb) : 0.0;
      }
      SMPC_LANES_END_WAVE
      fwave_gemm<NP, NP, GRK>(
        [&](int i, int k) { return s.rg[k] * s.C[k * LDC + i]; }, [&](int k, int j) { return s.C[k * LDC + j]; },
        [&](int i, int j, double v) { s.K[i * NP + j] = (Hg[i * NP + j] + (i == j ? sigma + s.red[i] : 0.0)) + v; });
      fwave_spd_inverse<NP>(s.K, s.swp);
    };
    // residuals of the iterate and the norms they are measured against (the same values in every lane):
    //   rs[0] = |C x - z|_inf, rs[1] = |H x + g + C^T lam|_inf, rs[2] = max(|C x|, |z|)_inf, rs[3] = max(|H x|, |C^T lam|, |g|)_inf
    double rs[4] = {0.0, 0.0, 0.0, 0.0};
    auto residual = [&]() {
      SMPC_LANES(NT)
      {
        double pr = 0.0, np = 0.0, du = 0.0, nd = 0.0;
        double cx0 = 0.0, cx1 = 0.0, hx = 0.0, cl = SMPC_PLV(lamb);
        const int r0 = (lane < GR ? lane : 0) * LDC, r1 = (lane + NT < GR ? lane + NT : 0) * LDC, col = lane < NP ? lane : 0;
        for (int i = 0; i < N; i++)
          cx0 += s.C[r0 + i] * SMPC_XLANE(x, i);
        if (GR > NT)
          for (int i = 0; i < N; i++)
            cx1 += s.C[r1 + i] * SMPC_XLANE(x, i);
        for (int j = 0; j < N; j++)
          hx += Hg[j * NP + col] * SMPC_XLANE(x, j); // (H is symmetric: coalesced along the row of j)
        for (int k = 0; k < GR0; k++)
          cl += s.C[k * LDC + col] * SMPC_XLANE(lamg0, k);
        for (int k = NT; k < GR; k++)
          cl += s.C[k * LDC + col] * SMPC_XLANE(lamg1, k - NT);
        if (lane < GR)
        {
          pr = fabs(cx0 - SMPC_PLV(zg0));
          np = fmax(fabs(cx0), fabs(SMPC_PLV(zg0)));
        }
        if (lane + NT < GR)
        {
          const double p1 = fabs(cx1 - SMPC_PLV(zg1)), n1 = fmax(fabs(cx1), fabs(SMPC_PLV(zg1)));
          pr = (p1 != p1) ? p1 : ((pr != pr) ? pr : fmax(pr, p1));
          np = (n1 != n1) ? n1 : ((np != np) ? np : fmax(np, n1));
        }
        if (lane < N)
        { // box rows: C x = x
          const double pb = fabs(SMPC_PLV(x) - SMPC_PLV(zb)), nb = fmax(fabs(SMPC_PLV(x)), fabs(SMPC_PLV(zb)));
          pr = (pb != pb) ? pb : ((pr != pr) ? pr : fmax(pr, pb));
          np = (nb != nb) ? nb : ((np != np) ? np : fmax(np, nb));
          du = fabs((SMPC_PLV(g) + hx) + cl);
          nd = fmax(fabs(hx), fmax(fabs(cl), fabs(SMPC_PLV(g))));
        }
        s.red[lane] = pr;
        s.red[64 + lane] = du;
        s.red[128 + lane] = np;
        s.red[192 + lane] = nd;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane < 4)
      {
        double m = 0.0; // (a NaN entry must survive the reduction: fmax would drop it and a failed solve would look converged)
        for (int i = 0; i < NT; i++)
        {
          const double v = s.red[64 * lane + i];
          m = (v != v) ? v : ((m != m) ? m : fmax(m, v));
        }
        s.red4[lane] = m;
      }
      SMPC_LANES_END_WAVE
      for (int i = 0; i < 4; i++)
        rs[i] = s.red4[i];
    };
    factor();
    bool done = false;
    for (int it = 0; it < st.admm_iters; it++)
    {
      if (it > 0 && it % ADMM_CHECK == 0)
      {
        residual();
        if (st.admm_tol >= 0.0 && fmax(rs[0], rs[1]) <= st.admm_tol)
        {
          done = true;
          break;
        }
        const double est = fmin(fmax(rho * sqrt((rs[0] / (rs[2] + 1e-10)) / (rs[1] / (rs[3] + 1e-10) + 1e-10)), 1e-6), 1e6);
        if (fmax(rs[0], rs[1]) > ADMM_ADAPT_FLOOR && (est > 5.0 * rho || est < 0.2 * rho)) // (below the floor the ratio is rounding noise)
        {
          rho = est;
          factor();
        }
      }
      SMPC_LANES(NT)
      {
        SMPC_PLV(wg0) = SMPC_PLV(rg0) * SMPC_PLV(zg0) - SMPC_PLV(lamg0);
        SMPC_PLV(wg1) = SMPC_PLV(rg1) * SMPC_PLV(zg1) - SMPC_PLV(lamg1);
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      { // rhs = sigma x - g + C^T (r z - lam): the box rows contribute their own entry
        const int col = lane < NP ? lane : 0;
        double acc = sigma * SMPC_PLV(x) - SMPC_PLV(g);
        acc += lane < N ? SMPC_PLV(rb) * SMPC_PLV(zb) - SMPC_PLV(lamb) : 0.0; // (a select, not a branch: the cross-lane reads below stay in this block)
        for (int k = 0; k < GR0; k++)
          acc += s.C[k * LDC + col] * SMPC_XLANE(wg0, k);
        for (int k = NT; k < GR; k++)
          acc += s.C[k * LDC + col] * SMPC_XLANE(wg1, k - NT);
        SMPC_PLV(rhs) = acc;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        const int col = lane < NP ? lane : 0;
        double acc = 0.0;
        for (int j = 0; j < N; j++) // (the padding variables are decoupled: their rows and columns of K^-1 are the identity's, their rhs is 0)
          acc += s.K[j * NP + col] * SMPC_XLANE(rhs, j); // (K^-1 is symmetric: read along the row of j, conflict-free)
        SMPC_PLV(xt) = acc;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        const int r0 = (lane < GR ? lane : 0) * LDC, r1 = (lane + NT < GR ? lane + NT : 0) * LDC;
        double zt0 = 0.0, zt1 = 0.0;
        for (int i = 0; i < N; i++) // (columns N .. NP - 1 of C are zero)
          zt0 += s.C[r0 + i] * SMPC_XLANE(xt, i);
        if (GR > NT)
          for (int i = 0; i < N; i++)
            zt1 += s.C[r1 + i] * SMPC_XLANE(xt, i);
        { // box rows: z~ = x~
          const double zh = alpha * SMPC_PLV(xt) + (1.0 - alpha) * SMPC_PLV(zb);
          const double zn = fmin(fmax(zh + SMPC_PLV(lamb) / SMPC_PLV(rb), SMPC_PLV(lb)), SMPC_PLV(ub));
          SMPC_PLV(lamb) += SMPC_PLV(rb) * (zh - zn);
          SMPC_PLV(zb) = zn;
        }
        {
          const double zh = alpha * zt0 + (1.0 - alpha) * SMPC_PLV(zg0);
          const double zn = fmin(fmax(zh + SMPC_PLV(lamg0) / SMPC_PLV(rg0), SMPC_PLV(lg0)), SMPC_PLV(ug0));
          SMPC_PLV(lamg0) += SMPC_PLV(rg0) * (zh - zn);
          SMPC_PLV(zg0) = zn;
        }
        {
          const double zh = alpha * zt1 + (1.0 - alpha) * SMPC_PLV(zg1);
          const double zn = fmin(fmax(zh + SMPC_PLV(lamg1) / SMPC_PLV(rg1), SMPC_PLV(lg1)), SMPC_PLV(ug1));
          SMPC_PLV(lamg1) += SMPC_PLV(rg1) * (zh - zn);
          SMPC_PLV(zg1) = zn;
        }
        SMPC_PLV(x) = alpha * SMPC_PLV(xt) + (1.0 - alpha) * SMPC_PLV(x);
      }
      SMPC_LANES_END_WAVE
    }
    if (!done)
      residual();
    const double res = (rs[0] != rs[0] || rs[1] != rs[1]) ? rs[0] + rs[1] : fmax(rs[0], rs[1]);
    // the solution through LDS for the torque rows (red is free now)
    SMPC_LANES(NT)
    if (lane < NP)
      s.red[lane] = SMPC_PLV(x);
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      // the iterate is kept as the next tick's warm start only when the solve ended finite (see qp_admm_body)
      const bool ok = res == res && res < 1e300;
      if (ok && lane < NP)
        b.x[(size_t)inst * NP + lane] = SMPC_PLV(x);
      if (ok && lane < N)
      {
        b.z[(size_t)inst * MP + lane] = SMPC_PLV(zb);
        b.lam[(size_t)inst * MP + lane] = SMPC_PLV(lamb);
      }
      if (ok && lane < GR)
      {
        b.z[(size_t)inst * MP + N + lane] = SMPC_PLV(zg0);
        b.lam[(size_t)inst * MP + N + lane] = SMPC_PLV(lamg0);
      }
      if (ok && lane + NT < GR)
      {
        b.z[(size_t)inst * MP + N + NT + lane] = SMPC_PLV(zg1);
        b.lam[(size_t)inst * MP + N + NT + lane] = SMPC_PLV(lamg1);
      }
      if (lane < NV)
        b.a[(size_t)inst * NV + lane] = s.red[lane];
      if (lane < 3 * NF)
        b.f[(size_t)inst * 3 * NF + lane] = s.red[NV + lane];
      if (lane < NA)
      { // tau = M_a a + h_a - J_a^T f
        const double * Mq = b.Mq + (size_t)inst * NV * NV;
        const double * J = b.J + (size_t)inst * 3 * NF * NV;
        double acc = b.nle[(size_t)inst * NV + 6 + lane];
        for (int k = 0; k < NV; k++)
          acc += Mq[(6 + lane) * NV + k] * s.red[k];
        for (int r = 0; r < 3 * NF; r++)
          acc -= J[r * NV + 6 + lane] * s.red[NV + r];
        b.tau[(size_t)inst * NA + lane] = acc;
      }
      if (lane == 0)
      {
        b.resid[inst] = res;
        b.rho[inst] = ok ? rho : st.rho;
        b.warm[inst] = ok ? 1 : 0;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // =====================================================================================================================
  // Flat feet (tsid Contact6d) on the run-time tree: any validated table with 2 flat feet.  n = nv + 24 variables (12 corner forces per foot),
  // general rows 6 dynamics | 12 LOCAL contact motion | 34 friction / normal-force bound | nv - 6 actuation.  The three kernels are
  // id_quant_body<FullTalos>'s flat-foot store phase, id6_assemble_body and qp6_admm_body (smpc_id.h) with run-time nv, strides and loop bounds.
  // =====================================================================================================================
  struct IdRt6Buffers : IdRtBuffers
  {
    double *footR = nullptr, *quad = nullptr; // [B][2][9] foot rotations ; [2][4][3] corners of the soles in their foot frames
  };

  // ---- kernel 1 (flat feet): the tree walk of id_quant_rt_body, then the LOCAL 6-D rows of every foot ----   grid = B, 64 lanes
  // rt_tree_phases leaves the LOCAL_WORLD_ALIGNED pieces (sim_rt_body's 6-D rows: [S.l + S.a x p ; S.a], drift [a_p ; alpha]); tsid's Contact6d
  // works in the foot's LOCAL frame: [R_f^T lin ; R_f^T ang] of the Jacobian, of the drift (classical acceleration at zero joint
  // accelerations) and of the frame velocity -- the convention of the oracle's id_quantities(force_size = 6).
  SMPC_DEV void id6_quant_rt_body(const IdRt6Buffers & b, int block)
  {
    typedef IdQuantRtScratch SC;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = ID_RT6_NFEET;
    static_assert(NF <= SC::NF && 6 * NF <= 32 && 32 + 3 * NF <= NT, "feet of the scratch block; lane maps of the store phase");
    const int inst = block;
    const IdRtDevModel & mi = *b.model;
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nx = 2 * nj + 11;
    SMPC_LDS(SC, scs, 1);
    SC & sc = scs[0];
    // ---- phases 0 .. 4 ----
    rt_tree_phases(sc, mi, b.X + (size_t)inst * nx, mk3(0.0, 0.0, -9.81));
    // ---- phase 5: every global store ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < nv * nv; idx += NT)
      {
        const int r = idx / nv, c = idx % nv;
        const int lo = r < c ? r : c, hi = r < c ? c : r; // (one expression for both triangles: M is symmetric bit for bit)
        const int jl = lo < 6 ? 0 : lo - 5, jh = hi < 6 ? 0 : hi - 5;
        b.Mq[(size_t)inst * nv * nv + idx] = ((sc.anc[jh] >> jl) & 1u) ? id_rt_dot6(&sc.S[lo * 6], &sc.F[hi * 6]) : 0.0;
      }
      if (lane < nv)
        b.nle[(size_t)inst * nv + lane] = sc.h[lane];
      for (int idx = lane; idx < 6 * NF * nv; idx += NT)
      {
        const int r = idx / nv, k = idx % nv, f = r / 6, blk = (r % 6) / 3, i = r % 3;
        const int jk = k < 6 ? 0 : k - 5, jf = sc.fj[f];
        double val = 0.0;
        if ((sc.anc[jf] >> jk) & 1u)
        { // twist of the foot frame under the unit velocity of column k, turned into the foot frame
          const SV s = ldsv(&sc.S[k * 6]);
          const V3 w = blk == 0 ? s.l + cross(s.a, ld3(&sc.footp[f * 3])) : s.a;
          const double * Rf = &sc.oR[jf * 9];
          val = Rf[i] * w.x + Rf[3 + i] * w.y + Rf[6 + i] * w.z;
        }
        b.J[(size_t)inst * 6 * NF * nv + idx] = val;
      }
      if (lane < 6 * NF)
      {
        const int f = lane / 6, blk = (lane % 6) / 3, i = lane % 3, jf = sc.fj[f];
        const double * Rf = &sc.oR[jf * 9];
        const V3 p = ld3(&sc.footp[f * 3]);
        const SV v = ldsv(&sc.vel[jf * 6]), a = ldsv(&sc.acc[jf * 6]);
        const V3 vp = v.l + cross(v.a, p);
        // classical acceleration of the frame origin at zero joint accelerations ; angular part: the bias angular acceleration
        const V3 ap = a.l + cross(a.a, p) + cross(v.a, vp);
        const V3 d = blk == 0 ? ap : a.a, w = blk == 0 ? vp : v.a;
        b.Jdv[(size_t)inst * 6 * NF + lane] = Rf[i] * d.x + Rf[3 + i] * d.y + Rf[6 + i] * d.z;
        b.vfoot[(size_t)inst * 6 * NF + lane] = Rf[i] * w.x + Rf[3 + i] * w.y + Rf[6 + i] * w.z;
      }
      if (lane >= 32 && lane < 32 + 3 * NF)
        b.footp[(size_t)inst * 3 * NF + lane - 32] = sc.footp[lane - 32];
      if (lane < 9 * NF)
        b.footR[(size_t)inst * 9 * NF + lane] = sc.oR[sc.fj[lane / 9] * 9 + lane % 9];
      if (lane < 3)
        b.com[(size_t)inst * 3 + lane] = sc.Ic[1 + lane] / sc.Ic[0];
    }
    SMPC_LANES_END_WAVE
  }

  // ---- kernel 2 (flat feet): QP data, id6_assemble_body term by term with run-time sizes ----
  SMPC_DEV void id6_assemble_rt_body(const IdRt6Buffers & b, int block)
  {
    constexpr int NT = 64, NF = ID_RT6_NFEET, NFV = ID_RT6_NFV, NM = ID_RT6_NM, NFR = ID_RT6_NFR, MAXV = ID_RT_MAX_NV;
    const int inst = block;
    const IdSettingsDev & s = b.s;
    const int NV = b.nv < MAXV ? (b.nv > 7 ? b.nv : 7) : MAXV, NQ = NV + 1, NX = 2 * NV + 1, NA = NV - 6;
    const int N = NV + NFV * NF, M = N + 6 + NM * NF + NFR * NF + NA, NP = ((N + 15) / 16) * 16, MP = ((M + 15) / 16) * 16;
    const int R_DYN = N, R_MOT = N + 6, R_FRI = R_MOT + NM * NF, R_ACT = R_FRI + NFR * NF;
    const double * x = b.X + (size_t)inst * NX;
    const double * q = x;
    const double * v = x + NQ;
    SMPC_LDS(double, sM, MAXV * MAXV);
    SMPC_LDS(double, sJ, NM * NF * MAXV);
    SMPC_LDS(double, JG, MAXV * NFV * NF); // J^T T per foot: generalised force of the corner forces
    SMPC_LDS(double, Jc, 3 * MAXV);
    SMPC_LDS(double, bc, 3);
    SMPC_LDS(double, bt, NM * NF);
    SMPC_LDS(double, e6, 6);
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NV * NV; idx += NT)
        sM[idx] = b.Mq[(size_t)inst * NV * NV + idx];
      for (int idx = lane; idx < NM * NF * NV; idx += NT)
        sJ[idx] = b.J[(size_t)inst * NM * NF * NV + idx];
    }
    SMPC_LANES_END_WAVE
    const double * Mq = sM;
    const double * nle = b.nle + (size_t)inst * NV;
    const double * J = sJ;
    const double * Jdv = b.Jdv + (size_t)inst * NM * NF;
    const double * vf = b.vfoot + (size_t)inst * NM * NF;
    const double *tq = b.tx + (size_t)inst * NX, *tv = tq + NQ, *ta = b.ta + (size_t)inst * NV, *tf = b.tf + (size_t)inst * 6 * NF;
    const unsigned mask = b.tmask[inst];
    double * H = b.H + (size_t)inst * NP * NP;
    double * g = b.g + (size_t)inst * NP;
    double * C = b.C + (size_t)inst * MP * NP;
    double * l = b.l + (size_t)inst * MP;
    double * u = b.u + (size_t)inst * MP;
    const double total_mass = b.model->total_mass;
    const double kdp = 2.0 * sqrt(s.kp_posture), kdb = 2.0 * sqrt(s.kp_base), kdc = 2.0 * sqrt(s.kp_contact);
    const double kdm = 2.0 * sqrt(s.kp_com), kdt = 2.0 * sqrt(s.kp_feet_tracking);
    const bool com_task = s.centroidal && s.w_com > 0, track_task = s.centroidal && s.w_feet_tracking > 0;
    const bool mot_cost = !s.contact_motion_equality && s.w_contact_motion > 0;
    const int base0 = s.centroidal ? 3 : 0;
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NV * NFV * NF; idx += NT)
      {
        const int k = idx / (NFV * NF), c = idx % (NFV * NF), f = c / NFV, cc = c % NFV;
        double acc = 0.0;
        for (int r = 0; r < 6; r++)
          acc += J[(6 * f + r) * NV + k] * id6_tgen(b.quad, f, r, cc);
        JG[idx] = acc;
      }
      if (com_task)
        for (int idx = lane; idx < 3 * NV; idx += NT)
        {
          const int i = idx / NV, k = idx % NV;
          const M3 Rb = quat_to_R(Quat{q[3], q[4], q[5], q[6]});
          const double im = 1.0 / total_mass;
          const double r0 = i == 0 ? Rb.a00 : (i == 1 ? Rb.a10 : Rb.a20), r1 = i == 0 ? Rb.a01 : (i == 1 ? Rb.a11 : Rb.a21),
                       r2 = i == 0 ? Rb.a02 : (i == 1 ? Rb.a12 : Rb.a22);
          Jc[idx] = im * (r0 * Mq[k] + r1 * Mq[NV + k] + r2 * Mq[2 * NV + k]);
        }
      if (lane == 63)
      { // base error log6(M_b^-1 M_t), local frame
        const SE3 Mb{quat_to_R(Quat{q[3], q[4], q[5], q[6]}), mk3(q[0], q[1], q[2])};
        const SE3 Mt{quat_to_R(Quat{tq[3], tq[4], tq[5], tq[6]}), mk3(tq[0], tq[1], tq[2])};
        V3 ev, ew;
        log6(se3_mul(se3_inv(Mb), Mt), ev, ew);
        st3(e6, ev);
        st3(e6 + 3, ew);
      }
      if (track_task && lane >= 32 && lane < 32 + NF)
      { // feet in the air: 6-D LOCAL task towards (identity rotation, target position), zero angular velocity target
        const int f = lane - 32;
        const size_t o = (size_t)inst * 3 * NF + 3 * f;
        const M3 Rf = ldm3(b.footR + ((size_t)inst * NF + f) * 9);
        const SE3 Mf{Rf, ld3(b.footp + o)}, Mr{m3_id(), ld3(b.tfp + o)};
        V3 ev, ew;
        log6(se3_mul(se3_inv(Mf), Mr), ev, ew);
        const V3 vr = tmul(Rf, ld3(b.tfv + o));
        const double e[6] = {ev.x, ev.y, ev.z, ew.x, ew.y, ew.z}, vrr[6] = {vr.x, vr.y, vr.z, 0.0, 0.0, 0.0};
        for (int i = 0; i < 6; i++)
          bt[6 * f + i] = s.kp_feet_tracking * e[i] + kdt * (vrr[i] - vf[6 * f + i]) - Jdv[6 * f + i];
      }
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    if (com_task && lane < 3)
    {
      const int i = lane;
      const M3 Rb = quat_to_R(Quat{q[3], q[4], q[5], q[6]});
      const double im = 1.0 / total_mass;
      const double r0 = i == 0 ? Rb.a00 : (i == 1 ? Rb.a10 : Rb.a20), r1 = i == 0 ? Rb.a01 : (i == 1 ? Rb.a11 : Rb.a21),
                   r2 = i == 0 ? Rb.a02 : (i == 1 ? Rb.a12 : Rb.a22);
      double vc = 0.0;
      for (int k = 0; k < NV; k++)
        vc += Jc[i * NV + k] * v[k];
      const double dr = im * (r0 * nle[0] + r1 * nle[1] + r2 * nle[2]) + (i == 2 ? -9.81 : 0.0);
      bc[i] = s.kp_com * (b.tcom[(size_t)inst * 3 + i] - b.com[(size_t)inst * 3 + i]) + kdm * (b.tvcom[(size_t)inst * 3 + i] - vc) - dr;
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      // ---- H (N x N, padded with unit diagonal) and g ----
      for (int idx = lane; idx < NP * NP; idx += NT)
      {
        const int i = idx / NP, j = idx % NP;
        double h = 0.0;
        if (i >= N || j >= N)
          h = (i == j) ? 1.0 : 0.0; // padding variables: pinned by their own unit curvature and zero gradient
        else
        {
          if (i == j && i >= 6 && i < NV && s.w_posture > 0)
            h += s.w_posture;
          if (i == j && i >= base0 && i < 6 && s.w_base > 0)
            h += s.w_base;
          if (i < NV && j < NV)
          {
            if (com_task)
              for (int r = 0; r < 3; r++)
                h += s.w_com * Jc[r * NV + i] * Jc[r * NV + j];
            for (int f = 0; f < NF; f++)
            {
              const bool on = (mask >> f) & 1u;
              const double w = on ? (mot_cost ? s.w_contact_motion : 0.0) : (track_task ? s.w_feet_tracking : 0.0);
              if (w != 0.0)
                for (int r = 6 * f; r < 6 * f + 6; r++)
                  h += w * J[r * NV + i] * J[r * NV + j];
            }
          }
          if (i >= NV && j >= NV && (i - NV) / NFV == (j - NV) / NFV && s.w_contact_force > 0 && ((mask >> ((i - NV) / NFV)) & 1u))
          { // force regularisation: T^T diag(w^2) T of the foot
            const int f = (i - NV) / NFV, a = (i - NV) % NFV, c = (j - NV) % NFV;
            double acc = 0.0;
            for (int r = 0; r < 6; r++)
              acc += id6_tgen(b.quad, f, r, a) * id6_wrench_w(r) * id6_wrench_w(r) * id6_tgen(b.quad, f, r, c);
            h += s.w_contact_force * acc;
          }
        }
        H[idx] = h;
      }
      for (int i = lane; i < NP; i += NT)
      {
        double gi = 0.0;
        if (i < N)
        {
          if (i >= 6 && i < NV && s.w_posture > 0)
            gi -= s.w_posture * (ta[i] + s.kp_posture * (tq[i + 1] - q[i + 1]) + kdp * (tv[i] - v[i]));
          if (i >= base0 && i < 6 && s.w_base > 0)
          {
            const V3 dr = cross(mk3(v[3], v[4], v[5]), mk3(v[0], v[1], v[2]));
            const double ades = s.base_as_coded ? s.kp_base * e6[i] + kdb * (ta[i] - v[i]) : s.kp_base * e6[i] + kdb * (tv[i] - v[i]) + ta[i];
            gi -= s.w_base * (ades - (i == 0 ? dr.x : (i == 1 ? dr.y : (i == 2 ? dr.z : 0.0))));
          }
          if (i < NV)
          {
            if (com_task)
              for (int r = 0; r < 3; r++)
                gi -= s.w_com * Jc[r * NV + i] * bc[r];
            for (int f = 0; f < NF; f++)
            {
              const bool on = (mask >> f) & 1u;
              if (on && mot_cost)
                for (int r = 6 * f; r < 6 * f + 6; r++)
                  gi -= s.w_contact_motion * J[r * NV + i] * (-Jdv[r] - kdc * vf[r]);
              if (!on && track_task)
                for (int r = 6 * f; r < 6 * f + 6; r++)
                  gi -= s.w_feet_tracking * J[r * NV + i] * bt[r];
            }
          }
          if (i >= NV && s.w_contact_force > 0 && ((mask >> ((i - NV) / NFV)) & 1u))
          {
            const int f = (i - NV) / NFV, a = (i - NV) % NFV;
            double acc = 0.0;
            for (int r = 0; r < 6; r++)
              acc += id6_tgen(b.quad, f, r, a) * id6_wrench_w(r) * id6_wrench_w(r) * tf[6 * f + r];
            gi -= s.w_contact_force * acc;
          }
        }
        g[i] = gi;
      }
      // ---- general rows of C, l, u ----  (rows 0 .. N-1, the box on y, are the identity and the padding rows are zero: written once when the
      //                                     engine is created)
      for (int idx = N * NP + lane; idx < M * NP; idx += NT)
      {
        const int r = idx / NP, c = idx % NP;
        double val = 0.0;
        if (c < N && r < R_MOT)
        { // dynamics rows: [M_b | -(J^T T)_b]
          const int i = r - R_DYN;
          val = c < NV ? Mq[i * NV + c] : -JG[i * (NFV * NF) + c - NV];
        }
        else if (c < N && r < R_FRI)
        { // contact motion rows (equality variant, feet in contact)
          const int rr = r - R_MOT;
          if (s.contact_motion_equality && ((mask >> (rr / 6)) & 1u) && c < NV)
            val = J[rr * NV + c];
        }
        else if (c < N && r < R_ACT)
        { // per corner k of foot f: rows 4 k + m: +-f_x - mu f_z, +-f_y - mu f_z ; row 16: sum of the normal forces
          const int rr = r - R_FRI, f = rr / 17, m = rr % 17;
          if (((mask >> f) & 1u) && c >= NV + NFV * f && c < NV + NFV * (f + 1))
          {
            const int cc = c - NV - NFV * f, k = cc / 3, j = cc % 3;
            if (m == 16)
              val = j == 2 ? 1.0 : 0.0;
            else if (m / 4 == k)
              val = j == 2 ? -s.friction_coefficient : (j == (m % 4) / 2 ? ((m % 2 == 0) ? 1.0 : -1.0) : 0.0);
          }
        }
        else if (c < N && r < M)
        { // actuation rows: [M_a | -(J^T T)_a]
          const int j = r - R_ACT;
          val = c < NV ? Mq[(6 + j) * NV + c] : -JG[(6 + j) * (NFV * NF) + c - NV];
        }
        C[idx] = val;
      }
      for (int r = lane; r < MP; r += NT)
      {
        double lo = -ID_INF, hi = ID_INF;
        const double W = total_mass * 9.81, dt = s.control_dt;
        if (r >= 6 && r < NV)
        {
          const int j = r - 6;
          const double qa = q[7 + j], va = v[6 + j];
          lo = fmax((-b.v_max[j] - va) / dt, 2.0 * (b.q_min[j] - qa - va * dt) / (dt * dt));
          hi = fmin((b.v_max[j] - va) / dt, 2.0 * (b.q_max[j] - qa - va * dt) / (dt * dt));
          if (lo > hi)
            lo = hi = fmin(lo, hi);
          if (s.tsid_bounds)
            id_tsid_acc_limits(qa, va, b.q_min[j], b.q_max[j], b.v_max[j], dt, lo, hi);
        }
        else if (r >= NV && r < N)
        {
          if (!((mask >> ((r - NV) / NFV)) & 1u))
            lo = hi = 0.0;
        }
        else if (r >= N && r < R_MOT)
          lo = hi = -nle[r - R_DYN];
        else if (r >= R_MOT && r < R_FRI)
        {
          const int rr = r - R_MOT;
          if (s.contact_motion_equality && ((mask >> (rr / 6)) & 1u))
            lo = hi = -Jdv[rr] - kdc * vf[rr];
        }
        else if (r >= R_FRI && r < R_ACT)
        {
          const int rr = r - R_FRI;
          if ((mask >> (rr / 17)) & 1u)
          {
            if (rr % 17 == 16)
            {
              lo = s.ratio_min * W;
              hi = s.ratio_max * W;
            }
            else
              hi = 0.0;
          }
        }
        else if (r >= R_ACT && r < M)
        {
          const int j = r - R_ACT;
          lo = -b.tau_max[j] - nle[6 + j];
          hi = b.tau_max[j] - nle[6 + j];
        }
        l[r] = lo;
        u[r] = hi;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // ---- kernel 3 (flat feet): ADMM ----
  // The row structure of qp6_admm_body: lane i < n owns variable i and box row i, lane d < dr the DENSE general row d (dynamics |
  // contact motion | actuation: dr = 18 + na <= 49), lane rr < 34 the friction row rr; the friction rows' products and their 12 x 12 blocks of
  // C^T diag(r) C go in closed form (fric_t / fric_r).  What qp6_admm_body keeps in registers -- rows of K^-1, rows and columns of the dense part
  // of C -- lives in LDS here, as in qp_admm_rt_body (row stride NP + 1: a product down a column and one along a row are both conflict-free);
  // sizes are kernel arguments.  Every dot product is ONE accumulator in ascending index order; K = (H + sigma I + box and friction terms) + the
  // dense product, in that order.  K stays in LDS beside its inverse: the linear solve of every iteration takes one step of iterative refinement.
  template <int NP>
  struct Qp6RtLds
  {
    static constexpr int DRMAX = NP - 12 < ID_RT6_MAX_DR ? NP - 12 : ID_RT6_MAX_DR; // n <= NP  =>  nv <= NP - 24  =>  dense rows nv + 12 <= NP - 12
    static constexpr int DRK = ((DRMAX + 3) / 4) * 4, LDC = NP + 1;
    double K[NP * NP];  // K, then its inverse
    double Kf[NP * NP]; // K itself: the refinement step of the linear solve needs it beside the inverse
    double C[DRK * LDC];
    double rd[64];
    double swp[2 * 4 * 16 * ((2 * NP + 15) / 16)];
    double wfl[64], xl[64]; // friction-row vector / variable vector handed across lanes
    double red[256], red4[4];
  };

  template <int NP>
  SMPC_DEV void qp6_admm_rt_body(const IdRt6Buffers & b, int block)
  {
    typedef Qp6RtLds<NP> L;
    constexpr int NT = 64, NF = ID_RT6_NFEET, NFV = ID_RT6_NFV, NM = ID_RT6_NM, FR = ID_RT6_FR, LDC = L::LDC, DRMAX = L::DRMAX, DRK = L::DRK;
    static_assert(NP <= NT && DRK <= NT && FR <= NT && ID_RT6_NFR == 17 && NFV == 12, "one variable / dense row / friction row per lane; Contact6d rows");
    const int inst = block;
    const IdSettingsDev & st = b.s;
    const double sigma = st.sigma, alpha = st.alpha, fmu = st.friction_coefficient;
    // (sizes: kernel arguments, clamped to what this instantiation holds)
    const int NVmax = NP - NFV * NF < ID_RT_MAX_NV ? NP - NFV * NF : ID_RT_MAX_NV;
    const int NV = b.nv < NVmax ? (b.nv > 7 ? b.nv : 7) : NVmax, NA = NV - 6, N = NV + NFV * NF;
    const int DR = 6 + NM * NF + NA, M = N + DR + FR, MP = ((M + 15) / 16) * 16;
    const int R_FRI = 6 + NM * NF; // first friction row among the general rows
    SMPC_LDS(L, ls, 1);
    L & s = ls[0];
    const double * Hg = b.H + (size_t)inst * NP * NP;
    const double * Cg = b.C + (size_t)inst * MP * NP + (size_t)N * NP; // general rows
    const unsigned mask = b.tmask[inst];
    const bool warm = b.warm[inst] != 0;
    double rho = warm ? b.rho[inst] : st.rho;
    // general row of dense row d
    auto drow = [&](int d) { return d < R_FRI ? d : d + FR; };
    SMPC_PL(double, x, NT);
    SMPC_PL(double, g, NT);
    SMPC_PL(double, rhs, NT);
    SMPC_PL(double, xt, NT);
    SMPC_PL(double, zb, NT);
    SMPC_PL(double, lamb, NT);
    SMPC_PL(double, lb, NT);
    SMPC_PL(double, ub, NT);
    SMPC_PL(double, rb, NT);
    SMPC_PL(double, zd, NT);
    SMPC_PL(double, lamd, NT);
    SMPC_PL(double, ld, NT);
    SMPC_PL(double, ud, NT);
    SMPC_PL(double, rdv, NT);
    SMPC_PL(double, wd, NT);
    SMPC_PL(double, zf, NT);
    SMPC_PL(double, lamf, NT);
    SMPC_PL(double, lf, NT);
    SMPC_PL(double, uf, NT);
    SMPC_PL(double, rf, NT);
    // ---- lane roles of the friction structure: those of qp6_admm_body ----
    // C^T w of the friction rows for variable lane `lane` (0 for the accelerations), w read from s.wfl
    auto fric_t = [&](int lane) {
      const int c = lane - NV;
      if (c < 0 || c >= NFV * NF)
        return 0.0;
      const int f = c / NFV, k = (c % NFV) / 3, j = c % 3;
      if (!((mask >> f) & 1u))
        return 0.0;
      const double * w = s.wfl + 17 * f;
      if (j < 2)
        return w[4 * k + 2 * j] - w[4 * k + 2 * j + 1];
      return w[16] - fmu * (w[4 * k] + w[4 * k + 1] + w[4 * k + 2] + w[4 * k + 3]);
    };
    // C y of friction row `lane` (y read from s.xl)
    auto fric_r = [&](int lane) {
      if (lane >= FR)
        return 0.0;
      const int f = lane / 17, m = lane % 17;
      if (!((mask >> f) & 1u))
        return 0.0;
      const double * y = s.xl + NV + NFV * f;
      if (m == 16)
        return y[2] + y[5] + y[8] + y[11];
      const int k = m / 4, j = (m % 4) / 2;
      return ((m % 2 == 0) ? y[3 * k + j] : -y[3 * k + j]) - fmu * y[3 * k + 2];
    };
    SMPC_LANES(NT)
    {
      // dense general rows of C -> LDS (rows DR .. DRK - 1: zero, they are K-steps of the matrix product below)
      for (int idx = lane; idx < DRK * NP; idx += NT)
      {
        const int k = idx / NP, i = idx % NP;
        s.C[k * LDC + i] = k < DR ? Cg[(size_t)drow(k) * NP + i] : 0.0;
      }
      const int i = lane < NP ? lane : 0, kb = lane < N ? lane : 0;
      const int kd = N + drow(lane < DR ? lane : 0), kf = N + R_FRI + (lane < FR ? lane : 0);
      SMPC_PLV(g) = b.g[(size_t)inst * NP + i];
      SMPC_PLV(x) = warm ? b.x[(size_t)inst * NP + i] : 0.0;
      SMPC_PLV(rhs) = SMPC_PLV(xt) = SMPC_PLV(wd) = 0.0;
      auto row = [&](int k, double & lo_, double & hi_, double & z_, double & lam_) {
        const double lo = b.l[(size_t)inst * MP + k], hi = b.u[(size_t)inst * MP + k];
        lo_ = lo;
        hi_ = hi;
        z_ = warm ? b.z[(size_t)inst * MP + k] : fmin(fmax(0.0, lo), hi);
        lam_ = warm ? b.lam[(size_t)inst * MP + k] : 0.0;
      };
      row(kb, SMPC_PLV(lb), SMPC_PLV(ub), SMPC_PLV(zb), SMPC_PLV(lamb));
      row(kd, SMPC_PLV(ld), SMPC_PLV(ud), SMPC_PLV(zd), SMPC_PLV(lamd));
      row(kf, SMPC_PLV(lf), SMPC_PLV(uf), SMPC_PLV(zf), SMPC_PLV(lamf));
      SMPC_PLV(rb) = SMPC_PLV(rdv) = SMPC_PLV(rf) = 1.0;
    }
    SMPC_LANES_END_WAVE
    // row weights r = rho (1e3 rho on equality rows, 1e-6 rho on free rows) ; K = H + sigma I + C^T diag(r) C -> its inverse in LDS
    auto factor = [&]() {
      SMPC_LANES(NT)
      {
        auto weight = [&](double lo, double hi) { return (hi - lo < 1e-12) ? 1e3 * rho : ((lo <= -ID_INF && hi >= ID_INF) ? 1e-6 * rho : rho); };
        SMPC_PLV(rb) = weight(SMPC_PLV(lb), SMPC_PLV(ub));
        SMPC_PLV(rdv) = weight(SMPC_PLV(ld), SMPC_PLV(ud));
        SMPC_PLV(rf) = weight(SMPC_PLV(lf), SMPC_PLV(uf));
        s.rd[lane] = lane < DR ? SMPC_PLV(rdv) : 0.0;
        s.wfl[lane] = lane < FR ? SMPC_PLV(rf) : 0.0;
        s.xl[lane] = lane < N ? SMPC_PLV(rb) : 0.0;
      }
      SMPC_LANES_END_WAVE
      // H + sigma I + the box and friction terms into K first (their own lane phase: the closed-form blocks need registers the accumulators
      // of the product hold afterwards) ; the dense product is added last
      SMPC_LANES(NT)
      for (int idx = lane; idx < NP * NP; idx += NT)
      {
        const int i = idx / NP, j = idx % NP;
        double kk = Hg[idx] + (i == j ? sigma + s.xl[i] : 0.0);
        // friction rows: 12 x 12 block per foot in contact
        const int ci = i - NV, cj = j - NV;
        if (ci >= 0 && cj >= 0 && ci < NFV * NF && cj < NFV * NF && ci / NFV == cj / NFV && ((mask >> (ci / NFV)) & 1u))
        {
          const int f = ci / NFV, ki = (ci % NFV) / 3, ji = ci % 3, kj = (cj % NFV) / 3, jj = cj % 3;
          const double * r = s.wfl + 17 * f;
          if (ki == kj)
          {
            const double * q = r + 4 * ki;
            if (ji == jj)
              kk += ji == 0 ? q[0] + q[1] : (ji == 1 ? q[2] + q[3] : fmu * fmu * (q[0] + q[1] + q[2] + q[3]) + r[16]);
            else if (ji == 2 || jj == 2)
            {
              const int t = ji == 2 ? jj : ji; // the tangential component of the pair
              kk -= fmu * (q[2 * t] - q[2 * t + 1]);
            }
          }
          else if (ji == 2 && jj == 2)
            kk += r[16];
        }
        s.K[idx] = kk;
      }
      SMPC_LANES_END_WAVE
      fwave_gemm<NP, NP, DRK>(
        [&](int i, int k) { return s.rd[k] * s.C[k * LDC + i]; }, [&](int k, int j) { return s.C[k * LDC + j]; },
        [&](int i, int j, double v) {
          const double kk = s.K[i * NP + j] + v;
          s.K[i * NP + j] = kk;
          s.Kf[i * NP + j] = kk;
        });
      fwave_spd_inverse<NP>(s.K, s.swp);
    };
    // residuals of the iterate and the norms they are measured against (the same values in every lane):
    //   rs[0] = |C x - z|_inf, rs[1] = |H x + g + C^T lam|_inf, rs[2] = max(|C x|, |z|)_inf, rs[3] = max(|H x|, |C^T lam|, |g|)_inf
    double rs[4] = {0.0, 0.0, 0.0, 0.0};
    auto residual = [&]() {
      SMPC_LANES(NT)
      {
        s.xl[lane] = lane < N ? SMPC_PLV(x) : 0.0;
        s.wfl[lane] = lane < FR ? SMPC_PLV(lamf) : 0.0;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        auto nmax = [](double m, double v) { return (v != v) ? v : ((m != m) ? m : fmax(m, v)); }; // (a NaN entry survives)
        double pr = 0.0, np = 0.0, du = 0.0, nd = 0.0;
        double cx = 0.0, hx = 0.0, cl = SMPC_PLV(lamb);
        const int r0 = (lane < DR ? lane : 0) * LDC, col = lane < NP ? lane : 0;
        for (int i = 0; i < N; i++)
          cx += s.C[r0 + i] * SMPC_XLANE(x, i);
        for (int j = 0; j < N; j++)
          hx += Hg[j * NP + col] * SMPC_XLANE(x, j); // (H is symmetric: coalesced along the row of j)
        for (int k = 0; k < DR; k++)
          cl += s.C[k * LDC + col] * SMPC_XLANE(lamd, k);
        cl += fric_t(lane);
        const double cf = fric_r(lane);
        if (lane < DR)
        {
          pr = fabs(cx - SMPC_PLV(zd));
          np = fmax(fabs(cx), fabs(SMPC_PLV(zd)));
        }
        if (lane < FR)
        {
          pr = nmax(pr, fabs(cf - SMPC_PLV(zf)));
          np = nmax(np, fmax(fabs(cf), fabs(SMPC_PLV(zf))));
        }
        if (lane < N)
        { // box rows: C x = x
          pr = nmax(pr, fabs(SMPC_PLV(x) - SMPC_PLV(zb)));
          np = nmax(np, fmax(fabs(SMPC_PLV(x)), fabs(SMPC_PLV(zb))));
          du = fabs((SMPC_PLV(g) + hx) + cl);
          nd = fmax(fabs(hx), fmax(fabs(cl), fabs(SMPC_PLV(g))));
        }
        s.red[lane] = pr;
        s.red[64 + lane] = du;
        s.red[128 + lane] = np;
        s.red[192 + lane] = nd;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane < 4)
      {
        double m = 0.0; // (a NaN entry must survive the reduction: fmax would drop it and a failed solve would look converged)
        for (int i = 0; i < NT; i++)
        {
          const double v = s.red[64 * lane + i];
          m = (v != v) ? v : ((m != m) ? m : fmax(m, v));
        }
        s.red4[lane] = m;
      }
      SMPC_LANES_END_WAVE
      for (int i = 0; i < 4; i++)
        rs[i] = s.red4[i];
    };
    factor();
    bool done = false;
    for (int it = 0; it < st.admm_iters; it++)
    {
      if (it > 0 && it % ADMM_CHECK == 0)
      {
        residual();
        if (st.admm_tol >= 0.0 && fmax(rs[0], rs[1]) <= st.admm_tol)
        {
          done = true;
          break;
        }
        const double est = fmin(fmax(rho * sqrt((rs[0] / (rs[2] + 1e-10)) / (rs[1] / (rs[3] + 1e-10) + 1e-10)), 1e-6), 1e6);
        if (fmax(rs[0], rs[1]) > ADMM_ADAPT_FLOOR && (est > 5.0 * rho || est < 0.2 * rho)) // (below the floor the ratio is rounding noise)
        {
          rho = est;
          factor();
        }
      }
      SMPC_LANES(NT)
      {
        SMPC_PLV(wd) = SMPC_PLV(rdv) * SMPC_PLV(zd) - SMPC_PLV(lamd);
        s.wfl[lane] = lane < FR ? SMPC_PLV(rf) * SMPC_PLV(zf) - SMPC_PLV(lamf) : 0.0;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      { // rhs = sigma x - g + C^T (r z - lam): the box rows contribute their own entry, the friction rows their closed form
        const int col = lane < NP ? lane : 0;
        double acc = sigma * SMPC_PLV(x) - SMPC_PLV(g);
        acc += lane < N ? SMPC_PLV(rb) * SMPC_PLV(zb) - SMPC_PLV(lamb) : 0.0; // (a select, not a branch: the cross-lane reads below stay in this block)
        for (int k = 0; k < DR; k++)
          acc += s.C[k * LDC + col] * SMPC_XLANE(wd, k);
        acc += fric_t(lane);
        SMPC_PLV(rhs) = lane < N ? acc : 0.0;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        const int col = lane < NP ? lane : 0;
        double acc = 0.0;
        for (int j = 0; j < N; j++) // (the padding variables are decoupled: their rows and columns of K^-1 are the identity's, their rhs is 0)
          acc += s.K[j * NP + col] * SMPC_XLANE(rhs, j); // (K^-1 is symmetric: read along the row of j, conflict-free)
        SMPC_PLV(xt) = lane < N ? acc : 0.0;
      }
      SMPC_LANES_END_WAVE
      // one step of iterative refinement, x~ += K^-1 (rhs - K x~): the explicit inverse of a K of condition ~1e9 alone leaves x~ 1e-10 off a
      // backward-stable solve, which the rho adaptation amplifies to 1e-8 .. 1e-6 on iterates that have not converged
      SMPC_LANES(NT)
      {
        const int col = lane < NP ? lane : 0;
        double acc = SMPC_PLV(rhs);
        for (int j = 0; j < N; j++)
          acc -= s.Kf[j * NP + col] * SMPC_XLANE(xt, j); // (K is symmetric to rounding: read along the row of j, conflict-free)
        SMPC_PLV(wd) = lane < N ? acc : 0.0; // (wd is free until the next iteration)
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        const int col = lane < NP ? lane : 0;
        double acc = 0.0;
        for (int j = 0; j < N; j++)
          acc += s.K[j * NP + col] * SMPC_XLANE(wd, j);
        SMPC_PLV(xt) = lane < N ? SMPC_PLV(xt) + acc : 0.0;
        s.xl[lane] = SMPC_PLV(xt);
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      {
        const int r0 = (lane < DR ? lane : 0) * LDC;
        double acc = 0.0;
        for (int i = 0; i < N; i++) // (columns N .. NP - 1 of C are zero)
          acc += s.C[r0 + i] * SMPC_XLANE(xt, i);
        const double ztd = acc, ztf = fric_r(lane);
        auto upd = [&](double zt, double & z, double & lam, double r, double lo, double hi) {
          const double zh = alpha * zt + (1.0 - alpha) * z;
          const double zn = fmin(fmax(zh + lam / r, lo), hi);
          lam += r * (zh - zn);
          z = zn;
        };
        upd(SMPC_PLV(xt), SMPC_PLV(zb), SMPC_PLV(lamb), SMPC_PLV(rb), SMPC_PLV(lb), SMPC_PLV(ub)); // box rows: z~ = x~
        upd(ztd, SMPC_PLV(zd), SMPC_PLV(lamd), SMPC_PLV(rdv), SMPC_PLV(ld), SMPC_PLV(ud));
        upd(ztf, SMPC_PLV(zf), SMPC_PLV(lamf), SMPC_PLV(rf), SMPC_PLV(lf), SMPC_PLV(uf));
        SMPC_PLV(x) = alpha * SMPC_PLV(xt) + (1.0 - alpha) * SMPC_PLV(x);
      }
      SMPC_LANES_END_WAVE
    }
    if (!done)
      residual();
    const double res = (rs[0] != rs[0] || rs[1] != rs[1]) ? rs[0] + rs[1] : fmax(rs[0], rs[1]);
    SMPC_LANES(NT)
    s.xl[lane] = SMPC_PLV(x);
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      // the iterate is kept as the next tick's warm start only when the solve ended finite (see qp_admm_body)
      const bool ok = res == res && res < 1e300;
      if (ok && lane < NP)
        b.x[(size_t)inst * NP + lane] = SMPC_PLV(x);
      if (ok && lane < N)
      {
        b.z[(size_t)inst * MP + lane] = SMPC_PLV(zb);
        b.lam[(size_t)inst * MP + lane] = SMPC_PLV(lamb);
      }
      if (ok && lane < DR)
      {
        b.z[(size_t)inst * MP + N + drow(lane)] = SMPC_PLV(zd);
        b.lam[(size_t)inst * MP + N + drow(lane)] = SMPC_PLV(lamd);
      }
      if (ok && lane < FR)
      {
        b.z[(size_t)inst * MP + N + R_FRI + lane] = SMPC_PLV(zf);
        b.lam[(size_t)inst * MP + N + R_FRI + lane] = SMPC_PLV(lamf);
      }
      if (lane < NV)
        b.a[(size_t)inst * NV + lane] = s.xl[lane];
      // contact wrenches T f (foot frames) -> red[0 .. 6 NF)
      if (lane < 6 * NF)
      {
        const int f = lane / 6, r = lane % 6;
        double acc = 0.0;
        for (int c = 0; c < NFV; c++)
          acc += id6_tgen(b.quad, f, r, c) * s.xl[NV + NFV * f + c];
        s.red[lane] = acc;
        b.f[(size_t)inst * 6 * NF + lane] = acc;
      }
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    {
      if (lane < NA)
      { // tau = M_a a + h_a - J_a^T (T f)
        const double * Mq = b.Mq + (size_t)inst * NV * NV;
        const double * J = b.J + (size_t)inst * 6 * NF * NV;
        double acc = b.nle[(size_t)inst * NV + 6 + lane];
        for (int k = 0; k < NV; k++)
          acc += Mq[(6 + lane) * NV + k] * s.xl[k];
        for (int r = 0; r < 6 * NF; r++)
          acc -= J[r * NV + 6 + lane] * s.red[r];
        b.tau[(size_t)inst * NA + lane] = acc;
      }
      if (lane == 0)
      {
        const bool ok = res == res && res < 1e300;
        b.resid[inst] = res;
        b.rho[inst] = ok ? rho : st.rho;
        b.warm[inst] = ok ? 1 : 0;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // ---- host engine on the run-time tree: the buffers, targets, limits, warm-start state, stream sharing and residual reporting of IdEngine<D> ----
  // flat = false: 4 point feet (id_quant_rt_body / id_assemble_rt_body / qp_admm_rt_body) ; flat = true: 2 flat feet (the id6 / qp6 kernels
  // above: wrench targets [2][6], 6 LOCAL motion rows per foot, footR, the corners of the soles)
  struct IdEngineRt : IdEngineBase
  {
    IdRt6Buffers buf; // (the point-foot kernels take its IdRtBuffers base)
    IdRtSizes sz;
    bool flat = false;
    stream_t stream, own_stream;
    int device_id = 0;
    double * Xd = nullptr;
    std::vector<void *> allocs;
    unsigned mask_all = 0;
    bool mask_all_valid = false; // (the per-robot setters invalidate it)
    IdEngineRt(const smpc_robot_model * rm, const HostIdSettings & hs, int batch, int device, bool flat_feet = false) : flat(flat_feet)
    {
      if (rm->nfeet != (flat ? ID_RT6_NFEET : ID_RT_NFEET) || rm->njoints < 2 || rm->njoints > SMPC_MAX_JOINTS)
        throw std::runtime_error("robot shape (njoints, nfeet) outside what the run-time inverse-dynamics kernels hold");
      sz = id_rt_sizes(rm->njoints);
      if (flat)
      {
        const IdRt6Sizes s6 = id_rt6_sizes(rm->njoints);
        sz = IdRtSizes{s6.nq, s6.nv, s6.na, s6.nf, s6.n, s6.m, s6.np, s6.mp, s6.gr};
        if ((int)hs.quad_points.size() != sz.nf * 12)
          throw std::runtime_error("inverse-dynamics settings: flat feet need the four corners of every sole (quad_points, [nfeet][4][3])");
      }
      if (batch <= 0)
        throw std::runtime_error("batch must be positive");
      {
        const std::string why = id_limits_error(sz.na, hs.tau_max.size(), hs.v_max.size(), hs.q_min.size(), hs.q_max.size());
        if (!why.empty())
          throw std::runtime_error(why);
      }
      if (!(hs.dev.control_dt > 0.0) || hs.dev.admm_iters <= 0)
        throw std::runtime_error("inverse-dynamics settings: control_dt and the iteration count must be positive");
      device_id = device;
      set_device(device);
      stream = own_stream = stream_create();
      try
      {
        construct(rm, hs, batch);
      }
      catch (...)
      { // (the destructor does not run for a partially constructed engine)
        for (void * p : allocs)
          dev_free(p);
        stream_destroy(own_stream);
        throw;
      }
    }
    void construct(const smpc_robot_model * rm, const HostIdSettings & hs, int batch)
    {
      B = batch;
      nq = sz.nq;
      nv = sz.nv;
      nf = sz.nf;
      nfw = flat ? 6 : 3;
      nmot = flat ? ID_RT6_NM : 3;
      n = sz.n;
      m = sz.m;
      np = sz.np;
      mp = sz.mp;
      std::vector<IdRtDevModel> hm(1);
      std::memset(&hm[0], 0, sizeof(IdRtDevModel));
      fill_rt_model(rm, hm[0].t);
      {
        const std::vector<unsigned> anc = id_rt_ancestors(rm);
        for (int j = 0; j < SMPC_MAX_JOINTS; j++)
          hm[0].anc[j] = anc[j];
      }
      hm[0].total_mass = rm->total_mass;
      buf.nv = nv;
      buf.n = n;
      buf.m = m;
      buf.np = np;
      buf.mp = mp;
      auto dalloc = [&](size_t cnt) {
        void * p = dev_alloc(cnt * sizeof(double));
        dev_zero(p, cnt * sizeof(double), stream);
        allocs.push_back(p);
        return (double *)p;
      };
      buf.B = B;
      buf.model = (IdRtDevModel *)dev_alloc(sizeof(IdRtDevModel));
      allocs.push_back((void *)buf.model);
      h2d((void *)buf.model, hm.data(), sizeof(IdRtDevModel), stream);
      const size_t Bs = (size_t)B;
      Xd = dalloc(Bs * (nq + nv));
      buf.X = Xd;
      buf.Mq = dalloc(Bs * nv * nv);
      buf.nle = dalloc(Bs * nv);
      buf.J = dalloc(Bs * nmot * nf * nv);
      buf.Jdv = dalloc(Bs * nmot * nf);
      buf.vfoot = dalloc(Bs * nmot * nf);
      buf.com = dalloc(Bs * 3);
      buf.footp = dalloc(Bs * 3 * nf);
      buf.tcom = dalloc(Bs * 3);
      buf.tvcom = dalloc(Bs * 3);
      buf.tfp = dalloc(Bs * 3 * nf);
      buf.tfv = dalloc(Bs * 3 * nf);
      buf.H = dalloc(Bs * np * np);
      buf.g = dalloc(Bs * np);
      buf.C = dalloc(Bs * mp * np);
      {
        std::vector<double> c0(Bs * mp * np, 0.0); // constant rows of C: the identity of the box on y
        for (size_t b = 0; b < Bs; b++)
          for (int i = 0; i < n; i++)
            c0[(b * mp + i) * np + i] = 1.0;
        h2d(buf.C, c0.data(), c0.size() * sizeof(double), stream);
        stream_sync(stream);
      }
      buf.l = dalloc(Bs * mp);
      buf.u = dalloc(Bs * mp);
      buf.x = dalloc(Bs * np);
      buf.z = dalloc(Bs * mp);
      buf.lam = dalloc(Bs * mp);
      buf.rho = dalloc(Bs);
      buf.warm = (int *)dev_alloc(Bs * sizeof(int));
      allocs.push_back(buf.warm);
      dev_zero(buf.warm, Bs * sizeof(int), stream);
      buf.tx = dalloc(Bs * (nq + nv));
      buf.ta = dalloc(Bs * nv);
      buf.tf = dalloc(Bs * nfw * nf);
      buf.tmask = (unsigned *)dev_alloc(Bs * sizeof(unsigned));
      allocs.push_back(buf.tmask);
      buf.tau = dalloc(Bs * sz.na);
      buf.a = dalloc(Bs * nv);
      buf.f = dalloc(Bs * nfw * nf);
      if (flat)
      {
        buf.footR = dalloc(Bs * 9 * nf);
        buf.quad = dalloc((size_t)nf * 12);
        h2d(buf.quad, hs.quad_points.data(), (size_t)nf * 12 * sizeof(double), stream);
      }
      buf.resid = dalloc(Bs);
      buf.tau_max = dalloc(sz.na);
      buf.v_max = dalloc(sz.na);
      buf.q_min = dalloc(sz.na);
      buf.q_max = dalloc(sz.na);
      h2d(buf.tau_max, hs.tau_max.data(), sz.na * sizeof(double), stream);
      h2d(buf.v_max, hs.v_max.data(), sz.na * sizeof(double), stream);
      h2d(buf.q_min, hs.q_min.data(), sz.na * sizeof(double), stream);
      h2d(buf.q_max, hs.q_max.data(), sz.na * sizeof(double), stream);
      buf.s = hs.dev;
      stream_sync(stream);
      // default target: the reference state, every foot in contact with an equal share of the weight (kinodynamics-id.cpp:96-112)
      std::vector<double> q(rm->q_ref, rm->q_ref + nq), z(nv, 0.0), f((size_t)nfw * nf, 0.0);
      for (int k = 0; k < nf; k++)
        f[nfw * k + 2] = rm->total_mass * 9.81 / nf;
      set_target(-1, q.data(), z.data(), z.data(), (1u << nf) - 1u, f.data());
      if (buf.s.centroidal)
      { // CoM of the reference state (one pass of the first kernel), feet at their reference placements (centroidal-id.cpp:60-84)
        std::vector<double> X((size_t)B * (nq + nv), 0.0);
        for (int b = 0; b < B; b++)
          std::copy(q.begin(), q.end(), X.begin() + (size_t)b * (nq + nv));
        h2d(Xd, X.data(), X.size() * sizeof(double), stream);
        launch_quant();
        double com[3];
        d2h(com, buf.com, sizeof(com), stream);
        stream_sync(stream);
        const M3 R0 = quat_to_R(Quat{q[3], q[4], q[5], q[6]});
        std::vector<double> fp(3 * nf), zf(3 * nf, 0.0);
        for (int k = 0; k < nf; k++)
          st3(&fp[3 * k], ld3(q.data()) + R0 * ld3(rm->foot_ref_p[k]));
        set_target_centroidal(-1, com, z.data(), fp.data(), zf.data(), (1u << nf) - 1u, f.data());
      }
    }
    ~IdEngineRt()
    {
      for (void * p : allocs)
        dev_free(p);
      stream_destroy(own_stream);
    }
    void set_target(int inst, const double * q, const double * v, const double * a, unsigned mask, const double * f) override
    {
      set_device(device_id);
      if (inst >= B)
        throw std::runtime_error("instance index exceeds the batch");
      const int i0 = inst < 0 ? 0 : inst, i1 = inst < 0 ? B : inst + 1;
      const int nx = nq + nv;
      std::vector<double> tx((size_t)(i1 - i0) * nx), ta((size_t)(i1 - i0) * nv), tf((size_t)(i1 - i0) * nfw * nf);
      std::vector<unsigned> tm(i1 - i0, mask);
      for (int i = 0; i < i1 - i0; i++)
      {
        std::copy(q, q + nq, tx.begin() + (size_t)i * nx);
        std::copy(v, v + nv, tx.begin() + (size_t)i * nx + nq);
        std::copy(a, a + nv, ta.begin() + (size_t)i * nv);
        std::copy(f, f + nfw * nf, tf.begin() + (size_t)i * nfw * nf);
      }
      h2d(buf.tx + (size_t)i0 * nx, tx.data(), tx.size() * sizeof(double), stream);
      h2d(buf.ta + (size_t)i0 * nv, ta.data(), ta.size() * sizeof(double), stream);
      h2d(buf.tf + (size_t)i0 * nfw * nf, tf.data(), tf.size() * sizeof(double), stream);
      h2d(buf.tmask + i0, tm.data(), tm.size() * sizeof(unsigned), stream);
      mask_all_valid = false;
      stream_sync(stream);
    }
    // one target per robot: Q [B][nq], V [B][nv], A [B][nv], contact [B][nf], F [B][3 nf]
    void set_targets(const double * Q, const double * V, const double * A, const unsigned char * contact, const double * F) override
    {
      set_device(device_id);
      std::vector<unsigned> tm(B, 0u);
      for (int b = 0; b < B; b++)
        for (int k = 0; k < nf; k++)
          tm[b] |= contact[(size_t)b * nf + k] ? (1u << k) : 0u;
      const int nx = nq + nv;
      std::vector<double> tx((size_t)B * nx);
      for (int b = 0; b < B; b++)
      {
        std::copy(Q + (size_t)b * nq, Q + (size_t)(b + 1) * nq, tx.begin() + (size_t)b * nx);
        std::copy(V + (size_t)b * nv, V + (size_t)(b + 1) * nv, tx.begin() + (size_t)b * nx + nq);
      }
      h2d(buf.tx, tx.data(), tx.size() * sizeof(double), stream);
      h2d(buf.ta, A, (size_t)B * nv * sizeof(double), stream);
      h2d(buf.tf, F, (size_t)B * nfw * nf * sizeof(double), stream);
      h2d(buf.tmask, tm.data(), (size_t)B * sizeof(unsigned), stream);
      mask_all_valid = false;
      stream_sync(stream);
    }
    void set_target_centroidal(int inst, const double * com, const double * vcom, const double * fp, const double * fv, unsigned mask, const double * f) override
    {
      set_device(device_id);
      if (!buf.s.centroidal)
        throw std::runtime_error("this inverse-dynamics engine was created as KinodynamicsID");
      if (inst >= B)
        throw std::runtime_error("instance index exceeds the batch");
      const int i0 = inst < 0 ? 0 : inst, i1 = inst < 0 ? B : inst + 1, cnt = i1 - i0;
      std::vector<double> c3((size_t)cnt * 3), v3((size_t)cnt * 3), tp((size_t)cnt * 3 * nf), tv((size_t)cnt * 3 * nf), tf((size_t)cnt * nfw * nf);
      std::vector<unsigned> tm(cnt, mask);
      for (int i = 0; i < cnt; i++)
      {
        std::copy(com, com + 3, c3.begin() + (size_t)i * 3);
        std::copy(vcom, vcom + 3, v3.begin() + (size_t)i * 3);
        std::copy(fp, fp + 3 * nf, tp.begin() + (size_t)i * 3 * nf);
        std::copy(fv, fv + 3 * nf, tv.begin() + (size_t)i * 3 * nf);
        std::copy(f, f + nfw * nf, tf.begin() + (size_t)i * nfw * nf);
      }
      h2d(buf.tcom + (size_t)i0 * 3, c3.data(), c3.size() * sizeof(double), stream);
      h2d(buf.tvcom + (size_t)i0 * 3, v3.data(), v3.size() * sizeof(double), stream);
      h2d(buf.tfp + (size_t)i0 * 3 * nf, tp.data(), tp.size() * sizeof(double), stream);
      h2d(buf.tfv + (size_t)i0 * 3 * nf, tv.data(), tv.size() * sizeof(double), stream);
      h2d(buf.tf + (size_t)i0 * nfw * nf, tf.data(), tf.size() * sizeof(double), stream);
      h2d(buf.tmask + i0, tm.data(), tm.size() * sizeof(unsigned), stream);
      mask_all_valid = false;
      stream_sync(stream);
    }
    void set_targets_centroidal(const double * COM, const double * VCOM, const double * FP, const double * FV, const unsigned char * contact, const double * F) override
    {
      set_device(device_id);
      if (!buf.s.centroidal)
        throw std::runtime_error("this inverse-dynamics engine was created as KinodynamicsID");
      std::vector<unsigned> tm(B, 0u);
      for (int b = 0; b < B; b++)
        for (int k = 0; k < nf; k++)
          tm[b] |= contact[(size_t)b * nf + k] ? (1u << k) : 0u;
      h2d(buf.tcom, COM, (size_t)B * 3 * sizeof(double), stream);
      h2d(buf.tvcom, VCOM, (size_t)B * 3 * sizeof(double), stream);
      h2d(buf.tfp, FP, (size_t)B * 3 * nf * sizeof(double), stream);
      h2d(buf.tfv, FV, (size_t)B * 3 * nf * sizeof(double), stream);
      h2d(buf.tf, F, (size_t)B * nfw * nf * sizeof(double), stream);
      h2d(buf.tmask, tm.data(), (size_t)B * sizeof(unsigned), stream);
      mask_all_valid = false;
      stream_sync(stream);
    }
    void launch_quant()
    {
      if (flat)
        launch<IdRt6Buffers, id6_quant_rt_body, 64, 1, 0>(B, stream, buf);
      else
        launch<IdRtBuffers, id_quant_rt_body, 64, 1, 0>(B, stream, buf);
    }
    void launch_all()
    {
      launch_quant();
      if (flat)
      {
        launch<IdRt6Buffers, id6_assemble_rt_body, 64, 1, 0>(B, stream, buf);
        if (np == 32)
          launch<IdRt6Buffers, qp6_admm_rt_body<32>, 64, 1, 0>(B, stream, buf);
        else if (np == 48)
          launch<IdRt6Buffers, qp6_admm_rt_body<48>, 64, 1, 0>(B, stream, buf);
        else
          launch<IdRt6Buffers, qp6_admm_rt_body<64>, 64, 1, 0>(B, stream, buf);
        return;
      }
      launch<IdRtBuffers, id_assemble_rt_body, 64, 1, 0>(B, stream, buf);
      if (np == 32) // (the solver is instantiated per padded size: its K inverse runs on compile-time tiles)
        launch<IdRtBuffers, qp_admm_rt_body<32>, 64, 1, 0>(B, stream, buf);
      else if (np == 48)
        launch<IdRtBuffers, qp_admm_rt_body<48>, 64, 1, 0>(B, stream, buf);
      else
        launch<IdRtBuffers, qp_admm_rt_body<64>, 64, 1, 0>(B, stream, buf);
    }
    void solve_device(const double * X_dev, double * tau_dev) override
    {
      set_device(device_id);
      buf.X = X_dev;
      launch_all();
      buf.X = Xd;
      if (tau_dev)
        d2d(tau_dev, buf.tau, (size_t)B * sz.na * sizeof(double), stream);
    }
    void wait() override
    {
      set_device(device_id);
      stream_sync(stream);
    }
    int device() const override { return device_id; }
    const double * tau_device() const override { return buf.tau; }
    double * x_device() override { return Xd; }
    void target_buffers(double ** x, double ** a, double ** f) override
    {
      *x = buf.tx;
      *a = buf.ta;
      *f = buf.tf;
    }
    void centroidal_target_buffers(double ** com, double ** vcom, double ** fp, double ** fv) override
    {
      const bool c = buf.s.centroidal != 0;
      *com = c ? buf.tcom : nullptr;
      *vcom = c ? buf.tvcom : nullptr;
      *fp = c ? buf.tfp : nullptr;
      *fv = c ? buf.tfv : nullptr;
    }
    void set_mask_all(unsigned mask) override
    {
      set_device(device_id);
      if (mask != mask_all || !mask_all_valid)
      {
        std::vector<unsigned> tm(B, mask);
        h2d(buf.tmask, tm.data(), tm.size() * sizeof(unsigned), stream);
        stream_sync(stream);
        mask_all = mask;
        mask_all_valid = true;
      }
    }
    stream_t solve_stream() override { return stream; }
    void adopt_stream(stream_t s, bool back_to_own) override
    {
      set_device(device_id);
      stream_sync(stream);
      stream = back_to_own ? own_stream : s;
    }
    void solve(const double * X, double * tau, double * a, double * f, double * resid) override
    {
      set_device(device_id);
      h2d(Xd, X, (size_t)B * (nq + nv) * sizeof(double), stream);
      launch_all();
      d2h(tau, buf.tau, (size_t)B * sz.na * sizeof(double), stream);
      d2h(a, buf.a, (size_t)B * nv * sizeof(double), stream);
      d2h(f, buf.f, (size_t)B * nfw * nf * sizeof(double), stream);
      if (resid)
        d2h(resid, buf.resid, (size_t)B * sizeof(double), stream);
      stream_sync(stream);
    }
    void reset(int inst) override
    {
      set_device(device_id);
      if (inst >= B)
        throw std::runtime_error("instance index exceeds the batch");
      const int i0 = inst < 0 ? 0 : inst, cnt = inst < 0 ? B : 1;
      dev_zero(buf.warm + i0, (size_t)cnt * sizeof(int), stream);
      stream_sync(stream);
    }
    void get_resid(double * out) override
    {
      set_device(device_id);
      d2h(out, buf.resid, (size_t)B * sizeof(double), stream);
      stream_sync(stream);
    }
    void debug_get(int what, double * out) override
    {
      set_device(device_id);
      const double * src[14] = {buf.Mq, buf.nle, buf.J, buf.Jdv, buf.vfoot, buf.H, buf.g, buf.C, buf.l, buf.u, buf.com, buf.footp, buf.tau, buf.footR};
      const size_t per[14] = {(size_t)nv * nv, (size_t)nv, (size_t)nmot * nf * nv, (size_t)nmot * nf, (size_t)nmot * nf, (size_t)np * np, (size_t)np, (size_t)mp * np, (size_t)mp, (size_t)mp, 3, (size_t)3 * nf, (size_t)sz.na, (size_t)9 * nf};
      if (what < 0 || what > (flat ? 13 : 12)) // (13: footR [B][nf][9], flat feet on this engine only)
        throw std::runtime_error("unknown quantity");
      d2h(out, src[what], (size_t)B * per[what] * sizeof(double), stream);
      stream_sync(stream);
    }
  };
} // namespace smpc
