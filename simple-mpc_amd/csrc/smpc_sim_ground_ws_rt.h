// smpc_sim_ground_ws_rt.h -- the ground of smpc_sim_ground_env_rt.h with a WARM-STARTED contact solve and a STOPPING RULE: robot i starts
// its projected Gauss-Seidel from its own forces of the previous step (the handle-owned warm buffer w [B][rows], laid out in the contact
// frame [point][t1 t2 n]), stops when a sweep has stopped moving them, and reports how many sweeps ran and what residual was left
// (DESIGN 3.25 states the model word for word).  sim_ground_ws_rt_body is a sibling of sim_ground_env_rt_body, which stays as it is: one
// wavefront per robot, one launch per step, the same phases with four additions
//   phase 0   the warm row with the other global loads into lambda, where the sibling fills zeros: lambda0_r = w_r if warm_start is set and
//             w_r is finite, else 0 (a null array stands for zeros)
//   before the sweeps   dt G_rr per row next to 1 / (dt G_rr), interleaved, so that the read of the one brings the other
//   phase 5   rho_s = max_r |lambda_r(new) - lambda_r(old)| dt G_rr as a running maximum on the lanes that hold the updates (lane 0: the
//             normal row and the first tangential row, lane 1: the second); once per sweep the two maxima go through LDS and the whole wave
//             reads the loop condition back: the solve stops after sweep s if tol > 0, s >= min_sweeps and rho_s <= tol.  One wavefront owns
//             one robot, so the exit is wave-uniform.  A NaN rho is kept (the maximum is NaN-sticky) and never stops the sweeps.
//   phase 7   lambda in the contact frame (the warm row of the next step), sweeps_used and residual with the other global stores
// The environment and the push are read as the sibling reads them (null arrays: the handle's values), so one kernel serves handles with
// and without an environment.  The sweep keeps its order, its single accumulator per dot product, its compile-time row bound and its
// multiplication by 1 / (dt G_rr); with warm_start = 0 and tol = 0 the results equal the sibling's bit for bit.  The bookkeeping adds no
// dependent LDS round trip per point: dt G_rr comes with the read of its reciprocal (a tangential row carries it in a register from the
// phase of the candidates to the projection) and the old tangential value is loaded beside the candidates.
// LDS: IdQuantRtScratch (19 024 B) + SimGroundWsLds<NROWS> = SimGroundEnvLds<NROWS> + 2 NROWS + 2 doubles.
#pragma once
#include "smpc_sim_ground_env_rt.h"
#include "smpc_sim_ground_ws_dims.h"
#include <vector>

namespace smpc
{
  struct SimGroundWsArgs
  {
    SimGroundEnvArgs e;
    const double * lam0;  // [n][nr] start vector in the contact frame (device), or null: zeros (read only if warm_start != 0)
    double * lamc_out;    // [n][nr] lambda in the contact frame, or null (a step writes the warm buffer here; may alias lam0)
    int * sweeps_out;     // [n] sweeps run
    double * resid_out;   // [n] rho of the last sweep run
    int warm_start, min_sweeps;
    double tol;
  };

  template <int NROWS>
  struct SimGroundWsLds
  {
    SimGroundEnvLds<NROWS> e;
    alignas(16) double ig[NROWS][2]; // (1 / (dt G_rr), dt G_rr) side by side: one LDS read brings both
    double rho[2];    // the running maxima of lanes 0 and 1 at the end of a sweep
  };
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundWsLds<24>) <= 163840 / 3, "three blocks per compute unit");
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundWsLds<12>) <= sizeof(IdQuantRtScratch) + sizeof(SimRtLds), "no more LDS than sim_rt_body");

  // max(m, d) that keeps a NaN once it has seen one
  SMPC_DEV double sim_ground_ws_max(double m, double d) { return (d > m || d != d) ? d : m; }

  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_ws_rt_body(const SimGroundWsArgs & wa, int block)
  {
    typedef IdQuantRtScratch SC;
    typedef SimGroundLds<NROWS> L;
    typedef SimGroundEnvLds<NROWS> LE;
    typedef SimGroundWsLds<NROWS> LW;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF, LDM = L::NV, NCM = L::NC, NR = L::NR, NPM = L::NP, LDG = L::LDG, NE = SIM_GROUND_ENV_DOUBLES;
    static_assert(LDM <= NT - NE - 1 && NR <= NT && NCM % 3 == 0 && NPM <= 24, "torques and environment load side by side; points on lanes 32 .. 55");
    const SimGroundEnvArgs & ea = wa.e;
    const SimGroundArgs & ka = ea.g;
    const int inst = block;
    const IdRtDevModel & mi = *ka.model;
    // (wave-uniform sizes from the device table and the arguments, clamped so that no value can index outside the LDS arrays)
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nq = nj + 6, nx = 2 * nj + 11, na = nv - 6;
    const int P = ka.P < SIM_GROUND_MAX_PPF ? (ka.P > 1 ? ka.P : 1) : SIM_GROUND_MAX_PPF;
    const int maxf = NPM / P < NF ? NPM / P : NF;
    const int nfeet = mi.t.nfeet < maxf ? (mi.t.nfeet > 0 ? mi.t.nfeet : 0) : maxf;
    const int npts = nfeet * P, nr = 3 * npts;
    const int jpush = ea.push_joint < nj ? (ea.push_joint > 0 ? ea.push_joint : 0) : nj - 1;
    const double dt = ka.dt;
    const bool warm = wa.warm_start != 0 && wa.lam0 != nullptr;
    SMPC_LDS(SC, scs, 1);
    SMPC_LDS(LW, ls, 1);
    SC & sc = scs[0];
    LW & w = ls[0];
    LE & e = w.e;
    L & s = e.s;
    // ---- phase 0: every global load (the state and the joint constants: first phase of rt_tree_phases) ----
    SMPC_LANES(NT)
    {
      if (lane < LDM)
        s.tau[lane] = lane >= 6 && lane < nv ? ka.tau[(size_t)inst * na + lane - 6] : 0.0;
      if (lane >= NT - NE)
      {
        const int k = lane - (NT - NE);
        double val;
        if (k < 4)
          val = ea.plane != nullptr ? ea.plane[(size_t)inst * 4 + k] : (k == 2 ? 1.0 : (k == 3 ? ka.ground_z : 0.0));
        else if (k == 4)
          val = ea.mu != nullptr ? ea.mu[inst] : ka.mu;
        else
          val = ea.push != nullptr ? ea.push[(size_t)inst * 6 + k - 5] : 0.0;
        e.env[k] = val;
      }
      if (lane < NCM) // the start vector: the robot's warm row, an entry that is not finite reads as exactly 0
      {
        double val = 0.0;
        if (warm && lane < nr)
        {
          const double v = wa.lam0[(size_t)inst * nr + lane];
          val = fabs(v) <= 1.7976931348623157e308 ? v : 0.0;
        }
        s.lam[lane] = val;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phases 1, 2 ----
    rt_tree_phases(sc, mi, ka.X + (size_t)inst * nx, mk3(ka.gravity[0], ka.gravity[1], ka.gravity[2]));
    // ---- joint-space inertia (both triangles from one expression: symmetric bit for bit); contact points, gaps, frame and push point ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < nv * nv; idx += NT)
      {
        const int r = idx / nv, c = idx % nv;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const int jl = lo < 6 ? 0 : lo - 5, jh = hi < 6 ? 0 : hi - 5;
        s.M[r * LDM + c] = ((sc.anc[jh] >> jl) & 1u) ? id_rt_dot6(&sc.S[lo * 6], &sc.F[hi * 6]) : 0.0;
      }
      for (int idx = lane; idx < NCM * LDM; idx += NT)
        s.J[idx] = 0.0;
      if (lane < NCM)
      {
        s.c0[lane] = 0.0;
        w.ig[lane][0] = 0.0;
        w.ig[lane][1] = 0.0;
      }
      if (lane >= 32 && lane < 32 + NPM)
      {
        const int c = lane - 32;
        double gap = 0.0;
        V3 p = mk3(0.0, 0.0, 0.0);
        if (c < npts)
        {
          const int f = c / P, k = c % P, jf = sc.fj[f];
          p = ld3(&sc.footp[f * 3]) + ldm3(&sc.oR[jf * 9]) * mk3(ka.points[k][0], ka.points[k][1], ka.points[k][2]); // foot frame rotation = joint rotation
          double acc = e.env[0] * p.x;
          acc += e.env[1] * p.y;
          acc += e.env[2] * p.z;
          gap = acc - e.env[3];
        }
        st3(&s.pc[c * 3], p);
        s.gap[c] = gap;
      }
      if (lane == 62) // t1 = (e_y x n) / |e_y x n|, t2 = n x t1 (sim_ground_env_frame)
      {
        const double n0 = e.env[0], n1 = e.env[1], n2 = e.env[2];
        const double cx = n2, cz = -n0;
        const double inv = 1.0 / sqrt(cx * cx + cz * cz);
        const V3 t1 = mk3(cx * inv, 0.0, cz * inv);
        st3(e.t1, t1);
        st3(e.t2, mk3(n1 * t1.z - n2 * t1.y, n2 * t1.x - n0 * t1.z, n0 * t1.y - n1 * t1.x));
      }
      if (lane == 63) // r = p_j + R_j o and r x f
      {
        const V3 r = ld3(&sc.op[jpush * 3]) + ldm3(&sc.oR[jpush * 9]) * ld3(&e.env[8]);
        st3(e.r, r);
        st3(e.rxf, cross(r, ld3(&e.env[5])));
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 3: the rows of every point, t1 t2 n in the contact frame ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < npts * nv; idx += NT)
    {
      const int c = idx / nv, k = idx % nv;
      const int jf = sc.fj[c / P], jk = k < 6 ? 0 : k - 5;
      if ((sc.anc[jf] >> jk) & 1u)
      {
        const SV Sk = ldsv(&sc.S[k * 6]);
        const V3 lin = Sk.l + cross(Sk.a, ld3(&s.pc[c * 3])); // velocity of the point under the unit twist of column k
        double r0 = e.t1[0] * lin.x;
        r0 += e.t1[1] * lin.y;
        r0 += e.t1[2] * lin.z;
        double r1 = e.t2[0] * lin.x;
        r1 += e.t2[1] * lin.y;
        r1 += e.t2[2] * lin.z;
        double r2 = e.env[0] * lin.x;
        r2 += e.env[1] * lin.y;
        r2 += e.env[2] * lin.z;
        s.J[(3 * c + 0) * LDM + k] = r0;
        s.J[(3 * c + 1) * LDM + k] = r1;
        s.J[(3 * c + 2) * LDM + k] = r2;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: M = L L^T ; W = M^-1 [S tau - h + Q | J^T] ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < nv * NR; idx += NT)
    {
      const int k = idx / NR, c = idx % NR;
      double val;
      if (c == 0)
      {
        double q = 0.0;
        if ((sc.anc[jpush] >> (k < 6 ? 0 : k - 5)) & 1u)
        {
          const SV Sk = ldsv(&sc.S[k * 6]);
          q = Sk.l.x * e.env[5];
          q += Sk.l.y * e.env[6];
          q += Sk.l.z * e.env[7];
          q += Sk.a.x * e.rxf[0];
          q += Sk.a.y * e.rxf[1];
          q += Sk.a.z * e.rxf[2];
        }
        val = s.tau[k] - sc.h[k] + q;
      }
      else
        val = s.J[(c - 1) * LDM + k];
      s.W[idx] = val;
    }
    SMPC_LANES_END_WAVE
    rt_wave_cholesky(s.M, LDM, nv, s.tmp);
    rt_wave_chol_solve<NR>(s.M, LDM, nv, s.W, NR, s.row);
    // free velocity
    SMPC_LANES(NT)
    if (lane < nv)
      s.vf[lane] = sc.x[nq + lane] + dt * s.W[lane * NR];
    SMPC_LANES_END_WAVE
    // Delassus matrix with the compliance on its diagonal, c0 = J v_f + the gap term on the normal rows
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NCM * NCM; idx += NT)
      {
        const int c = idx / NCM, d = idx % NCM;
        double acc = 0.0;
        if (c < nr && d < nr) // (zero beyond the rows of the robot's points: the sweep runs over the whole row)
        {
          for (int k = 0; k < nv; k++)
            acc += s.J[c * LDM + k] * s.W[k * NR + 1 + d];
          if (c == d)
            acc += ka.compliance;
        }
        s.G[c * LDG + d] = acc;
      }
      if (lane >= 32 && lane < 32 + nr)
      {
        const int r = lane - 32;
        double acc = 0.0;
        for (int k = 0; k < nv; k++)
          acc += s.J[r * LDM + k] * s.vf[k];
        if (r % 3 == 2)
        {
          const double phi = s.gap[r / 3];
          acc += phi >= 0.0 ? phi / dt : ka.erp * phi / dt;
        }
        s.c0[r] = acc;
      }
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    if (lane < nr)
    {
      const double dg = dt * s.G[lane * LDG + lane];
      w.ig[lane][0] = 1.0 / dg;
      w.ig[lane][1] = dg;
    }
    SMPC_LANES_END_WAVE
    // ---- phase 5: projected Gauss-Seidel from the start vector, points in ascending order (the sweep of sim_ground_rt_body), at most
    // `sweeps` sweeps; rho of a sweep on lanes 0 and 1, the stopping test once per sweep ----
    const int min_sweeps = wa.min_sweeps > 1 ? wa.min_sweeps : 1;
    const bool stopping = wa.tol > 0.0;
    int used = 0;
    double rho = 0.0;
    SMPC_PL(double, rmax, NT);
    SMPC_PL(double, tdg, NT); // dt G_rr of the lane's tangential row, from the phase of the candidates to the projection
    SMPC_LANES(NT)
    {
      SMPC_PLV(rmax) = 0.0;
      SMPC_PLV(tdg) = 0.0;
    }
    SMPC_LANES_END_WAVE
    for (int sw = 0; sw < ka.sweeps; sw++)
    {
      for (int c = 0; c < npts; c++)
      {
        const int rn = 3 * c + 2;
        SMPC_LANES(NT)
        if (lane == 0)
        {
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < NCM; j++) // (compile-time bound: the loads of the row are issued ahead of the chain of multiply-adds)
            acc += s.G[rn * LDG + j] * s.lam[j];
          const double old = s.lam[rn];
          const double idg = w.ig[rn][0], dg = w.ig[rn][1];
          const double val = fmax(0.0, old - (s.c0[rn] + dt * acc) * idg);
          s.lam[rn] = val;
          SMPC_PLV(rmax) = sim_ground_ws_max(SMPC_PLV(rmax), fabs(val - old) * dg);
        }
        SMPC_LANES_END_WAVE
        // both tangential candidates from the same lambda, the one that already holds the new normal force
        SMPC_LANES(NT)
        if (lane < 2)
        {
          const int rt = 3 * c + lane;
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < NCM; j++)
            acc += s.G[rt * LDG + j] * s.lam[j];
          const double idg = w.ig[rt][0];
          SMPC_PLV(tdg) = w.ig[rt][1];
          s.tc[lane] = s.lam[rt] - (s.c0[rt] + dt * acc) * idg;
        }
        SMPC_LANES_END_WAVE
        SMPC_LANES(NT)
        if (lane < 2)
        {
          const int rt = 3 * c + lane;
          const double t1 = s.tc[0], t2 = s.tc[1];
          const double nrm = sqrt(t1 * t1 + t2 * t2), lim = e.env[4] * s.lam[rn];
          const double old = s.lam[rt];
          double t = s.tc[lane];
          if (nrm > lim)
            t = t * (lim / nrm);
          if (nrm == 0.0)
            t = 0.0;
          s.lam[rt] = t;
          SMPC_PLV(rmax) = sim_ground_ws_max(SMPC_PLV(rmax), fabs(t - old) * SMPC_PLV(tdg));
        }
        SMPC_LANES_END_WAVE
      }
      SMPC_LANES(NT)
      if (lane < 2)
      {
        w.rho[lane] = SMPC_PLV(rmax);
        SMPC_PLV(rmax) = 0.0; // (the next sweep's maximum starts at 0)
      }
      SMPC_LANES_END_WAVE
      // (the whole wave reads the two maxima back: after the lanes' end-of-wave point, so that the sequential test backend sees both)
      rho = sim_ground_ws_max(w.rho[0], w.rho[1]);
      used = sw + 1;
      if (SMPC_UNIFORM_U32(stopping && used >= min_sweeps && rho <= wa.tol ? 1u : 0u) != 0u)
        break;
    }
    // ---- phase 6: a = W_0 + W_1 lambda ; v+ = v_f + dt W_1 lambda ; q+ = q (+) v+ dt ----
    SMPC_LANES(NT)
    if (lane < nv)
    {
      double acc = 0.0;
      for (int c = 0; c < nr; c++)
        acc += s.W[lane * NR + 1 + c] * s.lam[c];
      s.a[lane] = s.W[lane * NR] + acc;
      const double vn = s.vf[lane] + dt * acc;
      s.xn[nq + lane] = vn;
      s.dx[lane] = vn * dt;
    }
    SMPC_LANES_END_WAVE
    const bool step = ka.advance != 0;
    if (step)
    {
      SMPC_LANES(NT)
      if (lane == 0)
      {
        const double * x = sc.x;
        const V3 dv = ld3(s.dx), dw = ld3(s.dx + 3);
        const M3 R0 = quat_to_R(Quat{x[3], x[4], x[5], x[6]});
        const SE3 E = exp6(dv, dw);
        st3(s.xn, ld3(x) + R0 * E.p);
        Quat qn = quat_mul(Quat{x[3], x[4], x[5], x[6]}, quat_exp(dw));
        const double n = 1.0 / sqrt(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);
        s.xn[3] = qn.x * n;
        s.xn[4] = qn.y * n;
        s.xn[5] = qn.z * n;
        s.xn[6] = qn.w * n;
      }
      else if (lane >= 6 && lane < nv)
        s.xn[lane + 1] = sc.x[lane + 1] + s.dx[lane];
      SMPC_LANES_END_WAVE
    }
    // ---- phase 7: every global store; the forces in world axes, lambda_world(c) = Rc lambda_c, and in the contact frame ----
    SMPC_LANES(NT)
    {
      if (step)
        for (int i = lane; i < nx; i += NT)
          ka.X[(size_t)inst * nx + i] = s.xn[i];
      if (lane < nv)
      {
        ka.a_out[(size_t)inst * nv + lane] = s.a[lane];
        if (ka.vnext_out != nullptr)
          ka.vnext_out[(size_t)inst * nv + lane] = s.xn[nq + lane];
      }
      if (lane < nr)
      {
        const int c = lane / 3, i = lane % 3;
        double wl = e.t1[i] * s.lam[3 * c];
        wl += e.t2[i] * s.lam[3 * c + 1];
        wl += e.env[i] * s.lam[3 * c + 2];
        ka.lam_out[(size_t)inst * nr + lane] = wl;
        if (wa.lamc_out != nullptr)
          wa.lamc_out[(size_t)inst * nr + lane] = s.lam[lane];
      }
      if (lane < npts && ka.gap_out != nullptr)
        ka.gap_out[(size_t)inst * npts + lane] = s.gap[lane];
      if (lane == 0)
      {
        unsigned word = 0u;
        for (int c = 0; c < npts; c++)
          if (s.lam[3 * c + 2] > 0.0)
            word |= 1u << c;
        ka.contact_out[inst] = word;
      }
      if (lane == 1)
      {
        wa.sweeps_out[inst] = used;
        wa.resid_out[inst] = rho;
      }
    }
    SMPC_LANES_END_WAVE
  }

  // zero the warm rows of the robots with a non-zero mask byte.  grid = B, 64 lanes
  struct SimGroundWsResetArgs
  {
    double * warm;              // [B][nrows]
    const unsigned char * mask; // [B]
    int nrows;
  };
  SMPC_DEV void sim_ground_ws_reset_body(const SimGroundWsResetArgs & ra, int block)
  {
    SMPC_LANES(64)
    if (ra.mask[block] != 0 && lane < ra.nrows)
      ra.warm[(size_t)block * ra.nrows + lane] = 0.0;
    SMPC_LANES_END_WAVE
  }

  // ---- host: the solver settings, the warm buffer and the per-robot read-outs of one simulator handle's ground (a sibling of
  // RobotSimGroundEnv; the environment of a step is handed in by the caller).  `active` once the setter has been called: from then on the
  // handle's ground steps launch the kernel above.  The host-buffer solve needs no setter and never touches the warm buffer. ----
  struct RobotSimGroundWs
  {
    RobotSimGround & g;
    bool active = false;
    SimGroundWsSettings ws{0, 0.0, 1};
    double * warm = nullptr;  // [B][nrows], contact frame
    int * sweeps = nullptr;   // [B]
    double * resid = nullptr; // [B]
    unsigned char * mask = nullptr; // [B] the host-list form of the reset
    UploadRing mask_ring;
    // host-buffer form (n states, n need not be B): grown on demand
    int cap = 0;
    double *hX = nullptr, *hTau = nullptr, *hV = nullptr, *hA = nullptr, *hLam = nullptr, *hLamC = nullptr, *hLam0 = nullptr, *hGap = nullptr, *hEnv = nullptr,
           *hRes = nullptr;
    unsigned * hCon = nullptr;
    int * hSw = nullptr;

    explicit RobotSimGroundWs(RobotSimGround & ground) : g(ground)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const SimGroundWsSizes z = sim_ground_ws_sizes(sim.B, g.gz.nrows);
      AllocScope scope; // (a failing allocation below releases the ones before it)
      warm = (double *)dev_alloc(z.warm_bytes);
      sweeps = (int *)dev_alloc(z.sweeps_bytes);
      resid = (double *)dev_alloc(z.residual_bytes);
      mask = (unsigned char *)dev_alloc((size_t)sim.B);
      scope.commit();
      dev_zero(warm, z.warm_bytes, sim.stream);
      dev_zero(sweeps, z.sweeps_bytes, sim.stream);
      dev_zero(resid, z.residual_bytes, sim.stream);
      stream_sync(sim.stream);
    }
    RobotSimGroundWs(const RobotSimGroundWs &) = delete;
    RobotSimGroundWs & operator=(const RobotSimGroundWs &) = delete;
    void free_staging()
    {
      dev_free(hX);
      dev_free(hTau);
      dev_free(hV);
      dev_free(hA);
      dev_free(hLam);
      dev_free(hLamC);
      dev_free(hLam0);
      dev_free(hGap);
      dev_free(hEnv);
      dev_free(hRes);
      dev_free(hCon);
      dev_free(hSw);
      hX = hTau = hV = hA = hLam = hLamC = hLam0 = hGap = hEnv = hRes = nullptr;
      hCon = nullptr;
      hSw = nullptr;
      cap = 0;
    }
    ~RobotSimGroundWs()
    {
      free_staging();
      dev_free(warm);
      dev_free(sweeps);
      dev_free(resid);
      dev_free(mask);
    }
    // (the caller has run sim_ground_ws_admission_error) stores the settings and zeroes the warm buffer and the read-outs
    void set_solver(const smpc_ground_solver_settings * settings)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const SimGroundWsSizes z = sim_ground_ws_sizes(sim.B, g.gz.nrows);
      sim.wait(); // (a step in flight still reads and writes the buffers that are zeroed below)
      dev_zero(warm, z.warm_bytes, sim.stream);
      dev_zero(sweeps, z.sweeps_bytes, sim.stream);
      dev_zero(resid, z.residual_bytes, sim.stream);
      stream_sync(sim.stream);
      ws = sim_ground_ws_resolve(settings);
      active = true;
    }
    void reset_device(const unsigned char * mask_dev)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      SimGroundWsResetArgs ra;
      ra.warm = warm;
      ra.mask = mask_dev;
      ra.nrows = g.gz.nrows;
      launch<SimGroundWsResetArgs, sim_ground_ws_reset_body, 64, 1, 0>(sim.B, sim.stream, ra);
    }
    // (the caller has run sim_ground_ws_reset_error, which filled `m`)
    void reset_list(const std::vector<unsigned char> & m)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      mask_ring.upload(mask, m.data(), (size_t)sim.B, sim.stream); // (pinned staging: the caller's queue is not drained)
      reset_device(mask);
    }
    void run(int n, const SimGroundWsArgs & wa)
    {
      if (g.gz.inst == 12)
        launch<SimGroundWsArgs, sim_ground_ws_rt_body<12>, 64, 1, 0>(n, g.sim.stream, wa);
      else
        launch<SimGroundWsArgs, sim_ground_ws_rt_body<24>, 64, 1, 0>(n, g.sim.stream, wa);
    }
    // `env` may be null: the handle's uniform ground, no push
    void step_device(double * X_dev, const double * tau_dev, double dt, const RobotSimGroundEnv * env)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      SimGroundWsArgs wa;
      wa.e.g = g.args(dt);
      wa.e.g.X = X_dev;
      wa.e.g.tau = tau_dev;
      wa.e.g.advance = 1;
      wa.e.g.a_out = sim.a;
      wa.e.g.lam_out = g.lam;
      wa.e.g.contact_out = g.contact;
      const bool have = env != nullptr && env->active;
      wa.e.plane = have ? env->plane : nullptr;
      wa.e.mu = have ? env->mu : nullptr;
      wa.e.push = have ? env->push : nullptr;
      wa.e.push_joint = have ? env->push_joint : 0;
      wa.lam0 = warm;
      wa.lamc_out = warm;
      wa.sweeps_out = sweeps;
      wa.resid_out = resid;
      wa.warm_start = ws.warm_start;
      wa.min_sweeps = ws.min_sweeps;
      wa.tol = ws.tol;
      run(sim.B, wa);
    }
    void read_last(int * sweeps_out, double * resid_out)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      if (sweeps_out)
        d2h(sweeps_out, sweeps, (size_t)sim.B * sizeof(int), sim.stream);
      if (resid_out)
        d2h(resid_out, resid, (size_t)sim.B * sizeof(double), sim.stream);
      stream_sync(sim.stream);
    }
    void dynamics(int n, const double * X, const double * tau, double dt, const double * plane_h, const double * mu_h, const double * push_h, int joint,
                  const SimGroundWsSettings & st, const double * lam0_h, double * v_out, double * a_out, double * lam_out, double * lamc_out, double * gap_out,
                  unsigned * con_out, int * sweeps_out, double * resid_out)
    {
      if (n < 1)
        throw InvalidCall("n must be positive");
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const SimRtSizes & sz = sim.sz;
      const SimGroundSizes & gz = g.gz;
      stream_t stream = sim.stream;
      constexpr int NE = SIM_GROUND_ENV_DOUBLES;
      if (n > cap)
      {
        stream_sync(stream);
        free_staging();
        AllocScope scope; // (the pointers are kept only once every allocation has succeeded)
        double * nX = (double *)dev_alloc((size_t)n * sz.nx * sizeof(double));
        double * nTau = (double *)dev_alloc((size_t)n * sz.na * sizeof(double));
        double * nV = (double *)dev_alloc((size_t)n * sz.nv * sizeof(double));
        double * nA = (double *)dev_alloc((size_t)n * sz.nv * sizeof(double));
        double * nLam = (double *)dev_alloc((size_t)n * gz.nrows * sizeof(double));
        double * nLamC = (double *)dev_alloc((size_t)n * gz.nrows * sizeof(double));
        double * nLam0 = (double *)dev_alloc((size_t)n * gz.nrows * sizeof(double));
        double * nGap = (double *)dev_alloc((size_t)n * gz.npts * sizeof(double));
        double * nEnv = (double *)dev_alloc((size_t)n * NE * sizeof(double)); // planes [n][4] | mu [n] | pushes [n][6]
        double * nRes = (double *)dev_alloc((size_t)n * sizeof(double));
        unsigned * nCon = (unsigned *)dev_alloc((size_t)n * sizeof(unsigned));
        int * nSw = (int *)dev_alloc((size_t)n * sizeof(int));
        scope.commit();
        hX = nX;
        hTau = nTau;
        hV = nV;
        hA = nA;
        hLam = nLam;
        hLamC = nLamC;
        hLam0 = nLam0;
        hGap = nGap;
        hEnv = nEnv;
        hRes = nRes;
        hCon = nCon;
        hSw = nSw;
        cap = n;
      }
      double *dPlane = hEnv, *dMu = hEnv + (size_t)cap * 4, *dPush = hEnv + (size_t)cap * 5;
      h2d(hX, X, (size_t)n * sz.nx * sizeof(double), stream);
      h2d(hTau, tau, (size_t)n * sz.na * sizeof(double), stream);
      if (plane_h)
        h2d(dPlane, plane_h, (size_t)n * 4 * sizeof(double), stream);
      if (mu_h)
        h2d(dMu, mu_h, (size_t)n * sizeof(double), stream);
      if (push_h)
        h2d(dPush, push_h, (size_t)n * 6 * sizeof(double), stream);
      const bool start = st.warm_start != 0 && lam0_h != nullptr;
      if (start)
        h2d(hLam0, lam0_h, (size_t)n * gz.nrows * sizeof(double), stream);
      SimGroundWsArgs wa;
      wa.e.g = g.args(dt);
      wa.e.g.X = hX;
      wa.e.g.tau = hTau;
      wa.e.g.advance = 0;
      wa.e.g.a_out = hA;
      wa.e.g.lam_out = hLam;
      wa.e.g.contact_out = hCon;
      wa.e.g.vnext_out = hV;
      wa.e.g.gap_out = hGap;
      wa.e.plane = plane_h ? dPlane : nullptr;
      wa.e.mu = mu_h ? dMu : nullptr;
      wa.e.push = push_h ? dPush : nullptr;
      wa.e.push_joint = joint;
      wa.lam0 = start ? hLam0 : nullptr;
      wa.lamc_out = hLamC;
      wa.sweeps_out = hSw;
      wa.resid_out = hRes;
      wa.warm_start = start ? 1 : 0;
      wa.min_sweeps = st.min_sweeps;
      wa.tol = st.tol;
      run(n, wa);
      if (v_out)
        d2h(v_out, hV, (size_t)n * sz.nv * sizeof(double), stream);
      if (a_out)
        d2h(a_out, hA, (size_t)n * sz.nv * sizeof(double), stream);
      if (lam_out)
        d2h(lam_out, hLam, (size_t)n * gz.nrows * sizeof(double), stream);
      if (lamc_out)
        d2h(lamc_out, hLamC, (size_t)n * gz.nrows * sizeof(double), stream);
      if (gap_out)
        d2h(gap_out, hGap, (size_t)n * gz.npts * sizeof(double), stream);
      if (con_out)
        d2h(con_out, hCon, (size_t)n * sizeof(unsigned), stream);
      if (sweeps_out)
        d2h(sweeps_out, hSw, (size_t)n * sizeof(int), stream);
      if (resid_out)
        d2h(resid_out, hRes, (size_t)n * sizeof(double), stream);
      stream_sync(stream);
    }
  };
} // namespace smpc
