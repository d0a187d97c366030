// smpc_sim_ground_rt.h -- a ground plane with UNILATERAL contact and Coulomb friction for the rigid-body simulator on a run-time joint tree
// (smpc_sim_rt.h).  sim_rt_body applies the bilateral contacts its caller names in a mask; sim_ground_rt_body takes no mask: every contact
// point (P points per foot, offsets in the foot frame) is a row block [x y z] of a velocity-level complementarity problem that a fixed
// number of projected Gauss-Seidel sweeps solves, detected from the state alone (DESIGN 3.23 states the model word for word).
// One wavefront per robot, one launch per step; the phase discipline of sim_rt_body:
//   phase 0   every global load: torques here, state and the lane's joint constants in rt_tree_phases
//   phase 1-2 rt_tree_phases (smpc_id_rt.h): placements, motion subspace, subtree inertias and forces -> M (row stride 37), h
//   phase 3   contact points p_c = p_f + R_f o_k, gaps phi_c = p_c.z - ground_z, world-aligned rows J_c = [S.l + S.a x p_c] of every point
//   phase 4   M = L L^T, W = M^-1 [S tau - h | J^T];  v_f = v + dt W_0;  G = J W_1 + r I;  c0 = J v_f (+ phi / dt or erp phi / dt on normal rows)
//   phase 5   `sweeps` sweeps of projected Gauss-Seidel on lambda from 0, points in ascending order: the normal row on one lane, then the two
//             tangential rows on two lanes, then the projection onto the disc of radius mu lambda_n -- no early exit: the work is
//             wave-uniform and the result deterministic
//   phase 6   a = W_0 + W_1 lambda, v+ = v_f + dt W_1 lambda, q+ = q (+) v+ dt (the integration of sim_rt_body)
//   phase 7   every global store (the state in place: its loads are long done), vector stores in plain C++
// Every dot product is one accumulator summed in ascending index order.  The dot products of the sweep run over the whole row of the
// instantiation (a compile-time bound, unrolled: the LDS loads of a row go out together, ahead of the chain of multiply-adds); G and lambda
// are zero beyond the rows of the robot's points, so the extra terms add exact zeros.  The one deviation from the written model: the
// divisions by dt G_rr of the sweep are multiplications by 1 / (dt G_rr), computed once per row with a full division (the sweep is one
// chain of dependent operations: three divisions per point and sweep would be a third of it).
// LDS: IdQuantRtScratch (19 024 B) + SimGroundLds<NROWS>; G row-contiguous at the odd stride NROWS + 1, lambda read as broadcasts.
#pragma once
#include "smpc_sim_rt.h"
#include "smpc_sim_ground_dims.h"

namespace smpc
{
  struct SimGroundArgs
  {
    const IdRtDevModel * model;
    double * X;         // [n][2 nj + 11] states (device); updated in place when advance != 0
    const double * tau; // [n][nv - 6] joint torques (device)
    double gravity[3];
    double ground_z, mu, erp, compliance, dt; // dt > 0
    int sweeps, P, advance;
    double points[SIM_GROUND_MAX_PPF][3];
    double * a_out;          // [n][nv]
    double * lam_out;        // [n][3 nfeet P]: forces ON the robot, world axes, [point][x y z]
    unsigned * contact_out;  // [n] bit c: lambda_n of point c > 0
    double * vnext_out;      // [n][nv] or null
    double * gap_out;        // [n][nfeet P] or null
  };

  template <int NROWS>
  struct SimGroundLds
  {
    static constexpr int NV = SIM_RT_MAX_NV, NC = NROWS, NR = NC + 1, NP = NC / 3, LDG = NC + 1;
    double M[NV * NV]; // joint-space inertia -> its Cholesky factor
    double J[NC * NV]; // rows of the contact points, rows of absent points and columns beyond nv zero
    double W[NV * NR]; // [M^-1 (S tau - h) | M^-1 J^T], row-major
    double G[NC * LDG];
    double c0[NC], lam[NC], idg[NC];
    double pc[NP * 3], gap[NP], tc[2];
    double tmp[64], row[NR];
    double tau[NV], vf[NV], a[NV], dx[NV];
    double xn[2 * SMPC_MAX_JOINTS + 11];
  };
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundLds<24>) <= 163840 / 3, "three blocks per compute unit");
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundLds<12>) <= sizeof(IdQuantRtScratch) + sizeof(SimRtLds), "no more LDS than sim_rt_body");

  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_rt_body(const SimGroundArgs & ka, int block)
  {
    typedef IdQuantRtScratch SC;
    typedef SimGroundLds<NROWS> L;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF, LDM = L::NV, NCM = L::NC, NR = L::NR, NPM = L::NP, LDG = L::LDG;
    static_assert(LDM <= NT && NR <= NT && NCM % 3 == 0 && NPM <= 32, "one row / column per lane, one contact bit per point");
    const int inst = block;
    const IdRtDevModel & mi = *ka.model;
    // (wave-uniform sizes from the device table and the arguments, clamped so that no value can index outside the LDS arrays)
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nq = nj + 6, nx = 2 * nj + 11, na = nv - 6;
    const int P = ka.P < SIM_GROUND_MAX_PPF ? (ka.P > 1 ? ka.P : 1) : SIM_GROUND_MAX_PPF;
    const int maxf = NPM / P < NF ? NPM / P : NF;
    const int nfeet = mi.t.nfeet < maxf ? (mi.t.nfeet > 0 ? mi.t.nfeet : 0) : maxf;
    const int npts = nfeet * P, nr = 3 * npts;
    const double dt = ka.dt;
    SMPC_LDS(SC, scs, 1);
    SMPC_LDS(L, ls, 1);
    SC & sc = scs[0];
    L & s = ls[0];
    // ---- phase 0: every global load (the state and the joint constants: first phase of rt_tree_phases) ----
    SMPC_LANES(NT)
    if (lane < LDM)
      s.tau[lane] = lane >= 6 && lane < nv ? ka.tau[(size_t)inst * na + lane - 6] : 0.0;
    SMPC_LANES_END_WAVE
    // ---- phases 1, 2 ----
    rt_tree_phases(sc, mi, ka.X + (size_t)inst * nx, mk3(ka.gravity[0], ka.gravity[1], ka.gravity[2]));
    // ---- joint-space inertia (both triangles from one expression: symmetric bit for bit); contact points and gaps ----
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
        s.lam[lane] = 0.0;
        s.idg[lane] = 0.0;
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
          gap = p.z - ka.ground_z;
        }
        st3(&s.pc[c * 3], p);
        s.gap[c] = gap;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 3: the rows of every point, x y z in world axes ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < npts * nv; idx += NT)
    {
      const int c = idx / nv, k = idx % nv;
      const int jf = sc.fj[c / P], jk = k < 6 ? 0 : k - 5;
      if ((sc.anc[jf] >> jk) & 1u)
      {
        const SV Sk = ldsv(&sc.S[k * 6]);
        const V3 lin = Sk.l + cross(Sk.a, ld3(&s.pc[c * 3])); // velocity of the point under the unit twist of column k
        s.J[(3 * c + 0) * LDM + k] = lin.x;
        s.J[(3 * c + 1) * LDM + k] = lin.y;
        s.J[(3 * c + 2) * LDM + k] = lin.z;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: M = L L^T ; W = M^-1 [S tau - h | J^T] ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < nv * NR; idx += NT)
    {
      const int k = idx / NR, c = idx % NR;
      s.W[idx] = c == 0 ? s.tau[k] - sc.h[k] : s.J[(c - 1) * LDM + k];
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
      s.idg[lane] = 1.0 / (dt * s.G[lane * LDG + lane]);
    SMPC_LANES_END_WAVE
    // ---- phase 5: projected Gauss-Seidel, exactly `sweeps` sweeps, points in ascending order ----
    for (int sw = 0; sw < ka.sweeps; sw++)
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
          s.lam[rn] = fmax(0.0, s.lam[rn] - (s.c0[rn] + dt * acc) * s.idg[rn]);
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
          s.tc[lane] = s.lam[rt] - (s.c0[rt] + dt * acc) * s.idg[rt];
        }
        SMPC_LANES_END_WAVE
        SMPC_LANES(NT)
        if (lane < 2)
        {
          const double t1 = s.tc[0], t2 = s.tc[1];
          const double nrm = sqrt(t1 * t1 + t2 * t2), lim = ka.mu * s.lam[rn];
          double t = s.tc[lane];
          if (nrm > lim)
            t = t * (lim / nrm);
          if (nrm == 0.0)
            t = 0.0;
          s.lam[3 * c + lane] = t;
        }
        SMPC_LANES_END_WAVE
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
    // ---- phase 7: every global store ----
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
        ka.lam_out[(size_t)inst * nr + lane] = s.lam[lane];
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
    }
    SMPC_LANES_END_WAVE
  }

  // ---- host: the ground of one simulator handle (a sibling of RobotSimRt, which owns the robot table, the stream and the accelerations) ----
  struct RobotSimGround
  {
    RobotSimRt & sim;
    SimGroundSettings gs;
    SimGroundSizes gz;
    double * lam = nullptr;     // [B][3 npts]: the last ground step
    unsigned * contact = nullptr; // [B]
    // host-buffer form (n states, n need not be B): grown on demand
    int cap = 0;
    double *hX = nullptr, *hTau = nullptr, *hV = nullptr, *hA = nullptr, *hLam = nullptr, *hGap = nullptr;
    unsigned * hCon = nullptr;

    // (the caller has run sim_ground_admission_error on `g`)
    RobotSimGround(RobotSimRt & owner, const smpc_ground_settings * g) : sim(owner)
    {
      gs = sim_ground_resolve(g);
      gz = sim_ground_sizes(sim.sz.nfeet, gs.P);
      set_device(sim.device_id);
      AllocScope scope; // (a failing allocation below releases the one before it)
      lam = (double *)dev_alloc((size_t)sim.B * gz.nrows * sizeof(double));
      contact = (unsigned *)dev_alloc((size_t)sim.B * sizeof(unsigned));
      scope.commit();
    }
    RobotSimGround(const RobotSimGround &) = delete;
    RobotSimGround & operator=(const RobotSimGround &) = delete;
    void free_staging()
    {
      dev_free(hX);
      dev_free(hTau);
      dev_free(hV);
      dev_free(hA);
      dev_free(hLam);
      dev_free(hGap);
      dev_free(hCon);
      hX = hTau = hV = hA = hLam = hGap = nullptr;
      hCon = nullptr;
      cap = 0;
    }
    ~RobotSimGround()
    {
      free_staging();
      dev_free(lam);
      dev_free(contact);
    }
    SimGroundArgs args(double dt) const
    {
      SimGroundArgs ka;
      std::memset(&ka, 0, sizeof(ka));
      ka.model = sim.model;
      for (int i = 0; i < 3; i++)
        ka.gravity[i] = sim.gravity[i];
      ka.ground_z = gs.ground_z;
      ka.mu = gs.mu;
      ka.erp = gs.erp;
      ka.compliance = gs.compliance;
      ka.sweeps = gs.sweeps;
      ka.P = gs.P;
      for (int k = 0; k < SIM_GROUND_MAX_PPF; k++)
        for (int i = 0; i < 3; i++)
          ka.points[k][i] = gs.points[k][i];
      ka.dt = dt;
      return ka;
    }
    void run(int n, const SimGroundArgs & ka)
    {
      if (gz.inst == 12)
        launch<SimGroundArgs, sim_ground_rt_body<12>, 64, 1, 0>(n, sim.stream, ka);
      else
        launch<SimGroundArgs, sim_ground_rt_body<24>, 64, 1, 0>(n, sim.stream, ka);
    }
    void step_device(double * X_dev, const double * tau_dev, double dt)
    {
      set_device(sim.device_id);
      SimGroundArgs ka = args(dt);
      ka.X = X_dev;
      ka.tau = tau_dev;
      ka.advance = 1;
      ka.a_out = sim.a;
      ka.lam_out = lam;
      ka.contact_out = contact;
      run(sim.B, ka);
    }
    void dynamics(int n, const double * X, const double * tau, double dt, double * v_out, double * a_out, double * lam_out, double * gap_out, unsigned * con_out)
    {
      if (n < 1)
        throw InvalidCall("n must be positive");
      set_device(sim.device_id);
      const SimRtSizes & sz = sim.sz;
      stream_t stream = sim.stream;
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
        double * nGap = (double *)dev_alloc((size_t)n * gz.npts * sizeof(double));
        unsigned * nCon = (unsigned *)dev_alloc((size_t)n * sizeof(unsigned));
        scope.commit();
        hX = nX;
        hTau = nTau;
        hV = nV;
        hA = nA;
        hLam = nLam;
        hGap = nGap;
        hCon = nCon;
        cap = n;
      }
      h2d(hX, X, (size_t)n * sz.nx * sizeof(double), stream);
      h2d(hTau, tau, (size_t)n * sz.na * sizeof(double), stream);
      SimGroundArgs ka = args(dt);
      ka.X = hX;
      ka.tau = hTau;
      ka.advance = 0;
      ka.a_out = hA;
      ka.lam_out = hLam;
      ka.contact_out = hCon;
      ka.vnext_out = hV;
      ka.gap_out = hGap;
      run(n, ka);
      if (v_out)
        d2h(v_out, hV, (size_t)n * sz.nv * sizeof(double), stream);
      if (a_out)
        d2h(a_out, hA, (size_t)n * sz.nv * sizeof(double), stream);
      if (lam_out)
        d2h(lam_out, hLam, (size_t)n * gz.nrows * sizeof(double), stream);
      if (gap_out)
        d2h(gap_out, hGap, (size_t)n * gz.npts * sizeof(double), stream);
      if (con_out)
        d2h(con_out, hCon, (size_t)n * sizeof(unsigned), stream);
      stream_sync(stream);
    }
    void read_last(double * lam_out, unsigned * con_out)
    {
      set_device(sim.device_id);
      if (lam_out)
        d2h(lam_out, lam, (size_t)sim.B * gz.nrows * sizeof(double), sim.stream);
      if (con_out)
        d2h(con_out, contact, (size_t)sim.B * sizeof(unsigned), sim.stream);
      stream_sync(sim.stream);
    }
  };
} // namespace smpc
