// smpc_sim_rt.h -- a batched rigid-body simulator for ANY validated robot table (run-time joint tree, 2 .. SMPC_MAX_JOINTS joints): the
// constrained forward dynamics of full_fd_body / fdyn_fd_body (pinocchio::constraintDynamics as the reference's FullDynamicsOCP uses it,
// src/fulldynamics.cpp:39,50-75,139) and the semi-implicit Euler step of sim_integrate_body in ONE launch,
// with joint count, parents, axis types, feet and the contact size (3: CONTACT_3D LOCAL, 6: CONTACT_6D LOCAL_WORLD_ALIGNED) as DATA.
// One wavefront per robot, lane = joint / degree of freedom / contact row.
//   phase 0   every global load: torques and contact mask here, state and the lane's joint constants in rt_tree_phases
//   phase 1-2 rt_tree_phases (smpc_id_rt.h, shared with id_quant_rt_body): placements, motion subspace, velocities, bias accelerations,
//             subtree inertias and forces -> M (row stride 37), nle, foot Jacobians, drift
//   phase 3   contact rows of the feet in the mask, feet in contact first:  3-D  R^T J_lin, gamma = R^T a_p + Kd o R^T v_p + Kp o R^T p
//                                                                          6-D  [J_lin; S.a], gamma = [a_p + Kd v_p + Kp p ; alpha + Kd w + Kp log3(R)]
//   phase 4   M = L L^T, W = M^-1 [S tau - nle | J^T], G = J M^-1 J^T + mu I, G^-1; proximal iteration on lambda until the infinity norm of
//             the change is <= accuracy; a = M^-1 b + M^-1 J^T lambda
//   phase 5   dt > 0: v <- v + a dt, q <- q (+) v dt (SE3 exponential on the free-flyer, as lanes_integrate)
//   phase 6   every global store (the state in place: its loads are long done)
// Every dot product is one accumulator summed in ascending index order, as the oracle's loops; the one exception is the backward half of the
// two triangular solves (rt_wave_chol_solve), which takes its terms as they become final.  The factorisations and solves run on the run-time
// sizes in LDS with rolled loops: the compile-time forms (fwave_cholesky / fwave_chol_solve at 37) unroll into 984 spilled registers here.
// LDS: IdQuantRtScratch (tree walk) + SimRtLds below, both sized by SMPC_MAX_JOINTS and 12 contact rows.  M has the odd row stride 37: the
// factorisation's column accesses (lane = row, 37 doubles = 74 banks apart: lanes l and l + 32 share a bank, and a 64-bit access is served
// in two halves of 32 lanes) and the row reads of the solves (one broadcast address per step) are both conflict-free.
#pragma once
#include "smpc_id_rt.h"
#include "smpc_sim_rt_dims.h"

namespace smpc
{
  struct SimRtArgs
  {
    const IdRtDevModel * model;
    double * X;            // [n][2 nj + 11] states (device); updated in place when dt > 0
    const double * tau;    // [n][nv - 6] joint torques (device)
    const unsigned * mask; // [n] contact bit per foot (device), or null: mask_all for every robot
    unsigned mask_all;
    int fs;                // 3 or 6
    double Kp[6], Kd[6], gravity[3];
    double prox_accuracy, prox_mu;
    int prox_max_iter;
    double dt;        // <= 0: forward dynamics only
    double * a_out;   // [n][nv]
    double * lam_out; // [n][fs nfeet]: contact forces ON the robot, contact frame, feet in contact first (in order), rest 0
    int * iters_out;  // [n] proximal iterations taken (may be null)
  };

  struct SimRtLds
  {
    static constexpr int NV = SIM_RT_MAX_NV, NC = SIM_RT_MAX_ROWS, NR = NC + 1;
    double M[NV * NV]; // joint-space inertia, unit diagonal beyond nv -> its Cholesky factor
    double J[NC * NV]; // contact Jacobian, rows of absent contacts and columns beyond nv zero
    double W[NV * NR]; // [M^-1 (S tau - nle) | M^-1 J^T], row-major
    double G[NC * NC], Gi[NC * NC];
    double gam[NC], JMb[NC], lam[NC], rhs[NC], dl[NC];
    double tmp[64], row[NR];
    double tau[NV], a[NV], dx[NV];
    double xn[2 * SMPC_MAX_JOINTS + 11];
  };

  // In-place lower Cholesky of the leading n x n block of A (row-major, row stride ld), n at run time; lane = row, everything stays in LDS.
  // Row r is read with a stride of ld doubles between lanes (ld odd: conflict-free), row j is one broadcast address per step.  The sums
  // run over k ascending, as fwave_cholesky and the oracle's loops.
  SMPC_DEV void rt_wave_cholesky(double * A, int ld, int n, double * tmp)
  {
    constexpr int NT = 64;
    for (int j = 0; j < n; j++)
    {
      SMPC_LANES(NT)
      if (lane >= j && lane < n)
      {
        double s = A[lane * ld + j];
        for (int k = 0; k < j; k++)
          s -= A[lane * ld + k] * A[j * ld + k];
        tmp[lane] = s;
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane >= j && lane < n)
      {
        const double d = sqrt(tmp[j]);
        A[lane * ld + j] = lane == j ? d : tmp[lane] / d;
      }
      SMPC_LANES_END_WAVE
    }
  }
  // X (n rows, NCOL columns, row stride ldx) <- (L L^T)^-1 X, n at run time; lane = row, the lane's NCOL entries in registers, the finished row
  // k is published through `row` (NCOL doubles of LDS) and read back as broadcasts.  Forward substitution: every entry takes its terms in
  // ascending k, the oracle's order.  Backward substitution: in descending k, the order in which the y_k become final -- the ascending
  // order would make the whole substitution one chain of n (n - 1) / 2 dependent multiply-adds.
  template <int NCOL>
  SMPC_DEV void rt_wave_chol_solve(const double * L, int ld, int n, double * X, int ldx, double * row)
  {
    constexpr int NT = 64;
    SMPC_PLA(double, w, NT, NCOL);
    SMPC_LANES(NT)
    {
      const int r = lane < n ? lane : 0;
#pragma unroll
      for (int c = 0; c < NCOL; c++)
        SMPC_PLV(w)[c] = X[r * ldx + c];
    }
    SMPC_LANES_END_WAVE
    for (int k = 0; k < n; k++)
    {
      SMPC_LANES(NT)
      if (lane == k)
      {
        const double d = L[k * ld + k];
#pragma unroll
        for (int c = 0; c < NCOL; c++)
        {
          SMPC_PLV(w)[c] = SMPC_PLV(w)[c] / d;
          row[c] = SMPC_PLV(w)[c];
        }
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane > k && lane < n)
      {
        const double l = L[lane * ld + k];
#pragma unroll
        for (int c = 0; c < NCOL; c++)
          SMPC_PLV(w)[c] -= l * row[c];
      }
      SMPC_LANES_END_WAVE
    }
    for (int k = n - 1; k >= 0; k--)
    {
      SMPC_LANES(NT)
      if (lane == k)
      {
        const double d = L[k * ld + k];
#pragma unroll
        for (int c = 0; c < NCOL; c++)
        {
          SMPC_PLV(w)[c] = SMPC_PLV(w)[c] / d;
          row[c] = SMPC_PLV(w)[c];
        }
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane < k)
      {
        const double l = L[k * ld + lane];
#pragma unroll
        for (int c = 0; c < NCOL; c++)
          SMPC_PLV(w)[c] -= l * row[c];
      }
      SMPC_LANES_END_WAVE
    }
    SMPC_LANES(NT)
    if (lane < n)
    {
#pragma unroll
      for (int c = 0; c < NCOL; c++)
        X[lane * ldx + c] = SMPC_PLV(w)[c];
    }
    SMPC_LANES_END_WAVE
  }

  // grid = n, 64 lanes
  SMPC_DEV void sim_rt_body(const SimRtArgs & ka, int block)
  {
    typedef IdQuantRtScratch SC;
    typedef SimRtLds L;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF, LDM = L::NV, NCM = L::NC, NR = L::NR;
    static_assert(LDM <= NT && NR <= NT && 3 * NF <= NCM, "one row / column per lane");
    const int inst = block;
    const IdRtDevModel & mi = *ka.model;
    // (wave-uniform sizes from the device table, clamped so that no entry can index outside the LDS arrays)
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nq = nj + 6, nx = 2 * nj + 11, na = nv - 6;
    const int fs = ka.fs == 6 ? 6 : 3;
    const int maxf = NCM / fs < NF ? NCM / fs : NF;
    const int nfeet = mi.t.nfeet < maxf ? (mi.t.nfeet > 0 ? mi.t.nfeet : 0) : maxf;
    SMPC_LDS(SC, scs, 1);
    SMPC_LDS(L, ls, 1);
    SC & sc = scs[0];
    L & s = ls[0];
    // ---- phase 0: every global load (the state and the joint constants: first phase of rt_tree_phases) ----
    const unsigned mask = (ka.mask != nullptr ? ka.mask[inst] : ka.mask_all) & ((1u << nfeet) - 1u);
    SMPC_LANES(NT)
    if (lane < LDM)
      s.tau[lane] = lane >= 6 && lane < nv ? ka.tau[(size_t)inst * na + lane - 6] : 0.0;
    SMPC_LANES_END_WAVE
    // ---- phases 1, 2 ----
    rt_tree_phases(sc, mi, ka.X + (size_t)inst * nx, mk3(ka.gravity[0], ka.gravity[1], ka.gravity[2]));
    const int nc = fs * __builtin_popcount(mask);
    // ---- joint-space inertia (both triangles from one expression: symmetric bit for bit) ----
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
        s.gam[lane] = 0.0;
        s.lam[lane] = 0.0;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 3: contact rows, feet in contact first, in order ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < nfeet * nv; idx += NT)
      {
        const int f = idx / nv, k = idx % nv;
        const int jf = sc.fj[f], jk = k < 6 ? 0 : k - 5;
        if (((mask >> f) & 1u) && ((sc.anc[jf] >> jk) & 1u))
        {
          const int c = __builtin_popcount(mask & ((1u << f) - 1u));
          const SV Sk = ldsv(&sc.S[k * 6]);
          const V3 lin = Sk.l + cross(Sk.a, ld3(&sc.footp[f * 3])); // velocity of the foot point under the unit twist of column k
          if (fs == 3)
          {
            const V3 col = transpose(ldm3(&sc.oR[jf * 9])) * lin; // foot frame rotation = joint rotation
            s.J[(3 * c + 0) * LDM + k] = col.x;
            s.J[(3 * c + 1) * LDM + k] = col.y;
            s.J[(3 * c + 2) * LDM + k] = col.z;
          }
          else
          {
            s.J[(6 * c + 0) * LDM + k] = lin.x;
            s.J[(6 * c + 1) * LDM + k] = lin.y;
            s.J[(6 * c + 2) * LDM + k] = lin.z;
            s.J[(6 * c + 3) * LDM + k] = Sk.a.x;
            s.J[(6 * c + 4) * LDM + k] = Sk.a.y;
            s.J[(6 * c + 5) * LDM + k] = Sk.a.z;
          }
        }
      }
      if (lane >= 32 && lane < 32 + nfeet && ((mask >> (lane - 32)) & 1u))
      {
        const int f = lane - 32, jf = sc.fj[f];
        const int c = __builtin_popcount(mask & ((1u << f) - 1u));
        const M3 Rf = ldm3(&sc.oR[jf * 9]);
        const V3 p = ld3(&sc.footp[f * 3]);
        const SV v = ldsv(&sc.vel[jf * 6]), ab = ldsv(&sc.acc[jf * 6]);
        const V3 vp = v.l + cross(v.a, p);
        // classical acceleration of the body-fixed point at zero joint accelerations
        const V3 ap = ab.l + cross(ab.a, p) + cross(v.a, vp);
        if (fs == 3)
        {
          const M3 Rt = transpose(Rf);
          const V3 drift = Rt * ap, verr = Rt * vp, perr = Rt * ((-1.0) * p);
          s.gam[3 * c + 0] = drift.x + ka.Kd[0] * verr.x - ka.Kp[0] * perr.x;
          s.gam[3 * c + 1] = drift.y + ka.Kd[1] * verr.y - ka.Kp[1] * perr.y;
          s.gam[3 * c + 2] = drift.z + ka.Kd[2] * verr.z - ka.Kp[2] * perr.z;
        }
        else
        {
          const V3 rot = log3(Rf);
          s.gam[6 * c + 0] = ap.x + ka.Kd[0] * vp.x + ka.Kp[0] * p.x;
          s.gam[6 * c + 1] = ap.y + ka.Kd[1] * vp.y + ka.Kp[1] * p.y;
          s.gam[6 * c + 2] = ap.z + ka.Kd[2] * vp.z + ka.Kp[2] * p.z;
          s.gam[6 * c + 3] = ab.a.x + ka.Kd[3] * v.a.x + ka.Kp[3] * rot.x;
          s.gam[6 * c + 4] = ab.a.y + ka.Kd[4] * v.a.y + ka.Kp[4] * rot.y;
          s.gam[6 * c + 5] = ab.a.z + ka.Kd[5] * v.a.z + ka.Kp[5] * rot.z;
        }
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: M = L L^T ; W = M^-1 [S tau - nle | J^T] ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < nv * NR; idx += NT)
    {
      const int k = idx / NR, c = idx % NR;
      s.W[idx] = c == 0 ? s.tau[k] - sc.h[k] : s.J[(c - 1) * LDM + k];
    }
    SMPC_LANES_END_WAVE
    rt_wave_cholesky(s.M, LDM, nv, s.tmp);
    rt_wave_chol_solve<NR>(s.M, LDM, nv, s.W, NR, s.row);
    // damped Delassus matrix (unit diagonal on the rows of absent contacts), J M^-1 b
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NCM * NCM; idx += NT)
      {
        const int c = idx / NCM, d = idx % NCM;
        double acc = 0.0;
        for (int k = 0; k < nv; k++)
          acc += s.J[c * LDM + k] * s.W[k * NR + 1 + d];
        if (c == d)
          acc += c < nc ? ka.prox_mu : 1.0;
        s.G[idx] = acc;
        s.Gi[idx] = c == d ? 1.0 : 0.0;
      }
      if (lane < NCM)
      {
        double acc = 0.0;
        for (int k = 0; k < nv; k++)
          acc += s.J[lane * LDM + k] * s.W[k * NR];
        s.JMb[lane] = acc;
      }
    }
    SMPC_LANES_END_WAVE
    rt_wave_cholesky(s.G, NCM, NCM, s.tmp);
    rt_wave_chol_solve<NCM>(s.G, NCM, NCM, s.Gi, NCM, s.row);
    // proximal iteration:  lam <- G^-1 (mu lam - gamma - J M^-1 b)  until |d lam|_inf <= accuracy
    int iters = 0;
    if (nc > 0)
      for (int it = 0; it < ka.prox_max_iter; it++)
      {
        SMPC_LANES(NT)
        if (lane < NCM)
          s.rhs[lane] = lane < nc ? ka.prox_mu * s.lam[lane] - s.gam[lane] - s.JMb[lane] : 0.0;
        SMPC_LANES_END_WAVE
        SMPC_LANES(NT)
        if (lane < NCM)
        {
          double acc = 0.0;
          for (int d = 0; d < NCM; d++)
            acc += s.Gi[lane * NCM + d] * s.rhs[d];
          s.dl[lane] = fabs(acc - s.lam[lane]);
          s.lam[lane] = acc;
        }
        SMPC_LANES_END_WAVE
        iters = it + 1;
        double diff = 0.0; // wave-uniform: every lane reads the same values
        for (int c = 0; c < NCM; c++)
          diff = fmax(diff, s.dl[c]);
        if (diff <= ka.prox_accuracy)
          break;
      }
    // a = M^-1 (S tau - nle) + M^-1 J^T lam
    SMPC_LANES(NT)
    if (lane < nv)
    {
      double acc = s.W[lane * NR];
      for (int c = 0; c < NCM; c++)
        acc += s.W[lane * NR + 1 + c] * s.lam[c];
      s.a[lane] = acc;
    }
    SMPC_LANES_END_WAVE
    // ---- phase 5: semi-implicit Euler, v <- v + a dt ; q <- q (+) v dt ----
    const bool step = ka.dt > 0.0;
    if (step)
    {
      SMPC_LANES(NT)
      if (lane < nv)
      {
        const double vn = sc.x[nq + lane] + s.a[lane] * ka.dt;
        s.xn[nq + lane] = vn;
        s.dx[lane] = vn * ka.dt;
      }
      SMPC_LANES_END_WAVE
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
    // ---- phase 6: every global store ----
    SMPC_LANES(NT)
    {
      if (step)
        for (int i = lane; i < nx; i += NT)
          ka.X[(size_t)inst * nx + i] = s.xn[i];
      if (lane < nv)
        ka.a_out[(size_t)inst * nv + lane] = s.a[lane];
      if (lane < fs * nfeet)
        ka.lam_out[(size_t)inst * fs * nfeet + lane] = s.lam[lane];
      if (lane == 0 && ka.iters_out != nullptr)
        ka.iters_out[inst] = iters;
    }
    SMPC_LANES_END_WAVE
  }

  // ---- host engine: a robot table on the device, the results of the last step, staging buffers of the host-buffer form ----
  struct RobotSimRt
  {
    int B = 0, device_id = 0;
    SimRtSizes sz;
    double gravity[3] = {0.0, 0.0, -9.81};
    stream_t stream, own_stream;
    IdRtDevModel * model = nullptr;
    double *a = nullptr, *lam = nullptr; // [B][nv], [B][fs nfeet]: the last step
    // host-buffer form (n states, n need not be B): grown on demand
    int cap = 0;
    double *hX = nullptr, *hTau = nullptr, *hA = nullptr, *hLam = nullptr;
    unsigned * hMask = nullptr;
    int * hIt = nullptr;

    RobotSimRt(const smpc_robot_model * rm, int force_size, int batch, const double * g, int device)
    {
      const std::string why = sim_rt_admission_error(rm, force_size, batch);
      if (!why.empty())
        throw InvalidCall(why);
      sz = sim_rt_sizes(rm->njoints, rm->nfeet, force_size);
      B = batch;
      device_id = device;
      if (g)
        for (int i = 0; i < 3; i++)
          gravity[i] = g[i];
      set_device(device);
      AllocScope scope; // (a failing allocation below releases the ones before it)
      stream = own_stream = stream_create();
      try
      {
        IdRtDevModel hm;
        std::memset(&hm, 0, sizeof(hm));
        fill_rt_model(rm, hm.t);
        const std::vector<unsigned> anc = id_rt_ancestors(rm);
        for (int j = 0; j < SMPC_MAX_JOINTS; j++)
          hm.anc[j] = anc[j];
        hm.total_mass = rm->total_mass;
        model = (IdRtDevModel *)dev_alloc(sizeof(IdRtDevModel));
        a = (double *)dev_alloc((size_t)B * sz.nv * sizeof(double));
        lam = (double *)dev_alloc((size_t)B * sz.nlam * sizeof(double));
        h2d(model, &hm, sizeof(hm), stream);
        stream_sync(stream);
      }
      catch (...)
      { // (the destructor does not run for a partially constructed engine)
        stream_destroy(own_stream);
        throw;
      }
      scope.commit();
    }
    RobotSimRt(const RobotSimRt &) = delete;
    RobotSimRt & operator=(const RobotSimRt &) = delete;
    void free_staging()
    {
      dev_free(hX);
      dev_free(hTau);
      dev_free(hA);
      dev_free(hLam);
      dev_free(hMask);
      dev_free(hIt);
      hX = hTau = hA = hLam = nullptr;
      hMask = nullptr;
      hIt = nullptr;
      cap = 0;
    }
    ~RobotSimRt()
    {
      free_staging();
      dev_free(model);
      dev_free(a);
      dev_free(lam);
      stream_destroy(own_stream);
    }
    SimRtArgs args(const double * Kp, const double * Kd, double acc, double mu, int max_iter) const
    {
      SimRtArgs ka;
      std::memset(&ka, 0, sizeof(ka));
      ka.model = model;
      ka.fs = sz.fs;
      for (int i = 0; i < sz.fs; i++)
      {
        ka.Kp[i] = Kp ? Kp[i] : 0.0;
        ka.Kd[i] = Kd ? Kd[i] : 0.0;
      }
      for (int i = 0; i < 3; i++)
        ka.gravity[i] = gravity[i];
      // ProximalSettings(1e-9, 1e-10, 10) of the reference (src/fulldynamics.cpp:39) for arguments <= 0
      ka.prox_accuracy = acc > 0.0 ? acc : 1e-9;
      ka.prox_mu = mu > 0.0 ? mu : 1e-10;
      ka.prox_max_iter = max_iter > 0 ? max_iter : 10;
      return ka;
    }
    void forward_dynamics(int n, const double * X, const double * tau, const unsigned * mask, const double * Kp, const double * Kd, double acc, double mu,
                          int max_iter, double * a_out, double * lam_out, int * iters_out)
    {
      if (n < 1)
        throw InvalidCall("n must be positive");
      set_device(device_id);
      if (n > cap)
      {
        stream_sync(stream);
        free_staging();
        AllocScope scope; // (the pointers are kept only once every allocation has succeeded)
        double * nX = (double *)dev_alloc((size_t)n * sz.nx * sizeof(double));
        double * nTau = (double *)dev_alloc((size_t)n * sz.na * sizeof(double));
        double * nA = (double *)dev_alloc((size_t)n * sz.nv * sizeof(double));
        double * nLam = (double *)dev_alloc((size_t)n * sz.nlam * sizeof(double));
        unsigned * nMask = (unsigned *)dev_alloc((size_t)n * sizeof(unsigned));
        int * nIt = (int *)dev_alloc((size_t)n * sizeof(int));
        scope.commit();
        hX = nX;
        hTau = nTau;
        hA = nA;
        hLam = nLam;
        hMask = nMask;
        hIt = nIt;
        cap = n;
      }
      h2d(hX, X, (size_t)n * sz.nx * sizeof(double), stream);
      h2d(hTau, tau, (size_t)n * sz.na * sizeof(double), stream);
      h2d(hMask, mask, (size_t)n * sizeof(unsigned), stream);
      SimRtArgs ka = args(Kp, Kd, acc, mu, max_iter);
      ka.X = hX;
      ka.tau = hTau;
      ka.mask = hMask;
      ka.dt = 0.0;
      ka.a_out = hA;
      ka.lam_out = hLam;
      ka.iters_out = hIt;
      launch<SimRtArgs, sim_rt_body, 64, 1, 0>(n, stream, ka);
      d2h(a_out, hA, (size_t)n * sz.nv * sizeof(double), stream);
      d2h(lam_out, hLam, (size_t)n * sz.nlam * sizeof(double), stream);
      if (iters_out)
        d2h(iters_out, hIt, (size_t)n * sizeof(int), stream);
      stream_sync(stream);
    }
    void step_device(double * X_dev, const double * tau_dev, unsigned mask_all, const unsigned * mask_dev, const double * Kp, const double * Kd, double dt)
    {
      set_device(device_id);
      SimRtArgs ka = args(Kp, Kd, 0.0, 0.0, 0);
      ka.X = X_dev;
      ka.tau = tau_dev;
      ka.mask = mask_dev;
      ka.mask_all = mask_all;
      ka.dt = dt;
      ka.a_out = a;
      ka.lam_out = lam;
      ka.iters_out = nullptr;
      launch<SimRtArgs, sim_rt_body, 64, 1, 0>(B, stream, ka);
    }
    void wait()
    {
      set_device(device_id);
      stream_sync(stream);
    }
    void read_last(double * a_out, double * lam_out)
    {
      set_device(device_id);
      if (a_out)
        d2h(a_out, a, (size_t)B * sz.nv * sizeof(double), stream);
      if (lam_out)
        d2h(lam_out, lam, (size_t)B * sz.nlam * sizeof(double), stream);
      stream_sync(stream);
    }
    void adopt_stream(stream_t st, bool back_to_own)
    {
      set_device(device_id);
      stream_sync(stream);
      stream = back_to_own ? own_stream : st;
    }
  };
} // namespace smpc
