// smpc_sim_ground_env_rt.h -- the ground of smpc_sim_ground_rt.h with a PER-ROBOT environment: robot i stands on its own plane
// plane[i] = (n, d) = {p : n . p = d} with its own friction coefficient mu[i], and one external force push[i] = (f, o) acts on the body of
// joint push_joint at the point r = p_j + R_j o (DESIGN 3.24 states the model word for word).  sim_ground_env_rt_body is a sibling of
// sim_ground_rt_body, which stays as it is: one wavefront per robot, one launch per step, the same phases with three additions
//   phase 0   the 11 doubles of the robot's environment with the other global loads (a null array stands for the handle's setting:
//             (0, 0, 1, ground_z), the settings' mu, no push)
//   phase 2+  the contact frame t1 = (e_y x n) / |e_y x n|, t2 = n x t1 (one lane); the push point r and r x f (one lane); the gaps
//             phi_c = n . p_c - d
//   phase 3   the rows of point c are t1 . lin, t2 . lin, n . lin (each one accumulator over x, y, z), so the velocity-level problem, the
//             sweep, erp and the compliance live in the contact frame
//   phase 4   the right-hand side is S tau - h + Q with Q_d = S_d.l . f + S_d.a . (r x f) on the degrees of freedom of push_joint and
//             its ancestors
//   phase 7   the forces leave in world axes: lambda_world(c) = Rc lambda_c; the contact word from the normal component in the contact frame
// The sweep keeps its compile-time row bound and its summation order; only the radius mu lambda_n reads the robot's own mu.  With the identity
// frame and a zero push every addition is an exact zero: the results equal sim_ground_rt_body's bit for bit.
// LDS: IdQuantRtScratch (19 024 B) + SimGroundEnvLds<NROWS> = SimGroundLds<NROWS> + 26 doubles.
#pragma once
#include "smpc_sim_ground_rt.h"
#include "smpc_sim_ground_env_dims.h"

namespace smpc
{
  struct SimGroundEnvArgs
  {
    SimGroundArgs g;      // (g.ground_z and g.mu serve the robots of a null array)
    const double * plane; // [n][4] (n, d) per robot (device), or null
    const double * mu;    // [n] (device), or null
    const double * push;  // [n][6] (f, o) per robot (device), or null
    int push_joint;
  };

  template <int NROWS>
  struct SimGroundEnvLds
  {
    SimGroundLds<NROWS> s;
    double env[SIM_GROUND_ENV_DOUBLES + 1]; // n 0..2 | d 3 | mu 4 | f 5..7 | o 8..10
    double t1[3], t2[3];                    // the contact frame's tangents
    double r[3], rxf[3];                    // the push point and the moment of the push about the world origin
    double pad[2];
  };
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundEnvLds<24>) <= 163840 / 3, "three blocks per compute unit");
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundEnvLds<12>) <= sizeof(IdQuantRtScratch) + sizeof(SimRtLds), "no more LDS than sim_rt_body");

  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_env_rt_body(const SimGroundEnvArgs & ea, int block)
  {
    typedef IdQuantRtScratch SC;
    typedef SimGroundLds<NROWS> L;
    typedef SimGroundEnvLds<NROWS> LE;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF, LDM = L::NV, NCM = L::NC, NR = L::NR, NPM = L::NP, LDG = L::LDG, NE = SIM_GROUND_ENV_DOUBLES;
    static_assert(LDM <= NT - NE - 1 && NR <= NT && NCM % 3 == 0 && NPM <= 24, "torques and environment load side by side; points on lanes 32 .. 55");
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
    SMPC_LDS(SC, scs, 1);
    SMPC_LDS(LE, ls, 1);
    SC & sc = scs[0];
    LE & e = ls[0];
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
      s.idg[lane] = 1.0 / (dt * s.G[lane * LDG + lane]);
    SMPC_LANES_END_WAVE
    // ---- phase 5: projected Gauss-Seidel, exactly `sweeps` sweeps, points in ascending order (the sweep of sim_ground_rt_body) ----
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
          const double nrm = sqrt(t1 * t1 + t2 * t2), lim = e.env[4] * s.lam[rn];
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
    // ---- phase 7: every global store; the forces in world axes, lambda_world(c) = Rc lambda_c ----
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
        double w = e.t1[i] * s.lam[3 * c];
        w += e.t2[i] * s.lam[3 * c + 1];
        w += e.env[i] * s.lam[3 * c + 2];
        ka.lam_out[(size_t)inst * nr + lane] = w;
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
    }
    SMPC_LANES_END_WAVE
  }

  // ---- host: the per-robot environment of one simulator handle's ground (a sibling of RobotSimGround, which owns the settings, the sizes
  // and the buffers of the last step).  `active` once a setter has been called: from then on the handle's ground steps launch the kernel
  // above.  The host-buffer solve needs no setter. ----
  struct RobotSimGroundEnv
  {
    RobotSimGround & g;
    bool active = false;
    double *plane = nullptr, *mu = nullptr, *push = nullptr; // [B][4], [B], [B][6] (device), null: the handle's setting
    int push_joint = 0;
    // host-buffer form (n states, n need not be B): grown on demand
    int cap = 0;
    double *hX = nullptr, *hTau = nullptr, *hV = nullptr, *hA = nullptr, *hLam = nullptr, *hGap = nullptr, *hEnv = nullptr;
    unsigned * hCon = nullptr;

    explicit RobotSimGroundEnv(RobotSimGround & ground) : g(ground) {}
    RobotSimGroundEnv(const RobotSimGroundEnv &) = delete;
    RobotSimGroundEnv & operator=(const RobotSimGroundEnv &) = delete;
    void free_staging()
    {
      dev_free(hX);
      dev_free(hTau);
      dev_free(hV);
      dev_free(hA);
      dev_free(hLam);
      dev_free(hGap);
      dev_free(hEnv);
      dev_free(hCon);
      hX = hTau = hV = hA = hLam = hGap = hEnv = nullptr;
      hCon = nullptr;
      cap = 0;
    }
    ~RobotSimGroundEnv()
    {
      free_staging();
      dev_free(plane);
      dev_free(mu);
      dev_free(push);
    }
    // (the caller has run sim_ground_env_admission_error) either array may be null: uniform
    void set_env(const double * plane_h, const double * mu_h)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const size_t B = (size_t)sim.B;
      AllocScope scope; // (a failing allocation below releases the one before it; the previous environment stays)
      double * np = plane_h ? (double *)dev_alloc(B * 4 * sizeof(double)) : nullptr;
      double * nm = mu_h ? (double *)dev_alloc(B * sizeof(double)) : nullptr;
      sim.wait(); // (a step in flight still reads the buffers that are replaced below)
      if (np)
        h2d(np, plane_h, B * 4 * sizeof(double), sim.stream);
      if (nm)
        h2d(nm, mu_h, B * sizeof(double), sim.stream);
      stream_sync(sim.stream);
      scope.commit();
      dev_free(plane);
      dev_free(mu);
      plane = np;
      mu = nm;
      active = true;
    }
    // (the caller has run sim_ground_push_admission_error) null clears the push
    void set_push(int joint, const double * push_h)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const size_t bytes = (size_t)sim.B * 6 * sizeof(double);
      if (push_h && !push)
        push = (double *)dev_alloc(bytes);
      sim.wait();
      if (push_h)
      {
        h2d(push, push_h, bytes, sim.stream);
        stream_sync(sim.stream);
      }
      else
      {
        dev_free(push);
        push = nullptr;
      }
      push_joint = joint;
      active = true;
    }
    void run(int n, const SimGroundEnvArgs & ea)
    {
      if (g.gz.inst == 12)
        launch<SimGroundEnvArgs, sim_ground_env_rt_body<12>, 64, 1, 0>(n, g.sim.stream, ea);
      else
        launch<SimGroundEnvArgs, sim_ground_env_rt_body<24>, 64, 1, 0>(n, g.sim.stream, ea);
    }
    void step_device(double * X_dev, const double * tau_dev, double dt)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      SimGroundEnvArgs ea;
      ea.g = g.args(dt);
      ea.g.X = X_dev;
      ea.g.tau = tau_dev;
      ea.g.advance = 1;
      ea.g.a_out = sim.a;
      ea.g.lam_out = g.lam;
      ea.g.contact_out = g.contact;
      ea.plane = plane;
      ea.mu = mu;
      ea.push = push;
      ea.push_joint = push_joint;
      run(sim.B, ea);
    }
    void dynamics(int n, const double * X, const double * tau, double dt, const double * plane_h, const double * mu_h, const double * push_h, int joint,
                  double * v_out, double * a_out, double * lam_out, double * gap_out, unsigned * con_out)
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
        double * nGap = (double *)dev_alloc((size_t)n * gz.npts * sizeof(double));
        double * nEnv = (double *)dev_alloc((size_t)n * NE * sizeof(double)); // planes [n][4] | mu [n] | pushes [n][6]
        unsigned * nCon = (unsigned *)dev_alloc((size_t)n * sizeof(unsigned));
        scope.commit();
        hX = nX;
        hTau = nTau;
        hV = nV;
        hA = nA;
        hLam = nLam;
        hGap = nGap;
        hEnv = nEnv;
        hCon = nCon;
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
      SimGroundEnvArgs ea;
      ea.g = g.args(dt);
      ea.g.X = hX;
      ea.g.tau = hTau;
      ea.g.advance = 0;
      ea.g.a_out = hA;
      ea.g.lam_out = hLam;
      ea.g.contact_out = hCon;
      ea.g.vnext_out = hV;
      ea.g.gap_out = hGap;
      ea.plane = plane_h ? dPlane : nullptr;
      ea.mu = mu_h ? dMu : nullptr;
      ea.push = push_h ? dPush : nullptr;
      ea.push_joint = joint;
      run(n, ea);
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
  };
} // namespace smpc
