// smpc_full_engine.h -- the batched FULL-DYNAMICS MPC engine (reference FullDynamicsOCP under the MPC class: src/fulldynamics.cpp:30-455,
// src/mpc.cpp:19-392) and the kinodynamics OCP with 6-D feet on the same dense kernels: its constructor and its kernels.  State machine, ring
// discipline and launch schedule are StageEngine's (smpc_stage_engine.h), as for KinoEngine; the stage kernels are fdyn_deriv_body /
// fdyn_trial_body (smpc_full_stage.h), the sweeps are dense (riccati_dense_body on the matrix cores, or the VALU cross-check riccati_full_body
// with SMPC_RICCATI=valu).
#pragma once
#include <chrono>
#include "smpc_engine.h"
#include "smpc_full_solver.h"
#include "smpc_riccati_dense.h"
#include "smpc_full_stage.h"

namespace smpc
{
  struct HostFullSettings // FullDynamicsSettings, include/simple-mpc/fulldynamics.hpp:28-65
  {
    double timestep;
    std::vector<double> w_x, w_u, w_cent, w_forces, w_frame, umin, umax, qmin, qmax, Kp, Kd;
    std::vector<double> w_centder; // kinodynamics variant (FullDims<..., KIN = 1>): KinodynamicsSettings::w_centder
    double gravity[3];
    double mu, Lfoot, Wfoot;
    int force_size, torque_limits, kinematics_limits, force_cone, land_cstr;
    int terminal_constraint = 0; // createProblem(..., terminal_constraint)
  };

  constexpr StageKind FULL_KIND = {0x534d504346554c4cLL, "kind (full dynamics)", "smpc_create_fulldynamics", false};

  template <class D>
  class FullEngine : public StageEngine<D>
  {
  public:
    typedef StageEngine<D> Base;
    using MpcEngineBase::B;
    using MpcEngineBase::H;
    using MpcEngineBase::R;
    using MpcEngineBase::head;
    using MpcEngineBase::stream;
    using MpcEngineBase::ms;
    using MpcEngineBase::dims;
    using MpcEngineBase::device_id;
    using MpcEngineBase::profiling;
    using MpcEngineBase::force_size;
    using MpcEngineBase::x_model_ref;
    using MpcEngineBase::x_reference;
    using MpcEngineBase::vbase_dev;
    using MpcEngineBase::ref_rot;
    using MpcEngineBase::get_linear;
    using MpcEngineBase::open_stream;
    using MpcEngineBase::check_stage;
    using Base::buf;
    using Base::horizon;
    using Base::standing;
    using Base::X_dev;
    using Base::n_parts;
    using Base::solver_args;
    using Base::stage_args;
    template <class Args, void (*Body)(const Args &, int), int NT, int MINW = 1>
    void timed_launch(int kid, int grid, const Args & a, bool aux = false) // (a member template of a dependent base is not found unqualified)
    {
      static_cast<MpcEngineBase *>(this)->timed_launch<Args, Body, NT, MINW>(kid, grid, a, aux);
    }
    double * deriv_wide = nullptr; // D::WIDE_DEV: R1 / JT slices of the derivative kernel's blocks (FullDerivWide, smpc_full_stage.h)
    int n_res = 0;                 // blocks of its persistent grid (compute units x resident blocks per unit)
    // The batch as parts on streams of their own (StageEngine's parts; SMPC_FULL_PARTS=n, default 1): one wavefront per instance is all the sweeps have, so
    // at B = 1024 riccati_dense_body runs one wave per SIMD for its whole duration; with two parts the sweep of one could run beside the stage
    // kernel of the other.  Measured on the biped (B = 1024, H = 100): 10.77 k control-steps/s with 1 part, 10.29 k with 2, 10.43 k with 3 --
    // three derivative blocks fill a CU's LDS (3 x 53 KB), a sweep block (36 KB) finds no room beside them and the two kernels take turns as
    // before; the quadruped (B = 4096): 70.5 k -> 71.3 k.  Kept off.  Instances are independent: bit-identical results (tests).
    bool valu_riccati = xcheck_env("SMPC_RICCATI") && std::string(xcheck_env("SMPC_RICCATI")) == "valu";
#ifndef SMPC_FDYN_DERIV_MINW
#define SMPC_FDYN_DERIV_MINW 1
#endif
    static constexpr int DERIV_MINW = D::NV <= 20 ? SMPC_FDYN_DERIV_MINW : 1; // (register-cap experiment: -DSMPC_FDYN_DERIV_MINW=2)
    static constexpr int TRIAL_MINW = D::NV <= 20 ? 2 : 1; // waves per SIMD the evaluation kernel's register budget is capped for

    FullEngine(const smpc_robot_model * rm, const HostFullSettings & fs, const HostMpcSettings & ms_, int batch, double gravity_arg, int device)
    : Base(FULL_KIND, ms_, batch, device)
    {
      AllocScope ctor_scope; // (a throw below releases what was allocated so far: smpc_alloc_scope.h)
      if (rm->njoints != D::NJ || rm->nfeet != D::NF)
        throw std::runtime_error("robot shape (njoints, nfeet) does not match this kernel instantiation");
      if (fs.force_size != D::FS)
        throw std::runtime_error("force size in settings does not match reference force size");
      if (batch <= 0)
        throw std::runtime_error("batch must be positive");
      if ((int)fs.Kp.size() != D::FS)
        throw std::runtime_error("Force must be of same size as Kp correction"); // src/fulldynamics.cpp:41-44
      if ((int)fs.Kd.size() != D::FS)
        throw std::runtime_error("Force must be of same size as Kd correction"); // src/fulldynamics.cpp:45-48
      if ((int)fs.w_x.size() != D::NDX * D::NDX || (int)fs.w_u.size() != D::NU * D::NU || (int)fs.w_cent.size() != 36
          || (int)fs.w_forces.size() != D::FS * D::FS || (int)fs.w_frame.size() != D::FS * D::FS || (int)fs.umin.size() != D::NU
          || (int)fs.umax.size() != D::NU || (int)fs.qmin.size() != D::NA || (int)fs.qmax.size() != D::NA)
        throw std::runtime_error("full-dynamics settings: weight / limit sizes do not match the robot");
      if (fs.land_cstr && D::NLAND1 == 0)
        throw std::runtime_error("internal: land_cstr needs the instantiation with land rows");
      if (fs.force_cone && D::NCONE1 == 0)
        throw std::runtime_error("internal: force_cone needs the instantiation with cone rows");
      open_stream();
      force_size = D::FS;
      const int dd[8] = {D::NQ, D::NV, D::NX, D::NDX, D::NU, D::NC, D::NF, H};
      std::copy(dd, dd + 8, dims);
      // ---- model table ----
      std::vector<DevModel<D>> hm(1);
      DevModel<D> & m = hm[0];
      std::memset(&m, 0, sizeof(m));
      fill_tree_model<D>(rm, m);
      m.dt = fs.timestep;
      for (int i = 0; i < 3; i++)
        m.gravity[i] = fs.gravity[i];
      std::copy(fs.w_x.begin(), fs.w_x.end(), m.w_x);
      std::copy(fs.w_u.begin(), fs.w_u.end(), m.w_u);
      m.w_diag = 1;
      for (int i = 0; i < D::NDX; i++)
        for (int j = 0; j < D::NDX; j++)
          if (i != j && m.w_x[i * D::NDX + j] != 0.0)
            m.w_diag = 0;
      for (int i = 0; i < D::NU; i++)
        for (int j = 0; j < D::NU; j++)
          if (i != j && m.w_u[i * D::NU + j] != 0.0)
            m.w_diag = 0;
      if (xcheck_env("SMPC_FORCE_DENSE_WEIGHTS"))
        m.w_diag = 0;
      for (int i = 0; i < D::NDX; i++)
        m.wxd[i] = m.w_x[i * D::NDX + i];
      for (int i = 0; i < D::NU; i++)
        m.wud[i] = m.w_u[i * D::NU + i];
      std::copy(fs.w_cent.begin(), fs.w_cent.end(), m.w_cent);
      std::copy(fs.w_forces.begin(), fs.w_forces.end(), m.w_forces);
      std::copy(fs.w_frame.begin(), fs.w_frame.end(), m.w_frame);
      if constexpr (D::KINO)
      {
        if ((int)fs.w_centder.size() != 36)
          throw std::runtime_error("kinodynamics settings: w_centder must be 6 x 6");
        std::copy(fs.w_centder.begin(), fs.w_centder.end(), m.w_centder);
      }
      std::copy(fs.Kp.begin(), fs.Kp.end(), m.Kp);
      std::copy(fs.Kd.begin(), fs.Kd.end(), m.Kd);
      std::copy(fs.umin.begin(), fs.umin.end(), m.umin);
      std::copy(fs.umax.begin(), fs.umax.end(), m.umax);
      std::copy(fs.qmin.begin(), fs.qmin.end(), m.qmin);
      std::copy(fs.qmax.begin(), fs.qmax.end(), m.qmax);
      m.fric_mu = fs.mu;
      m.Lfoot = fs.Lfoot;
      m.Wfoot = fs.Wfoot;
      m.prox_accuracy = 1e-9; // ProximalSettings(1e-9, 1e-10, 10), src/fulldynamics.cpp:39
      m.prox_mu = 1e-10;
      m.prox_max_iter = 10;
      m.torque_limits = fs.torque_limits;
      m.kinematics_limits = fs.kinematics_limits;
      m.force_cone = fs.force_cone;
      m.mu = ms.mu_init;
      x_model_ref.assign(D::NX, 0.0);
      for (int i = 0; i < D::NQ; i++)
        x_model_ref[i] = rm->q_ref[i];
      x_reference = x_model_ref;
      for (int i = 0; i < D::NX; i++)
        m.x_term[i] = x_model_ref[i];
      m.land_cstr = fs.land_cstr;
      {
        // contact poses of the cycle stages: the feet at the reference state (src/mpc.cpp:162); land_cstr pins the height of a landing 3-D foot to them
        std::vector<double> ft((size_t)D::NF * 6);
        host_foot_positions<D>(m, x_model_ref.data(), ft.data());
        for (int f = 0; f < D::NF; f++)
          m.land_z[f] = ft[f * 6 + 2];
      }
      // ---- buffers ----
      buf.B = B;
      buf.H = H;
      buf.R = R;
      auto dalloc = [&](size_t n) { return (double *)dev_alloc(n * sizeof(double)); };
      const size_t BR = (size_t)B * R, BH = (size_t)B * H;
      buf.xs = dalloc(BR * D::NX);
      buf.us = dalloc(BR * D::NU);
      buf.vs = dalloc(BR * D::NC);
      buf.lams = dalloc(BR * D::NDX);
      buf.vs_e = dalloc(BR * D::NC);
      buf.lams_e = dalloc(BR * D::NDX);
      buf.xs_b = dalloc(BR * D::NX);
      buf.us_b = dalloc(BR * D::NU);
      buf.vs_b = dalloc(BR * D::NC);
      buf.lams_b = dalloc(BR * D::NDX);
      buf.dxs = dalloc((size_t)B * (H + 1) * D::NDX);
      buf.dus = dalloc(BH * D::NU);
      buf.dvs = dalloc(BH * D::NC);
      buf.dlams = dalloc(BH * D::NDX);
      buf.foot_ref = dalloc(BH * D::NF * 3);
      buf.ftraj = dalloc((size_t)B * D::NF * 6);
      buf.vbase = vbase_dev = dalloc((size_t)B * 6);
      buf.vref = dalloc(BR * 6);
      buf.lq = dalloc(BH * D::LQ_STRIDE);
      buf.gains = dalloc(BH * (size_t)D::G_STRIDE);
      buf.QN = dalloc((size_t)B * D::NDX * D::NDX);
      buf.qN = dalloc((size_t)B * D::NDX);
      buf.parts0 = dalloc((size_t)B * (H + 1) * 4);
      buf.partsT = dalloc((size_t)B * D::LS_N * (H + 1) * 2);
      buf.scal = dalloc((size_t)B * SC_N);
      buf.xdotT = dalloc((size_t)B * D::LS_N * 4 * D::NV);
      buf.xdot01 = dalloc((size_t)B * 4 * D::NV);
      buf.nforce = D::NCM;
      buf.forcesT = dalloc(BH * D::LS_N * D::NCM);
      buf.forces = dalloc(BH * D::NCM);
      buf.ls_sel = (int *)dev_alloc((size_t)B * sizeof(int));
      buf.und_list = (int *)dev_alloc((size_t)(B + 1) * sizeof(int));
      buf.stages = (StageShared<D> *)dev_alloc((size_t)H * sizeof(StageShared<D>));
      buf.model = (DevModel<D> *)dev_alloc(sizeof(DevModel<D>));
      X_dev = dalloc((size_t)B * D::NX);
      {
        const char * pe = std::getenv("SMPC_FULL_PARTS");
        int n = pe ? std::atoi(pe) : 1;
        if (n < 1 || n > Base::MAX_PARTS || B < 64 * n)
          n = 1;
        if constexpr (D::WIDE_DEV)
        {
          // one slice per RESIDENT block of fdyn_deriv_body (its grid is persistent: smpc_full_stage.h), per part of the batch: LDS decides how
          // many blocks a CU holds
          n_res = dev_cu_count(device_id) * (int)(160 * 1024 / sizeof(FullScratch<D, true>));
          deriv_wide = (double *)dev_alloc((size_t)n_res * n * sizeof(FullDerivWide<D>));
        }
        this->open_parts(n);
      }
      if (fs.terminal_constraint)
        alloc_terminal_constraint<D>(buf, x_model_ref.data(), host_com_height(m, x_model_ref.data()), stream);
      if (std::getenv("SMPC_PHASE_PROFILE"))
        buf.dbg = dalloc(64);
      h2d(buf.model, hm.data(), sizeof(DevModel<D>), stream);
      stream_sync(stream);
      // ---- default problem (OCPHandler::createProblem, src/ocp-handler.cpp:96-137) ----
      StageShared<D> def;
      std::memset(&def, 0, sizeof(def));
      def.mask = (1u << D::NF) - 1u;
      for (int f = 0; f < D::NF; f++)
      {
        def.f_ref[D::FS * f + 2] = -rm->total_mass * gravity_arg / (double)D::NF;
        if constexpr (D::KINO) // the force references are the head of the control reference (computeControlFromForces, src/kinodynamics.cpp:229-240)
          def.u_ref[D::FS * f + 2] = def.f_ref[D::FS * f + 2];
      }
      for (int i = 0; i < D::NX; i++)
        def.x_tgt[i] = x_model_ref[i];
      horizon.assign(H, def);
      standing = def;
      this->cold_solve(def, m);
      ref_rot.init(H, D::NF);
      ctor_scope.commit();
    }
    ~FullEngine()
    {
      this->free_buffers();
      dev_free(deriv_wide);
    }

    // (a view of a part of the batch: the slices of its blocks lie behind those of the parts before it)
    double * wide_scratch(const Buffers<D> & b) const override
    {
      const long long i0 = (long long)((size_t)(b.xs - buf.xs) / ((size_t)R * D::NX));
      const int part = (int)((i0 * n_parts + B - 1) / B);
      return deriv_wide ? deriv_wide + (size_t)part * n_res * (sizeof(FullDerivWide<D>) / sizeof(double)) : nullptr;
    }
    void launch_deriv(const Buffers<D> & b, int slots = 0)
    {
      StageKernelArgs<D> sk = stage_args(b, slots);
      int grid = (slots > 0 ? slots : b.B) * (H + 1);
      if constexpr (D::WIDE_DEV)
      {
        sk.nwork = grid;
        sk.nres = grid < n_res ? grid : n_res;
        grid = sk.nres;
      }
      timed_launch<StageKernelArgs<D>, fdyn_deriv_body<D>, 64, DERIV_MINW>(slots > 0 ? KID_SELECT : KID_DERIV, grid, sk, slots > 0);
    }
    void launch_sweeps(const Buffers<D> & b)
    {
      if constexpr (D::NCD == 0 && kCrossCheck)
      {
        if (valu_riccati)
        {
          timed_launch<SolverArgs<D>, riccati_full_body<D, 256>, 256>(KID_RICCATI, b.B, solver_args(b)); // cross-check (box rows only)
          timed_launch<SolverArgs<D>, forward_full_body<D>, 64>(KID_FORWARD, b.B, solver_args(b));
          this->launch_term_step(b);
          return;
        }
      }
      timed_launch<SolverArgs<D>, riccati_dense_body<D>, 64, (RiccatiDenseGeom<D>::NT2 > 6 ? 1 : 2)>(KID_RICCATI, b.B, solver_args(b));
      timed_launch<SolverArgs<D>, forward_full_body<D>, 64>(KID_FORWARD, b.B, solver_args(b));
      this->launch_term_step(b);
    }
    void launch_first_trial(const Buffers<D> & b) override
    {
      timed_launch<StageKernelArgs<D>, fdyn_trial_body<D>, 64, TRIAL_MINW>(KID_TRIAL, b.B * (H + 1), stage_args(b, 0, 0, 1));
    }
    // The backtracking candidates alpha = 1/2, 1/4, .. of the instances in und_list, in two batches over the same list: the first LS_FIRST, then --
    // for the instances none of them decided (fdyn_trial_body skips the others) -- the rest.  One batch of all nine cost what a full trial of the
    // batch costs (the biped: 4.4 ms per launch, three launches per control step, with ~ 10 % of the instances backtracking); most of them
    // accept 1/2 or 1/4.  Same decisions: select_body takes the first candidate that passes, in order.
    static constexpr int LS_FIRST = 2;
    void launch_backtracking_trials(const Buffers<D> & b, int slots) override
    {
      for (int j0 = 1; j0 < D::LS_N; j0 += (j0 == 1 ? LS_FIRST : D::LS_N))
      {
        const int nj = j0 == 1 ? (LS_FIRST < D::LS_N - 1 ? LS_FIRST : D::LS_N - 1) : D::LS_N - j0;
        timed_launch<StageKernelArgs<D>, fdyn_trial_body<D>, 64, TRIAL_MINW>(KID_SELECT, slots * (H + 1), stage_args(b, slots, j0, nj), true);
        this->launch_select(b, j0, nj);
      }
    }
    size_t gains_stride() const override { return D::G_STRIDE; }
    void set_force_ref(StageShared<D> & s, int foot, double fz) const override
    {
      s.f_ref[D::FS * foot + 2] = fz;
      if constexpr (D::KINO) // the force references are the head of the control reference (computeControlFromForces, src/kinodynamics.cpp:229-240)
        s.u_ref[D::FS * foot + 2] = fz;
    }
    // (per-launch event timings mean nothing once launches overlap: one part while profiling)
    bool parts_enabled() const override { return n_parts > 1 && buf.CN == nullptr && !profiling; }
    void issue_parts(const Buffers<D> * part, int k) override // part after part
    {
      for (int i = 0; i < n_parts; i++)
      {
        this->begin_part(part[i], i);
        this->run_iterations(part[i], k);
      }
    }
    void launch_interp(int knots, double delay, double * x, double * acc, double * f, double * u) override
    {
      FullInterpArgs<D> ia;
      ia.b = buf;
      ia.head = head;
      ia.knots = knots;
      ia.delay = delay;
      ia.timestep = ms.timestep;
      ia.x_out = x;
      ia.acc_out = acc;
      ia.f_out = f;
      ia.u_out = u;
      launch<FullInterpArgs<D>, full_interp_body<D>, 64>(B, stream, ia);
    }
    void launch_gains_out(int nt, double * out) override
    {
      FullGainOutArgs<D> ga;
      ga.b = buf;
      ga.nt = nt;
      ga.out = out;
      launch<FullGainOutArgs<D>, full_gains_out_body<D>, 64>(B * nt, stream, ga);
    }
    void launch_frontend(const FrontendArgs<D> & fa) override { launch<FrontendArgs<D>, frontend_full_body<D>, 64, 1, 1>(B, stream, fa); }
    void require_forward_dynamics(const char * who) const override
    {
      if constexpr (D::KINO)
        throw std::runtime_error(std::string(who) + ": the kinodynamics variant has no constrained forward dynamics (use a full-dynamics handle)");
    }
    void launch_forward_dynamics(int n, const double * X, const double * tau, const unsigned * mask, const double * Kp, const double * Kd, double prox_accuracy,
                                 double prox_mu, int prox_max_iter, double * a, double * lam, int * iters) override
    {
      if constexpr (!D::KINO)
      {
        FdynFdArgs<D> fa;
        fa.b = buf;
        fa.X = X;
        fa.tau = tau;
        fa.mask = mask;
        for (int i = 0; i < 6; i++)
        {
          fa.Kp[i] = (Kp && i < D::FS) ? Kp[i] : 0.0;
          fa.Kd[i] = (Kd && i < D::FS) ? Kd[i] : 0.0;
        }
        fa.prox_accuracy = prox_accuracy;
        fa.prox_mu = prox_mu;
        fa.prox_max_iter = prox_max_iter;
        fa.a_out = a;
        fa.lam_out = lam;
        fa.iters_out = iters;
        launch<FdynFdArgs<D>, fdyn_fd_body<D>, 64, 1, 1>(n, stream, fa);
      }
    }
    void launch_sim_integrate(const SimStepArgs<D> & sa) override
    {
      if constexpr (!D::KINO)
        launch<SimStepArgs<D>, sim_integrate_body<D>, 64, 1, 1>(B, stream, sa);
    }
    void state_derivatives(double * out) override
    {
      set_device(device_id);
      XdotArgs<Buffers<D>> a;
      a.b = buf;
      a.head = head;
      a.out = out;
      launch<XdotArgs<Buffers<D>>, xdot_all_body<D, Buffers<D>, XD_FULL>, 64>(xdot_grid(XD_FULL, B, H), stream, a);
    }
    // what: 0 = control target (nu), 1 = state target (nx), 2 = contact-force references (force_size * nfeet)
    void set_stage_reference(int t, int what, const double * v, int n) override
    {
      if (what != 2)
      {
        Base::set_stage_reference(t, what, v, n);
        if constexpr (D::KINO) // getReferenceForce is a segment of the reference control (src/kinodynamics.cpp:258-265): keep the mirror in step
          if (what == 0)
            std::copy(v, v + D::NCM, horizon[t].f_ref);
        return;
      }
      check_stage(t);
      if (n != D::NCM)
        throw std::runtime_error("Reference forces do not have the right dimension");
      std::copy(v, v + n, horizon[t].f_ref);
      if constexpr (D::KINO)
        std::copy(v, v + n, horizon[t].u_ref);
    }
    void get_stage_reference(int t, int what, double * v, int n) override
    {
      if (what != 2 || n != D::NCM)
        return Base::get_stage_reference(t, what, v, n);
      check_stage(t);
      std::copy(horizon[t].f_ref, horizon[t].f_ref + n, v);
    }
    int lq_size() const override { return D::LQ_STRIDE; }
    void debug_lq(int inst, int t, double * out) override
    {
      if (inst < 0 || inst >= B || t < 0 || t >= H)
        throw std::runtime_error("Stage index exceeds stage vector size");
      get_linear(buf.lq + ((size_t)inst * H + t) * D::LQ_STRIDE, D::LQ_STRIDE, out);
      // the derivative pass writes the upper 16 x 16 tiles of Q and R only (readers take the upper triangle): mirror here
      for (int i = 0; i < D::NDX; i++)
        for (int j = 0; j < i; j++)
          out[D::O_Q + i * D::NDX + j] = out[D::O_Q + j * D::NDX + i];
      for (int i = 0; i < D::NU; i++)
        for (int j = 0; j < i; j++)
          out[D::O_R + i * D::NU + j] = out[D::O_R + j * D::NU + i];
    }
  };
} // namespace smpc
