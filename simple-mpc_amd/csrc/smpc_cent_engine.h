// smpc_cent_engine.h -- host side of the batched centroidal MPC: the reference's MPC class (smpc_stage_engine.h cites it line
// by line; the stage that enters the horizon is MpcEngineBase::recede_horizon for all three engines) over a CentroidalOCP
// (reference src/centroidal-dynamics.cpp).  One control step = two launches:
//   frontend_body   measured multibody states -> getCentroidalState + foot positions (src/mpc.cpp:192,200)
//   cent_step_body  recede + references + k ProxDDP iterations, one wavefront per instance (smpc_cent_kernels.h)
// What differs from the kinodynamics host logic:
//   - the problem state is RobotDataHandler::getCentroidalState() of the measured multibody state
//     (src/mpc.cpp:200, src/centroidal-dynamics.cpp:261-264, src/robot-handler.cpp:142-149)
//   - setReferencePose writes the contact POSITION of the stage's contact map (src/centroidal-dynamics.cpp:151-169)
//   - setReferenceState = setPoseBase + setVelocityBase, and setVelocityBase stores momentum references m v
//     (src/centroidal-dynamics.cpp:227-239, 286-291)
//   - x_reference_ starts as getReferenceState(0) of the default problem = 0 (src/centroidal-dynamics.cpp:36)
//   - the default problem has identity contact poses, i.e. contact positions at the origin (src/ocp-handler.cpp:117)
//   - no terminal constraint (src/centroidal-dynamics.cpp:318-337)
#pragma once
#include "smpc_cent6_kernels.h"
#include "smpc_cent_split.h"
#include "smpc_engine.h"
#include "smpc_frontend_rt.h"

namespace smpc
{
  struct HostCentSettings // include/simple-mpc/centroidal-dynamics.hpp:27-43
  {
    double timestep;
    std::vector<double> w_u, w_com, w_linear_mom, w_angular_mom, w_linear_acc, w_angular_acc;
    double gravity[3];
    double mu;
    double Lfoot = 0.1, Wfoot = 0.075; // sole half-length / half-width (wrench cones of 6-D feet)
    int force_size = 3;
  };

  enum CentKernelId
  {
    CKID_FRONTEND = 0,
    CKID_STEP,    // recede (point feet with SMPC_CENT_FUSED=1: the one-kernel control step)
    CKID_DERIV,   // point feet (smpc_cent_split.h): lane-per-stage pre-pass ; 6-D feet (smpc_cent6_kernels.h): stage evaluation + derivatives + knot
    CKID_RICCATI, //   backward sweep
    CKID_FORWARD, //   forward sweep
    CKID_LS,      //   line search + step
    CKID_TRIAL,   //   6-D feet: stage merits of the line-search candidates (cent6_trial_body)
    CKID_N
  };
  static_assert(CKID_N <= KID_N, "the kernel-time slots of MpcEngineBase hold every centroidal kernel");

  template <class DK>
  struct cent_is_full_dims
  {
    static constexpr bool value = false;
  };
  template <int NJ_, int NF_, int FS_, int CN_, int LN_, int KIN_>
  struct cent_is_full_dims<FullDims<NJ_, NF_, FS_, CN_, LN_, KIN_>>
  {
    static constexpr bool value = true;
  };
  // what the engine keeps for its state front end: the device model of a compile-time stage-kernel family, or nothing for the run-time
  // joint tree (RtDims: the table is CentEngine::rt_model, nq / nv are members)
  template <class DK>
  struct CentFront
  {
    static constexpr bool RT = false;
    static constexpr int NJ = DK::NJ;
    typedef Buffers<DK> Model; // only .model is used
    typedef DevModel<DK> HostModel;
  };
  template <>
  struct CentFront<RtDims>
  {
    static constexpr bool RT = true;
    static constexpr int NJ = 0;
    struct Model
    {
      void * model = nullptr;
    };
    typedef RtDevModel HostModel;
  };
  // buffers of the dense path (6-D feet); empty for point feet
  template <class DC, int FS>
  struct Cent6Extra
  {
  };
  template <class DC>
  struct Cent6Extra<DC, 6>
  {
    Buffers<typename DC::DD> sb;
    double *parts0 = nullptr, *partsT = nullptr, *xdotT = nullptr; // (Cent6Args, smpc_cent6_kernels.h)
  };

  // DK: Dims of the multibody robot (front-end FK; a FullDims selects the front end of the dense stage kernels; RtDims: the front end on the
  // run-time joint tree, smpc_frontend_rt.h -- any robot table with DC's feet), DC: CentDims
  template <class DK, class DC>
  class CentEngine : public MpcEngineBase
  {
  public:
    CentBuffers<DC> buf;
    Cent6Extra<DC, DC::FS> x6; // 6-D feet: knots, dense gains, terminal node, merit partials
    CentSplitBuffers sbuf;     // point feet: hand-over records of the kernel pipeline (smpc_cent_split.h)
    bool fused = false;        // point feet: SMPC_CENT_FUSED=1 runs the one-kernel control step (cross-check)
    // point feet: the batch runs as `nparts` contiguous parts, each on its own stream (SMPC_CENT_PARTS; instances are independent): the
    // backward sweep is bound by VALU / matrix-core issue, the pre-pass, forward sweep and line search by memory -- launches of different
    // parts fill each other's idle units.  Part p > 0 starts one kernel late (it waits for part p - 1's first pre-pass), so that the parts do
    // not march in step.
    int nparts = 1;
    int ls_passes = 1;      // 6-D feet: SMPC_CENT6_LS_PASSES=2 evaluates the full step first, the backtracking candidates where it failed
    bool ls_direct = false; // SMPC_CENT_LS=direct: the per-candidate re-evaluation (cent_ls_body) also for horizons the polynomial form covers
    std::vector<stream_t> part_stream; // [nparts - 1] (part 0 runs on `stream`)
    std::vector<event_t> part_event;   // [nparts - 1] completion of a part, [nparts] stagger events
    event_t ev_fork{};
    static constexpr bool RT = CentFront<DK>::RT;
    typename CentFront<DK>::Model fk; // only .model is used (front-end kernel)
    RtDevModel * rt_model = nullptr;  // the robot table of frontend_rt_body: the front end of an RtDims engine; on the others allocated by the first debug_frontend_rt
    smpc_robot_model robot;           // (host copy: the source of rt_model)
    int nq_mb = 0, nv_mb = 0, nx_mb = 0; // sizes of the measured multibody state
    std::vector<CentStage<DC>> horizon, cycle;
    CentStage<DC> standing;
    double com_ref_member[3] = {0, 0, 0}; // CentroidalOCP::com_ref_ (last setPoseBase)
    double mass;
    UploadRing stage_ring; // pinned staging of the per-step stage table
    double *X_dev = nullptr, *cstate_dev = nullptr, *feet_dev = nullptr;
    static constexpr double ARMIJO_C1 = 1e-4, REG_INIT = 1e-9, REG_MIN = 1e-10, REG_MAX = 1e9, REG_INC = 10.0, REG_DEC = 1.0 / 3.0, STALL_REL = 1e-9;

    CentEngine(const smpc_robot_model * rm, const HostCentSettings & cs, const HostMpcSettings & ms_, int batch, double gravity_arg, int device)
    : MpcEngineBase(ms_, batch, device)
    {
      AllocScope ctor_scope; // (a throw below releases what was allocated so far: smpc_alloc_scope.h)
      if (batch <= 0)
        throw std::runtime_error("batch must be positive");
      if (cs.force_size != DC::FS)
        throw std::runtime_error("force size in settings does not match reference force size");
      if (rm->nfeet != DC::NF || (!RT && rm->njoints != CentFront<DK>::NJ))
        throw std::runtime_error("robot shape (njoints, nfeet) does not match this kernel instantiation");
      if ((int)cs.w_u.size() != DC::NU * DC::NU || cs.w_com.size() != 9 || cs.w_linear_mom.size() != 9 || cs.w_angular_mom.size() != 9
          || cs.w_linear_acc.size() != 9 || cs.w_angular_acc.size() != 9)
        throw std::runtime_error("centroidal settings: weight sizes do not match the robot");
      if (ms.T < 2)
        throw std::runtime_error("horizon must have at least 2 stages");
      if (DC::FS == 6 && ms.T + 1 > 256) // (before anything is allocated: a constructor that throws runs no destructor)
        throw std::runtime_error("centroidal OCP with 6-D feet: at most 255 stages");
      open_stream();
      force_size = DC::FS;
      robot = *rm;
      nq_mb = rm->njoints + 6;
      nv_mb = rm->njoints + 5;
      nx_mb = nq_mb + nv_mb;
      const int dd[8] = {nq_mb, nv_mb, 9, 9, DC::NU, DC::NC, DC::NF, H}; // nq, nv of the robot; the problem state is [com; h_lin; h_ang]
      std::copy(dd, dd + 8, dims);
      x_reference.assign(9, 0.0);
      mass = rm->total_mass;
      // ---- models ----
      std::vector<typename CentFront<DK>::HostModel> hk(1);
      if constexpr (RT)
      {
        fill_rt_model(rm, hk[0]);
        rt_model = (RtDevModel *)dev_alloc(sizeof(RtDevModel));
        h2d(rt_model, hk.data(), sizeof(RtDevModel), stream);
      }
      else
      {
        std::memset(&hk[0], 0, sizeof(DevModel<DK>));
        fill_tree_model<DK>(rm, hk[0]);
        fk.model = (DevModel<DK> *)dev_alloc(sizeof(DevModel<DK>));
        h2d(fk.model, hk.data(), sizeof(DevModel<DK>), stream);
      }
      std::vector<CentDevModel<DC>> hc(1);
      CentDevModel<DC> & m = hc[0];
      std::memset(&m, 0, sizeof(m));
      m.mass = mass;
      m.dt = cs.timestep;
      m.mu = ms.mu_init;
      m.mu_fric = cs.mu;
      m.cone_eps = 1e-4; // src/centroidal-dynamics.cpp:96
      m.Lfoot = cs.Lfoot;
      m.Wfoot = cs.Wfoot;
      for (int i = 0; i < 3; i++)
        m.gravity[i] = cs.gravity[i];
      std::copy(cs.w_com.begin(), cs.w_com.end(), m.w_com);
      std::copy(cs.w_linear_mom.begin(), cs.w_linear_mom.end(), m.w_lm);
      std::copy(cs.w_angular_mom.begin(), cs.w_angular_mom.end(), m.w_am);
      std::copy(cs.w_linear_acc.begin(), cs.w_linear_acc.end(), m.w_la);
      std::copy(cs.w_angular_acc.begin(), cs.w_angular_acc.end(), m.w_aa);
      std::copy(cs.w_u.begin(), cs.w_u.end(), m.w_u);
      for (int f = 0; f < DC::NF; f++)
        for (int i = 0; i < 3; i++)
          m.foot_ref_p[f][i] = rm->foot_ref_p[f][i];
      // ---- buffers ----
      buf.B = B;
      buf.H = H;
      buf.R = R;
      auto dalloc = [&](size_t n) { return (double *)dev_alloc(n * sizeof(double)); };
      const size_t BR = (size_t)B * R, BH = (size_t)B * H;
      buf.xs = dalloc(BR * 9);
      buf.us = dalloc(BR * DC::NU);
      buf.vs = dalloc(BR * DC::NC);
      buf.lams = dalloc(BR * 9);
      buf.vs_e = dalloc(BR * DC::NC);
      buf.lams_e = dalloc(BR * 9);
      buf.dxs = dalloc((size_t)B * (H + 1) * 9);
      // (steps: [B][H][.] linear in t for the one-kernel / 6-D paths; the kernel pipeline of point feet keeps them on the iterate's ring slots, [B][R][.])
      buf.dus = dalloc(BR * DC::NU);
      buf.dvs = dalloc(BR * DC::NC);
      buf.dlams = dalloc(BR * 9);
      buf.foot = dalloc(BH * DC::NF * 3);
      buf.ftraj = dalloc((size_t)B * DC::NF * 6);
      buf.vbase = vbase_dev = dalloc((size_t)B * 6);
      buf.vref = dalloc(BR * 6);
      buf.gains = dalloc(BH * DC::G_STRIDE);
      if constexpr (DC::FS == 6)
      {
        typedef typename DC::DD DD;
        x6.sb.B = B;
        x6.sb.H = H;
        x6.sb.R = R;
        x6.sb.lq = dalloc(BH * DD::LQ_STRIDE);
        x6.sb.gains = buf.gains; // (the dense gains block: [K | k] rows at G_K with stride GKS, read by the interpolation / gain read-out kernels)
        x6.sb.QN = dalloc((size_t)B * DD::NDX * DD::NDX);
        x6.sb.qN = dalloc((size_t)B * DD::NDX);
        x6.sb.model = (DevModel<DD> *)dev_alloc(sizeof(DevModel<DD>));
        DevModel<DD> hm;
        hm.mu = ms.mu_init;
        h2d(x6.sb.model, &hm, sizeof(hm), stream);
        stream_sync(stream);
        x6.parts0 = dalloc((size_t)B * (H + 1) * 4);
        x6.partsT = dalloc((size_t)B * DC::LS_N * (H + 1) * 2);
        x6.xdotT = dalloc((size_t)B * DC::LS_N * 18);
        ls_passes = (xcheck_env("SMPC_CENT6_LS_PASSES") && xcheck_env("SMPC_CENT6_LS_PASSES")[0] == '2' && DC::LS_N > 1) ? 2 : 1;
      }
      if constexpr (DC::FS == 3)
      {
        fused = xcheck_env("SMPC_CENT_FUSED") != nullptr && xcheck_env("SMPC_CENT_FUSED")[0] == '1';
        if (!fused)
        {
          if (BH * CentRec<DC>::STRIDE >= ((size_t)1 << 32))
            throw std::runtime_error("centroidal OCP: batch x horizon too large for the 32-bit record offsets");
          sbuf.rec = dalloc(BH * CentRec<DC>::STRIDE);
          sbuf.term = dalloc((size_t)B * CentRec<DC>::T_STRIDE);
          const char * le = xcheck_env("SMPC_CENT_LS");
          ls_direct = le != nullptr && le[0] == 'd';
          const char * pe = std::getenv("SMPC_CENT_PARTS");
          nparts = pe ? std::atoi(pe) : (B >= 1024 ? 2 : 1);
          if (nparts < 1 || nparts > 8 || B < 64 * nparts)
            nparts = 1;
          ev_fork = side.event();
          for (int p = 1; p < nparts; p++)
            part_stream.push_back(side.stream());
          for (int p = 0; p < 2 * nparts; p++)
            part_event.push_back(side.event());
        }
      }
      buf.scal = dalloc((size_t)B * SC_N);
      buf.xdot01 = dalloc((size_t)B * 18);
      buf.zeros = dalloc(64);
      if (std::getenv("SMPC_PHASE_PROFILE"))
        buf.dbg = dalloc(64);
      buf.stages = (CentStage<DC> *)dev_alloc((size_t)H * sizeof(CentStage<DC>));
      buf.model = (CentDevModel<DC> *)dev_alloc(sizeof(CentDevModel<DC>));
      X_dev = dalloc((size_t)B * nx_mb);
      cstate_dev = dalloc((size_t)B * 9);
      feet_dev = dalloc((size_t)B * DC::NF * 3);
      h2d(buf.model, hc.data(), sizeof(CentDevModel<DC>), stream);
      stream_sync(stream);
      x_model_ref.assign(nx_mb, 0.0);
      for (int i = 0; i < nq_mb; i++)
        x_model_ref[i] = rm->q_ref[i];

      // ---- default problem (OCPHandler::createProblem, src/ocp-handler.cpp:96-137): all feet in contact, identity
      //      contact poses, zero references ----
      CentStage<DC> def;
      std::memset(&def, 0, sizeof(def));
      def.mask = (1u << DC::NF) - 1u;
      for (int f = 0; f < DC::NF; f++)
        def.u_ref[DC::FS * f + 2] = -mass * gravity_arg / (double)DC::NF;
      horizon.assign(H, def);
      standing = def;
      cold_solve(def);
      ref_rot.init(H, DC::NF);
      ctor_scope.commit();
    }
    ~CentEngine()
    {
      for (double * p : {buf.xs, buf.us, buf.vs, buf.lams, buf.vs_e, buf.lams_e, buf.dxs, buf.dus, buf.dvs, buf.dlams, buf.foot, buf.ftraj, buf.vbase, buf.vref, buf.gains, buf.scal, buf.xdot01,
                         buf.zeros, buf.dbg, X_dev, cstate_dev, feet_dev, sbuf.rec, sbuf.term})
        dev_free(p);
      if constexpr (DC::FS == 6)
      {
        for (double * p : {x6.sb.lq, x6.sb.QN, x6.sb.qN, x6.parts0, x6.partsT, x6.xdotT})
          dev_free(p);
        dev_free(x6.sb.model);
      }
      dev_free(buf.stages);
      dev_free(buf.model);
      dev_free(fk.model);
      dev_free(rt_model);
      dev_free(cold.dev);
    }

    void upload_stages()
    {
      stage_ring.upload(buf.stages, horizon.data(), (size_t)H * sizeof(CentStage<DC>), stream);
    }
    void launch_frontend(const double * Xd, bool aux = false, int inst0 = 0, int count = -1, const stream_t * on = nullptr)
    {
      if (count < 0)
        count = B;
      if constexpr (RT)
      {
        FrontendRtArgs fa;
        fa.model = rt_model;
        fa.X = Xd + (size_t)inst0 * nx_mb;
        fa.feet = feet_dev + (size_t)inst0 * DC::NF * 3;
        fa.com = nullptr;
        fa.hg = nullptr;
        fa.cstate = cstate_dev + (size_t)inst0 * 9;
        timed_launch<FrontendRtArgs, frontend_rt_body, 64>(CKID_FRONTEND, count, fa, aux, on);
      }
      else
      {
        FrontendArgs<DK> fa;
        fa.b = fk;
        fa.X = Xd + (size_t)inst0 * nx_mb;
        fa.feet = feet_dev + (size_t)inst0 * DC::NF * 3;
        fa.com = nullptr;
        fa.hg = nullptr;
        fa.cstate = cstate_dev + (size_t)inst0 * 9;
        if constexpr (cent_is_full_dims<DK>::value)
          timed_launch<FrontendArgs<DK>, frontend_full_body<DK>, 64>(CKID_FRONTEND, count, fa, aux, on);
        else
          timed_launch<FrontendArgs<DK>, frontend_body<DK>, 64>(CKID_FRONTEND, count, fa, aux, on);
      }
    }
    // first instance / instance count of part p (whole wavefront groups of 64)
    void part_range(int p, int np, int & i0, int & n) const
    {
      const int per = ((B + np - 1) / np + 63) / 64 * 64;
      i0 = p * per < B ? p * per : B;
      n = i0 + per <= B ? per : B - i0;
    }
    // the kernel pipeline of one part of the batch, on stream `on` (null: the engine's stream); with_frontend: the state front end of the part first
    void launch_split_part(const CentStepArgs<DC> & a, bool aux, int inst0, int count, const stream_t * on, const double * Xfront, event_t * after_first_pre, const event_t * wait_before_pre)
    {
      if (count <= 0)
        return;
      if (Xfront)
        launch_frontend(Xfront, aux, inst0, count, on);
      CentSplitArgs<DC> c;
      c.a = a;
      c.sb = sbuf;
      c.last = 0;
      c.inst0 = inst0;
      timed_launch<CentSplitArgs<DC>, cent_recede_body<DC>, 64>(CKID_STEP, count, c, aux, on);
      if (wait_before_pre)
        stream_wait_event(on ? *on : stream, *wait_before_pre);
      for (int it = 0; it < a.iters; it++)
      {
        c.last = it + 1 == a.iters ? 1 : 0;
        timed_launch<CentSplitArgs<DC>, cent_pre_body<DC>, 64, 2>(CKID_DERIV, count, c, aux, on);
        if (it == 0 && after_first_pre)
          event_record(*after_first_pre, on ? *on : stream);
        if (buf.dbg != nullptr)
          timed_launch<CentSplitArgs<DC>, cent_bwd_body<DC, true>, 64, 4>(CKID_RICCATI, count, c, aux, on);
        else
          timed_launch<CentSplitArgs<DC>, cent_bwd_body<DC, false>, 64, 4>(CKID_RICCATI, count, c, aux, on);
        timed_launch<CentSplitArgs<DC>, cent_fwd_body<DC>, 64, 4>(CKID_FORWARD, count, c, aux, on);
        // (line search: the polynomial form needs one lane per stage and the terminal node; longer horizons re-evaluate per candidate)
        if (H + 1 <= 64 && !ls_direct)
          timed_launch<CentSplitArgs<DC>, cent_ls_poly_body<DC>, 64, 2>(CKID_LS, count, c, aux, on);
        else
          timed_launch<CentSplitArgs<DC>, cent_ls_body<DC>, 64, 1>(CKID_LS, count, c, aux, on);
      }
    }
    // one solver run of `a.iters` iterations (with the recede / centre bookkeeping the flags of `a` ask for)
    void launch_step(const CentStepArgs<DC> & a, bool aux = false)
    {
      if constexpr (DC::FS == 6)
      {
        Cent6Args<DC> c;
        c.b = buf;
        c.sb = x6.sb;
        c.parts0 = x6.parts0;
        c.partsT = x6.partsT;
        c.xdotT = x6.xdotT;
        c.head = a.head;
        c.shift = a.shift;
        c.set_centres = a.set_centres;
        c.reset_preg = a.reset_preg;
        c.X = a.X;
        c.nx_mb = a.nx_mb;
        c.cstate = a.cstate;
        c.feet = a.feet;
        for (int f = 0; f < DC::NF; f++)
          c.land[f] = a.land[f];
        c.T_fly = a.T_fly;
        c.T_contact = a.T_contact;
        c.swing_apex = a.swing_apex;
        c.timestep = a.timestep;
        c.armijo_c1 = a.armijo_c1;
        c.reg_init = a.reg_init;
        c.reg_min = a.reg_min;
        c.reg_max = a.reg_max;
        c.reg_inc = a.reg_inc;
        c.reg_dec = a.reg_dec;
        typedef typename DC::DD DD;
        SolverArgs<DD> sa;
        sa.b = x6.sb;
        sa.head = a.head;
        sa.j0 = 0;
        sa.nj = 0;
        sa.armijo_c1 = a.armijo_c1;
        sa.reg_min = a.reg_min;
        sa.reg_max = a.reg_max;
        sa.reg_inc = a.reg_inc;
        sa.reg_dec = a.reg_dec;
        timed_launch<Cent6Args<DC>, cent6_recede_body<DC>, 64>(CKID_STEP, B, c, aux);
        for (int it = 0; it < a.iters; it++)
        {
          timed_launch<Cent6Args<DC>, cent6_deriv_body<DC>, 64>(CKID_DERIV, B * (H + 1), c, aux);
          timed_launch<SolverArgs<DD>, riccati_dense_body<DD>, 64, 2>(CKID_RICCATI, B, sa, aux);
          timed_launch<Cent6Args<DC>, cent6_forward_body<DC>, 64>(CKID_FORWARD, B, c, aux);
          // line search: every candidate in one pair of launches -- a launch of B (H + 1) one-wave blocks costs 0.3 ms whatever it evaluates (measured:
          // the full step alone 0.30 ms, the nine backtracking candidates 0.32 ms), so the split `full step first, the rest where it failed'
          // (SMPC_CENT6_LS_PASSES=2; the kernels take any candidate range) only pays when no instance backtracks
          for (int pass = 0; pass < ls_passes; pass++)
          {
            c.j0 = pass;
            c.nj = ls_passes == 1 ? DC::LS_N : (pass == 0 ? 1 : DC::LS_N - 1);
            timed_launch<Cent6Args<DC>, cent6_trial_body<DC>, 64>(CKID_TRIAL, B * (H + 1), c, aux);
            timed_launch<Cent6Args<DC>, cent6_ls_body<DC>, 64>(CKID_LS, B, c, aux);
          }
        }
      }
      else if (fused)
      {
        if constexpr (kCrossCheck) // (the one-kernel form: SMPC_CENT_FUSED=1 of a cross-check build)
          timed_launch<CentStepArgs<DC>, cent_step_body<DC>, 64, 2>(CKID_STEP, B, a, aux);
      }
      else
        launch_split_part(a, aux, 0, B, nullptr, nullptr, nullptr, nullptr);
    }
    CentStepArgs<DC> step_args(const double * Xd) const
    {
      CentStepArgs<DC> a;
      a.b = buf;
      a.head = head;
      a.shift = 0;
      a.set_centres = 0;
      a.reset_preg = 0;
      a.iters = 1;
      a.X = Xd;
      a.nx_mb = nx_mb;
      a.cstate = cstate_dev;
      a.feet = feet_dev;
      for (int f = 0; f < DC::NF; f++)
        a.land[f] = -1;
      a.T_fly = ms.T_fly;
      a.T_contact = ms.T_contact;
      a.swing_apex = ms.swing_apex;
      a.timestep = ms.timestep;
      a.armijo_c1 = ARMIJO_C1;
      a.reg_init = REG_INIT;
      a.reg_min = REG_MIN;
      a.reg_max = REG_MAX;
      a.reg_inc = REG_INC;
      a.reg_dec = REG_DEC;
      return a;
    }

    // MPC constructor (src/mpc.cpp:62-91): every instance starts from the solution of the default problem at the
    // reference state.  All B wavefronts run the same cold solve (it is identical work, and cheaper than a broadcast).
    void cold_solve(const CentStage<DC> & def)
    {
      std::vector<double> X((size_t)B * nx_mb);
      for (int b = 0; b < B; b++)
        std::copy(x_model_ref.begin(), x_model_ref.end(), X.begin() + (size_t)b * nx_mb);
      h2d(X_dev, X.data(), X.size() * sizeof(double), stream);
      launch_frontend(X_dev, true);
      std::vector<double> cst((size_t)B * 9), feet((size_t)B * DC::NF * 3);
      d2h(cst.data(), cstate_dev, cst.size() * sizeof(double), stream);
      d2h(feet.data(), feet_dev, feet.size() * sizeof(double), stream);
      stream_sync(stream);
      std::vector<double> xs((size_t)B * R * 9), us((size_t)B * R * DC::NU), ft((size_t)B * DC::NF * 6);
      for (int b = 0; b < B; b++)
      {
        for (int t = 0; t < R; t++)
        {
          std::copy(cst.begin() + (size_t)b * 9, cst.begin() + (size_t)(b + 1) * 9, xs.begin() + ((size_t)b * R + t) * 9);
          std::copy(def.u_ref, def.u_ref + DC::NU, us.begin() + ((size_t)b * R + t) * DC::NU);
        }
        for (int f = 0; f < DC::NF; f++)
          for (int i = 0; i < 3; i++)
            ft[((size_t)b * DC::NF + f) * 6 + i] = ft[((size_t)b * DC::NF + f) * 6 + 3 + i] = feet[((size_t)b * DC::NF + f) * 3 + i];
      }
      h2d(buf.xs, xs.data(), xs.size() * sizeof(double), stream);
      h2d(buf.us, us.data(), us.size() * sizeof(double), stream);
      h2d(buf.ftraj, ft.data(), ft.size() * sizeof(double), stream);
      upload_stages();
      stream_sync(stream);
      bool centres = true;
      std::vector<double> sc(SC_N);
      for (int it = 0; it < 100; it++)
      {
        CentStepArgs<DC> a = step_args(X_dev);
        a.set_centres = centres ? 1 : 0;
        a.reset_preg = it == 0 ? 1 : 0;
        launch_step(a, true);
        d2h(sc.data(), buf.scal, SC_N * sizeof(double), stream);
        stream_sync(stream);
        cold_iters = it + 1;
        cold_trace.insert(cold_trace.end(), {sc[SC_PHI0], sc[SC_PRIM], sc[SC_DUAL], sc[SC_ALPHA]});
        centres = false;
        if (std::fmax(sc[SC_PRIM], sc[SC_DUAL]) <= ms.TOL)
          break;
        if (std::fabs(sc[SC_DPHI0]) <= STALL_REL * std::fmax(1.0, std::fabs(sc[SC_PHI0])))
          break;
        if (sc[SC_DUAL] <= ms.TOL)
          centres = true;
      }
      for (int i = 0; i < CKID_N; i++)
        kernel_calls[i] = 0;
      // instance 0 as the cold solve left it, kept for reset_instances_device (every instance holds the same; DESIGN.md "Resetting single
      // instances" classifies every buffer)
      cold.begin(B, H, R, (size_t)R * (2 * 9 + DC::NU + 2 * DC::NC + 9) + SC_N + 18 + DC::NF * 6);
      cold.retain(buf.xs, 9, RESET_RING, stream);
      cold.retain(buf.us, DC::NU, RESET_RING, stream);
      cold.retain(buf.vs, DC::NC, RESET_RING, stream);
      cold.retain(buf.lams, 9, RESET_RING, stream);
      cold.retain(buf.vs_e, DC::NC, RESET_RING, stream);
      cold.retain(buf.lams_e, 9, RESET_RING, stream);
      cold.retain(buf.scal, SC_N, RESET_INST, stream);
      cold.retain(buf.xdot01, 18, RESET_INST, stream);
      cold.retain(buf.ftraj, DC::NF * 6, RESET_INST, stream);
      stream_sync(stream);
    }
    void reset_instances_device(const uint8_t * mask_dev) override { launch_reset(mask_dev); }

    void generate_cycle_horizon(const unsigned char * cs, int n) override
    {
      if (n <= 0)
        throw std::runtime_error("contact sequence must not be empty");
      timer.generate(cs, n, DC::NF, H);
      cycle.clear();
      for (auto & st : timer.states)
      {
        int active = 0;
        for (int f = 0; f < DC::NF; f++)
          active += st[f] ? 1 : 0;
        CentStage<DC> s;
        std::memset(&s, 0, sizeof(s));
        for (int f = 0; f < DC::NF; f++)
          if (st[f])
          {
            s.mask |= 1u << f;
            s.u_ref[DC::FS * f + 2] = ms.support_force / (double)active;
          }
        for (int i = 0; i < 3; i++)
          s.x_tgt[i] = com_ref_member[i];
        cycle.push_back(s);
      }
    }
    void iterate_device(const double * Xd) override
    {
      ref_rot.reset(); // (every control step rewrites every stage's reference pose with the identity rotation: src/mpc.cpp:303-309)
      if (cycle.empty())
        throw std::runtime_error("generateCycleHorizon must be called before iterate");
      recede_horizon(horizon, cycle, standing, DC::NF);
      // setReferenceState(H-1, x_reference_) ; setVelocityBase(H-1, velocity_base_): momentum references are m v
      for (int i = 0; i < 3; i++)
      {
        horizon[H - 1].x_tgt[i] = x_reference[i];
        com_ref_member[i] = x_reference[i];
        horizon[H - 1].x_tgt[3 + i] = mass * velocity_base[i];
        horizon[H - 1].x_tgt[6 + i] = mass * velocity_base[3 + i];
      }
      upload_stages();
      head = head + 1 == R ? 0 : head + 1;
      CentStepArgs<DC> a = step_args(Xd);
      a.shift = 1;
      a.set_centres = 1;
      a.reset_preg = 1;
      a.iters = ms.max_iters;
      for (int f = 0; f < DC::NF; f++)
        a.land[f] = timer.land[f].empty() ? -1 : timer.land[f][0];
      if constexpr (DC::FS == 3)
      {
        if (!fused && nparts > 1 && !profiling) // (per-kernel event times mean something only when launches do not overlap: one part while profiling)
        {
          // fork: every part's stream sees what the engine's stream has done so far (the stage table upload, the caller's writes of Xd)
          event_record(ev_fork, stream);
          for (int p = 0; p < nparts; p++)
          {
            int i0, n;
            part_range(p, nparts, i0, n);
            const stream_t * on = p == 0 ? nullptr : &part_stream[p - 1];
            if (p > 0)
              stream_wait_event(*on, ev_fork);
            launch_split_part(a, false, i0, n, on, Xd, &part_event[nparts + p], p > 0 ? &part_event[nparts + p - 1] : nullptr);
          }
          // join
          for (int p = 1; p < nparts; p++)
          {
            event_record(part_event[p - 1], part_stream[p - 1]);
            stream_wait_event(stream, part_event[p - 1]);
          }
          return;
        }
      }
      launch_frontend(Xd);
      launch_step(a);
    }
    // ---- per-stage references (OCPHandler setters / getters of the centroidal OCP, reference src/centroidal-dynamics.cpp:
    //      120-304), broadcast over the batch ----
    // what: 0 = control target (nu); 1 = reference state as get / setReferenceState define it: [com_ref; v_lin; v_ang]
    // (setReferenceState = setPoseBase + setVelocityBase, which stores the momenta m v; getReferenceState divides by m)
    void set_stage_reference(int t, int what, const double * v, int n) override
    {
      check_stage(t);
      if (what == 0)
      {
        if (n != DC::NU)
          throw std::runtime_error("u_ref not of the right size");
        std::copy(v, v + n, horizon[t].u_ref);
      }
      else if (what == 1)
      {
        if (n != 9)
          throw std::runtime_error("x_ref not of the right size");
        double mv[6];
        for (int i = 0; i < 3; i++)
        {
          horizon[t].x_tgt[i] = v[i];
          com_ref_member[i] = v[i]; // setPoseBase updates CentroidalOCP::com_ref_
        }
        for (int i = 0; i < 6; i++)
          horizon[t].x_tgt[3 + i] = mv[i] = mass * v[3 + i];
        fill_strided(buf.vref + (size_t)ring_slot(head, t, R) * 6, (size_t)R * 6, B, mv, 6);
      }
      else
        throw std::runtime_error("unknown stage reference");
    }
    void get_stage_reference(int t, int what, double * v, int n) override
    {
      check_stage(t);
      if (what == 0 && n == DC::NU)
        std::copy(horizon[t].u_ref, horizon[t].u_ref + n, v);
      else if (what == 1 && n == 9)
      {
        double mv[6];
        get_linear(buf.vref + (size_t)ring_slot(head, t, R) * 6, 6, mv); // instance 0
        for (int i = 0; i < 3; i++)
          v[i] = horizon[t].x_tgt[i];
        for (int i = 0; i < 6; i++)
          v[3 + i] = mv[i] / mass;
      }
      else
        throw std::runtime_error("unknown stage reference or wrong size");
    }
    void set_reference_pose(int t, int foot, const double * p3) override
    {
      check_stage(t);
      check_foot(foot);
      ref_rot.set(t, foot, nullptr); // (a translation: identity rotation)
      fill_strided(buf.foot + ((size_t)t * DC::NF + foot) * 3, (size_t)H * DC::NF * 3, B, p3, 3);
    }
    void get_reference_pose(int t, int foot, int inst, double * p3) override
    {
      check_stage(t);
      if (foot < 0 || foot >= DC::NF || inst < 0 || inst >= B)
        throw std::runtime_error("unknown end effector or instance");
      get_linear(buf.foot + (((size_t)inst * H + t) * DC::NF + foot) * 3, 3, p3);
    }
    unsigned contact_mask(int t) const override
    {
      check_stage(t);
      return horizon[t].mask;
    }

    // state feedback front-end on measured states X [B][nq + nv] (host): host outputs, any may be null
    void update_internal_data(const double * X, double * feet, double * com, double * hg, double * cstate) override
    {
      const size_t nf = (size_t)B * DC::NF * 3, nc = (size_t)B * 3, nh = (size_t)B * 6, ns = (size_t)B * 9;
      double * st = staging((nf + nc + nh + ns) * sizeof(double));
      h2d(X_dev, X, (size_t)B * nx_mb * sizeof(double), stream);
      if constexpr (RT)
        launch_rt_aux(st, st + nf, st + nf + nc, st + nf + nc + nh);
      else
      {
        FrontendArgs<DK> fa;
        fa.b = fk;
        fa.X = X_dev;
        fa.feet = st;
        fa.com = st + nf;
        fa.hg = st + nf + nc;
        fa.cstate = st + nf + nc + nh;
        if constexpr (cent_is_full_dims<DK>::value)
          launch<FrontendArgs<DK>, frontend_full_body<DK>, 64, 1, 1>(B, stream, fa);
        else
          launch<FrontendArgs<DK>, frontend_body<DK>, 64, 1, 1>(B, stream, fa);
      }
      read_front(st, nf, nc, nh, ns, feet, com, hg, cstate);
    }
    // frontend_rt_body on X_dev (auxiliary kernel symbol: not a launch of the control loop)
    void launch_rt_aux(double * feet, double * com, double * hg, double * cstate)
    {
      FrontendRtArgs fa;
      fa.model = rt_model;
      fa.X = X_dev;
      fa.feet = feet;
      fa.com = com;
      fa.hg = hg;
      fa.cstate = cstate;
      launch<FrontendRtArgs, frontend_rt_body, 64, 1, 1>(B, stream, fa);
    }
    // smpc_debug_frontend_rt: update_internal_data through the front end on the run-time joint tree, whatever front end the handle uses
    void debug_frontend_rt(const double * X, double * feet, double * com, double * hg, double * cstate) override
    {
      set_device(device_id);
      if (!rt_model)
      {
        RtDevModel hrt;
        fill_rt_model(&robot, hrt);
        rt_model = (RtDevModel *)dev_alloc(sizeof(RtDevModel));
        h2d(rt_model, &hrt, sizeof(RtDevModel), stream);
        stream_sync(stream);
      }
      const size_t nf = (size_t)B * DC::NF * 3, nc = (size_t)B * 3, nh = (size_t)B * 6, ns = (size_t)B * 9;
      double * st = staging((nf + nc + nh + ns) * sizeof(double));
      h2d(X_dev, X, (size_t)B * nx_mb * sizeof(double), stream);
      launch_rt_aux(st, st + nf, st + nf + nc, st + nf + nc + nh);
      read_front(st, nf, nc, nh, ns, feet, com, hg, cstate);
    }
    void read_front(const double * st, size_t nf, size_t nc, size_t nh, size_t ns, double * feet, double * com, double * hg, double * cstate)
    {
      if (feet)
        d2h(feet, st, nf * sizeof(double), stream);
      if (com)
        d2h(com, st + nf, nc * sizeof(double), stream);
      if (hg)
        d2h(hg, st + nf + nc, nh * sizeof(double), stream);
      if (cstate)
        d2h(cstate, st + nf + nc + nh, ns * sizeof(double), stream);
      stream_sync(stream);
    }
    // interpolated targets at `delay` after the last solve (host outputs, any may be null): x [B][9], xdot [B][9],
    // forces [B][NU]; with X_meas (measured multibody states [B][nq + nv]) also the Riccati feedback u [B][NU]
    // targets of a CentroidalID controller written into its device buffers; asynchronous on this engine's stream
    void interpolate_device_id(double delay, int knots, double * com, double * vcom, double * fp, double * fv, double * f) override
    {
      if (knots < 2 || knots > H + 1)
        throw std::runtime_error("interpolate: knots must be in [2, horizon + 1]");
      if (!(delay >= 0.0))
        throw std::runtime_error("interpolate: delay must be non-negative");
      set_device(device_id);
      CentInterpArgs<DC> ia;
      ia.b = buf;
      ia.head = head;
      ia.knots = knots;
      ia.delay = delay;
      ia.timestep = ms.timestep;
      ia.x_meas = nullptr;
      ia.x_out = nullptr;
      ia.xdot_out = nullptr;
      ia.f_out = f;
      ia.u_out = nullptr;
      ia.com_out = com;
      ia.vcom_out = vcom;
      ia.fp_out = fp;
      ia.fv_out = fv;
      ia.mass = mass;
      launch<CentInterpArgs<DC>, cent_interp_body<DC>, 64>(B, stream, ia);
    }
    bool centroidal() const override { return true; }
    // smpc_interpolate on a centroidal handle: x_out [B][9], acc_out = state derivative [B][9], force_out [B][3 nfeet]
    void interpolate(double delay, int knots, double * x_out, double * acc_out, double * f_out) override
    {
      interpolate_cent(delay, knots, nullptr, x_out, acc_out, f_out, nullptr);
    }
    void riccati_feedback(double delay, const double * X, double * u_out) override { interpolate_cent(delay, 2, X, nullptr, nullptr, nullptr, u_out); }
    void interpolate_cent(double delay, int knots, const double * X_meas, double * x_out, double * xdot_out, double * f_out, double * u_out)
    {
      if (knots < 2 || knots > H + 1)
        throw std::runtime_error("interpolate: knots must be in [2, horizon + 1]");
      if (!(delay >= 0.0))
        throw std::runtime_error("interpolate: delay must be non-negative");
      const size_t n9 = (size_t)B * 9, nu = (size_t)B * DC::NU;
      double * st = staging((2 * n9 + 2 * nu) * sizeof(double));
      if (X_meas)
      {
        h2d(X_dev, X_meas, (size_t)B * nx_mb * sizeof(double), stream);
        launch_frontend(X_dev, true);
      }
      CentInterpArgs<DC> ia;
      ia.b = buf;
      ia.head = head;
      ia.knots = knots;
      ia.delay = delay;
      ia.timestep = ms.timestep;
      ia.x_meas = X_meas ? cstate_dev : nullptr;
      ia.x_out = st;
      ia.xdot_out = st + n9;
      ia.f_out = st + 2 * n9;
      ia.u_out = X_meas ? st + 2 * n9 + nu : nullptr;
      launch<CentInterpArgs<DC>, cent_interp_body<DC>, 64>(B, stream, ia);
      if (x_out)
        d2h(x_out, st, n9 * sizeof(double), stream);
      if (xdot_out)
        d2h(xdot_out, st + n9, n9 * sizeof(double), stream);
      if (f_out)
        d2h(f_out, st + 2 * n9, nu * sizeof(double), stream);
      if (u_out && X_meas)
        d2h(u_out, st + 2 * n9 + nu, nu * sizeof(double), stream);
      stream_sync(stream);
    }

    size_t state_io(StateIO & io) override
    {
      set_device(device_id);
      stream_sync(stream);
      io.tag(0x534d504343454e54LL, "kind (centroidal)");
      io.tag(B, "batch");
      io.tag(H, "horizon");
      io.tag(DC::NU, "nu");
      if constexpr (RT)
        io.tag(nq_mb, "nq of the robot"); // (the built shapes follow from nu)
      io.pod(head);
      io.pod(walking);
      io.host(velocity_base, sizeof(velocity_base));
      io.host(x_reference.data(), 9 * sizeof(double));
      io.host(com_ref_member, sizeof(com_ref_member));
      io.vec(horizon);
      io.vec(cycle);
      io.timer(timer);
      const size_t BR = (size_t)B * R;
      io.dev(buf.xs, BR * 9 * sizeof(double));
      io.dev(buf.us, BR * DC::NU * sizeof(double));
      io.dev(buf.vs, BR * DC::NC * sizeof(double));
      io.dev(buf.lams, BR * 9 * sizeof(double));
      io.dev(buf.ftraj, (size_t)B * DC::NF * 6 * sizeof(double));
      io.dev(buf.foot, (size_t)B * H * DC::NF * 3 * sizeof(double));
      io.dev(buf.vbase, (size_t)B * 6 * sizeof(double));
      io.dev(buf.vref, BR * 6 * sizeof(double));
      io.dev(buf.scal, (size_t)B * SC_N * sizeof(double));
      io.dev(buf.xdot01, (size_t)B * 18 * sizeof(double));
      if (io.mode == StateIO::LOAD)
        upload_stages();
      stream_sync(stream);
      return io.pos;
    }
    void iterate_host(const double * X) override
    {
      set_device(device_id);
      h2d(X_dev, X, (size_t)B * nx_mb * sizeof(double), stream);
      iterate_device(X_dev);
      stream_sync(stream);
    }
    void state_derivatives(double * out) override
    {
      set_device(device_id);
      XdotArgs<CentBuffers<DC>> a;
      a.b = buf;
      a.head = head;
      a.out = out;
      launch<XdotArgs<CentBuffers<DC>>, xdot_all_body<DC, CentBuffers<DC>, XD_CENT>, 64>(xdot_grid(XD_CENT, B, H), stream, a);
    }
    size_t xdot_doubles() const override { return (size_t)B * H * 9; }
    void get_K(double * out, bool all)
    {
      const int nt = all ? H : 1;
      const size_t n = (size_t)B * nt * DC::NU * 9;
      double * dev = staging(n * sizeof(double));
      CentGainsOutArgs<DC> ga;
      ga.b = buf;
      ga.out = dev;
      ga.all = all ? 1 : 0;
      launch<CentGainsOutArgs<DC>, cent_gains_out_body<DC>, 64>(B * nt, stream, ga);
      d2h(out, dev, n * sizeof(double), stream);
      stream_sync(stream);
    }
    void get_output(Output what, double * out) override
    {
      switch (what)
      {
      case OUT_XS:
        return get_ring(buf.xs, 9, H + 1, out);
      case OUT_US:
        return get_ring(buf.us, DC::NU, H, out);
      case OUT_K0:
        return get_K(out, false);
      case OUT_KS:
        return get_K(out, true);
      case OUT_VS:
        return get_ring(buf.vs, DC::NC, H, out);
      case OUT_LAMS:
        return get_lams(buf.lams, 9, out);
      case OUT_XDOT01:
        return get_linear(buf.xdot01, (size_t)B * 18, out);
      case OUT_FOOT_REFS:
        return get_linear(buf.foot, (size_t)B * H * DC::NF * 3, out);
      case OUT_INFO:
        return get_linear(buf.scal, (size_t)B * SC_N, out);
      default:
        throw InvalidCall("smpc_get_contact_forces needs a full-dynamics handle (the other problems carry the forces in us)");
      }
    }
    void set_early_exit(bool) override
    {
      throw InvalidCall("smpc_set_early_exit_on_tol: kinodynamics and full-dynamics handles (the centroidal step is one fused kernel)");
    }
    // the kernel pipeline of point feet keeps its steps on the iterate's ring slots [B][R][.] (smpc_cent_split.h); the 6-D path and the
    // one-kernel form keep them linear in t
    bool steps_on_ring() const { return DC::FS == 3 && !fused; }
    void debug_steps(double * dxs, double * dus) override
    {
      if (steps_on_ring())
      {
        get_ring(buf.dxs, 9, H + 1, dxs);
        get_ring(buf.dus, DC::NU, H, dus);
        return;
      }
      get_linear(buf.dxs, (size_t)B * (H + 1) * 9, dxs);
      get_linear(buf.dus, (size_t)B * H * DC::NU, dus);
    }
    // smpc_debug_get_dual_steps: dvs [B][H][nc], dlams [B][H][9] with dlams[t] = dlambda_{t+1}
    void debug_dual_steps(double * dvs, double * dlams) override
    {
      if (steps_on_ring())
      {
        get_ring(buf.dvs, DC::NC, H, dvs);
        get_ring(buf.dlams, 9, H, dlams);
        return;
      }
      get_linear(buf.dvs, (size_t)B * H * DC::NC, dvs);
      get_linear(buf.dlams, (size_t)B * H * 9, dlams);
    }
    // ---- the LQ knot the sweeps of the last iteration solved (debug surface; TEST INFRASTRUCTURE of tests/sweep_check.py) ----
    // point feet: the record of stage (inst, t), unpacked through CentRec's own maps (the maps cent_bwd_body gathers through) into
    //   A 9x9 | B 9xNU | Q 9x9 | S 9xNU | R NUxNU | Dd NCxNU | q 9 | r NU | f 9 | d NC | act NC | any | preg
    // in the vector conventions of the oracle's Knot (Cd is structurally zero; a cone row is active when its Jacobian row is in the record).
    // 6-D feet: the dense knot of the sweep, layout DC::DD (state padded to 12).
    static constexpr int KN_A = 0, KN_B = KN_A + 81, KN_Q = KN_B + 9 * DC::NU, KN_S = KN_Q + 81, KN_R = KN_S + 9 * DC::NU, KN_D = KN_R + DC::NU * DC::NU,
                         KN_q = KN_D + DC::NC * DC::NU, KN_r = KN_q + 9, KN_f = KN_r + DC::NU, KN_d = KN_f + 9, KN_act = KN_d + DC::NC, KN_any = KN_act + DC::NC,
                         KN_preg = KN_any + 1, KN_N = KN_preg + 1;
    int lq_size() const override
    {
      if constexpr (DC::FS == 6)
        return DC::DD::LQ_STRIDE;
      else
        return KN_N;
    }
    void check_knot_source() const
    {
      if (fused)
        throw InvalidCall("a centroidal handle created with SMPC_CENT_FUSED=1 runs the one-kernel control step, which keeps no stage record: no knot to return");
    }
    void debug_lq(int inst, int t, double * out) override
    {
      check_knot_source();
      if (inst < 0 || inst >= B || t < 0 || t >= H)
        throw InvalidCall("Stage index exceeds stage vector size");
      if constexpr (DC::FS == 6)
      {
        typedef typename DC::DD DD;
        get_linear(x6.sb.lq + ((size_t)inst * H + t) * DD::LQ_STRIDE, DD::LQ_STRIDE, out);
        // (upper triangles of Q and R are what the derivative pass writes and the sweep reads: mirror, as FullEngine::debug_lq)
        for (int i = 0; i < DD::NDX; i++)
          for (int j = 0; j < i; j++)
            out[DD::O_Q + i * DD::NDX + j] = out[DD::O_Q + j * DD::NDX + i];
        for (int i = 0; i < DD::NU; i++)
          for (int j = 0; j < i; j++)
            out[DD::O_R + i * DD::NU + j] = out[DD::O_R + j * DD::NU + i];
      }
      else
      {
        typedef CentRec<DC> RC;
        constexpr int NU = DC::NU, NC = DC::NC;
        std::vector<double> stg(RC::STAGE_N, 0.0), sc(SC_N);
        get_linear(sbuf.rec + ((size_t)inst * H + t) * RC::STRIDE, RC::STRIDE, stg.data());
        get_linear(buf.scal + (size_t)inst * SC_N, SC_N, sc.data());
        CentDevModel<DC> mg;
        static_assert(sizeof(CentDevModel<DC>) % sizeof(double) == 0, "the device model is an array of doubles");
        get_linear(reinterpret_cast<const double *>(buf.model), sizeof(mg) / sizeof(double), reinterpret_cast<double *>(&mg));
        // the constants cent_bwd_body keeps behind the record in LDS; preg: the value the last iteration used, parked by the line search
        const double preg = sc[SC_PREG_OLD];
        stg[RC::C_ONE] = 1.0;
        stg[RC::C_DTM] = mg.dt / mg.mass;
        stg[RC::C_NMU] = -mg.mu;
        for (int a = 0, e = 0; a < 3; a++)
          for (int bb = a; bb < 3; bb++, e++)
          {
            stg[RC::C_QLM + e] = mg.w_lm[a * 3 + bb] + (a == bb ? preg : 0.0);
            stg[RC::C_QAM + e] = mg.w_am[a * 3 + bb] + (a == bb ? preg : 0.0);
          }
        const double * s = stg.data();
        for (int k = 0; k < 9; k++)
        {
          for (int i = 0; i < 9; i++)
          {
            out[KN_A + k * 9 + i] = s[RC::ab_off(k, RC::XO + i)];
            out[KN_Q + k * 9 + i] = s[RC::m2_off(RC::XO + k, RC::XO + i)];
          }
          for (int j = 0; j < NU; j++)
          {
            out[KN_B + k * NU + j] = s[RC::ab_off(k, j)];
            out[KN_S + k * NU + j] = s[RC::m2_off(j, RC::XO + k)];
          }
          out[KN_q + k] = s[RC::m2_off(RC::XO + k, RC::ZC)];
          out[KN_f + k] = s[RC::O_F + k];
        }
        for (int i = 0; i < NU; i++)
        {
          for (int j = 0; j < NU; j++)
            out[KN_R + i * NU + j] = s[RC::m2_off(i, j)];
          out[KN_r + i] = s[RC::m2_off(i, RC::ZC)];
        }
        for (int row = 0; row < NC; row++)
        {
          bool act = false;
          for (int j = 0; j < NU; j++)
          {
            const double v = s[RC::m2_off(j, RC::cone_slot(row))];
            out[KN_D + row * NU + j] = v;
            act = act || v != 0.0;
          }
          out[KN_d + row] = s[RC::m2_off(RC::cone_slot(row), RC::ZC)];
          out[KN_act + row] = act ? 1.0 : 0.0;
        }
        out[KN_any] = s[RC::O_ANY];
        out[KN_preg] = preg;
      }
    }
    void debug_terminal(int inst, double * QN, double * qN) override
    {
      check_knot_source();
      if (inst < 0 || inst >= B)
        throw InvalidCall("instance index out of range");
      if constexpr (DC::FS == 6)
      {
        typedef typename DC::DD DD;
        get_linear(x6.sb.QN + (size_t)inst * DD::NDX * DD::NDX, DD::NDX * DD::NDX, QN);
        get_linear(x6.sb.qN + (size_t)inst * DD::NDX, DD::NDX, qN);
      }
      else
      {
        typedef CentRec<DC> RC;
        std::vector<double> tr(RC::T_STRIDE);
        get_linear(sbuf.term + (size_t)inst * RC::T_STRIDE, RC::T_STRIDE, tr.data());
        std::copy(tr.begin() + RC::T_P, tr.begin() + RC::T_P + 81, QN);
        std::copy(tr.begin() + RC::T_p, tr.begin() + RC::T_p + 9, qN);
      }
    }
    void phase_cycles(double * out64) override
    {
      if (!buf.dbg)
        throw InvalidCall("phase timers are off (set SMPC_PHASE_PROFILE=1 before smpc_create)");
      get_linear(buf.dbg, 64, out64);
    }
  };
} // namespace smpc
