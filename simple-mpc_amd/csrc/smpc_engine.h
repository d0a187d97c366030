// smpc_engine.h -- the batched kinodynamics MPC engine (reference KinodynamicsOCP under the MPC class): its constructor (model upload,
// allocation, lane hand-over), its stage and sweep kernels and the kinodynamics-only outputs.  The ProxDDP schedule of a control step, the
// gait state machine and the host halves of the getters are StageEngine's (smpc_stage_engine.h).
#pragma once
#ifndef SMPC_TRIAL_MINW
#define SMPC_TRIAL_MINW 3
#endif
#ifndef SMPC_LANE_MINW
#define SMPC_LANE_MINW 1
#endif
#ifndef SMPC_DERIV2_MINW
#define SMPC_DERIV2_MINW 2 // waves per SIMD the register allocation of deriv2_body is capped for (3: measured refusal)
#endif
#include "smpc_stage_engine.h"
#include "smpc_riccati_kino.h"
#include "smpc_kino_deriv2.h"
#include "smpc_solver_kernels.h"
#include "smpc_full_kernels.h"
#include "smpc_xdot.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace smpc
{
  struct HostKinoSettings
  {
    double timestep;
    std::vector<double> w_x, w_u, w_frame, w_cent, w_centder, qmin, qmax;
    double gravity[3];
    int kinematics_limits;
    int terminal_constraint = 0; // createProblem(..., terminal_constraint)
    int force_cone = 0;          // friction-cone rows per foot in contact (3-D feet)
    int land_cstr = 0;           // height of a landing foot pinned to its contact pose
    double mu = 0.8;             // friction coefficient
  };

  // CoM height at state x from the host copy of a device model (MPC::com0_ at the reference state, reference src/mpc.cpp:93)
  template <class M>
  double host_com_height(const M & m, const double * x)
  {
    constexpr int NJ = sizeof(m.mass) / sizeof(double);
    M3 Rj[NJ];
    V3 pj[NJ];
    double mt = 0.0, mz = 0.0;
    for (int j = 0; j < NJ; j++)
    {
      if (j == 0)
      {
        Rj[0] = quat_to_R(Quat{x[3], x[4], x[5], x[6]});
        pj[0] = ld3(x);
      }
      else
      {
        const double ang = x[6 + j], s = std::sin(ang), c = std::cos(ang);
        const int jt = m.jtype[j];
        M3 Rq = jt == 1 ? M3{1, 0, 0, 0, c, -s, 0, s, c} : (jt == 2 ? M3{c, 0, s, 0, 1, 0, -s, 0, c} : M3{c, -s, 0, s, c, 0, 0, 0, 1});
        Rj[j] = Rj[m.parent[j]] * (ldm3(m.jpR[j]) * Rq);
        pj[j] = pj[m.parent[j]] + Rj[m.parent[j]] * ld3(m.jpp[j]);
      }
      const V3 cw = pj[j] + Rj[j] * ld3(m.com[j]);
      mt += m.mass[j];
      mz += m.mass[j] * cw.z;
    }
    return mz / mt;
  }

  // createTerminalConstraint(x0.head<3>()): tau = sqrt(x0_z / 9.81), reference = the base position until the first control step
  // (reference src/ocp-handler.cpp:133-136, src/kinodynamics.cpp:366-377); multipliers start at zero
  template <class D>
  void alloc_terminal_constraint(Buffers<D> & bf, const double * x0, double com_height, stream_t stream)
  {
    auto dalloc = [&](size_t n) {
      double * p = (double *)dev_alloc(n * sizeof(double));
      dev_zero(p, n * sizeof(double), stream);
      return p;
    };
    bf.CN = dalloc((size_t)bf.B * (3 * D::NDX + 3));
    bf.vN = dalloc((size_t)bf.B * 3);
    bf.vN_e = dalloc((size_t)bf.B * 3);
    bf.vN_b = dalloc((size_t)bf.B * 3);
    bf.dvN = dalloc((size_t)bf.B * 3);
    bf.dcm_ref = dalloc((size_t)bf.B * 3);
    bf.dcm_tau = std::sqrt(x0[2] / 9.81);
    bf.com0z = com_height;
    h2d(bf.dcm_ref, x0, 3 * sizeof(double), stream);
  }

  // kinematic tree, inertias and feet of the robot table -> device model (shared by the kinodynamics engine and the
  // front-end of the centroidal engine)
  template <class D>
  inline void fill_tree_model(const smpc_robot_model * rm, DevModel<D> & m)
  {
    if (rm->njoints != D::NJ || rm->nfeet != D::NF)
      throw std::runtime_error("robot shape (njoints, nfeet) does not match this kernel instantiation");
    int maxlev = 0;
    for (int j = 0; j < D::NJ; j++)
    {
      m.parent[j] = rm->parent[j];
      if (j > 0 && (rm->parent[j] < 0 || rm->parent[j] >= j))
        throw std::runtime_error("robot joints must be topologically ordered");
      m.jtype[j] = rm->jtype[j];
      m.level[j] = j == 0 ? 0 : m.level[rm->parent[j]] + 1;
      maxlev = std::max(maxlev, m.level[j]);
      m.anc[j] = (j == 0 ? 0u : m.anc[rm->parent[j]]) | (1u << j);
      if (j > 0)
        m.children[rm->parent[j]] |= 1u << j;
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
    for (int f = 0; f < D::NF; f++)
    {
      m.foot_joint[f] = rm->foot_joint[f];
      for (int i = 0; i < 3; i++)
      {
        m.foot_p[f][i] = rm->foot_p[f][i];
        m.foot_ref_p[f][i] = rm->foot_ref_p[f][i];
      }
    }
    m.total_mass = rm->total_mass;
  }

  // branch joints of the lane-per-problem evaluation (smpc_kino_lane.h): parents that are not the joint right before their child
  template <class D>
  inline void fill_lane_slots(const smpc_robot_model * rm, DevModel<D> & m)
  {
    int nslots = 0;
    bool ok = true;
    for (int j = 0; j < D::NJ; j++)
      m.par_slot[j] = m.save_slot[j] = -1;
    for (int j = 1; j < D::NJ; j++)
      if (rm->parent[j] != j - 1)
      {
        const int par = rm->parent[j];
        if (m.save_slot[par] < 0)
        {
          if (nslots == LANE_SLOTS)
          {
            ok = false;
            break;
          }
          m.save_slot[par] = nslots++;
        }
        m.par_slot[j] = m.save_slot[par];
      }
    m.lane_slots = ok ? std::max(nslots, 1) : 0;
  }

  // doubles of the row-major form of a kinodynamics knot (smpc_debug_get_lq)
  template <class D>
  constexpr int kino_lq_size()
  {
    return (D::O_T - D::O_A) + D::NDX * D::NDX + D::NDX * D::NU + D::NU * D::NU + (D::O_vpd + D::NC - D::O_C);
  }

  constexpr StageKind KINO_KIND = {0x534d50434b494e4fLL, "kind (kinodynamics)", "smpc_create", true};

  template <class D>
  class KinoEngine : public StageEngine<D>
  {
  public:
    typedef Dims<D::NJ, D::NF> DD;
    typedef StageEngine<D> Base;
    using MpcEngineBase::B;
    using MpcEngineBase::H;
    using MpcEngineBase::R;
    using MpcEngineBase::head;
    using MpcEngineBase::stream;
    using MpcEngineBase::cur;
    using MpcEngineBase::ms;
    using MpcEngineBase::dims;
    using MpcEngineBase::device_id;
    using MpcEngineBase::profiling;
    using MpcEngineBase::x_model_ref;
    using MpcEngineBase::x_reference;
    using MpcEngineBase::vbase_dev;
    using MpcEngineBase::ref_rot;
    using MpcEngineBase::staging;
    using MpcEngineBase::get_ring;
    using MpcEngineBase::get_linear;
    using MpcEngineBase::open_stream;
    using Base::buf;
    using Base::horizon;
    using Base::standing;
    using Base::X_dev;
    using Base::ref_foot_pos;
    using Base::n_parts;
    using Base::part_stream;
    using Base::solver_args;
    using Base::stage_args;
    template <class Args, void (*Body)(const Args &, int), int NT, int MINW = 1>
    void timed_launch(int kid, int grid, const Args & a, bool aux = false) // (a member template of a dependent base is not found unqualified)
    {
      static_cast<MpcEngineBase *>(this)->timed_launch<Args, Body, NT, MINW>(kid, grid, a, aux);
    }
    // SMPC_STREAMS=2: the iterations of the two halves of the batch run on two streams, so that workgroups of the matrix-core bound
    // Riccati sweep of one half share the CUs with the VALU bound stage kernels of the other (StageEngine's parts)
    int riccati_nt = xcheck_env("SMPC_RICCATI_NT") ? std::atoi(xcheck_env("SMPC_RICCATI_NT")) : 128; // dense sweep: lanes per instance
    // SMPC_RICCATI=dense selects the model-independent sweep (A/B comparison and cross-check in the tests)
    bool structured_riccati = !(xcheck_env("SMPC_RICCATI") && std::string(xcheck_env("SMPC_RICCATI")) == "dense");
    // lane-per-problem stage evaluation (smpc_kino_lane.h) for problems without optional constraint blocks; SMPC_LANE_EVAL=0: the
    // wavefront-per-problem kernels throughout (A/B comparison)
    int lane_slots = 1;
    // The derivative pass starts from the lane-per-problem evaluation too (lane_tree_body + deriv2_body: 0.27 + 3.1 ms per launch at
    // B = 4096 against 4.3 - 4.7 ms for the one-kernel path); SMPC_LANE_DERIV=0: the one-kernel path (A/B comparison)
    bool lane_deriv = !(xcheck_env("SMPC_LANE_DERIV") && std::atoi(xcheck_env("SMPC_LANE_DERIV")) == 0);
    size_t handover_bytes = 0; // device memory of the lane hand-over (tiles + stream)
    bool lane_eval = !(xcheck_env("SMPC_LANE_EVAL") && std::atoi(xcheck_env("SMPC_LANE_EVAL")) == 0);
    bool lane_stream = !(xcheck_env("SMPC_LANE_STREAM") && std::atoi(xcheck_env("SMPC_LANE_STREAM")) == 0);
    bool stream_order_recorded = false;
    int foot_joint_h[D::NF] = {0}; // (host copy for deriv2_commit_code)
    static constexpr int TRIAL_MINW = SMPC_TRIAL_MINW; // waves per SIMD the trial kernel's register budget allows
    static constexpr int RICCATI_MINW = 2;             // the Riccati sweep is latency bound: 2 waves per SIMD (8 per CU, 19.8 KB LDS each)
    // Both sweeps as ONE staggered persistent launch (sweeps_kino_body): blocks of its grid, 0 = the two-launch form.
    // One block per resident slot: (resident blocks per CU of the fused kernel) x (CUs of the device), unless the fused kernel keeps
    // fewer blocks resident than the backward sweep alone -- then the handle stays with the two launches.  Read at handle creation:
    // SMPC_FUSED_SWEEPS=0 forces the two-launch form, SMPC_FUSED_SWEEPS=1 the fused one, then with SMPC_SWEEP_SLOTS=n blocks if given.
    int sweep_slots = 0;
    // bit of the slot index that selects a slot's order (smpc_sweep_order.h); SMPC_SWEEP_STAGGER=n: an experiment switch, read with the others
    int sweep_stagger = std::getenv("SMPC_SWEEP_STAGGER") ? std::min(std::max(std::atoi(std::getenv("SMPC_SWEEP_STAGGER")), 0), 30) : 0;
    int fused_sweep_slots() const
    {
      const char * fs = std::getenv("SMPC_FUSED_SWEEPS");
      const int want = fs ? std::atoi(fs) : -1;
      if (!structured_riccati || want == 0)
        return 0;
      if (want == 1 && std::getenv("SMPC_SWEEP_SLOTS") && std::atoi(std::getenv("SMPC_SWEEP_SLOTS")) > 0)
        return std::atoi(std::getenv("SMPC_SWEEP_SLOTS"));
#ifdef SMPC_HAS_OCCUPANCY_QUERY
      const int fused = resident_blocks_per_cu<SolverArgs<D>, sweeps_kino_body<D>, 64, RICCATI_MINW>();
      const int alone = resident_blocks_per_cu<SolverArgs<D>, riccati_kino_body<D, false>, 64, RICCATI_MINW>();
#else
      const int fused = 8, alone = 8; // (a backend that runs the blocks one after the other has nothing to ask: the figures of the device)
#endif
      if (fused <= 0 || (want != 1 && fused < alone))
        return 0;
      return fused * dev_cu_count(device_id);
    }

    KinoEngine(const smpc_robot_model * rm, const HostKinoSettings & ks, const HostMpcSettings & ms_, int batch, double gravity_arg, int device)
    : Base(KINO_KIND, ms_, batch, device)
    {
      AllocScope ctor_scope; // (a throw below releases what was allocated so far: smpc_alloc_scope.h)
      if (rm->njoints != D::NJ || rm->nfeet != D::NF)
        throw std::runtime_error("robot shape (njoints, nfeet) does not match this kernel instantiation");
      if (batch <= 0)
        throw std::runtime_error("batch must be positive");
      if ((int)ks.w_x.size() != D::NDX * D::NDX || (int)ks.w_u.size() != D::NU * D::NU || (int)ks.w_frame.size() != 9 || (int)ks.w_cent.size() != 36
          || (int)ks.w_centder.size() != 36 || (int)ks.qmin.size() != D::NA || (int)ks.qmax.size() != D::NA)
        throw std::runtime_error("kinodynamics settings: weight / limit sizes do not match the robot");
      {
        // LDS layout the rigid-body kernel relies on: the velocity-product matrices run across the end of the evaluation part
        // into the start of the derivative part (KinoScratch: late block | WJl | JWJ)
        static KinoScratch<D, true> probe;
        if ((const char *)probe.WJl - (const char *)probe.cval != (std::ptrdiff_t)(KinoScratchEval<D>::LATE_DOUBLES * sizeof(double)))
          throw std::runtime_error("internal: KinoScratch layout is not contiguous across its two parts");
      }
      open_stream();
      const int dd[8] = {D::NQ, D::NV, D::NX, D::NDX, D::NU, D::NC, D::NF, H};
      std::copy(dd, dd + 8, dims);
      // ---- model table ----
      std::vector<DevModel<D>> hm(1);
      DevModel<D> & m = hm[0];
      std::memset(&m, 0, sizeof(m));
      fill_tree_model<D>(rm, m);
      fill_lane_slots<D>(rm, m);
      lane_slots = m.lane_slots;
      for (int f = 0; f < D::NF; f++)
        foot_joint_h[f] = m.foot_joint[f];
      m.dt = ks.timestep;
      for (int i = 0; i < 3; i++)
        m.gravity[i] = ks.gravity[i];
      std::copy(ks.w_x.begin(), ks.w_x.end(), m.w_x);
      std::copy(ks.w_u.begin(), ks.w_u.end(), m.w_u);
      for (int i = 0; i < D::NDX; i++)
        for (int j = 0; j < D::NDX; j++)
          m.w_xT[j * D::NDX + i] = m.w_x[i * D::NDX + j];
      for (int i = 0; i < D::NU; i++)
        for (int j = 0; j < D::NU; j++)
          m.w_uT[j * D::NU + i] = m.w_u[i * D::NU + j];
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
        m.w_diag = 0; // test hook: exercise the general path with diagonal data
      for (int i = 0; i < D::NDX; i++)
        m.wxd[i] = m.w_x[i * D::NDX + i];
      for (int i = 0; i < D::NU; i++)
        m.wud[i] = m.w_u[i * D::NU + i];
      std::copy(ks.w_frame.begin(), ks.w_frame.end(), m.w_frame);
      std::copy(ks.w_cent.begin(), ks.w_cent.end(), m.w_cent);
      std::copy(ks.w_centder.begin(), ks.w_centder.end(), m.w_centder);
      std::copy(ks.qmin.begin(), ks.qmin.end(), m.qmin);
      std::copy(ks.qmax.begin(), ks.qmax.end(), m.qmax);
      m.kinematics_limits = ks.kinematics_limits;
      m.mu = ms.mu_init;
      x_model_ref.assign(D::NX, 0.0);
      for (int i = 0; i < D::NQ; i++)
        x_model_ref[i] = rm->q_ref[i];
      x_reference = x_model_ref;
      for (int i = 0; i < D::NX; i++)
        m.x_term[i] = x_model_ref[i];
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
      buf.lqc = dalloc(D::N_CT); // (written once, by lq_init_body below)
      buf.gains = dalloc(BH * (size_t)std::max((int)D::G_STRIDE, (int)GainsK<D>::STRIDE));
      if (lane_eval && m.lane_slots > 0 && !ks.terminal_constraint && !ks.force_cone && !ks.land_cstr)
      {
        // hand-over of the lane-per-problem evaluation.  With the stream (derivative pass: per-problem contiguous run, 688 doubles per
        // problem on Go2) the tiles hold the line-search heads only; without it (SMPC_LANE_STREAM=0, or no memory for it) every field.
        // A failed allocation falls back one level -- stream -> tiles -> the one-kernel evaluation -- instead of failing the handle.
        // (the flush addresses a problem's block by a 32-bit offset in doubles: 34 GB of stream -- B = 134 000 at H = 50)
        const size_t tiles = (((size_t)B + EV_LS - 1) / EV_LS) * (H + 1);
        auto try_alloc = [&](size_t doubles) -> double * {
          try
          {
            return dalloc(doubles);
          }
          catch (const std::exception &)
          {
            dev_clear_error();
            return nullptr;
          }
        };
        if (lane_deriv && lane_stream && (size_t)B * (H + 1) * EvStream<D>::STRIDE < ((size_t)1 << 32))
          buf.evd = try_alloc((size_t)B * (H + 1) * EvStream<D>::STRIDE);
        buf.ev_tile = ev_tile_doubles<D>(buf.evd != nullptr);
        buf.ev = try_alloc(tiles * buf.ev_tile);
        if (buf.ev == nullptr && buf.evd != nullptr)
        {
          // stream allocated, heads-only tiles not: give the stream back and try the full-field tiles (the second level of the fall-back:
          // stream -> tiles -> one-kernel stage evaluation)
          dev_free(buf.evd);
          buf.evd = nullptr;
          buf.ev_tile = ev_tile_doubles<D>(false);
          buf.ev = try_alloc(tiles * buf.ev_tile);
        }
        if (buf.evd != nullptr)
          buf.ev_order = (int *)dev_alloc((size_t)EvStream<D>::STRIDE * sizeof(int));
        handover_bytes = (buf.ev ? tiles * buf.ev_tile : 0) * sizeof(double) + (buf.evd ? (size_t)B * (H + 1) * EvStream<D>::STRIDE * sizeof(double) : 0);
      }
      buf.QN = dalloc((size_t)B * D::NDX * D::NDX);
      buf.qN = dalloc((size_t)B * D::NDX);
      buf.parts0 = dalloc((size_t)B * (H + 1) * 4);
      buf.partsT = dalloc((size_t)B * D::LS_N * (H + 1) * 2);
      buf.scal = dalloc((size_t)B * SC_N);
      buf.xdotT = dalloc((size_t)B * D::LS_N * 4 * D::NV);
      buf.xdot01 = dalloc((size_t)B * 4 * D::NV);
      buf.ls_sel = (int *)dev_alloc((size_t)B * sizeof(int));
      buf.und_list = (int *)dev_alloc((size_t)(B + 1) * sizeof(int));
      this->open_parts(std::getenv("SMPC_STREAMS") ? std::min(std::max(std::atoi(std::getenv("SMPC_STREAMS")), 1), (int)Base::MAX_PARTS) : 1);
      sweep_slots = fused_sweep_slots();
      buf.stages = (StageShared<D> *)dev_alloc((size_t)H * sizeof(StageShared<D>));
      buf.model = (DevModel<D> *)dev_alloc(sizeof(DevModel<D>));
      X_dev = dalloc((size_t)B * D::NX);
      if (ks.terminal_constraint)
        alloc_terminal_constraint<D>(buf, x_model_ref.data(), host_com_height(m, x_model_ref.data()), stream);
      if (ks.force_cone)
      {
        if (!structured_riccati)
          throw std::runtime_error("force_cone needs the structured Riccati sweep (unset SMPC_RICCATI)");
        auto zalloc = [&](size_t n) {
          double * p = dalloc(n);
          dev_zero(p, n * sizeof(double), stream);
          return p;
        };
        buf.es = zalloc(BR * 2 * D::NF);
        buf.es_e = zalloc(BR * 2 * D::NF);
        buf.es_b = zalloc(BR * 2 * D::NF);
        buf.des = zalloc(BH * 2 * D::NF);
        buf.ek = zalloc(BH * 12 * D::NF);
        buf.cone_mu2 = ks.mu * ks.mu;
      }
      land_cstr = ks.land_cstr != 0;
      if (land_cstr)
      {
        if (!structured_riccati)
          throw std::runtime_error("land_cstr needs the structured Riccati sweep (unset SMPC_RICCATI)");
        auto zalloc = [&](size_t n) {
          double * p = dalloc(n);
          dev_zero(p, n * sizeof(double), stream);
          return p;
        };
        buf.ls = zalloc(BR * D::NF);
        buf.ls_e = zalloc(BR * D::NF);
        buf.ls_b = zalloc(BR * D::NF);
        buf.dls = zalloc(BH * D::NF);
        buf.lk = zalloc(BH * D::NF * (D::NV + 2));
      }
      if (std::getenv("SMPC_PHASE_PROFILE"))
        buf.dbg = dalloc(64);
      h2d(buf.model, hm.data(), sizeof(DevModel<D>), stream);
      stream_sync(stream);

      // ---- default problem (OCPHandler::createProblem, src/ocp-handler.cpp:96-137) ----
      StageShared<D> def;
      std::memset(&def, 0, sizeof(def));
      def.mask = (1u << D::NF) - 1u;
      for (int f = 0; f < D::NF; f++)
        def.u_ref[3 * f + 2] = -rm->total_mass * gravity_arg / (double)D::NF;
      for (int i = 0; i < D::NX; i++)
        def.x_tgt[i] = x_model_ref[i];
      horizon.assign(H, def);
      standing = def;
      {
        StageKernelArgs<D> sk;
        sk.b = buf;
        sk.head = 0;
        sk.j0 = sk.nj = sk.slots = 0;
        launch<StageKernelArgs<D>, lq_init_body<D>, 64>(B * H, stream, sk);
      }
      this->cold_solve(def, m);
      for (int f = 0; f < D::NF; f++)
        buf.land_z[f] = ref_foot_pos[f][2]; // contact poses of the cycle stages: the feet at the reference state (src/mpc.cpp:162)
      ref_rot.init(H, D::NF);
      ctor_scope.commit();
    }
    bool land_cstr = false;
    ~KinoEngine() { this->free_buffers(); }

    // optional constraint blocks present: the kernels' EXT instantiations (the default ones carry none of that code)
    static bool has_ext(const Buffers<D> & b) { return b.es != nullptr || b.ls != nullptr || b.CN != nullptr; }
    void launch_deriv(const Buffers<D> & b, int slots = 0)
    {
      // list-mode launches (backtracking path, normally empty) are booked under "select" so that the per-kernel
      // averages of deriv / trial / apply stay those of full-batch launches
      if (b.ev != nullptr && lane_deriv)
      {
        // lane-per-problem evaluation, then the wavefront-per-problem derivative kernel that starts from it
        LaneKernelArgs<D> la;
        la.b = b;
        la.head = head;
        la.j0 = la.nj = 0;
        la.slots = slots;
        la.deriv = 1;
        la.order = nullptr;
        const int n = slots > 0 ? slots : b.B, kid = slots > 0 ? KID_SELECT : KID_DERIV, kid_tree = slots > 0 ? KID_SELECT : KID_TREE;
        if (b.evd != nullptr && !stream_order_recorded)
        {
          // once per handle: the tree kernel itself records the order in which it produces a problem's fields (one wavefront: the order
          // does not depend on the problem); the derivative kernel reads the fields back by that table
          LaneKernelArgs<D> lo = la;
          lo.b.B = b.B < 64 ? b.B : 64;
          lo.slots = 0;
          lo.order = b.ev_order;
          const bool prof = profiling;
          profiling = false;
          if (lane_slots == 1)
            timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 1, true, true>, 64, SMPC_LANE_MINW>(KID_SELECT, 1, lo, true);
          else
            timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 2, true, true>, 64, SMPC_LANE_MINW>(KID_SELECT, 1, lo, true);
          profiling = prof;
          // field ids -> commit codes of the derivative kernel (where each element of the stream goes in its scratch)
          std::vector<int> ord(EvStream<D>::STRIDE);
          d2h(ord.data(), b.ev_order, ord.size() * sizeof(int), cur);
          stream_sync(cur);
          for (int & v : ord)
            v = deriv2_commit_code<D>(foot_joint_h, v);
          h2d(b.ev_order, ord.data(), ord.size() * sizeof(int), cur);
          stream_sync(cur); // (ord is a local)
          stream_order_recorded = true;
        }
        const int gtree = (H + 1) * ((n + 63) / 64);
        if (b.evd != nullptr)
        {
          if (lane_slots == 1)
            timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 1, true>, 64, SMPC_LANE_MINW>(kid_tree, gtree, la, slots > 0);
          else
            timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 2, true>, 64, SMPC_LANE_MINW>(kid_tree, gtree, la, slots > 0);
        }
        else if (lane_slots == 1)
          timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 1>, 64, SMPC_LANE_MINW>(kid_tree, gtree, la, slots > 0);
        else
          timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 2>, 64, SMPC_LANE_MINW>(kid_tree, gtree, la, slots > 0);
        if (b.evd != nullptr)
          timed_launch<StageKernelArgs<D>, deriv2_body<D, true>, 64, SMPC_DERIV2_MINW>(kid, xcd_grid(n, H), stage_args(b, slots), slots > 0);
        else
          timed_launch<StageKernelArgs<D>, deriv2_body<D, false>, 64, SMPC_DERIV2_MINW>(kid, xcd_grid(n, H), stage_args(b, slots), slots > 0);
      }
      else if (has_ext(b) || !kCrossCheck) // (without the lane hand-over -- allocation refused -- the shipped library runs the instantiation it has)
        timed_launch<StageKernelArgs<D>, deriv_body<D, true>, 64, 2>(slots > 0 ? KID_SELECT : KID_DERIV, (slots > 0 ? slots : b.B) * (H + 1), stage_args(b, slots), slots > 0);
      else if constexpr (kCrossCheck)
        timed_launch<StageKernelArgs<D>, deriv_body<D, false>, 64, 2>(slots > 0 ? KID_SELECT : KID_DERIV, (slots > 0 ? slots : b.B) * (H + 1), stage_args(b, slots), slots > 0);
    }
    // line-search evaluation of the candidates sk.j0 .. sk.j0 + sk.nj - 1 (sk.slots > 0: for the compacted list of undecided instances)
    void launch_trial(const Buffers<D> & b, const StageKernelArgs<D> & sk, int kid, bool aux)
    {
      if (b.ev != nullptr)
      {
        LaneKernelArgs<D> la;
        la.b = b;
        la.head = sk.head;
        la.j0 = sk.j0;
        la.nj = sk.nj;
        la.slots = sk.slots;
        la.deriv = 0;
        la.order = nullptr;
        const int n = sk.slots > 0 ? sk.slots : b.B, kid_tree = kid == KID_TRIAL ? KID_TREE_LS : kid;
        if (lane_slots == 1)
          timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 1>, 64, SMPC_LANE_MINW>(kid_tree, (H + 1) * ((n + 63) / 64), la, aux);
        else
          timed_launch<LaneKernelArgs<D>, lane_tree_body<D, 2>, 64, SMPC_LANE_MINW>(kid_tree, (H + 1) * ((n + 63) / 64), la, aux);
        timed_launch<StageKernelArgs<D>, trial_rows_body<D>, 64>(kid, xcd_grid(n, H), sk, aux);
      }
      else if (has_ext(b) || !kCrossCheck)
        timed_launch<StageKernelArgs<D>, trial_body<D, true>, 64, TRIAL_MINW>(kid, (sk.slots > 0 ? sk.slots : b.B) * (H + 1), sk, aux);
      else if constexpr (kCrossCheck)
        timed_launch<StageKernelArgs<D>, trial_body<D, false>, 64, TRIAL_MINW>(kid, (sk.slots > 0 ? sk.slots : b.B) * (H + 1), sk, aux);
    }
    // backward + forward sweep: Newton step and merit directional derivative
    void launch_sweeps(const Buffers<D> & b)
    {
      if (structured_riccati)
      {
        // kinodynamics-structured sweep, one wavefront per instance
        if (has_ext(b))
        {
          timed_launch<SolverArgs<D>, riccati_kino_body<D, true>, 64, RICCATI_MINW>(KID_RICCATI, b.B, solver_args(b));
          timed_launch<SolverArgs<D>, forward_kino_body<D, true>, 64>(KID_FORWARD, b.B, solver_args(b));
        }
        else if (sweep_slots > 0 && b.B > sweep_slots && !this->aux_launches && !parts_enabled())
        {
          // more instances than resident slots: one persistent launch walks both sweeps of every instance, the slots' orders staggered.
          // Booked under the backward sweep's slot; the forward slot records no launch for it
          SolverArgs<D> sa = solver_args(b);
          sa.nslots = sweep_slots;
          sa.stagger = sweep_stagger;
          timed_launch<SolverArgs<D>, sweeps_kino_body<D>, 64, RICCATI_MINW>(KID_RICCATI, sweep_slots, sa);
        }
        else
        {
          timed_launch<SolverArgs<D>, riccati_kino_body<D, false>, 64, RICCATI_MINW>(KID_RICCATI, b.B, solver_args(b));
          timed_launch<SolverArgs<D>, forward_kino_body<D, false>, 64>(KID_FORWARD, b.B, solver_args(b));
        }
      }
      else if constexpr (kCrossCheck)
      {
        // dense, model-independent sweep (cross-check of the structured one: SMPC_RICCATI=dense)
        switch (riccati_nt)
        {
        case 64:
          timed_launch<SolverArgs<D>, riccati_body<D, 64>, 64>(KID_RICCATI, b.B, solver_args(b));
          break;
        case 128:
          timed_launch<SolverArgs<D>, riccati_body<D, 128>, 128>(KID_RICCATI, b.B, solver_args(b));
          break;
        default:
          timed_launch<SolverArgs<D>, riccati_body<D, 256>, 256>(KID_RICCATI, b.B, solver_args(b));
        }
        timed_launch<SolverArgs<D>, forward_body<D>, 64>(KID_FORWARD, b.B, solver_args(b));
      }
      this->launch_term_step(b);
    }
    void launch_first_trial(const Buffers<D> & b) override { launch_trial(b, stage_args(b, 0, 0, 1), KID_TRIAL, false); }
    // backtracking candidates 2^-1 .. 2^-9 in one batch, one select
    void launch_backtracking_trials(const Buffers<D> & b, int slots) override
    {
      launch_trial(b, stage_args(b, slots, 1, D::LS_N - 1), KID_SELECT, true);
      this->launch_select(b, 1, D::LS_N - 1);
    }
    // the stride of the sweep in use, which every reader of the whole buffer indexes by (gains_out_body, pack_outputs_body, get_K);
    // the allocation holds the larger of the two.  A part's view (slice) must start where those readers look for its first instance
    size_t gains_stride() const override { return structured_riccati ? (size_t)GainsK<D>::STRIDE : (size_t)D::G_STRIDE; }
    void set_force_ref(StageShared<D> & s, int foot, double fz) const override { s.u_ref[3 * foot + 2] = fz; }
    bool parts_enabled() const override { return n_parts > 1 && B >= 64 * n_parts && !has_ext(buf); }
    // the parts' launches are issued alternately, so that every queue stays filled: the tail of one part's launch is filled by the next
    // launch of another part (every launch alone is a whole number of rounds of resident waves plus a partial one)
    void issue_parts(const Buffers<D> * part, int k) override
    {
      for (int i = 0; i < n_parts; i++)
        this->begin_part(part[i], i);
      auto on = [&](int i) -> const Buffers<D> & { cur = part_stream[i]; return part[i]; };
      if (this->sequential(k))
      {
        for (int it = 0; it < k; it++)
          for (int i = 0; i < n_parts; i++)
            this->run_iteration(on(i));
        return;
      }
      for (int i = 0; i < n_parts; i++)
        this->speculative_start(on(i));
      for (int it = 0; it < k; it++)
        for (int i = 0; i < n_parts; i++)
          this->speculative_step(on(i), it == k - 1);
    }
    void launch_interp(int knots, double delay, double * x, double * acc, double * f, double * u) override
    {
      InterpArgs<D> ia;
      ia.b = buf;
      ia.head = head;
      ia.knots = knots;
      ia.delay = delay;
      ia.timestep = ms.timestep;
      ia.x_out = x;
      ia.acc_out = acc;
      ia.f_out = f;
      ia.u_out = u;
      launch<InterpArgs<D>, interp_body<D>, 64>(B, stream, ia);
    }
    // feedback is stored factored (W, L_R): K_t = -L_R^-T W_x, expanded on the device on request
    void launch_gains_out(int nt, double * out) override
    {
      GainOutArgs<D> ga;
      ga.b = buf;
      ga.nt = nt;
      ga.out = out;
      launch<GainOutArgs<D>, gains_out_body<D>, 64>(B * nt, stream, ga);
    }
    void launch_frontend(const FrontendArgs<D> & fa) override { launch<FrontendArgs<D>, frontend_body<D>, 64>(B, stream, fa); }
    // constrained forward dynamics of the full-dynamics model of the same robot (point feet)
    void launch_forward_dynamics(int n, const double * X, const double * tau, const unsigned * mask, const double * Kp, const double * Kd, double prox_accuracy,
                                 double prox_mu, int prox_max_iter, double * a, double * lam, int * iters) override
    {
      FullFdArgs<D> fa;
      fa.b = buf;
      fa.X = X;
      fa.tau = tau;
      fa.mask = mask;
      for (int i = 0; i < 3; i++)
      {
        fa.Kp[i] = Kp ? Kp[i] : 0.0;
        fa.Kd[i] = Kd ? Kd[i] : 0.0;
      }
      fa.prox_accuracy = prox_accuracy;
      fa.prox_mu = prox_mu;
      fa.prox_max_iter = prox_max_iter;
      fa.a_out = a;
      fa.lam_out = lam;
      fa.iters_out = iters;
      launch<FullFdArgs<D>, full_fd_body<D>, 64, 2>(n, stream, fa); // 256 registers: 8 waves per CU with the 20.2 KB of LDS
    }
    void launch_sim_integrate(const SimStepArgs<D> & sa) override { launch<SimStepArgs<D>, sim_integrate_body<D>, 64>(B, stream, sa); }

    // xdot of every stage at the iterate of the last solve, out [B][H][2 NV] (device): one launch on the handle's stream (smpc_xdot.h)
    void state_derivatives(double * out) override
    {
      set_device(device_id);
      XdotArgs<Buffers<D>> a;
      a.b = buf;
      a.head = head;
      a.out = out;
      if (lane_slots == 1)
        launch<XdotArgs<Buffers<D>>, xdot_all_body<D, Buffers<D>, XD_KINO_LANE, 1>, 64>(xdot_grid(XD_KINO_LANE, B, H), stream, a);
      else if (lane_slots == 2)
        launch<XdotArgs<Buffers<D>>, xdot_all_body<D, Buffers<D>, XD_KINO_LANE, 2>, 64>(xdot_grid(XD_KINO_LANE, B, H), stream, a);
      else
        launch<XdotArgs<Buffers<D>>, xdot_all_body<D, Buffers<D>, XD_KINO_WAVE>, 64>(xdot_grid(XD_KINO_WAVE, B, H), stream, a);
    }
    // the same without the final synchronisation: X must stay valid until sync() (one host thread can then keep several devices busy)
    void iterate_host_async(const double * X) override
    {
      set_device(device_id);
      h2d(X_dev, X, (size_t)B * D::NX * sizeof(double), stream);
      this->iterate_device(X_dev);
    }
    // What a controller consumes of a control step -- xs[1], us[0], K_0 -- of every instance as rows [x1 (NX) | u0 (NU) | K0 (NU x NDX)] of
    // `out`, `row_doubles` apart (the small return set of the sharded batch, gathered into ONE host buffer -- pinned by the
    // caller for full PCIe rate -- that several handles, one per device, fill side by side).  Asynchronous: sync() completes it.
    static constexpr int GATHER_ROW = D::NX + D::NU + D::NU * D::NDX;
    void gather_outputs_async(double * out, size_t row_doubles) override
    {
      set_device(device_id);
      if (row_doubles < (size_t)GATHER_ROW)
        throw std::runtime_error("smpc_gather_outputs: the row stride is smaller than nx + nu + nu * ndx");
      const size_t dp = row_doubles * sizeof(double);
      const int s1 = ring_slot(head, 1, R), s0 = ring_slot(head, 0, R);
      d2h_2d(out, dp, buf.xs + (size_t)s1 * D::NX, (size_t)R * D::NX * sizeof(double), D::NX * sizeof(double), B, stream);
      d2h_2d(out + D::NX, dp, buf.us + (size_t)s0 * D::NU, (size_t)R * D::NU * sizeof(double), D::NU * sizeof(double), B, stream);
      const size_t n = (size_t)B * D::NU * D::NDX;
      double * dev = staging(n * sizeof(double));
      if (structured_riccati)
      {
        GainOutArgs<D> ga;
        ga.b = buf;
        ga.nt = 1;
        ga.out = dev;
        launch<GainOutArgs<D>, gains_out_body<D>, 64>(B, stream, ga);
        d2h_2d(out + D::NX + D::NU, dp, dev, (size_t)D::NU * D::NDX * sizeof(double), (size_t)D::NU * D::NDX * sizeof(double), B, stream);
      }
      else
        for (int i = 0; i < D::NU; i++) // dense sweep: rows of [K k] are NDX + 1 apart
          d2h_2d(out + D::NX + D::NU + (size_t)i * D::NDX, dp, buf.gains + D::G_K + (size_t)i * (D::NDX + 1), (size_t)H * D::G_STRIDE * sizeof(double),
                 D::NDX * sizeof(double), B, stream);
    }
    // the same rows packed into a DEVICE buffer (one kernel), for a caller that moves them itself: a collective towards the rank that
    // owns the controllers, or one copy into pinned memory from a side stream.  Asynchronous on the engine's stream.
    void gather_outputs_device(double * out_dev, size_t row_doubles) override
    {
      set_device(device_id);
      if (row_doubles < (size_t)GATHER_ROW)
        throw std::runtime_error("smpc_gather_outputs_device: the row stride is smaller than nx + nu + nu * ndx");
      PackOutArgs<D> pa;
      pa.b = buf;
      pa.s1 = ring_slot(head, 1, R);
      pa.s0 = ring_slot(head, 0, R);
      pa.R = R;
      pa.g_off = structured_riccati ? GainsK<D>::G_W : D::G_K;
      pa.g_str = structured_riccati ? GainsK<D>::STRIDE : D::G_STRIDE;
      pa.g_tr = structured_riccati ? 1 : 0;
      pa.row = row_doubles;
      pa.out = out_dev;
      launch<PackOutArgs<D>, pack_outputs_body<D>, 64>(B, stream, pa);
    }
    // ... and into a buffer of ANOTHER device of the node: packed here, then one peer copy over xGMI on this engine's stream (the form
    // SURVEY 8e lists for a single process that drives all devices: every device's rows land in one buffer on the device -- or next to the
    // host thread -- that runs the controllers).  dst: [batch][GATHER_ROW] doubles, contiguous.
    void gather_outputs_peer(double * dst, int dst_device) override
    {
      if (dst_device < 0 || dst_device >= device_count())
        throw InvalidCall("destination device out of range");
      const size_t bytes = (size_t)B * GATHER_ROW * sizeof(double);
      double * dev = staging(bytes);
      gather_outputs_device(dev, GATHER_ROW);
      d2peer(dst, dst_device, dev, device_id, bytes, stream);
    }
    void riccati_feedback(double delay, const double * X, double * u_out) override
    {
      if (!structured_riccati)
        throw std::runtime_error("riccati_feedback needs the structured Riccati sweep (unset SMPC_RICCATI)");
      Base::riccati_feedback(delay, X, u_out);
    }
    // (the dense sweep keeps rows of [K k], strided out of the gains block)
    void get_K(double * out, bool all) override
    {
      if (structured_riccati)
        return Base::get_K(out, all);
      stream_sync(stream);
      const int nt = all ? H : 1;
      std::vector<double> row(D::NU * (D::NDX + 1));
      for (int b = 0; b < B; b++)
        for (int t = 0; t < nt; t++)
        {
          d2h(row.data(), buf.gains + ((size_t)b * H + t) * D::G_STRIDE + D::G_K, row.size() * sizeof(double), stream);
          stream_sync(stream);
          for (int i = 0; i < D::NU; i++)
            std::memcpy(out + (((size_t)b * nt + t) * D::NU + i) * D::NDX, row.data() + (size_t)i * (D::NDX + 1), D::NDX * sizeof(double));
        }
    }
    // multipliers of the optional rows: 0 = friction cones [B][H][2 NF], 1 = land rows [B][H][NF]
    void get_extra_multipliers(int which, double * out) override
    {
      double * src = which == 0 ? buf.es : buf.ls;
      if (!src)
        throw InvalidCall("the problem has no such rows");
      get_ring(src, which == 0 ? 2 * D::NF : D::NF, H, out);
    }
    int lq_size() const override { return kino_lq_size<D>(); }
    void debug_lq(int inst, int t, double * out) override
    {
      if (inst < 0 || inst >= B || t < 0 || t >= H)
        throw InvalidCall("Stage index exceeds stage vector size");
      // the device keeps [Q S; S^T R] as accumulator-layout tiles (Dims::O_T); returned in the documented row-major order
      // A | B | Q | S | R | C | q | r | f | d | lx | lu | lpd | vpd
      // (the last tile column of the grid is the handle's image, its diagonal and the selectors of the box rows of C two runs of the knot:
      // Dims::S_at / R_at / C_at put them back where the row-major form has them)
      std::vector<double> raw(D::LQ_STRIDE), img(D::N_CT);
      get_linear(buf.lq + ((size_t)inst * H + t) * D::LQ_STRIDE, D::LQ_STRIDE, raw.data());
      get_linear(buf.lqc, D::N_CT, img.data());
      constexpr int n = D::NDX, m = D::NU;
      double * o = out;
      std::copy(raw.begin() + D::O_A, raw.begin() + D::O_T, o); // A | B
      o += D::O_T - D::O_A;
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
          *o++ = raw[D::q_off(i, j)];
      for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++)
          *o++ = D::S_at(raw.data(), img.data(), i, j);
      for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++)
          *o++ = D::R_at(raw.data(), img.data(), i, j);
      for (int r = 0; r < D::NC; r++)
        for (int j = 0; j < n; j++)
          *o++ = D::C_at(raw.data(), r, j);
      std::copy(raw.begin() + D::O_q, raw.begin() + D::O_vpd + D::NC, o);
    }
  };
} // namespace smpc
