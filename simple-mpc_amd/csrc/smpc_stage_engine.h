// smpc_stage_engine.h -- the ProxDDP host driver KinoEngine (smpc_engine.h) and FullEngine (smpc_full_engine.h) share: the data of a
// stage-wise MPC handle, the launch schedule of one control step and the host halves of the getters.  An engine derives from
// StageEngine<D> and supplies its constructor (model upload, allocation), its stage and sweep kernels and the few launches whose kernel
// differs (the hooks below).  No kernel lives here.
//
// Mirrors, for a batch of B instances, the reference's MPC class:
//   MPC::MPC                   src/mpc.cpp:19-99      -> the engine's constructor + cold_solve (cold solve once, broadcast)
//   MPC::generateCycleHorizon  src/mpc.cpp:101-187    -> generate_cycle_horizon
//   MPC::iterate               src/mpc.cpp:189-218    -> iterate_device
//   MPC::recedeWithCycle       src/mpc.cpp:220-254    -> MpcEngineBase::recede_horizon (+ ring head increment)
//   MPC::updateCycleTiming     src/mpc.cpp:256-276    -> GaitTimer::update_timing
#pragma once
#include "smpc_engine_base.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace smpc
{
  // foot positions at state x, [NF][6] = (start, end) of a swing, both at the foot position.
  // Host restatement of FK limited to what the constructors need (src/mpc.cpp:24-39).
  template <class D>
  void host_foot_positions(const DevModel<D> & m, const double * x, double * out)
  {
    M3 Rj[D::NJ];
    V3 pj[D::NJ];
    for (int j = 0; j < D::NJ; j++)
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
    }
    for (int f = 0; f < D::NF; f++)
    {
      const V3 p = Rj[m.foot_joint[f]] * ld3(m.foot_p[f]) + pj[m.foot_joint[f]];
      st3(out + f * 6, p);
      st3(out + f * 6 + 3, p);
    }
  }

  // what the C ABI answers per handle kind where the two kinds differ: the kind tag of a checkpoint (a kinodynamics checkpoint also tags
  // its optional rows), and the class the debug getters refuse with (InvalidCall -> SMPC_ERR_INVALID, runtime_error -> SMPC_ERR_RUNTIME)
  struct StageKind
  {
    long long state_tag;
    const char * state_name;
    const char * create_fn;
    bool kino;
  };

  template <class D>
  class StageEngine : public MpcEngineBase
  {
  public:
    const StageKind kind;
    Buffers<D> buf;
    std::vector<StageShared<D>> horizon, cycle;
    StageShared<D> standing;
    UploadRing stage_ring;
    double * X_dev = nullptr;
    double ref_foot_pos[D::NF][3];
    // The batch as parts on streams of their own (KinoEngine: SMPC_STREAMS, FullEngine: SMPC_FULL_PARTS); part 0 is the handle's stream
    static constexpr int MAX_PARTS = 4;
    int n_parts = 1;
    stream_t part_stream[MAX_PARTS] = {};
    event_t ev_fork{}, ev_join[MAX_PARTS] = {};
    int * und_part[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr}; // undecided-lists; [0] == buf.und_list
    static constexpr int LS_SLOTS = 64; // instance slots of the list-mode (backtracking) launches: 64 x (H+1) blocks when the list is empty
    bool speculative_ls = xcheck_env("SMPC_NO_SPECULATIVE_LS") == nullptr; // tentative full steps (run_iterations)
    static constexpr double ARMIJO_C1 = 1e-4, REG_INIT = 1e-9, REG_MIN = 1e-10, REG_MAX = 1e9, REG_INC = 10.0, REG_DEC = 1.0 / 3.0, STALL_REL = 1e-9;
    double *sim_a = nullptr, *sim_lam = nullptr; // sim_step_device
    unsigned * sim_mask = nullptr;
    unsigned sim_mask_value = ~0u;

    StageEngine(const StageKind & k, const HostMpcSettings & ms_, int batch, int device) : MpcEngineBase(ms_, batch, device), kind(k) {}
    // (what sim_step_device allocated on first use; the engine's destructor releases what its constructor allocated: free_buffers)
    ~StageEngine()
    {
      dev_free(sim_a);
      dev_free(sim_lam);
      dev_free(sim_mask);
    }
    // every device array an engine's constructor allocates (what its problem does not have is null).  Called by the engine's destructor,
    // not by this class's: after a constructor that threw, the AllocScope has released them already
    void free_buffers()
    {
      for (double * p : {buf.CN, buf.vN, buf.vN_e, buf.vN_b, buf.dvN, buf.dcm_ref, buf.es, buf.es_e, buf.es_b, buf.des, buf.ek, buf.ls, buf.ls_e, buf.ls_b, buf.dls, buf.lk})
        dev_free(p);
      for (double * p : {buf.xs_b, buf.us_b, buf.vs_b, buf.lams_b, buf.xs, buf.us, buf.vs, buf.lams, buf.vs_e, buf.lams_e, buf.dxs, buf.dus, buf.dvs, buf.dlams, buf.foot_ref, buf.ftraj,
                         buf.vbase, buf.vref, buf.lq, buf.lqc, buf.gains, buf.ev, buf.evd, buf.QN, buf.qN, buf.parts0, buf.partsT, buf.scal, buf.xdotT, buf.xdot01, buf.forces, buf.forcesT,
                         buf.dbg, X_dev})
        dev_free(p);
      dev_free(buf.ls_sel);
      dev_free(buf.und_list);
      dev_free(buf.ev_order);
      for (int i = 1; i < n_parts; i++)
        dev_free(und_part[i]);
      dev_free(buf.stages);
      dev_free(buf.model);
      dev_free(cold.dev);
    }

    // ---- what an engine supplies ----
    virtual void launch_deriv(const Buffers<D> & b, int slots = 0) = 0; // derivative pass (slots > 0: of the compacted list of undecided instances)
    virtual void launch_sweeps(const Buffers<D> & b) = 0;               // backward + forward sweep: Newton step and merit directional derivative
    virtual void launch_first_trial(const Buffers<D> & b) = 0;          // line-search evaluation of alpha = 1 for everybody
    // ... of the candidates 2^-1 .. for the `slots` instance slots of the compacted list, with the select_body launches that decide them
    virtual void launch_backtracking_trials(const Buffers<D> & b, int slots) = 0;
    virtual double * wide_scratch(const Buffers<D> &) const { return nullptr; } // StageKernelArgs::wide of a view of the batch
    virtual size_t gains_stride() const = 0;                                    // doubles per (instance, stage) of buf.gains
    virtual void set_force_ref(StageShared<D> & s, int foot, double fz) const = 0; // vertical contact-force reference of a foot in support
    virtual bool parts_enabled() const = 0;
    virtual void issue_parts(const Buffers<D> * part, int k) = 0; // begin_part + the k iterations of every part, in the engine's order of issue
    virtual void launch_interp(int knots, double delay, double * x, double * acc, double * f, double * u) = 0;
    virtual void launch_gains_out(int nt, double * out) = 0;
    virtual void launch_frontend(const FrontendArgs<D> & fa) = 0;
    virtual void require_forward_dynamics(const char *) const {} // (throws where the model has no constrained forward dynamics)
    virtual void launch_forward_dynamics(int n, const double * X, const double * tau, const unsigned * mask, const double * Kp, const double * Kd, double prox_accuracy,
                                         double prox_mu, int prox_max_iter, double * a, double * lam, int * iters) = 0;
    virtual void launch_sim_integrate(const SimStepArgs<D> & sa) = 0;

    // streams, events and undecided-lists of n parts of the batch (after buf.und_list is allocated)
    void open_parts(int n)
    {
      n_parts = n;
      part_stream[0] = stream;
      und_part[0] = buf.und_list;
      if (n > 1)
        ev_fork = side.event();
      for (int i = 1; i < n; i++)
      {
        part_stream[i] = side.stream();
        ev_join[i] = side.event();
        und_part[i] = (int *)dev_alloc((size_t)(B + 1) * sizeof(int));
      }
    }
    int force_doubles() const { return force_size * D::NF; } // contact forces / wrenches of one stage
    [[noreturn]] void refuse(const std::string & why) const
    {
      if (kind.kino)
        throw InvalidCall(why);
      throw std::runtime_error(why);
    }

    SolverArgs<D> solver_args(const Buffers<D> & b, int j0 = 0, int nj = 0) const
    {
      SolverArgs<D> a;
      a.b = b;
      a.head = head;
      a.j0 = j0;
      a.nj = nj;
      a.armijo_c1 = ARMIJO_C1;
      a.reg_min = REG_MIN;
      a.reg_max = REG_MAX;
      a.reg_inc = REG_INC;
      a.reg_dec = REG_DEC;
      a.stop_tol = early_exit_on_tol ? ms.TOL : -1.0;
      return a;
    }
    StageKernelArgs<D> stage_args(const Buffers<D> & b, int slots = 0, int j0 = 0, int nj = 0) const
    {
      StageKernelArgs<D> sk;
      sk.b = b;
      sk.head = head;
      sk.j0 = j0;
      sk.nj = nj;
      sk.slots = slots;
      sk.wide = wide_scratch(b);
      return sk;
    }
    void launch_select(const Buffers<D> & b, int j0, int nj) { timed_launch<SolverArgs<D>, select_body<D>, 64>(KID_SELECT, (b.B + 63) / 64, solver_args(b, j0, nj)); }
    // the instances that are still undecided as a compacted list; returns the instance slots of the list-mode launches that walk it
    int launch_backtracking(const Buffers<D> & b)
    {
      timed_launch<SolverArgs<D>, compact_body<D>, 64>(KID_SELECT, 1, solver_args(b));
      return b.B < LS_SLOTS ? b.B : LS_SLOTS;
    }
    // line search with explicit trial evaluations: alpha = 1 for everybody, then the rest for the undecided
    void launch_line_search(const Buffers<D> & b)
    {
      launch_first_trial(b);
      launch_select(b, 0, 1);
      launch_backtracking_trials(b, launch_backtracking(b));
      timed_launch<SolverArgs<D>, apply_body<D>, 64>(KID_APPLY, b.B, solver_args(b));
    }
    // one ProxDDP iteration for the instances covered by b (b.B may be < B for the cold solve)
    void run_iteration(const Buffers<D> & b)
    {
      launch_deriv(b);
      launch_sweeps(b);
      launch_line_search(b);
    }
    bool sequential(int k) const { return !speculative_ls || k <= 1 || early_exit_on_tol; } // (the convergence test belongs to the sequential scheme)
    // k ProxDDP iterations of one control step.  Iterations before the last take the full step TENTATIVELY and run the
    // next derivative pass at once: its merit IS the line-search value phi(1), so in the common case (Armijo accepts
    // alpha = 1) no separate trial evaluation is launched, and the result is the sequential algorithm's.  Instances
    // that reject alpha = 1 are restored, backtracked with explicit trial evaluations and re-derived (compacted list).
    void run_iterations(const Buffers<D> & b, int k)
    {
      if (sequential(k))
      {
        for (int it = 0; it < k; it++)
          run_iteration(b);
        return;
      }
      speculative_start(b);
      for (int it = 0; it < k; it++)
        speculative_step(b, it == k - 1);
    }
    void speculative_start(const Buffers<D> & b)
    {
      launch_deriv(b);
      timed_launch<SolverArgs<D>, merit0_body<D>, 64>(KID_SELECT, (b.B + 63) / 64, solver_args(b));
    }
    // one iteration of the speculative scheme: sweeps, then either the explicit line search (last iteration) or the tentative
    // full step + next derivative pass + repair of the instances that rejected it
    void speculative_step(const Buffers<D> & b, bool last)
    {
      const int nb = (b.B + 63) / 64;
      launch_sweeps(b);
      if (last)
      {
        launch_line_search(b);
        return;
      }
      SolverArgs<D> sa = solver_args(b);
      sa.mode = 1;
      timed_launch<SolverArgs<D>, apply_body<D>, 64>(KID_APPLY, b.B, sa);
      launch_deriv(b);
      timed_launch<SolverArgs<D>, spec_select_body<D>, 64>(KID_SELECT, nb, solver_args(b));
      // rejected instances (usually none: every launch below then exits at once)
      const int slots = launch_backtracking(b);
      sa = solver_args(b);
      sa.slots = slots;
      sa.mode = 2;
      timed_launch<SolverArgs<D>, apply_body<D>, 64>(KID_SELECT, slots, sa, true);
      launch_backtracking_trials(b, slots);
      sa.mode = 0;
      timed_launch<SolverArgs<D>, apply_body<D>, 64>(KID_SELECT, slots, sa, true);
      launch_deriv(b, slots);
      timed_launch<SolverArgs<D>, merit0_body<D>, 64>(KID_SELECT, nb, sa);
    }
    void launch_term_step(const Buffers<D> & b)
    {
      if (b.CN != nullptr)
        timed_launch<SolverArgs<D>, term_step_body<D>, 64>(KID_FORWARD, (b.B + 63) / 64, solver_args(b));
    }
    // AL centres <- multipliers (the optional rows where the problem has them)
    void copy_centres(const Buffers<D> & b)
    {
      d2d(b.vs_e, b.vs, (size_t)b.B * R * D::NC * sizeof(double), cur);
      d2d(b.lams_e, b.lams, (size_t)b.B * R * D::NDX * sizeof(double), cur);
      if (b.CN != nullptr)
        d2d(b.vN_e, b.vN, (size_t)b.B * 3 * sizeof(double), cur);
      if (b.es != nullptr)
        d2d(b.es_e, b.es, (size_t)b.B * R * 2 * D::NF * sizeof(double), cur);
      if (b.ls != nullptr)
        d2d(b.ls_e, b.ls, (size_t)b.B * R * D::NF * sizeof(double), cur);
    }
    void upload_stages() { stage_ring.upload(buf.stages, horizon.data(), (size_t)H * sizeof(StageShared<D>), stream); }

    // reference: src/mpc.cpp:72-91.  All instances share x0 = reference state: solve instance 0, broadcast.  m: host copy of the model
    void cold_solve(const StageShared<D> & def, const DevModel<D> & m)
    {
      std::vector<double> xs0((size_t)R * D::NX), us0((size_t)R * D::NU);
      for (int t = 0; t < R; t++)
      {
        std::copy(x_model_ref.begin(), x_model_ref.end(), xs0.begin() + (size_t)t * D::NX);
        std::copy(def.u_ref, def.u_ref + D::NU, us0.begin() + (size_t)t * D::NU); // getReferenceControl(0) (src/mpc.cpp:75)
      }
      head = 0;
      h2d(buf.xs, xs0.data(), xs0.size() * sizeof(double), stream);
      h2d(buf.us, us0.data(), us0.size() * sizeof(double), stream);
      std::vector<double> sc0(SC_N, 0.0);
      sc0[SC_PREG] = REG_INIT;
      h2d(buf.scal, sc0.data(), SC_N * sizeof(double), stream);
      upload_stages();
      // foot refs of the default problem are the identity placements: translation 0 (src/ocp-handler.cpp:116)
      dev_zero(buf.foot_ref, (size_t)H * D::NF * 3 * sizeof(double), stream);
      Buffers<D> b1 = buf;
      b1.B = 1;
      aux_launches = true;
      copy_centres(b1);
      std::vector<double> sc(SC_N);
      cold_trace.clear();
      const int cold_max = std::getenv("SMPC_COLD_MAX_ITERS") ? std::atoi(std::getenv("SMPC_COLD_MAX_ITERS")) : 100; // (diagnostics)
      for (int it = 0; it < cold_max; it++)
      {
        run_iteration(b1);
        d2h(sc.data(), buf.scal, SC_N * sizeof(double), stream);
        stream_sync(stream);
        cold_iters = it + 1;
        cold_trace.insert(cold_trace.end(), {sc[SC_PHI0], sc[SC_PRIM], sc[SC_DUAL], sc[SC_ALPHA]});
        if (std::fmax(sc[SC_PRIM], sc[SC_DUAL]) <= ms.TOL)
          break;
        // stalled: predicted merit decrease below FP64 resolution (DESIGN.md "solver constants")
        if (std::fabs(sc[SC_DPHI0]) <= STALL_REL * std::fmax(1.0, std::fabs(sc[SC_PHI0])))
          break;
        if (sc[SC_DUAL] <= ms.TOL)
          copy_centres(b1);
      }
      aux_launches = false;
      // broadcast instance 0 to the whole batch
      auto bc = [&](double * p, size_t per) {
        for (size_t done = 1; p != nullptr && done < (size_t)B;)
        {
          const size_t n = std::min(done, (size_t)B - done);
          d2d(p + done * per, p, n * per * sizeof(double), stream);
          done += n;
        }
      };
      bc(buf.xs, (size_t)R * D::NX);
      bc(buf.us, (size_t)R * D::NU);
      bc(buf.vs, (size_t)R * D::NC);
      bc(buf.lams, (size_t)R * D::NDX);
      bc(buf.scal, SC_N);
      bc(buf.forces, (size_t)H * force_doubles());
      bc(buf.vN, 3);
      bc(buf.dcm_ref, 3);
      bc(buf.es, (size_t)R * 2 * D::NF);
      bc(buf.ls, (size_t)R * D::NF);
      // swing start/end = reference foot positions (FootTrajectory ctor, src/foot-trajectory.cpp:20-39):
      // a reference-only recede call with land = -1 < T_fly keeps them, so initialise them here on the host
      std::vector<double> ft((size_t)D::NF * 6);
      host_foot_positions(m, x_model_ref.data(), ft.data());
      h2d(buf.ftraj, ft.data(), ft.size() * sizeof(double), stream);
      stream_sync(stream);
      bc(buf.ftraj, (size_t)D::NF * 6);
      stream_sync(stream);
      for (int f = 0; f < D::NF; f++)
        for (int i = 0; i < 3; i++)
          ref_foot_pos[f][i] = ft[f * 6 + i];
      retain_cold();
    }
    // Instance 0 as the cold solve left it, kept for reset_instances_device: what the broadcast above gave every instance, and the rest
    // of the solver state a later iterate reads (DESIGN.md "Resetting single instances" classifies every buffer)
    int cold_ls_sel = 0;
    void retain_cold()
    {
      const size_t Rs = (size_t)R, Hs = (size_t)H;
      const int fd = buf.forces ? force_doubles() : 0, ne = buf.es ? 2 * D::NF : 0, nl = buf.ls ? D::NF : 0, n3 = buf.vN ? 3 : 0;
      cold.begin(B, H, R, Rs * (D::NX + D::NU + 2 * D::NC + 2 * D::NDX + 2 * ne + 2 * nl) + Hs * fd + SC_N + 4 * D::NV + D::NF * 6 + 3 * n3);
      cold.retain(buf.xs, D::NX, RESET_RING, stream);
      cold.retain(buf.us, D::NU, RESET_RING, stream);
      cold.retain(buf.vs, D::NC, RESET_RING, stream);
      cold.retain(buf.lams, D::NDX, RESET_RING, stream);
      cold.retain(buf.vs_e, D::NC, RESET_RING, stream);
      cold.retain(buf.lams_e, D::NDX, RESET_RING, stream);
      cold.retain(buf.es, ne, RESET_RING, stream);
      cold.retain(buf.es_e, ne, RESET_RING, stream);
      cold.retain(buf.ls, nl, RESET_RING, stream);
      cold.retain(buf.ls_e, nl, RESET_RING, stream);
      cold.retain(buf.forces, fd, RESET_STAGE, stream);
      cold.retain(buf.scal, SC_N, RESET_INST, stream);
      cold.retain(buf.xdot01, 4 * D::NV, RESET_INST, stream);
      cold.retain(buf.ftraj, D::NF * 6, RESET_INST, stream);
      cold.retain(buf.vN, n3, RESET_INST, stream);
      cold.retain(buf.vN_e, n3, RESET_INST, stream);
      cold.retain(buf.dcm_ref, n3, RESET_INST, stream);
      d2h(&cold_ls_sel, buf.ls_sel, sizeof(int), stream);
      stream_sync(stream);
    }
    void reset_instances_device(const uint8_t * mask_dev) override { launch_reset(mask_dev, buf.ls_sel, cold_ls_sel); }

    void generate_cycle_horizon(const unsigned char * cs, int n) override
    {
      if (n <= 0)
        throw std::runtime_error("contact sequence must not be empty");
      timer.generate(cs, n, D::NF, H);
      cycle.clear();
      unsigned previous = (1u << D::NF) - 1u; // land flags: in contact here, not in the stage before (src/mpc.cpp:133-137,167-185)
      for (auto & st : timer.states)
      {
        int active = 0;
        for (int f = 0; f < D::NF; f++)
          active += st[f] ? 1 : 0;
        StageShared<D> s;
        std::memset(&s, 0, sizeof(s));
        for (int f = 0; f < D::NF; f++)
          if (st[f])
          {
            s.mask |= 1u << f;
            set_force_ref(s, f, ms.support_force / (double)active); // src/mpc.cpp:149-167
          }
        s.land = s.mask & ~previous;
        previous = s.mask;
        for (int i = 0; i < D::NX; i++)
          s.x_tgt[i] = x_model_ref[i];
        cycle.push_back(s);
      }
    }
    // One control step for the whole batch; Xd: device pointer [B][NX]
    void iterate_device(const double * Xd) override
    {
      ref_rot.reset(); // (every control step rewrites every stage's reference pose with the identity rotation: src/mpc.cpp:303-309)
      if (cycle.empty())
        throw std::runtime_error("generateCycleHorizon must be called before iterate");
      recede_horizon(horizon, cycle, standing, D::NF);
      // setReferenceState(H-1, x_reference_) ; setVelocityBase(H-1, velocity_base_)  (src/mpc.cpp:311-312)
      for (int i = 0; i < D::NX; i++)
        horizon[H - 1].x_tgt[i] = x_reference[i];
      for (int i = 0; i < 6; i++)
        horizon[H - 1].x_tgt[D::NQ + i] = velocity_base[i];
      upload_stages();
      head = head + 1 == R ? 0 : head + 1; // replaceStageCircular + cycleProblem as a ring advance
      RecedeArgs<D> ra;
      ra.b = buf;
      ra.head = head;
      ra.X = Xd;
      for (int f = 0; f < D::NF; f++)
        ra.land[f] = timer.land[f].empty() ? -1 : timer.land[f][0];
      ra.T_fly = ms.T_fly;
      ra.T_contact = ms.T_contact;
      ra.swing_apex = ms.swing_apex;
      ra.timestep = ms.timestep;
      ra.shift = 1;
      ra.reg_init = REG_INIT;
      timed_launch<RecedeArgs<D>, recede_body<D>, 64>(KID_RECEDE, B, ra);
      if (!parts_enabled())
      {
        copy_centres(buf);
        run_iterations(buf, ms.max_iters);
        return;
      }
      // the parts of the batch run their iterations on streams of their own, between a fork and a join on the handle's stream
      Buffers<D> part[MAX_PARTS];
      for (int i = 0; i < n_parts; i++)
      {
        const int i0 = (int)((long long)B * i / n_parts), i1 = (int)((long long)B * (i + 1) / n_parts);
        part[i] = slice(buf, i0, i1 - i0, und_part[i]);
      }
      event_record(ev_fork, stream);
      issue_parts(part, ms.max_iters);
      for (int i = 1; i < n_parts; i++)
      {
        event_record(ev_join[i], part_stream[i]);
        stream_wait_event(stream, ev_join[i]);
      }
      cur = stream;
    }
    // the launches that follow go to the stream of part i, behind the fork; its first work are the AL centres of its instances
    void begin_part(const Buffers<D> & part, int i)
    {
      cur = part_stream[i];
      if (i > 0)
        stream_wait_event(cur, ev_fork);
      copy_centres(part);
    }
    // instances i0 .. i0 + n of every per-instance array (problems without optional constraint blocks)
    Buffers<D> slice(const Buffers<D> & b, int i0, int n, int * und) const
    {
      Buffers<D> s = b;
      s.B = n;
      const size_t o = (size_t)i0, Rs = (size_t)R, Hs = (size_t)H;
      auto adv = [&](double *& p, size_t per) {
        if (p)
          p += o * per;
      };
      adv(s.xs, Rs * D::NX); adv(s.us, Rs * D::NU); adv(s.vs, Rs * D::NC); adv(s.lams, Rs * D::NDX);
      adv(s.vs_e, Rs * D::NC); adv(s.lams_e, Rs * D::NDX);
      adv(s.xs_b, Rs * D::NX); adv(s.us_b, Rs * D::NU); adv(s.vs_b, Rs * D::NC); adv(s.lams_b, Rs * D::NDX);
      adv(s.dxs, (Hs + 1) * D::NDX); adv(s.dus, Hs * D::NU); adv(s.dvs, Hs * D::NC); adv(s.dlams, Hs * D::NDX);
      adv(s.foot_ref, Hs * D::NF * 3); adv(s.ftraj, (size_t)D::NF * 6); adv(s.vbase, 6); adv(s.vref, Rs * 6);
      s.ev_inst0 = b.ev_inst0 + i0;
      adv(s.lq, Hs * D::LQ_STRIDE); adv(s.gains, Hs * gains_stride()); // (lqc: one image for every part)
      adv(s.QN, (size_t)D::NDX * D::NDX); adv(s.qN, D::NDX);
      adv(s.parts0, (Hs + 1) * 4); adv(s.partsT, (size_t)D::LS_N * (Hs + 1) * 2); adv(s.scal, SC_N);
      adv(s.xdotT, (size_t)D::LS_N * 4 * D::NV); adv(s.xdot01, (size_t)4 * D::NV);
      adv(s.forcesT, Hs * D::LS_N * force_doubles()); adv(s.forces, Hs * force_doubles());
      s.ls_sel = b.ls_sel + i0;
      s.und_list = und;
      return s;
    }
    void iterate_host(const double * X) override
    {
      set_device(device_id);
      h2d(X_dev, X, (size_t)B * D::NX * sizeof(double), stream);
      iterate_device(X_dev);
      stream_sync(stream);
    }
    // xs[t] of every instance -> dense device buffer [B][NX], asynchronous on the engine's stream
    void gather_x_device(int t, double * out_dev) override
    {
      if (t < 0 || t > H)
        throw std::runtime_error("Stage index exceeds stage vector size");
      GatherArgs<D> ga;
      ga.b = buf;
      ga.head = head;
      ga.t = t;
      ga.out = out_dev;
      launch<GatherArgs<D>, gather_x_body<D>, 256>((int)(((size_t)B * D::NX + 255) / 256), stream, ga);
    }
    // ---- per-stage references of the horizon: the OCPHandler setters / getters (reference src/kinodynamics.cpp:154-306,
    //      src/ocp-handler.cpp:58-81), broadcast over the batch.  The next iterate() overwrites the foot references of
    //      every stage and the state target of stage H-1, exactly like MPC::updateStepTrackerReferences does. ----
    // what: 0 = control target (nu), 1 = state target (nx)
    void set_stage_reference(int t, int what, const double * v, int n) override
    {
      check_stage(t);
      if (what == 0)
      {
        if (n != D::NU)
          throw std::runtime_error("u_ref not of the right size");
        std::copy(v, v + n, horizon[t].u_ref);
      }
      else if (what == 1)
      {
        if (n != D::NX)
          throw std::runtime_error("x_ref not of the right size");
        std::copy(v, v + n, horizon[t].x_tgt);
        fill_strided(buf.vref + (size_t)ring_slot(head, t, R) * 6, (size_t)R * 6, B, v + D::NQ, 6); // velocity part is per instance
      }
      else
        throw std::runtime_error("unknown stage reference");
    }
    void get_stage_reference(int t, int what, double * v, int n) override
    {
      check_stage(t);
      if (what == 0 && n == D::NU)
        std::copy(horizon[t].u_ref, horizon[t].u_ref + n, v);
      else if (what == 1 && n == D::NX)
      {
        std::copy(horizon[t].x_tgt, horizon[t].x_tgt + n, v);
        get_linear(buf.vref + (size_t)ring_slot(head, t, R) * 6, 6, v + D::NQ); // instance 0
      }
      else
        throw std::runtime_error("unknown stage reference or wrong size");
    }
    void set_reference_pose(int t, int foot, const double * p3) override
    {
      check_stage(t);
      check_foot(foot);
      ref_rot.set(t, foot, nullptr); // (a translation: identity rotation)
      fill_strided(buf.foot_ref + ((size_t)t * D::NF + foot) * 3, (size_t)H * D::NF * 3, B, p3, 3);
    }
    void get_reference_pose(int t, int foot, int inst, double * p3) override
    {
      check_stage(t);
      if (foot < 0 || foot >= D::NF || inst < 0 || inst >= B)
        throw std::runtime_error("unknown end effector or instance");
      get_linear(buf.foot_ref + (((size_t)inst * H + t) * D::NF + foot) * 3, 3, p3);
    }
    unsigned contact_mask(int t) const override
    {
      check_stage(t);
      return horizon[t].mask;
    }

    // Everything a later iterate() depends on: iterate, multipliers, swing trajectories, references, velocity commands, gait
    // bookkeeping.  Not included: the feedback gains and the LQ knots of the last solve (recomputed by the next iterate).
    size_t state_io(StateIO & io) override
    {
      set_device(device_id);
      stream_sync(stream);
      io.tag(kind.state_tag, kind.state_name);
      io.tag(B, "batch");
      io.tag(H, "horizon");
      io.tag(D::NX, "nx");
      io.tag(D::NU, "nu");
      io.tag(buf.CN != nullptr ? 1 : 0, "terminal constraint");
      if (kind.kino)
      {
        io.tag(buf.es != nullptr ? 1 : 0, "friction-cone rows");
        io.tag(buf.ls != nullptr ? 1 : 0, "land rows");
      }
      io.pod(head);
      io.pod(walking);
      io.host(velocity_base, sizeof(velocity_base));
      io.vec(x_reference);
      io.vec(horizon);
      io.vec(cycle);
      io.timer(timer);
      const size_t BR = (size_t)B * R;
      auto arr = [&](double * p, size_t n) {
        if (p != nullptr)
          io.dev(p, n * sizeof(double));
      };
      arr(buf.xs, BR * D::NX);
      arr(buf.us, BR * D::NU);
      arr(buf.vs, BR * D::NC);
      arr(buf.lams, BR * D::NDX);
      arr(buf.ftraj, (size_t)B * D::NF * 6);
      arr(buf.foot_ref, (size_t)B * H * D::NF * 3);
      arr(buf.vbase, (size_t)B * 6);
      arr(buf.vref, BR * 6);
      arr(buf.scal, (size_t)B * SC_N);
      arr(buf.xdot01, (size_t)B * 4 * D::NV);
      arr(buf.forces, (size_t)B * H * force_doubles());
      arr(buf.vN, (size_t)B * 3);
      arr(buf.es, BR * 2 * D::NF);
      arr(buf.ls, BR * D::NF);
      if (io.mode == StateIO::LOAD)
        upload_stages();
      stream_sync(stream);
      return io.pos;
    }

    // interpolated whole-body targets at `delay` after the last solve into device buffers (the inverse-dynamics engine's target buffers),
    // asynchronous on this engine's stream
    void check_interp(int knots, double delay) const
    {
      if (knots < 2 || knots > H + 1)
        throw std::runtime_error("interpolate: knots must be in [2, horizon + 1]");
      if (!(delay >= 0.0))
        throw std::runtime_error("interpolate: delay must be non-negative");
    }
    void interpolate_device(double delay, int knots, double * x_dev, double * acc_dev, double * f_dev) override
    {
      check_interp(knots, delay);
      set_device(device_id);
      launch_interp(knots, delay, x_dev, acc_dev, f_dev, nullptr);
    }
    // the same to the host; any output may be null
    void interpolate(double delay, int knots, double * x_out, double * acc_out, double * f_out) override
    {
      check_interp(knots, delay);
      const size_t nx = (size_t)B * D::NX, na = (size_t)B * D::NV, nf = (size_t)B * force_doubles();
      double * st = staging((nx + na + nf) * sizeof(double));
      launch_interp(knots, delay, x_out ? st : nullptr, acc_out ? st + nx : nullptr, f_out ? st + nx + na : nullptr, nullptr);
      if (x_out)
        d2h(x_out, st, nx * sizeof(double), stream);
      if (acc_out)
        d2h(acc_out, st + nx, na * sizeof(double), stream);
      if (f_out)
        d2h(f_out, st + nx + na, nf * sizeof(double), stream);
      stream_sync(stream);
    }
    // u = u_interp - K_0 (x_interp (-) x_meas) at `delay` after the last solve, for measured states X [B][NX] (host)
    // (reference examples/go2_fulldynamics.py:271-285)
    void riccati_feedback(double delay, const double * X, double * u_out) override
    {
      if (!(delay >= 0.0))
        throw std::runtime_error("riccati_feedback: delay must be non-negative");
      const size_t nx = (size_t)B * D::NX, nu = (size_t)B * D::NU, nk = (size_t)B * D::NU * D::NDX;
      double * st = staging((nx + 2 * nu + nk) * sizeof(double));
      double *xi = st, *ui = st + nx, *uo = ui + nu, *k0 = uo + nu;
      h2d(X_dev, X, nx * sizeof(double), stream);
      launch_interp(2, delay, xi, nullptr, nullptr, ui);
      launch_gains_out(1, k0);
      FeedbackArgs<D> fa;
      fa.b = buf;
      fa.X_meas = X_dev;
      fa.x_interp = xi;
      fa.u_interp = ui;
      fa.K0 = k0;
      fa.u_out = uo;
      launch<FeedbackArgs<D>, feedback_body<D>, 64>(B, stream, fa);
      d2h(u_out, uo, nu * sizeof(double), stream);
      stream_sync(stream);
    }
    // state feedback front-end on measured states X [B][nq + nv] (host): feet [B][NF][3], com [B][3], hg [B][6], centroidal state [B][9]
    // (host outputs, any may be null) -- RobotDataHandler::updateInternalData + getCentroidalState on the stage kernel's kinematics
    void update_internal_data(const double * X, double * feet, double * com, double * hg, double * cstate) override
    {
      set_device(device_id);
      const size_t nf = (size_t)B * D::NF * 3, nc = (size_t)B * 3, nh = (size_t)B * 6, ns = (size_t)B * 9;
      double * st = staging((nf + nc + nh + ns) * sizeof(double));
      h2d(X_dev, X, (size_t)B * D::NX * sizeof(double), stream);
      FrontendArgs<D> fa;
      fa.b = buf;
      fa.X = X_dev;
      fa.feet = feet ? st : nullptr;
      fa.com = com ? st + nf : nullptr;
      fa.hg = hg ? st + nf + nc : nullptr;
      fa.cstate = cstate ? st + nf + nc + nh : nullptr;
      launch_frontend(fa);
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
    // constrained forward dynamics of n states (host buffers): a [n][NV], lam [n][force_size NF] (feet in contact first); iters [n] and
    // kernel_ms may be null
    void full_forward_dynamics(int n, const double * X, const double * tau, const unsigned * mask, const double * Kp, const double * Kd, double prox_accuracy,
                               double prox_mu, int prox_max_iter, double * a, double * lam, int * iters, double * kernel_ms) override
    {
      require_forward_dynamics("full_forward_dynamics");
      if (n < 1)
        throw std::runtime_error("full_forward_dynamics: n must be positive");
      set_device(device_id);
      constexpr int NV = D::NV, NX = D::NX;
      const int NCM = force_doubles();
      // staging layout (doubles): X | tau | a | lam | mask (unsigned) | iters (int)
      const size_t oX = 0, oT = oX + (size_t)n * NX, oA = oT + (size_t)n * (NV - 6), oL = oA + (size_t)n * NV, oM = oL + (size_t)n * NCM,
                   oI = oM + ((size_t)n + 1) / 2, total = oI + ((size_t)n + 1) / 2;
      double * st = staging(total * sizeof(double));
      h2d(st + oX, X, (size_t)n * NX * sizeof(double), stream);
      h2d(st + oT, tau, (size_t)n * (NV - 6) * sizeof(double), stream);
      h2d(st + oM, mask, (size_t)n * sizeof(unsigned), stream);
      stream_sync(stream);
      const auto t0 = std::chrono::steady_clock::now();
      // ProximalSettings(1e-9, 1e-10, 10), src/fulldynamics.cpp:39
      launch_forward_dynamics(n, st + oX, st + oT, reinterpret_cast<const unsigned *>(st + oM), Kp, Kd, prox_accuracy > 0 ? prox_accuracy : 1e-9,
                              prox_mu > 0 ? prox_mu : 1e-10, prox_max_iter > 0 ? prox_max_iter : 10, st + oA, st + oL, reinterpret_cast<int *>(st + oI));
      stream_sync(stream);
      if (kernel_ms)
        *kernel_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      d2h(a, st + oA, (size_t)n * NV * sizeof(double), stream);
      d2h(lam, st + oL, (size_t)n * NCM * sizeof(double), stream);
      if (iters)
        d2h(iters, st + oI, (size_t)n * sizeof(int), stream);
      stream_sync(stream);
    }
    // One step of a simulated batch with states and torques resident in HBM (what the reference's examples do with a physics engine
    // between two controller ticks): constrained forward dynamics of the feet in `mask` (Baumgarte gains Kp, Kd; proximal settings of
    // record), then semi-implicit Euler over dt, X updated in place.  Asynchronous on this engine's stream.
    void sim_step_device(double * X, const double * tau_dev, unsigned mask, const double * Kp, const double * Kd, double dt) override
    {
      require_forward_dynamics("sim_step_device");
      set_device(device_id);
      if (!sim_a)
      {
        sim_a = (double *)dev_alloc((size_t)B * D::NV * sizeof(double));
        sim_lam = (double *)dev_alloc((size_t)B * force_doubles() * sizeof(double));
        sim_mask = (unsigned *)dev_alloc((size_t)B * sizeof(unsigned));
      }
      if (mask != sim_mask_value)
      {
        std::vector<unsigned> m(B, mask);
        h2d(sim_mask, m.data(), m.size() * sizeof(unsigned), stream);
        stream_sync(stream); // (m goes out of scope)
        sim_mask_value = mask;
      }
      launch_forward_dynamics(B, X, tau_dev, sim_mask, Kp, Kd, 1e-9, 1e-10, 10, sim_a, sim_lam, nullptr);
      SimStepArgs<D> sa;
      sa.X = X;
      sa.a = sim_a;
      sa.dt = dt;
      launch_sim_integrate(sa);
    }

    // K_t of every stage [B][H][NU][NDX] or only K_0 [B][NU][NDX], expanded on the device
    virtual void get_K(double * out, bool all)
    {
      stream_sync(stream);
      const int nt = all ? H : 1;
      const size_t n = (size_t)B * nt * D::NU * D::NDX;
      double * dev = staging(n * sizeof(double));
      launch_gains_out(nt, dev);
      d2h(out, dev, n * sizeof(double), stream);
      stream_sync(stream);
    }
    void get_output(Output what, double * out) override
    {
      switch (what)
      {
      case OUT_XS:
        return get_ring(buf.xs, D::NX, H + 1, out);
      case OUT_US:
        return get_ring(buf.us, D::NU, H, out);
      case OUT_K0:
        return get_K(out, false);
      case OUT_KS:
        return get_K(out, true);
      case OUT_VS:
        return get_ring(buf.vs, D::NC, H, out);
      case OUT_LAMS:
        return get_lams(buf.lams, D::NDX, out);
      case OUT_XDOT01:
        return get_linear(buf.xdot01, (size_t)B * 4 * D::NV, out);
      case OUT_FOOT_REFS:
        return get_linear(buf.foot_ref, (size_t)B * H * D::NF * 3, out);
      case OUT_INFO:
        return get_linear(buf.scal, (size_t)B * SC_N, out);
      case OUT_CONTACT_FORCES:
        if (!buf.forces)
          throw InvalidCall("smpc_get_contact_forces needs a full-dynamics handle (the other problems carry the forces in us)");
        return get_linear(buf.forces, (size_t)B * H * force_doubles(), out);
      }
      throw std::runtime_error("unknown output");
    }
    void debug_steps(double * dxs, double * dus) override
    {
      get_linear(buf.dxs, (size_t)B * (H + 1) * D::NDX, dxs);
      get_linear(buf.dus, (size_t)B * H * D::NU, dus);
    }
    void debug_terminal(int inst, double * QN, double * qN) override
    {
      if (inst < 0 || inst >= B)
        refuse("instance index out of range");
      get_linear(buf.QN + (size_t)inst * D::NDX * D::NDX, D::NDX * D::NDX, QN);
      get_linear(buf.qN + (size_t)inst * D::NDX, D::NDX, qN);
    }
    void phase_cycles(double * out64) override
    {
      if (!buf.dbg)
        refuse(std::string("phase timers are off (set SMPC_PHASE_PROFILE=1 before ") + kind.create_fn + ")");
      get_linear(buf.dbg, 64, out64);
    }
  };
} // namespace smpc
