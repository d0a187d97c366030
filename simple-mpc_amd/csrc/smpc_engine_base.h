// smpc_engine_base.h -- the one host interface behind smpc_handle (smpc_capi.cpp): what the kinodynamics, full-dynamics and centroidal
// engines share as data and as host code, and the virtual entry points the C ABI calls.  No kernel lives here.
#pragma once
#include "smpc_solver_kernels.h"
#include "smpc_reset.h"
#include "smpc_reset_mask.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace smpc
{
  struct HostMpcSettings
  {
    double swing_apex, support_force, TOL, mu_init, timestep;
    int max_iters, num_threads, T_fly, T_contact, T;
  };

  // integer gait bookkeeping (reference src/mpc.cpp:101-132, 220-276)
  struct GaitTimer
  {
    int H = 0, nf = 0;
    std::vector<std::vector<unsigned char>> states;
    std::vector<std::vector<int>> takeoff, land;
    void generate(const unsigned char * cs, int n, int nf_, int H_)
    {
      H = H_;
      nf = nf_;
      states.clear();
      const int reps = 1 + H / n; // original + m copies, m = H / n (integer division)
      for (int r = 0; r < reps; r++)
        for (int i = 0; i < n; i++)
          states.emplace_back(cs + (size_t)i * nf, cs + (size_t)(i + 1) * nf);
      takeoff.assign(nf, {});
      land.assign(nf, {});
      const int N = (int)states.size();
      for (int f = 0; f < nf; f++)
      {
        for (int i = 1; i < N; i++)
        {
          const bool now = states[i][f], prev = states[i - 1][f];
          if (!now && prev)
            takeoff[f].push_back(i + H);
          if (now && !prev)
            land[f].push_back(i + H);
        }
        if (states[N - 1][f] && !states[0][f])
          takeoff[f].push_back(N - 1 + H);
        if (!states[N - 1][f] && states[0][f])
          land[f].push_back(N - 1 + H);
      }
    }
    void update_timing(bool only_horizon)
    {
      for (int f = 0; f < nf; f++)
      {
        for (auto * v : {&land[f], &takeoff[f]})
        {
          for (int & t : *v)
            if (!only_horizon || t < H)
              t -= 1;
          if (!v->empty() && (*v)[0] < 0)
            v->erase(v->begin());
        }
      }
    }
    void recede_cycle()
    {
      std::rotate(states.begin(), states.begin() + 1, states.end());
      const int N = (int)states.size();
      for (int f = 0; f < nf; f++)
      {
        if (!states[N - 1][f] && states[N - 2][f])
          takeoff[f].push_back(N + H);
        if (states[N - 1][f] && !states[N - 2][f])
          land[f].push_back(N + H);
      }
      update_timing(false);
    }
  };

  enum KernelId
  {
    KID_RECEDE = 0,
    KID_DERIV,
    KID_RICCATI,
    KID_FORWARD,
    KID_TRIAL,
    KID_SELECT,
    KID_APPLY,
    KID_TREE,    // lane-per-problem tree pass (smpc_kino_lane.h) of the full-batch derivative launches
    KID_TREE_LS, // ... of the full-batch line-search launches (evaluation mode: heads only)
    KID_N
  };

  // checkpoint / resume of a handle (smpc_save_state / smpc_load_state): one pass over the state in a fixed order, in one
  // of three modes (count the bytes, copy out, copy in)
  struct StateIO
  {
    enum Mode
    {
      COUNT,
      SAVE,
      LOAD
    } mode;
    char * buf;
    size_t cap, pos = 0;
    stream_t st;
    StateIO(Mode m, void * b, size_t c, stream_t s) : mode(m), buf((char *)b), cap(c), st(s) {}
    void need(size_t n) const
    {
      if (mode != COUNT && pos + n > cap)
        throw std::runtime_error(mode == SAVE ? "state buffer too small" : "state buffer truncated");
    }
    void host(void * p, size_t n)
    {
      need(n);
      if (mode == SAVE)
        std::memcpy(buf + pos, p, n);
      else if (mode == LOAD)
        std::memcpy(p, buf + pos, n);
      pos += n;
    }
    void dev(void * p, size_t n)
    {
      need(n);
      if (mode == SAVE)
        d2h(buf + pos, p, n, st);
      else if (mode == LOAD)
        h2d(p, buf + pos, n, st);
      pos += n;
    }
    template <class T>
    void pod(T & v)
    {
      host(&v, sizeof(T));
    }
    // a value that must be the same in the handle and in the buffer (shape of the problem)
    void tag(long long v, const char * what)
    {
      long long w = v;
      pod(w);
      if (mode == LOAD && w != v)
        throw std::runtime_error(std::string("saved state does not match this handle: ") + what);
    }
    template <class T>
    void vec(std::vector<T> & v)
    {
      unsigned long long n = v.size();
      pod(n);
      if (mode == LOAD)
      {
        if (n * sizeof(T) > cap)
          throw std::runtime_error("state buffer corrupt");
        v.resize((size_t)n);
      }
      if (n)
        host(v.data(), (size_t)n * sizeof(T));
    }
    void timer(GaitTimer & t)
    {
      pod(t.H);
      pod(t.nf);
      unsigned long long ns = t.states.size();
      pod(ns);
      if (mode == LOAD)
        t.states.assign((size_t)ns, std::vector<unsigned char>());
      for (auto & s : t.states)
        vec(s);
      if (mode == LOAD)
      {
        t.takeoff.assign(t.nf, {});
        t.land.assign(t.nf, {});
      }
      for (int f = 0; f < t.nf; f++)
      {
        vec(t.takeoff[f]);
        vec(t.land[f]);
      }
    }
  };

  // an entry point answers SMPC_ERR_INVALID with this text: the handle's kind has no such operation, or an index is out of its range
  struct InvalidCall : std::runtime_error
  {
    using std::runtime_error::runtime_error;
  };
  constexpr const char * KINO_ONLY = "this entry point needs a kinodynamics handle (smpc_create)";

  enum Output // MpcEngineBase::get_output
  {
    OUT_XS = 0,
    OUT_US,
    OUT_K0,
    OUT_KS,
    OUT_VS,
    OUT_LAMS,
    OUT_XDOT01,
    OUT_FOOT_REFS,
    OUT_INFO,
    OUT_CONTACT_FORCES
  };

  // streams and events an engine creates beside its own stream (parts of the batch): released with the engine, also when its constructor throws
  struct SideQueues
  {
    std::vector<stream_t> streams;
    std::vector<event_t> events;
    stream_t stream()
    {
      streams.push_back(stream_create());
      return streams.back();
    }
    event_t event()
    {
      events.push_back(event_create());
      return events.back();
    }
    SideQueues() = default;
    SideQueues(const SideQueues &) = delete;
    SideQueues & operator=(const SideQueues &) = delete;
    ~SideQueues()
    {
      for (event_t e : events)
        event_destroy(e);
      for (stream_t s : streams)
        stream_destroy(s);
    }
  };

  class MpcEngineBase
  {
  public:
    int B, H, R, head = 0;
    int device_id; // every entry point makes this the current device first: a process may hold handles on several GPUs
    int dims[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // nq nv nx ndx nu nc nf H (smpc_get_dims)
    int force_size = 3;
    stream_t stream{};
    stream_t cur{}; // stream of the launches being issued (an engine that runs parts of the batch on streams of their own moves it)
    SideQueues side;
    GaitTimer timer;
    HostMpcSettings ms;
    bool walking = true;
    double velocity_base[6] = {0, 0, 0, 0, 0, 0};
    double * vbase_dev = nullptr; // the engine's velocity commands [B][6] (owned by its buffers)
    std::vector<double> x_reference, x_model_ref;
    bool early_exit_on_tol = false; // smpc_set_early_exit_on_tol: iterate() stops an instance's iterations once it is converged to TOL
    bool aux_launches = false;      // true during the cold start: every launch uses the auxiliary kernel symbols
    bool profiling = false;
    double kernel_ms[KID_N] = {0}; // (a centroidal handle fills its CentKernelId slots, the others stay 0)
    long kernel_calls[KID_N] = {0};
    std::vector<std::pair<int, std::pair<event_t, event_t>>> pending_events;
    int cold_iters = 0;
    std::vector<double> cold_trace; // [n][4] phi0, prim, dual, alpha
    RefRotations ref_rot;           // rotations of the foot reference placements: API state (smpc_model.h)
    double * stage_out = nullptr;   // staging for linearised outputs
    size_t stage_out_bytes = 0;
    event_t ev_handoff{};
    bool ev_handoff_valid = false;
    ColdSolution cold; // one instance's copy of the constructor's cold solve (smpc_reset.h); its block is released with the engine's buffers
    unsigned char * reset_mask_dev = nullptr; // [B] mask of reset_instances (the host-list form), allocated on first use
    UploadRing reset_mask_ring;

    MpcEngineBase(const HostMpcSettings & ms_, int batch, int device) : B(batch), H(ms_.T), R(ms_.T + 1), device_id(device), ms(ms_) {}
    MpcEngineBase(const MpcEngineBase &) = delete;
    MpcEngineBase & operator=(const MpcEngineBase &) = delete;
    // the base releases what it owns (also after a derived constructor has thrown); a derived destructor releases what that engine created
    virtual ~MpcEngineBase()
    {
      dev_free(stage_out);
      dev_free(reset_mask_dev);
      if (ev_handoff_valid)
        event_destroy(ev_handoff);
      if (stream_open)
        stream_destroy(stream);
    }
    // (called by the derived constructor once its arguments are checked)
    void open_stream()
    {
      set_device(device_id);
      stream = stream_create();
      stream_open = true;
      cur = stream;
    }

    // aux: auxiliary launch (cold start on one instance, list-mode launch of the backtracking path): same code under a
    // second kernel symbol, so that profiler averages of the main symbol are those of full-batch launches
    template <class Args, void (*Body)(const Args &, int), int NT, int MINW = 1>
    void timed_launch(int kid, int grid, const Args & a, bool aux = false, const stream_t * on = nullptr)
    {
      set_device(device_id);
      aux = aux || aux_launches;
      const stream_t st = on ? *on : cur;
      event_t e0{}, e1{};
      if (profiling)
      {
        e0 = event_create();
        e1 = event_create();
        event_record(e0, st);
      }
      if (aux)
        launch<Args, Body, NT, MINW, 1>(grid, st, a);
      else
        launch<Args, Body, NT, MINW, 0>(grid, st, a);
      if (profiling)
      {
        event_record(e1, st);
        pending_events.push_back({kid, {e0, e1}});
      }
      kernel_calls[kid]++;
    }
    void collect_profile()
    {
      stream_sync(stream);
      for (auto & pe : pending_events)
      {
        kernel_ms[pe.first] += event_elapsed_ms(pe.second.first, pe.second.second);
        event_destroy(pe.second.first);
        event_destroy(pe.second.second);
      }
      pending_events.clear();
    }
    void reset_profile()
    {
      collect_profile();
      for (int i = 0; i < KID_N; i++)
      {
        kernel_ms[i] = 0;
        kernel_calls[i] = 0;
      }
    }

    void sync()
    {
      set_device(device_id);
      stream_sync(stream);
    }
    // work issued on `other` from now on starts after what this engine's stream holds now
    void wait_stream(stream_t other)
    {
      set_device(device_id);
      if (!ev_handoff_valid)
      {
        ev_handoff = event_create();
        ev_handoff_valid = true;
      }
      event_record(ev_handoff, stream);
      stream_wait_event(other, ev_handoff);
    }
    double * staging(size_t bytes)
    {
      set_device(device_id);
      if (bytes > stage_out_bytes)
      {
        stream_sync(stream); // (nothing queued reads the block that goes)
        dev_free(stage_out);
        stage_out = nullptr;
        stage_out_bytes = 0;
        stage_out = (double *)dev_alloc(bytes);
        stage_out_bytes = bytes;
      }
      return stage_out;
    }
    // ring array [B][R][n] -> host linear [B][count][n] for t = 0..count-1
    void get_ring(const double * src, int n, int count, double * out)
    {
      set_device(device_id);
      stream_sync(stream);
      std::vector<double> tmp((size_t)B * R * n);
      d2h(tmp.data(), src, tmp.size() * sizeof(double), stream);
      stream_sync(stream);
      for (int b = 0; b < B; b++)
        for (int t = 0; t < count; t++)
          std::memcpy(out + ((size_t)b * count + t) * n, tmp.data() + ((size_t)b * R + ring_slot(head, t, R)) * n, n * sizeof(double));
    }
    void get_linear(const double * src, size_t n, double * out)
    {
      set_device(device_id);
      stream_sync(stream);
      d2h(out, src, n * sizeof(double), stream);
      stream_sync(stream);
    }
    // device arrays hold lambda_{t+1} at stage t; the API returns lams[0..H] with lams[0] = 0
    void get_lams(const double * src, int n, double * out)
    {
      std::vector<double> tmp((size_t)B * H * n);
      get_ring(src, n, H, tmp.data());
      for (int b = 0; b < B; b++)
      {
        double * o = out + (size_t)b * (H + 1) * n;
        std::memset(o, 0, n * sizeof(double));
        std::memcpy(o + n, tmp.data() + (size_t)b * H * n, (size_t)H * n * sizeof(double));
      }
    }
    void check_stage(int t) const
    {
      if (t < 0 || t >= H)
        throw std::runtime_error("Stage index exceeds stage vector size");
    }
    void check_foot(int foot) const
    {
      if (foot < 0 || foot >= dims[6])
        throw std::runtime_error("unknown end effector");
    }
    void fill_strided(double * base, size_t stride, int count, const double * v, int n)
    {
      set_device(device_id);
      FillStridedArgs fa;
      fa.base = base;
      fa.stride = stride;
      fa.count = count;
      fa.n = n;
      for (int i = 0; i < n; i++)
        fa.v[i] = v[i];
      launch<FillStridedArgs, fill_strided_body, 64>((count + 63) / 64, stream, fa);
      stream_sync(stream);
    }
    void set_reference_rotation(int t, int foot, const double * R9)
    {
      check_stage(t);
      check_foot(foot);
      ref_rot.set(t, foot, R9);
    }
    void get_reference_rotation(int t, int foot, double * R9)
    {
      check_stage(t);
      check_foot(foot);
      ref_rot.get(t, foot, R9);
    }
    // velocity commands live on the device, one per instance; the reference's single velocity_base_ is a broadcast
    void upload_velocity(double * vbase, const double * V, bool broadcast)
    {
      set_device(device_id);
      std::vector<double> h((size_t)B * 6);
      for (int b = 0; b < B; b++)
        for (int i = 0; i < 6; i++)
          h[(size_t)b * 6 + i] = broadcast ? V[i] : V[(size_t)b * 6 + i];
      h2d(vbase, h.data(), h.size() * sizeof(double), stream);
      stream_sync(stream);
    }
    void switch_to_walk(const double * v6)
    {
      walking = true;
      for (int i = 0; i < 6; i++)
        velocity_base[i] = v6[i];
      upload_velocity(vbase_dev, v6, true);
    }
    void switch_to_stand()
    {
      walking = false;
      for (int i = 0; i < 6; i++)
        velocity_base[i] = 0.0;
      upload_velocity(vbase_dev, velocity_base, true);
    }
    // one velocity command per instance, V: [B][6] (the walking state is unchanged, like assigning MPC::velocity_base_)
    void set_velocity_base_batched(const double * V)
    {
      for (int i = 0; i < 6; i++)
        velocity_base[i] = V[i];
      upload_velocity(vbase_dev, V, false);
    }

    // ---- reset of single instances to the cold start (re-applies what the constructor did, reference src/mpc.cpp:72-89) ----
    // the solver state of the instances with a non-zero byte in mask_dev [B] (device) becomes what the constructor left, relative to the
    // current ring head; the problem data stay.  One launch on the handle's stream, no host synchronisation.
    void launch_reset(const unsigned char * mask_dev, int * ls_sel = nullptr, int ls_sel0 = 0)
    {
      set_device(device_id);
      ResetArgs a = cold.plan;
      a.mask = mask_dev;
      a.head = head;
      a.ls_sel = ls_sel;
      a.ls_sel0 = ls_sel0;
      launch<ResetArgs, reset_body, 64>(B * R, stream, a);
    }
    // the same for a host list of instances (unsorted, duplicates allowed): mask built here, uploaded on the stream
    void reset_instances(const int * idx, int n)
    {
      if (n < 0)
        throw InvalidCall("smpc_reset_instances: negative count");
      if (n == 0)
        return;
      std::vector<unsigned char> m((size_t)B);
      if (reset_mask_from_list(idx, n, B, m.data()) >= 0)
        throw InvalidCall("smpc_reset_instances: instance index out of range");
      set_device(device_id);
      if (!reset_mask_dev)
        reset_mask_dev = (unsigned char *)dev_alloc((size_t)B);
      reset_mask_ring.upload(reset_mask_dev, m.data(), (size_t)B, stream); // (pinned staging: the caller's queue is not drained)
      reset_instances_device(reset_mask_dev);
    }

    // MPC::recedeWithCycle on the host, shared by the batch (src/mpc.cpp:220-254): the stage that enters the horizon is the next one of the
    // cycle while walking -- or until every foot of the last stage is in support --, the standing stage after that
    template <class Stage>
    void recede_horizon(std::vector<Stage> & horizon, std::vector<Stage> & cycle, const Stage & standing, int nf)
    {
      int last_support = 0;
      for (int f = 0; f < nf; f++)
        last_support += (horizon[H - 1].mask >> f) & 1u;
      Stage incoming;
      if (walking || last_support < nf)
      {
        incoming = cycle[0];
        std::rotate(cycle.begin(), cycle.begin() + 1, cycle.end());
        timer.recede_cycle();
      }
      else
      {
        incoming = standing;
        timer.update_timing(true);
      }
      horizon.erase(horizon.begin());
      horizon.push_back(incoming);
    }

    // ---- what differs per problem ----
    virtual void generate_cycle_horizon(const unsigned char * cs, int n) = 0;
    virtual void iterate_device(const double * Xd) = 0; // one control step for the whole batch; Xd: device pointer [B][nq + nv]
    virtual void iterate_host(const double * X) = 0;
    virtual void iterate_host_async(const double * X) { iterate_host(X); } // (synchronous unless the engine says otherwise)
    virtual void set_stage_reference(int t, int what, const double * v, int n) = 0;
    virtual void get_stage_reference(int t, int what, double * v, int n) = 0;
    virtual void set_reference_pose(int t, int foot, const double * p3) = 0;
    virtual void get_reference_pose(int t, int foot, int inst, double * p3) = 0;
    virtual unsigned contact_mask(int t) const = 0;
    virtual void update_internal_data(const double * X, double * feet, double * com, double * hg, double * cstate) = 0;
    virtual void interpolate(double delay, int knots, double * x_out, double * acc_out, double * f_out) = 0;
    virtual void riccati_feedback(double delay, const double * X, double * u_out) = 0;
    virtual size_t state_io(StateIO & io) = 0;
    virtual void state_derivatives(double * out) = 0; // xdot of every stage at the last solve's iterate, [B][H][xdot_doubles() / (B H)] (device, handle's stream)
    virtual size_t xdot_doubles() const { return (size_t)B * H * 2 * dims[1]; }
    virtual void get_output(Output what, double * out) = 0;
    virtual void reset_instances_device(const uint8_t * mask_dev) = 0; // smpc_reset_instances_device
    virtual void debug_steps(double * dxs, double * dus) = 0;

    // ---- what only some handle kinds have: the others answer SMPC_ERR_INVALID with the text below ----
    virtual bool centroidal() const { return false; } // feeds a CentroidalID controller (interpolate_device_id), not a KinodynamicsID one (interpolate_device)
    virtual void interpolate_device(double, int, double *, double *, double *) { throw InvalidCall("a centroidal MPC handle feeds a CentroidalID controller"); }
    virtual void interpolate_device_id(double, int, double *, double *, double *, double *, double *)
    {
      throw InvalidCall("a kinodynamics MPC handle feeds a KinodynamicsID controller");
    }
    virtual void gather_outputs_async(double *, size_t) { throw InvalidCall(KINO_ONLY); }
    virtual void gather_outputs_device(double *, size_t) { throw InvalidCall(KINO_ONLY); }
    virtual void gather_outputs_peer(double *, int) { throw InvalidCall(KINO_ONLY); }
    virtual void gather_x_device(int, double *) { throw InvalidCall(KINO_ONLY); }
    virtual void get_extra_multipliers(int, double *) { throw InvalidCall("kinodynamics handles only"); }
    virtual void set_early_exit(bool on) { early_exit_on_tol = on; }
    virtual int lq_size() const { return 0; } // doubles of what debug_lq returns (0: no knots to return)
    virtual void debug_lq(int, int, double *) { throw InvalidCall(KINO_ONLY); }
    virtual void debug_terminal(int, double *, double *) { throw InvalidCall(KINO_ONLY); }
    virtual void debug_dual_steps(double *, double *) { throw InvalidCall("smpc_debug_get_dual_steps needs a centroidal handle (smpc_create_centroidal)"); }
    virtual void phase_cycles(double * out64) = 0;
    virtual void debug_frontend_rt(const double *, double *, double *, double *, double *)
    {
      throw InvalidCall("smpc_debug_frontend_rt needs a centroidal handle (smpc_create_centroidal)");
    }
    virtual void full_forward_dynamics(int, const double *, const double *, const unsigned *, const double *, const double *, double, double, int, double *,
                                       double *, int *, double *)
    {
      throw InvalidCall("smpc_full_forward_dynamics needs a kinodynamics or a full-dynamics handle (they carry the multibody model)");
    }
    virtual void sim_step_device(double *, const double *, unsigned, const double *, const double *, double)
    {
      throw InvalidCall("smpc_sim_step_device needs a kinodynamics or a full-dynamics handle (they carry the multibody model)");
    }

  private:
    bool stream_open = false;
  };
} // namespace smpc
