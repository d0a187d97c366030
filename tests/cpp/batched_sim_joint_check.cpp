// The joint model of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setJointModel, lastAppliedTorques, lastJointStops,
// jointModelDevicePointers, groundJointDynamics) on the built-in quadruped: the mirror against the C ABI bit for bit, the inert model against
// groundSolveDynamics bit for bit, then 150 steps of free fall with a constant torque that drives one knee into its upper stop (the torque
// clipped, the stop loaded, the joint held), and the refusals.  "Device" memory: plain host memory for the sequential-lane test build,
// hipMalloc'ed memory for the HIP library (SMPC_CHECK_HIP).
#include "simple-mpc/batched-sim.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#ifdef SMPC_CHECK_HIP
#include <hip/hip_runtime.h>
#endif

#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);                                                      \
      return 1;                                                                                                        \
    }                                                                                                                  \
  } while (0)

template <class F>
static std::string refusal(F && f)
{
  try
  {
    f();
  }
  catch (const std::runtime_error & e)
  {
    return e.what();
  }
  return std::string();
}

// a buffer the simulator's stream can reach
struct DeviceBuffer
{
  double * p = nullptr;
  size_t n;
  explicit DeviceBuffer(const std::vector<double> & v) : n(v.size())
  {
#ifdef SMPC_CHECK_HIP
    if (hipMalloc((void **)&p, n * sizeof(double)) != hipSuccess || hipMemcpy(p, v.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("device buffer");
#else
    p = new double[n];
    std::memcpy(p, v.data(), n * sizeof(double));
#endif
  }
  std::vector<double> get() const
  {
    std::vector<double> v(n);
#ifdef SMPC_CHECK_HIP
    if (hipMemcpy(v.data(), p, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("device buffer");
#else
    std::memcpy(v.data(), p, n * sizeof(double));
#endif
    return v;
  }
  ~DeviceBuffer()
  {
#ifdef SMPC_CHECK_HIP
    (void)hipFree(p);
#else
    delete[] p;
#endif
  }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer & operator=(const DeviceBuffer &) = delete;
};

int main()
{
  const smpc_robot_model * robot = smpc_builtin_robot("go2_like");
  CHECK(robot != nullptr);
  const int B = 2, NJ = SMPC_JOINT_MAX_STOPS, knee = 2;
  const double dt = 1e-3;
  simple_mpc::BatchedRobotSim sim(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv, na = nv - 6;
  typedef simple_mpc::BatchedRobotSim::JointModel JM;
  typedef simple_mpc::BatchedRobotSim::GroundJoint GJ;
  typedef simple_mpc::BatchedRobotSim::GroundSolve GS;
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * na, 0.0);
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
    for (int k = 0; k < na; k++)
      tau[(size_t)i * na + k] = (k % 2 ? -1.0 : 1.0) * (2.0 + k + 3 * i);
  }
  // before setGround
  CHECK(refusal([&] { sim.setJointModel(JM()); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.lastAppliedTorques(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.lastJointStops(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  // the plane 10 m under the reference pose: the robot falls freely
  smpc_ground_settings gs;
  std::memset(&gs, 0, sizeof(gs));
  gs.ground_z = -10.0;
  sim.setGround(gs);
  // before the setter: null pointers and zeros
  {
    double *t = (double *)1, *l = (double *)1;
    int32_t *r = (int32_t *)1, *d = (int32_t *)1;
    sim.jointModelDevicePointers(&t, &r, &l, &d);
    CHECK(t == nullptr && r == nullptr && l == nullptr && d == nullptr);
    for (double v : sim.lastAppliedTorques())
      CHECK(v == 0.0);
    for (int32_t v : sim.lastJointStops().stop_rows)
      CHECK(v == 0);
  }
  // robot 1: the knee 0.01 rad beyond its upper limit and moving on; a hip 0.02 rad inside its lower limit
  X[(size_t)nx + 7 + knee] = robot->q_hi[knee] + 0.01;
  X[(size_t)nx + nq + 6 + knee] = 2.0;
  X[(size_t)nx + 7 + 3] = robot->q_lo[3] + 0.02;
  JM model;
  model.tau_max.assign((size_t)B * na, 6.0);
  model.tau_max[0] = INFINITY;
  model.damping.assign(na, 0.1);
  model.armature.assign(na, 0.01);
  model.stops = true;
  // the host-buffer solve: the mirror against the C ABI, bit for bit
  {
    const GJ r = sim.groundJointDynamics(X, tau, dt, model);
    std::vector<double> dmp((size_t)B * na, 0.1), arm((size_t)B * na, 0.01);
    const smpc_joint_model_settings m = {model.tau_max.data(), dmp.data(), arm.data(), nullptr, nullptr, 1, 1, 0.0, 0.0};
    std::vector<double> v((size_t)B * nv), a((size_t)B * nv), lam((size_t)B * 12), lamc((size_t)B * 12), gap((size_t)B * 4), res(B), ta((size_t)B * na),
        ls((size_t)B * NJ);
    std::vector<uint32_t> con(B);
    std::vector<int32_t> sw(B), rows((size_t)B * NJ), dr(B);
    CHECK(smpc_robot_sim_ground_joint_dynamics(sim.handle(), B, X.data(), tau.data(), dt, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &m, v.data(), a.data(),
                                               lam.data(), lamc.data(), gap.data(), con.data(), sw.data(), res.data(), ta.data(), rows.data(), ls.data(),
                                               dr.data()) == 0);
    CHECK(r.s.g.v_next == v && r.s.g.a == a && r.s.g.lambda == lam && r.s.lambda_contact == lamc && r.s.g.gap == gap && r.s.g.contact == con);
    CHECK(r.s.sweeps == sw && r.s.residual == res && r.tau_applied == ta && r.stops.stop_rows == rows && r.stops.lam_stop == ls && r.stops.dropped == dr);
    // clipped to 6 N m except where tau_max is infinite; the knee's upper stop is loaded, the hip's lower stop is listed
    CHECK(ta[0] == tau[0]);
    for (int k = 1; k < B * na; k++)
      CHECK(std::fabs(ta[k]) <= 6.0 && (std::fabs(tau[k]) > 6.0 ? std::fabs(ta[k]) == 6.0 : ta[k] == tau[k]));
    CHECK(rows[0] == 0 && rows[NJ] == -(knee + 1) && rows[NJ + 1] == 3 + 1 && rows[NJ + 2] == 0 && ls[NJ] > 0.0 && dr[0] == 0 && dr[1] == 0);
    CHECK(v[(size_t)nv + 6 + knee] < 1e-9); // (the stop has taken the knee's speed)
    // the inert model against groundSolveDynamics
    JM inert;
    inert.stops = false;
    const GJ q = sim.groundJointDynamics(X, tau, dt, inert);
    const GS p = sim.groundSolveDynamics(X, tau, dt);
    CHECK(q.s.g.v_next == p.g.v_next && q.s.g.a == p.g.a && q.s.g.lambda == p.g.lambda && q.s.sweeps == p.sweeps && q.s.residual == p.residual);
    CHECK(q.tau_applied == tau);
  }
  // 150 steps with the knees driven into their upper stops by 10 N m, clipped to 6
  sim.setJointModel(model);
  for (int i = 0; i < B; i++)
    tau[(size_t)i * na + knee] = 10.0;
  {
    DeviceBuffer Xd(X), td(tau);
    int loaded = 0;
    for (int k = 0; k < 150; k++)
    {
      sim.stepGroundDevice(Xd.p, td.p, dt);
      sim.wait();
      const simple_mpc::BatchedRobotSim::JointStops st = sim.lastJointStops();
      bool both = true;
      for (int i = 0; i < B; i++)
      {
        bool hit = false;
        for (int r = 0; r < NJ; r++)
          hit = hit || (st.stop_rows[(size_t)i * NJ + r] == -(knee + 1) && st.lam_stop[(size_t)i * NJ + r] > 0.0);
        both = both && hit;
      }
      loaded += both ? 1 : 0;
    }
    const std::vector<double> Xe = Xd.get(), ta = sim.lastAppliedTorques();
    for (int i = 0; i < B; i++)
    {
      CHECK(std::fabs(Xe[(size_t)i * nx + 7 + knee] - robot->q_hi[knee]) < 1e-6);
      CHECK(ta[(size_t)i * na + knee] == 6.0);
    }
    CHECK(loaded >= 50);
    std::printf("knee held at q_hi: q - q_hi = %.3e rad, steps with both stops loaded %d\n", Xe[7 + knee] - robot->q_hi[knee], loaded);
    double *t = nullptr, *l = nullptr;
    int32_t *r = nullptr, *d = nullptr;
    sim.jointModelDevicePointers(&t, &r, &l, &d);
    CHECK(t != nullptr && r != nullptr && l != nullptr && d != nullptr);
  }
  // refusals: the field and the first offending index; the previous model stays
  {
    JM bad = model;
    bad.tau_max[(size_t)na + 4] = -1.0;
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("tau_max[1][4]") != std::string::npos);
    bad = model;
    bad.damping[5] = NAN;
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("damping[0][5]") != std::string::npos);
    bad = model;
    bad.q_lo.assign(na, 5.0);
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("q_lo[0][0]") != std::string::npos);
    bad = model;
    bad.stop_erp = 1.5;
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("stop_erp = 1.5") != std::string::npos);
    bad = model;
    bad.activation = -1.0;
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("activation = -1") != std::string::npos);
    bad = model;
    bad.armature.assign(na + 1, 0.0);
    CHECK(refusal([&] { sim.setJointModel(bad); }).find("armature [na]") != std::string::npos);
    DeviceBuffer Xd(X), td(tau);
    sim.stepGroundDevice(Xd.p, td.p, dt);
    sim.wait();
    CHECK(sim.lastAppliedTorques()[knee] == 6.0);
  }
  // setGround drops the model
  sim.setGround(gs);
  {
    double * t = (double *)1;
    sim.jointModelDevicePointers(&t, nullptr, nullptr, nullptr);
    CHECK(t == nullptr);
  }
  std::printf("batched sim joint mirror: OK\n");
  return 0;
}
