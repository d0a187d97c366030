// The body parameters of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setBodyParams, bodyParams, bodyParamsDevicePointer,
// groundBodyDynamics, body_params, scale_bodies) on the built-in quadruped: the mirror against the C ABI called directly, bit for bit, in
// the host-buffer solve and over 30 steps on the ground; the table's rows against the kernels without body parameters bit for bit; a
// heavier robot pressing harder on the ground; clearing, setGround and the refusals.  "Device" memory: plain host memory for the
// sequential-lane test build, hipMalloc'ed memory for the HIP library (SMPC_CHECK_HIP).
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
  const int B = 3, NJ = SMPC_JOINT_MAX_STOPS, steps = 30;
  const double dt = 1e-3;
  typedef simple_mpc::BatchedRobotSim Sim;
  typedef Sim::JointModel JM;
  typedef Sim::GroundJoint GJ;
  Sim sim(robot, 3, B), twin(robot, 3, B), plain(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv, na = nv - 6, nj = robot->njoints;
  CHECK(nj == nq - 6);
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * na, 0.0);
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
    X[(size_t)i * nx + nq + 2] = -0.2 - 0.1 * i; // (moving down onto the plane)
    for (int k = 0; k < na; k++)
      tau[(size_t)i * na + k] = (k % 2 ? -1.0 : 1.0) * (0.5 + 0.1 * k + 0.3 * i);
  }
  // the helpers: the table's rows in the layout of the C ABI; masses and inertias scaled, centres of mass kept
  const std::vector<double> nom = simple_mpc::body_params(robot);
  CHECK((int)nom.size() == nj * 10 && nom[3 * 10] == robot->mass[3] && nom[3 * 10 + 2] == robot->com[3][1] && nom[3 * 10 + 7] == robot->inertia[3][3]);
  std::vector<double> nom3, scales;
  for (int i = 0; i < B; i++)
  {
    nom3.insert(nom3.end(), nom.begin(), nom.end());
    for (int j = 0; j < nj; j++)
      scales.push_back(1.0 + 0.2 * i + 0.01 * j);
  }
  const std::vector<double> body = simple_mpc::scale_bodies(nom3, scales);
  for (int r = 0; r < B * nj; r++)
  {
    CHECK(body[(size_t)r * 10] == nom3[(size_t)r * 10] * scales[r] && body[(size_t)r * 10 + 2] == nom3[(size_t)r * 10 + 2]);
    CHECK(body[(size_t)r * 10 + 9] == nom3[(size_t)r * 10 + 9] * scales[r]);
  }
  CHECK(simple_mpc::scale_bodies(nom, {2.0})[10] == 2.0 * nom[10]);
  CHECK(refusal([&] { simple_mpc::scale_bodies(nom, std::vector<double>(5, 1.0)); }).find("scale_bodies") != std::string::npos);
  // before setGround
  CHECK(refusal([&] { sim.setBodyParams(body); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(sim.bodyParams() == nom3 && sim.bodyParamsDevicePointer() == nullptr);
  smpc_ground_settings gs;
  std::memset(&gs, 0, sizeof(gs));
  gs.ground_z = robot->q_ref[2] + robot->foot_ref_p[0][2] + 0.002; // (the feet of the reference pose 2 mm inside the ground)
  sim.setGround(gs);
  twin.setGround(gs);
  plain.setGround(gs);
  CHECK(sim.bodyParams() == nom3 && sim.bodyParamsDevicePointer() == nullptr);
  JM model;
  model.damping.assign(na, 0.1);
  model.tau_max.assign((size_t)B * na, 20.0);
  model.stops = true;
  // the host-buffer solve: the mirror against the C ABI, bit for bit; the table's rows and no rows against groundJointDynamics
  {
    const GJ r = sim.groundBodyDynamics(X, tau, dt, model, body);
    std::vector<double> dmp((size_t)B * na, 0.1);
    const smpc_joint_model_settings m = {model.tau_max.data(), dmp.data(), nullptr, nullptr, nullptr, 1, 1, 0.0, 0.0};
    std::vector<double> v((size_t)B * nv), a((size_t)B * nv), lam((size_t)B * 12), lamc((size_t)B * 12), gap((size_t)B * 4), res(B), ta((size_t)B * na),
        ls((size_t)B * NJ);
    std::vector<uint32_t> con(B);
    std::vector<int32_t> sw(B), rows((size_t)B * NJ), dr(B);
    CHECK(smpc_robot_sim_ground_body_dynamics(sim.handle(), B, X.data(), tau.data(), dt, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &m, body.data(), v.data(),
                                              a.data(), lam.data(), lamc.data(), gap.data(), con.data(), sw.data(), res.data(), ta.data(), rows.data(), ls.data(),
                                              dr.data()) == 0);
    CHECK(r.s.g.v_next == v && r.s.g.a == a && r.s.g.lambda == lam && r.s.lambda_contact == lamc && r.s.g.gap == gap && r.s.g.contact == con);
    CHECK(r.s.sweeps == sw && r.s.residual == res && r.tau_applied == ta && r.stops.stop_rows == rows && r.stops.lam_stop == ls && r.stops.dropped == dr);
    CHECK(con[0] != 0 && con[1] != 0 && con[2] != 0);
    const GJ q = sim.groundJointDynamics(X, tau, dt, model), t = sim.groundBodyDynamics(X, tau, dt, model, nom3), e = sim.groundBodyDynamics(X, tau, dt, model, {});
    CHECK(q.s.g.v_next == t.s.g.v_next && q.s.g.a == t.s.g.a && q.s.g.lambda == t.s.g.lambda && q.s.sweeps == t.s.sweeps && q.tau_applied == t.tau_applied);
    CHECK(q.s.g.v_next == e.s.g.v_next && q.s.g.a == e.s.g.a && q.s.g.lambda == e.s.g.lambda && q.s.residual == e.s.residual);
    CHECK(!(q.s.g.a == r.s.g.a));
    // one state of the three: n need not be the batch
    const std::vector<double> X1(X.begin() + nx, X.begin() + 2 * nx), t1(tau.begin() + na, tau.begin() + 2 * na), b1(body.begin() + nj * 10, body.begin() + 2 * nj * 10);
    JM one = model;
    one.tau_max.assign(na, 20.0);
    const GJ s = sim.groundBodyDynamics(X1, t1, dt, one, b1);
    CHECK(std::vector<double>(a.begin() + nv, a.begin() + 2 * nv) == s.s.g.a && std::vector<double>(lam.begin() + 12, lam.begin() + 24) == s.s.g.lambda);
  }
  // 30 steps: setBodyParams of the mirror against smpc_robot_sim_set_body_params called directly; the table's rows against no rows
  sim.setBodyParams(body);
  CHECK(smpc_robot_sim_set_body_params(twin.handle(), body.data()) == 0);
  CHECK(sim.bodyParams() == body && twin.bodyParams() == body && sim.bodyParamsDevicePointer() != nullptr);
  Sim inert(robot, 3, B);
  inert.setGround(gs);
  inert.setBodyParams(nom3);
  {
    DeviceBuffer Xa(X), Xb(X), Xc(X), Xd(X), td(tau);
    std::vector<double> heavy(B, 0.0), light(B, 0.0);
    for (int k = 0; k < steps; k++)
    {
      sim.stepGroundDevice(Xa.p, td.p, dt);
      twin.stepGroundDevice(Xb.p, td.p, dt);
      plain.stepGroundDevice(Xc.p, td.p, dt);
      inert.stepGroundDevice(Xd.p, td.p, dt);
      sim.wait();
      twin.wait();
      plain.wait();
      inert.wait();
      CHECK(Xa.get() == Xb.get() && sim.lastGroundForces() == twin.lastGroundForces() && sim.lastAccelerations() == twin.lastAccelerations());
      CHECK(Xc.get() == Xd.get() && plain.lastGroundForces() == inert.lastGroundForces() && plain.lastContacts() == inert.lastContacts());
      if (k >= steps - 10)
      {
        const std::vector<double> fa = sim.lastGroundForces(), fc = plain.lastGroundForces();
        for (int i = 0; i < B; i++)
          for (int c = 0; c < 4; c++)
          {
            heavy[i] += fa[(size_t)i * 12 + 3 * c + 2];
            light[i] += fc[(size_t)i * 12 + 3 * c + 2];
          }
      }
    }
    CHECK(!(Xa.get() == Xc.get()));
    std::printf("summed normal force over the last 10 steps: table %.3f %.3f %.3f N, scaled bodies %.3f %.3f %.3f N\n", light[0], light[1], light[2], heavy[0],
                heavy[1], heavy[2]);
    CHECK(light[0] > 0.0 && heavy[1] > light[1] && heavy[2] > heavy[1]);
  }
  // refusals: the field and the first offending [robot][joint]; the previous parameters stay
  {
    double * const ptr = sim.bodyParamsDevicePointer();
    std::vector<double> bad = body;
    bad[(size_t)(1 * nj + 4) * 10] = 0.0;
    CHECK(refusal([&] { sim.setBodyParams(bad); }).find("mass[1][4]") != std::string::npos);
    bad = body;
    bad[(size_t)(2 * nj + 7) * 10 + 3] = INFINITY;
    CHECK(refusal([&] { sim.setBodyParams(bad); }).find("com[2][7]") != std::string::npos);
    bad = body;
    bad[(size_t)(0 * nj + 12) * 10 + 8] = NAN;
    CHECK(refusal([&] { sim.setBodyParams(bad); }).find("inertia[0][12]") != std::string::npos);
    CHECK(refusal([&] { sim.groundBodyDynamics(X, tau, dt, model, bad); }).find("inertia[0][12]") != std::string::npos);
    bad.pop_back();
    CHECK(refusal([&] { sim.setBodyParams(bad); }).find("body [B][njoints][10]") != std::string::npos);
    CHECK(refusal([&] { sim.groundBodyDynamics(X, tau, dt, model, bad); }).find("body [n][njoints][10]") != std::string::npos);
    CHECK(sim.bodyParams() == body && sim.bodyParamsDevicePointer() == ptr);
  }
  // cleared: the handle that never had any; setGround drops them
  sim.setBodyParams({});
  CHECK(sim.bodyParamsDevicePointer() == nullptr && sim.bodyParams() == nom3);
  twin.setGround(gs);
  CHECK(twin.bodyParamsDevicePointer() == nullptr && twin.bodyParams() == nom3);
  Sim fresh(robot, 3, B);
  fresh.setGround(gs);
  {
    DeviceBuffer Xa(X), Xb(X), Xc(X), td(tau);
    for (int k = 0; k < 5; k++)
    {
      sim.stepGroundDevice(Xa.p, td.p, dt);
      twin.stepGroundDevice(Xb.p, td.p, dt);
      fresh.stepGroundDevice(Xc.p, td.p, dt);
    }
    sim.wait();
    twin.wait();
    fresh.wait();
    CHECK(Xa.get() == Xc.get() && Xb.get() == Xc.get());
  }
  std::printf("batched sim body mirror: OK\n");
  return 0;
}
