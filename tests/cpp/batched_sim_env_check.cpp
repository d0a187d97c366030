// Per-robot slopes, friction and pushes of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setGroundEnv, setPush, pushDevicePointer,
// groundEnvDynamics) on the built-in quadruped.  A push on the base origin does not go through the centre of mass, so the closed form
// R^T (g + f / m) does not hold for this table: the mirror is compared with smpc_robot_sim_ground_env_dynamics through the C ABI instead,
// and a step on the handle's environment with the host-buffer solve.  Then a drop onto a slope of 0.2 rad with mu = 1.2 that ends on all
// four feet with gaps within 1 mm inside 200 steps, and the refusals.  "Device" memory: plain host memory for the sequential-lane test
// build, hipMalloc'ed memory for the HIP library (SMPC_CHECK_HIP).
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
  const int B = 2;
  const double dt = 1e-3;
  simple_mpc::BatchedRobotSim sim(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv, na = nv - 6;
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * na, 0.0);
  // before setGround
  CHECK(refusal([&] { sim.setGroundEnv(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.setPush(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.pushDevicePointer(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  // the plane under the reference pose
  smpc_ground_settings gs;
  std::memset(&gs, 0, sizeof(gs));
  sim.setGround(gs);
  for (int i = 0; i < B; i++)
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
  double ground_z = sim.groundDynamics(X, tau, dt).gap[0];
  for (int c = 1; c < 4; c++)
    ground_z = std::fmin(ground_z, sim.groundDynamics(X, tau, dt).gap[c]);
  gs.ground_z = ground_z;
  gs.mu = 0.7;
  sim.setGround(gs);
  CHECK(sim.pushDevicePointer() == nullptr);
  // the slope: e_z turned by 0.2 rad about x; its frame Rc = [t1 t2 n] is that rotation
  const double th = 0.2, s = std::sin(th), c = std::cos(th);
  const std::vector<double> planes = {0.0, -s, c, ground_z, 0.0, 0.0, 1.0, ground_z};
  const std::vector<double> mu = {1.2, 0.7};
  // robot 0: the reference posture turned with the slope; robot 1: on the flat plane; both 2 cm above their plane along its normal, at rest
  {
    const double qx[4] = {std::sin(th / 2), 0.0, 0.0, std::cos(th / 2)}; // (x y z w)
    const double * r = robot->q_ref;
    const double p[3] = {r[0], r[1], r[2] + 0.02};
    X[0] = p[0];
    X[1] = c * p[1] - s * p[2];
    X[2] = s * p[1] + c * p[2];
    X[3] = qx[3] * r[3] + qx[0] * r[6] + qx[1] * r[5] - qx[2] * r[4];
    X[4] = qx[3] * r[4] - qx[0] * r[5] + qx[1] * r[6] + qx[2] * r[3];
    X[5] = qx[3] * r[5] + qx[0] * r[4] - qx[1] * r[3] + qx[2] * r[6];
    X[6] = qx[3] * r[6] - qx[0] * r[3] - qx[1] * r[4] - qx[2] * r[5];
    X[(size_t)nx + 2] += 0.02;
  }
  typedef simple_mpc::BatchedRobotSim::GroundDynamics GD;
  const GD up = sim.groundEnvDynamics(X, tau, dt, planes, mu);
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < 4; k++)
      CHECK(std::fabs(up.gap[(size_t)i * 4 + k] - 0.02) < 1e-9);
    CHECK(up.contact[i] == 0u);
  }
  // a push on the base of robot 0 and on a foot's joint of robot 1: the mirror against the C ABI, bit for bit; the push changes the answer
  const std::vector<double> push = {25.0, -10.0, 5.0, 0.05, 0.0, -0.02, -8.0, 30.0, 12.0, 0.0, 0.01, -0.1};
  for (int joint : {0, (int)robot->foot_joint[3]})
  {
    const GD g = sim.groundEnvDynamics(X, tau, dt, planes, mu, push, joint);
    std::vector<double> v((size_t)B * nv), a((size_t)B * nv), lam((size_t)B * 12), gap((size_t)B * 4);
    std::vector<uint32_t> con(B);
    CHECK(smpc_robot_sim_ground_env_dynamics(sim.handle(), B, X.data(), tau.data(), dt, planes.data(), mu.data(), push.data(), joint, v.data(), a.data(), lam.data(),
                                             gap.data(), con.data()) == SMPC_OK);
    CHECK(g.v_next == v && g.a == a && g.lambda == lam && g.gap == gap && g.contact == con);
    double diff = 0.0;
    for (int k = 0; k < B * nv; k++)
      diff = std::fmax(diff, std::fabs(g.a[k] - up.a[k]));
    CHECK(diff > 1.0);
    // the total force on the robot is m (a_com - g); above the plane it is the push: sum over the bodies is not available here, so the
    // cheap part of that statement: no ground force, no contact
    for (int k = 0; k < B * 12; k++)
      CHECK(g.lambda[k] == 0.0);
  }
  // the handle's environment: one step equals the host-buffer solve of the pre-step states
  sim.setGroundEnv(planes, mu);
  sim.setPush(push, 0);
  CHECK(sim.pushDevicePointer() != nullptr);
  {
    DeviceBuffer Xd(X), td(tau);
    const GD want = sim.groundEnvDynamics(X, tau, dt, planes, mu, push, 0);
    sim.stepGroundDevice(Xd.p, td.p, dt);
    const std::vector<double> a = sim.lastAccelerations(), Xn = Xd.get();
    CHECK(a == want.a);
    for (int i = 0; i < B; i++)
      for (int k = 0; k < nv; k++)
        CHECK(Xn[(size_t)i * nx + nq + k] == want.v_next[(size_t)i * nv + k]);
  }
  // the drop: inside 200 steps of 1 ms both robots stand on all four feet, every gap within 1 mm
  sim.setPush();
  CHECK(sim.pushDevicePointer() == nullptr);
  {
    DeviceBuffer Xd(X), td(tau);
    bool landed = false;
    int k = 0;
    for (; k < 200 && !landed; k++)
    {
      sim.stepGroundDevice(Xd.p, td.p, dt);
      const std::vector<uint32_t> w = sim.lastContacts();
      landed = w[0] == 0b1111u && w[1] == 0b1111u;
    }
    CHECK(landed && k > 50); // (2 cm of free fall along the normal take 64 ms on the flat plane, longer on the slope)
    const GD g = sim.groundEnvDynamics(Xd.get(), tau, dt, planes, mu);
    for (int i = 0; i < B * 4; i++)
      CHECK(std::fabs(g.gap[i]) <= 1e-3);
    std::printf("drop onto 0.2 rad: all feet down after %d steps\n", k);
    // forces in world axes: inside the cone of each robot's own mu about its own normal
    const std::vector<double> f = sim.lastGroundForces();
    for (int i = 0; i < B; i++)
      for (int p = 0; p < 4; p++)
      {
        const double * l = &f[(size_t)i * 12 + p * 3];
        const double * n = &planes[(size_t)i * 4];
        const double ln = l[0] * n[0] + l[1] * n[1] + l[2] * n[2];
        const double lt = std::sqrt(std::fmax(0.0, l[0] * l[0] + l[1] * l[1] + l[2] * l[2] - ln * ln));
        CHECK(ln > 0.0 && lt <= mu[i] * ln * (1 + 1e-9) + 1e-9);
      }
  }
  // refusals keep the environment; setGround drops it
  std::vector<double> bad = planes;
  bad[2] = 1.5;
  std::string why = refusal([&] { sim.setGroundEnv(bad, mu); });
  CHECK(why.find("plane[0]") != std::string::npos && why.find("robot 0") != std::string::npos);
  why = refusal([&] { sim.setGroundEnv({}, {0.5, -1.0}); });
  CHECK(why.find("mu[1]") != std::string::npos && why.find("robot 1") != std::string::npos);
  CHECK(refusal([&] { sim.setPush(push, nq - 6); }).find("push_joint") != std::string::npos);
  CHECK(refusal([&] { sim.setPush({1.0, 2.0}); }).find("push [B][6]") != std::string::npos);
  CHECK(refusal([&] { sim.setGroundEnv({1.0}); }).find("planes [B][4]") != std::string::npos);
  CHECK(refusal([&] { sim.groundEnvDynamics(X, tau, dt, planes, {0.5}); }).find("mu [n]") != std::string::npos);
  const GD kept = sim.groundEnvDynamics(X, tau, dt, planes, mu);
  {
    DeviceBuffer Xd(X), td(tau);
    sim.stepGroundDevice(Xd.p, td.p, dt);
    CHECK(sim.lastAccelerations() == kept.a);
    sim.setGround(gs);
    DeviceBuffer Xe(X);
    sim.stepGroundDevice(Xe.p, td.p, dt);
    CHECK(sim.lastAccelerations() == sim.groundDynamics(X, tau, dt).a && sim.lastAccelerations() != kept.a);
  }
  std::printf("batched sim env mirror: OK\n");
  return 0;
}
