// The ground plane of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setGround, stepGroundDevice, groundDynamics, lastGroundForces,
// lastContacts) on the built-in quadruped: free fall above the plane as a known answer, a drop from 2 cm that ends with every foot on
// the ground, and the refusals.  The states and torques of stepGroundDevice live in "device" memory: plain host memory for the
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
  const int B = 2;
  simple_mpc::BatchedRobotSim sim(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv;
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * (nv - 6), 0.0);
  // before setGround
  CHECK(sim.groundPoints() == 0);
  {
    DeviceBuffer Xd(X), td(tau);
    CHECK(refusal([&] { sim.stepGroundDevice(Xd.p, td.p, 1e-3); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  }
  // the plane under the reference pose: the gaps over the plane z = 0 are the heights of the feet (and setGround may be called again)
  smpc_ground_settings gs;
  std::memset(&gs, 0, sizeof(gs));
  sim.setGround(gs);
  CHECK(sim.groundPointsPerFoot() == 1 && sim.groundPoints() == 4);
  for (int i = 0; i < B; i++)
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
  double ground_z = sim.groundDynamics(X, tau, 1e-3).gap[0];
  for (int c = 1; c < 4; c++)
    ground_z = std::fmin(ground_z, sim.groundDynamics(X, tau, 1e-3).gap[c]);
  CHECK(ground_z < robot->q_ref[2] - 0.1);
  gs.ground_z = ground_z;
  sim.setGround(gs);
  CHECK(sim.groundPointsPerFoot() == 1 && sim.groundPoints() == 4);
  // robot 0: 1 m above the plane; robot 1: 2 cm above it; both at rest, zero torque
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
    X[(size_t)i * nx + 2] += i == 0 ? 1.0 : 0.02;
  }
  // free fall above the plane: the known answer a_z = -9.81, nothing else moves, no force, no contact
  simple_mpc::BatchedRobotSim::GroundDynamics g = sim.groundDynamics(X, tau, 1e-3);
  CHECK(g.a.size() == (size_t)B * nv && g.lambda.size() == (size_t)B * 12 && g.gap.size() == (size_t)B * 4 && g.contact.size() == (size_t)B);
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < nv; k++)
    {
      CHECK(std::fabs(g.a[(size_t)i * nv + k] - (k == 2 ? -9.81 : 0.0)) < 1e-9);
      CHECK(std::fabs(g.v_next[(size_t)i * nv + k] - (k == 2 ? -9.81e-3 : 0.0)) < 1e-12);
    }
    for (int k = 0; k < 12; k++)
      CHECK(g.lambda[(size_t)i * 12 + k] == 0.0);
    for (int c = 0; c < 4; c++)
      CHECK(std::fabs(g.gap[(size_t)i * 4 + c] - (i == 0 ? 1.0 : 0.02)) < 1e-6);
    CHECK(g.contact[i] == 0u);
  }
  // the drop: within 100 steps of 1 ms robot 1 stands on all four feet; robot 0 is still falling
  {
    DeviceBuffer Xd(X), td(tau);
    bool landed = false;
    int k = 0;
    for (; k < 100 && !landed; k++)
    {
      sim.stepGroundDevice(Xd.p, td.p, 1e-3);
      const std::vector<uint32_t> w = sim.lastContacts();
      CHECK(w.size() == (size_t)B && w[0] == 0u);
      landed = w[1] == 0b1111u;
    }
    CHECK(landed && k > 50); // (2 cm of free fall take 64 ms)
    const std::vector<double> f = sim.lastGroundForces(), a = sim.lastAccelerations(), Xn = Xd.get();
    CHECK(f.size() == (size_t)B * 12);
    for (int c = 0; c < 4; c++)
    {
      CHECK(f[c * 3 + 2] == 0.0 && f[12 + c * 3 + 2] > 0.0);
      CHECK(std::hypot(f[12 + c * 3], f[12 + c * 3 + 1]) <= 0.7 * f[12 + c * 3 + 2] * (1 + 1e-12));
    }
    CHECK(std::fabs(a[2] + 9.81) < 1e-9);
    CHECK(std::fabs(Xn[2] - (robot->q_ref[2] + 1.0 - 0.5 * 9.81 * 1e-3 * 1e-3 * k * (k + 1))) < 1e-9); // semi-implicit Euler: z_k = z_0 - g dt^2 k (k + 1) / 2
    double *lam_dev = nullptr;
    uint32_t * con_dev = nullptr;
    sim.groundForceDevicePointers(&lam_dev, &con_dev);
    CHECK(lam_dev != nullptr && con_dev != nullptr);
    // refusals
    CHECK(refusal([&] { sim.stepGroundDevice(Xd.p, td.p, 0.0); }).find("dt must be positive") != std::string::npos);
  }
  smpc_ground_settings bad = gs;
  bad.points_per_foot = 4;
  CHECK(refusal([&] { sim.setGround(bad); }).find("4 * 4 = 16") != std::string::npos);
  bad = gs;
  bad.erp = 2.0;
  CHECK(refusal([&] { sim.setGround(bad); }).find("erp = 2") != std::string::npos);
  CHECK(sim.groundPoints() == 4); // (a refused call keeps the ground)
  tau.pop_back();
  CHECK(refusal([&] { sim.groundDynamics(X, tau, 1e-3); }).find("tau [n][nv - 6]") != std::string::npos);
  std::printf("batched sim ground mirror: OK\n");
  return 0;
}
