// The warm-started ground contact solve of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setGroundSolver, resetGroundWarmStart,
// lastGroundSweeps, lastGroundResiduals, groundSolverDevicePointers, groundSolveDynamics) on the built-in quadruped: the mirror against the C
// ABI bit for bit, then a 2 cm drop with warm start and tol = 1e-6 that ends on all four feet with fewer sweeps at the last step than at the
// first step in contact, and the refusals.  "Device" memory: plain host memory for the sequential-lane test build, hipMalloc'ed memory for
// the HIP library (SMPC_CHECK_HIP).
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
  simple_mpc::BatchedRobotSim sim(robot, 3, B), plain(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv, na = nv - 6;
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * na, 0.0);
  // before setGround
  CHECK(refusal([&] { sim.setGroundSolver(true, 1e-6); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.resetGroundWarmStart(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(refusal([&] { sim.lastGroundSweeps(); }).find("smpc_robot_sim_set_ground") != std::string::npos);
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
  gs.sweeps = 60;
  sim.setGround(gs);
  plain.setGround(gs);
  // robot 0: 2 cm above the plane; robot 1: 1 cm above it, moving sideways
  X[2] += 0.02;
  X[(size_t)nx + 2] += 0.01;
  X[(size_t)nx + nq + 1] = 0.3;
  // the host-buffer solve: the mirror against the C ABI, bit for bit, from a start vector with a NaN in it
  typedef simple_mpc::BatchedRobotSim::GroundSolve GS;
  {
    std::vector<double> Xc = X, lam0((size_t)B * 12, 0.0);
    Xc[2] -= 0.021;
    Xc[(size_t)nx + 2] -= 0.0105; // (both touch)
    for (int k = 0; k < B * 12; k++)
      lam0[k] = k % 3 == 2 ? 30.0 + k : 0.5 * (k % 5) - 1.0;
    lam0[4] = std::nan("");
    const GS g = sim.groundSolveDynamics(Xc, tau, dt, {}, {}, {}, 0, lam0, true, 1e-6, 2);
    std::vector<double> v((size_t)B * nv), a((size_t)B * nv), lam((size_t)B * 12), lamc((size_t)B * 12), gap((size_t)B * 4), res(B);
    std::vector<uint32_t> con(B);
    std::vector<int32_t> sw(B);
    const smpc_ground_solver_settings s = {1, 1e-6, 2};
    CHECK(smpc_robot_sim_ground_solve_dynamics(sim.handle(), B, Xc.data(), tau.data(), dt, nullptr, nullptr, nullptr, 0, &s, lam0.data(), v.data(), a.data(), lam.data(),
                                               lamc.data(), gap.data(), con.data(), sw.data(), res.data()) == SMPC_OK);
    CHECK(g.g.v_next == v && g.g.a == a && g.g.lambda == lam && g.lambda_contact == lamc && g.g.gap == gap && g.g.contact == con && g.sweeps == sw && g.residual == res);
    CHECK(con[0] == 0b1111u && con[1] == 0b1111u && sw[0] >= 2 && sw[0] < 60 && res[0] <= 1e-6 && res[0] >= 0.0);
    CHECK(lam == lamc); // (the flat plane's frame is the identity)
    // inert settings: the bits of groundDynamics, exactly `sweeps` sweeps
    const GS inert = sim.groundSolveDynamics(Xc, tau, dt);
    const simple_mpc::BatchedRobotSim::GroundDynamics flat = sim.groundDynamics(Xc, tau, dt);
    CHECK(inert.g.a == flat.a && inert.g.lambda == flat.lambda && inert.g.v_next == flat.v_next && inert.sweeps[0] == 60 && inert.sweeps[1] == 60);
  }
  // the setter and the read-outs: the mirror against the C ABI
  sim.setGroundSolver(true, 1e-6, 1);
  {
    int32_t * sw_dev = nullptr;
    double *res_dev = nullptr, *warm_dev = nullptr;
    sim.groundSolverDevicePointers(&sw_dev, &res_dev, &warm_dev);
    CHECK(sw_dev != nullptr && res_dev != nullptr && warm_dev != nullptr);
    const std::vector<int32_t> s0 = sim.lastGroundSweeps();
    CHECK(s0[0] == 0 && s0[1] == 0);
  }
  // the drop: both robots end on all four feet; at the last step the warm start needs fewer sweeps than at the first step in contact,
  // and fewer than a handle that starts every step from zero
  {
    plain.setGroundSolver(false, 1e-6, 1);
    DeviceBuffer Xd(X), Xp(X), td(tau);
    int first[2] = {0, 0}, last[2] = {0, 0}, last_cold[2] = {0, 0};
    std::vector<uint32_t> w;
    for (int k = 0; k < 200; k++)
    {
      sim.stepGroundDevice(Xd.p, td.p, dt);
      plain.stepGroundDevice(Xp.p, td.p, dt);
      w = sim.lastContacts();
      const std::vector<int32_t> sw = sim.lastGroundSweeps(), swc = plain.lastGroundSweeps();
      std::vector<int32_t> abi(B);
      std::vector<double> res(B);
      CHECK(smpc_robot_sim_read_ground_solver_last(sim.handle(), abi.data(), res.data()) == SMPC_OK);
      CHECK(abi == sw && res == sim.lastGroundResiduals());
      for (int i = 0; i < B; i++)
      {
        if (w[i] != 0u && first[i] == 0)
          first[i] = sw[i];
        last[i] = sw[i];
        last_cold[i] = swc[i];
        CHECK(sw[i] >= 1 && sw[i] <= 60 && (res[i] <= 1e-6 || sw[i] == 60));
      }
    }
    CHECK(w[0] == 0b1111u && w[1] == 0b1111u);
    std::printf("2 cm drop: sweeps at the first step in contact %d %d, at the last step %d %d (cold start %d %d)\n", first[0], first[1], last[0], last[1], last_cold[0],
                last_cold[1]);
    for (int i = 0; i < B; i++)
      CHECK(first[i] > 0 && last[i] < first[i] && last[i] < last_cold[i]);
    const simple_mpc::BatchedRobotSim::GroundDynamics g = sim.groundDynamics(Xd.get(), tau, dt);
    for (int i = 0; i < B * 4; i++)
      CHECK(std::fabs(g.gap[i]) <= 1e-3);
    // a reset of robot 1: its next step starts from zero again and needs the cold start's sweeps; robot 0 keeps its warm row
    sim.resetGroundWarmStart({1});
    sim.stepGroundDevice(Xd.p, td.p, dt);
    const std::vector<int32_t> sw = sim.lastGroundSweeps();
    CHECK(sw[0] == last[0] && sw[1] > last[1]);
  }
  // refusals keep the settings; setGround drops them
  CHECK(refusal([&] { sim.setGroundSolver(true, -1.0); }).find("tol") != std::string::npos);
  CHECK(refusal([&] { sim.setGroundSolver(true, 1e-6, 61); }).find("min_sweeps = 61") != std::string::npos);
  CHECK(refusal([&] { sim.resetGroundWarmStart({0, B}); }).find("indices[1]") != std::string::npos);
  CHECK(refusal([&] { sim.groundSolveDynamics(X, tau, dt, {}, {}, {}, 0, {1.0}); }).find("lam0 [n][3 points]") != std::string::npos);
  {
    DeviceBuffer Xd(X), td(tau);
    sim.stepGroundDevice(Xd.p, td.p, dt);
    const std::vector<int32_t> sw = sim.lastGroundSweeps();
    CHECK(sw[0] >= 1 && sw[0] < 60); // (still the stopping rule)
    sim.setGround(gs);
    DeviceBuffer Xe(X);
    sim.stepGroundDevice(Xe.p, td.p, dt);
    CHECK(sim.lastAccelerations() == sim.groundDynamics(X, tau, dt).a);
    const std::vector<int32_t> none = sim.lastGroundSweeps();
    CHECK(none[0] == 0 && none[1] == 0);
  }
  std::printf("batched sim ws mirror: OK\n");
  return 0;
}
