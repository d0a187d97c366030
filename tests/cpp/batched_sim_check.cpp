// The C++ host mirror of the batched rigid-body simulator (include/simple-mpc/batched-sim.hpp over the C ABI) on the built-in quadruped:
// sizes, free fall as a known answer, contact forces, n != batch, and the refusals of the constructor and of the mirror.
#include "simple-mpc/batched-sim.hpp"
#include <cmath>
#include <cstdio>
#include <memory>

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

int main()
{
  const smpc_robot_model * robot = smpc_builtin_robot("go2_like");
  CHECK(robot != nullptr);
  simple_mpc::BatchedRobotSim sim(robot, 3, 2);
  CHECK(sim.batch() == 2 && sim.nq() == robot->nq && sim.nv() == robot->nv && sim.nfeet() == 4 && sim.force_size() == 3);
  const int nq = sim.nq(), nv = sim.nv(), n = 5; // (n is not the batch)
  std::vector<double> X((size_t)n * (nq + nv), 0.0), tau((size_t)n * (nv - 6), 0.0), a, lam;
  std::vector<int> iters;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < nq; k++)
      X[(size_t)i * (nq + nv) + k] = robot->q_ref[k];
  // free fall from rest: every body accelerates with gravity, no joint moves
  sim.forwardDynamics(X, tau, std::vector<unsigned>(n, 0u), {}, {}, a, lam, iters);
  for (int i = 0; i < n; i++)
  {
    for (int k = 0; k < nv; k++)
      CHECK(std::fabs(a[(size_t)i * nv + k] - (k == 2 ? -9.81 : 0.0)) < 1e-9);
    for (int k = 0; k < 12; k++)
      CHECK(lam[(size_t)i * 12 + k] == 0.0);
    CHECK(iters[i] == 0);
  }
  // feet 0 and 3 in contact: their forces come first, the rest is exactly 0, the feet carry weight
  sim.forwardDynamics(X, tau, std::vector<unsigned>(n, 0b1001u), {0.0, 0.0, 0.0}, {50.0, 50.0, 50.0}, a, lam, iters);
  for (int i = 0; i < n; i++)
  {
    CHECK(iters[i] >= 1 && lam[(size_t)i * 12 + 2] > 0.0 && lam[(size_t)i * 12 + 5] > 0.0);
    for (int k = 6; k < 12; k++)
      CHECK(lam[(size_t)i * 12 + k] == 0.0);
    for (int k = 0; k < nv; k++)
      CHECK(std::isfinite(a[(size_t)i * nv + k]) && a[(size_t)i * nv + k] == a[k]); // (the same state in every row)
  }
  // refusals
  CHECK(refusal([&] { simple_mpc::BatchedRobotSim s(robot, 6, 1); }).find("nfeet = 4") != std::string::npos);
  CHECK(refusal([&] { simple_mpc::BatchedRobotSim s(robot, 4, 1); }).find("force_size = 4") != std::string::npos);
  CHECK(refusal([&] { simple_mpc::BatchedRobotSim s(robot, 3, 0); }).find("batch = 0") != std::string::npos);
  CHECK(refusal([&] { sim.stepDevice(X.data(), tau.data(), {true, true, true, true}, 0.0); }).find("dt must be positive") != std::string::npos);
  CHECK(refusal([&] { sim.stepDevice(X.data(), tau.data(), {true, true}, 1e-3); }).find("one entry per foot") != std::string::npos);
  tau.pop_back();
  CHECK(refusal([&] { sim.forwardDynamics(X, tau, std::vector<unsigned>(n, 0u), {}, {}, a, lam, iters); }).find("tau [n][nv - 6]") != std::string::npos);
  std::printf("batched sim mirror: OK\n");
  return 0;
}
