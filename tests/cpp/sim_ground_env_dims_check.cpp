// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_ground_env_dims.h (admission of the per-robot planes, friction coefficients and
// pushes of the simulator's ground, and the contact frame of a plane), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/sim_ground_env_dims_check.cpp -o sim_ground_env_dims_check && ./sim_ground_env_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_ground_env_dims.h"
#include <limits>
#include <vector>

using namespace smpc;
#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);                                                      \
      return 1;                                                                                                        \
    }                                                                                                                  \
  } while (0)

static bool has(const std::string & s, const char * w) { return s.find(w) != std::string::npos; }

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int n = 5;
  // heap arrays of exactly the admitted sizes: a read past [n][4], [n] or [n][6] is the sanitizer's to report
  std::vector<double> plane(n * 4), mu(n), push(n * 6);
  auto reset = [&] {
    for (int i = 0; i < n; i++)
    {
      const double th = 0.1 * i; // tilted about y, then about x
      plane[i * 4 + 0] = std::sin(th) * std::cos(0.05 * i);
      plane[i * 4 + 1] = -std::sin(0.05 * i);
      plane[i * 4 + 2] = std::cos(th) * std::cos(0.05 * i);
      plane[i * 4 + 3] = 0.01 * i - 0.3;
      mu[i] = 0.2 + 0.25 * i;
      for (int k = 0; k < 6; k++)
        push[i * 6 + k] = 3.0 * k - 7.0 * i;
    }
  };
  reset();
  CHECK(sim_ground_env_admission_error(n, plane.data(), mu.data()).empty());
  CHECK(sim_ground_env_admission_error(n, nullptr, mu.data()).empty());
  CHECK(sim_ground_env_admission_error(n, plane.data(), nullptr).empty());
  CHECK(sim_ground_env_admission_error(n, nullptr, nullptr).empty());
  CHECK(has(sim_ground_env_admission_error(0, nullptr, nullptr), "n = 0"));
  CHECK(sim_ground_push_admission_error(n, 13, 0, push.data()).empty());
  CHECK(sim_ground_push_admission_error(n, 13, 12, push.data()).empty());
  CHECK(sim_ground_push_admission_error(n, 13, 5, nullptr).empty());
  // planes: every number finite, a unit normal, n.z >= 0.5; the message names the field and the robot
  std::string why;
  plane[3 * 4 + 1] = nan;
  why = sim_ground_env_admission_error(n, plane.data(), mu.data());
  CHECK(has(why, "plane[3][1]") && has(why, "robot 3") && has(why, "not finite"));
  reset();
  plane[4 * 4 + 3] = -inf;
  why = sim_ground_env_admission_error(n, plane.data(), nullptr);
  CHECK(has(why, "plane[4][3]") && has(why, "robot 4"));
  reset();
  plane[2 * 4 + 2] += 1e-6;
  why = sim_ground_env_admission_error(n, plane.data(), mu.data());
  CHECK(has(why, "plane[2]") && has(why, "robot 2") && has(why, "unit normal"));
  reset();
  for (int k = 0; k < 3; k++)
    plane[1 * 4 + k] *= 1.0 + 5e-10; // inside the tolerance
  CHECK(sim_ground_env_admission_error(n, plane.data(), mu.data()).empty());
  for (int k = 0; k < 3; k++)
    plane[1 * 4 + k] = 0.0; // the zero vector is no normal
  why = sim_ground_env_admission_error(n, plane.data(), mu.data());
  CHECK(has(why, "plane[1]") && has(why, "unit normal"));
  reset();
  plane[0] = std::sqrt(1.0 - 0.49 * 0.49);
  plane[1] = 0.0;
  plane[2] = 0.49;
  why = sim_ground_env_admission_error(n, plane.data(), mu.data());
  CHECK(has(why, "plane[0]") && has(why, "robot 0") && has(why, "n.z = 0.49"));
  plane[0] = 0.0;
  plane[2] = -1.0;
  CHECK(has(sim_ground_env_admission_error(n, plane.data(), mu.data()), "n.z = -1"));
  plane[0] = std::sqrt(0.75);
  plane[2] = 0.5; // the bound itself is admitted
  CHECK(sim_ground_env_admission_error(n, plane.data(), mu.data()).empty());
  // the first offending robot is the one named
  reset();
  plane[1 * 4 + 0] = nan;
  plane[3 * 4 + 0] = nan;
  CHECK(has(sim_ground_env_admission_error(n, plane.data(), mu.data()), "robot 1"));
  // mu: finite and positive
  reset();
  mu[2] = 0.0;
  why = sim_ground_env_admission_error(n, plane.data(), mu.data());
  CHECK(has(why, "mu[2] = 0") && has(why, "robot 2") && has(why, "not positive"));
  mu[2] = -0.3;
  CHECK(has(sim_ground_env_admission_error(n, nullptr, mu.data()), "mu[2] = -0.3"));
  mu[2] = nan;
  why = sim_ground_env_admission_error(n, nullptr, mu.data());
  CHECK(has(why, "mu[2]") && has(why, "not finite"));
  mu[2] = inf;
  CHECK(has(sim_ground_env_admission_error(n, nullptr, mu.data()), "not finite"));
  // the push: the joint in range whether or not an array is given, every number finite
  reset();
  CHECK(has(sim_ground_push_admission_error(n, 13, 13, push.data()), "push_joint = 13 is outside [0, 12]"));
  CHECK(has(sim_ground_push_admission_error(n, 13, -1, nullptr), "push_joint = -1"));
  CHECK(has(sim_ground_push_admission_error(n, 13, 1 << 30, push.data()), "push_joint = 1073741824"));
  push[4 * 6 + 5] = nan;
  why = sim_ground_push_admission_error(n, 13, 0, push.data());
  CHECK(has(why, "push[4][5]") && has(why, "robot 4") && has(why, "not finite"));
  CHECK(sim_ground_push_admission_error(n - 1, 13, 0, push.data()).empty()); // (robot 4 is not looked at)
  CHECK(has(sim_ground_push_admission_error(-2, 13, 0, push.data()), "n = -2"));
  // the contact frame: the identity for e_z; orthonormal, right-handed and with t1.y = 0 for every admitted normal
  double t1[3], t2[3];
  const double ez[3] = {0.0, 0.0, 1.0};
  sim_ground_env_frame(ez, t1, t2);
  CHECK(t1[0] == 1.0 && t1[1] == 0.0 && t1[2] == 0.0 && t2[0] == 0.0 && t2[1] == 1.0 && t2[2] == 0.0);
  reset();
  for (int i = 0; i < n; i++)
  {
    const double * nn = &plane[i * 4];
    sim_ground_env_frame(nn, t1, t2);
    auto dot = [](const double * a, const double * b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    CHECK(t1[1] == 0.0 && std::fabs(dot(t1, t1) - 1.0) < 1e-14 && std::fabs(dot(t2, t2) - 1.0) < 1e-14);
    CHECK(std::fabs(dot(t1, t2)) < 1e-14 && std::fabs(dot(t1, nn)) < 1e-14 && std::fabs(dot(t2, nn)) < 1e-14);
    const double c[3] = {t1[1] * t2[2] - t1[2] * t2[1], t1[2] * t2[0] - t1[0] * t2[2], t1[0] * t2[1] - t1[1] * t2[0]};
    CHECK(std::fabs(c[0] - nn[0]) < 1e-14 && std::fabs(c[1] - nn[1]) < 1e-14 && std::fabs(c[2] - nn[2]) < 1e-14); // t1 x t2 = n
  }
  std::printf("sim_ground_env_dims_check: ok\n");
  return 0;
}
