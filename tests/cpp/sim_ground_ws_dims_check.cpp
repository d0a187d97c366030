// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_ground_ws_dims.h (admission, defaults and sizes of the warm-started ground contact
// solve with a stopping rule, and the validation of a reset list), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/sim_ground_ws_dims_check.cpp -o sim_ground_ws_dims_check && ./sim_ground_ws_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_ground_ws_dims.h"
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
  // admitted: warm_start 0 / 1, tol >= 0 finite, min_sweeps 0 .. sweeps
  smpc_ground_solver_settings s = {0, 0.0, 0};
  CHECK(sim_ground_ws_admission_error(30, &s).empty());
  s = {1, 1e-6, 30};
  CHECK(sim_ground_ws_admission_error(30, &s).empty());
  s = {1, 1e300, 1};
  CHECK(sim_ground_ws_admission_error(1, &s).empty());
  // the settings as the kernel reads them: min_sweeps 0 stands for 1
  s = {0, 0.0, 0};
  SimGroundWsSettings r = sim_ground_ws_resolve(&s);
  CHECK(r.warm_start == 0 && r.tol == 0.0 && r.min_sweeps == 1);
  s = {1, 2.5e-7, 7};
  r = sim_ground_ws_resolve(&s);
  CHECK(r.warm_start == 1 && r.tol == 2.5e-7 && r.min_sweeps == 7);
  // refusals, each with the field named
  std::string why;
  s = {1, -1e-9, 0};
  why = sim_ground_ws_admission_error(30, &s);
  CHECK(has(why, "ground solver settings") && has(why, "tol = -1e-09") && has(why, "negative"));
  s = {1, nan, 0};
  why = sim_ground_ws_admission_error(30, &s);
  CHECK(has(why, "tol") && has(why, "not finite"));
  s = {0, inf, 0};
  CHECK(has(sim_ground_ws_admission_error(30, &s), "not finite"));
  s = {0, -inf, 0};
  CHECK(has(sim_ground_ws_admission_error(30, &s), "not finite"));
  s = {1, 1e-6, -1};
  CHECK(has(sim_ground_ws_admission_error(30, &s), "min_sweeps = -1"));
  s = {1, 1e-6, 31};
  why = sim_ground_ws_admission_error(30, &s);
  CHECK(has(why, "min_sweeps = 31") && has(why, "sweeps = 30"));
  s = {1, 1e-6, std::numeric_limits<int>::max()};
  CHECK(!sim_ground_ws_admission_error(400, &s).empty());
  s = {2, 1e-6, 1};
  CHECK(has(sim_ground_ws_admission_error(30, &s), "warm_start = 2"));
  s = {-1, 1e-6, 1};
  CHECK(has(sim_ground_ws_admission_error(30, &s), "warm_start = -1"));
  // sizes: no 32-bit overflow for a large batch
  SimGroundWsSizes z = sim_ground_ws_sizes(3, 12);
  CHECK(z.warm_bytes == 3 * 12 * 8 && z.sweeps_bytes == 3 * 4 && z.residual_bytes == 3 * 8);
  z = sim_ground_ws_sizes(1 << 27, 24);
  CHECK(z.warm_bytes == (size_t)(1 << 27) * 24 * 8);
  // reset lists: a heap mask of exactly B bytes, so that a write past it is the sanitizer's to report
  const int B = 5;
  std::vector<unsigned char> mask(B, 7);
  CHECK(sim_ground_ws_reset_error(nullptr, 0, B, mask.data()).empty()); // n = 0: every robot
  for (int b = 0; b < B; b++)
    CHECK(mask[b] == 1);
  std::vector<int> idx = {4, 0, 4, 4};
  CHECK(sim_ground_ws_reset_error(idx.data(), (int)idx.size(), B, mask.data()).empty()); // unsorted, duplicates
  CHECK(mask[0] == 1 && mask[1] == 0 && mask[2] == 0 && mask[3] == 0 && mask[4] == 1);
  std::fill(mask.begin(), mask.end(), 7);
  idx = {1, B, 2};
  why = sim_ground_ws_reset_error(idx.data(), (int)idx.size(), B, mask.data());
  CHECK(has(why, "indices[1] = 5") && has(why, "[0, 4]"));
  for (int b = 0; b < B; b++)
    CHECK(mask[b] == 7); // (a refused list writes nothing)
  idx = {-1};
  CHECK(has(sim_ground_ws_reset_error(idx.data(), 1, B, mask.data()), "indices[0] = -1"));
  CHECK(has(sim_ground_ws_reset_error(idx.data(), -3, B, mask.data()), "n = -3"));
  CHECK(has(sim_ground_ws_reset_error(nullptr, 2, B, mask.data()), "null"));
  for (int b = 0; b < B; b++)
    CHECK(mask[b] == 7);
  std::printf("sim_ground_ws_dims_check: ok\n");
  return 0;
}
