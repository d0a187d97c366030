// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_joint_dims.h (admission, defaults and sizes of the simulator's joint model), meant
// to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/sim_joint_dims_check.cpp -o sim_joint_dims_check && ./sim_joint_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_joint_dims.h"
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
  const int B = 3, na = 5;
  // heap arrays of exactly the admitted sizes, so that a read past them is the sanitizer's to report
  const std::vector<double> tab_lo(na, -1.0), tab_hi(na, 1.0);
  std::vector<double> row(na, 0.5), rows((size_t)B * na, 0.5);
  auto check = [&](const smpc_joint_model_settings & m) { return sim_joint_admission_error(B, na, tab_lo.data(), tab_hi.data(), &m); };
  smpc_joint_model_settings none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.0, 0.0};
  // admitted: the null model, the empty model, broadcast rows, per-robot rows, infinite effort limits and joint limits, zeros
  CHECK(sim_joint_admission_error(B, na, tab_lo.data(), tab_hi.data(), nullptr).empty());
  CHECK(sim_joint_admission_error(B, na, nullptr, nullptr, &none).empty());
  smpc_joint_model_settings m = none;
  m.tau_max = m.damping = m.armature = row.data();
  m.stops = 1;
  m.activation = 0.05;
  m.stop_erp = 1.0;
  CHECK(check(m).empty());
  m.per_robot = 1;
  m.tau_max = m.damping = m.armature = rows.data();
  CHECK(check(m).empty());
  std::vector<double> infs((size_t)B * na, inf), ninfs((size_t)B * na, -inf), zeros((size_t)B * na, 0.0);
  m.tau_max = infs.data();
  m.q_lo = ninfs.data();
  m.q_hi = infs.data();
  m.damping = m.armature = zeros.data();
  CHECK(check(m).empty());
  m.tau_max = zeros.data();
  m.q_lo = m.q_hi = zeros.data(); // (q_lo = q_hi: a locked joint)
  CHECK(check(m).empty());
  // the scalars as the kernel reads them
  SimJointScalars r = sim_joint_resolve(nullptr);
  CHECK(r.stops == 0 && r.activation == 0.1 && r.stop_erp == 0.2);
  r = sim_joint_resolve(&none);
  CHECK(r.stops == 0 && r.activation == 0.1 && r.stop_erp == 0.2);
  m.stops = 1;
  m.activation = 0.05;
  m.stop_erp = 1.0;
  r = sim_joint_resolve(&m);
  CHECK(r.stops == 1 && r.activation == 0.05 && r.stop_erp == 1.0);
  // refusals, each with the field and the first offending index named
  std::string why;
  auto bad = [&](const double ** field, double v, int i, int k, bool per_robot) {
    smpc_joint_model_settings x = none;
    std::vector<double> a(per_robot ? (size_t)B * na : (size_t)na, 0.25);
    a[(size_t)i * na + k] = v;
    if ((size_t)i * na + k + 1 < a.size())
      a[(size_t)i * na + k + 1] = v; // (a later offender: the first one is named)
    x.per_robot = per_robot ? 1 : 0;
    x.tau_max = field == &none.tau_max ? a.data() : nullptr;
    x.damping = field == &none.damping ? a.data() : nullptr;
    x.armature = field == &none.armature ? a.data() : nullptr;
    x.q_lo = field == &none.q_lo ? a.data() : nullptr;
    x.q_hi = field == &none.q_hi ? a.data() : nullptr;
    const std::string w = check(x);
    return w;
  };
  why = bad(&none.tau_max, -1.0, 2, 3, true);
  CHECK(has(why, "joint model") && has(why, "tau_max[2][3] = -1") && has(why, "negative"));
  CHECK(has(bad(&none.tau_max, nan, 0, 4, false), "tau_max[0][4]"));
  CHECK(bad(&none.tau_max, inf, 0, 4, false).empty());
  why = bad(&none.damping, -0.5, 1, 0, true);
  CHECK(has(why, "damping[1][0] = -0.5") && has(why, "negative or not finite"));
  CHECK(has(bad(&none.damping, inf, 1, 1, true), "damping[1][1]"));
  CHECK(has(bad(&none.damping, nan, 0, 2, false), "damping[0][2]"));
  CHECK(has(bad(&none.armature, -1e-3, 2, 4, true), "armature[2][4] = -0.001"));
  CHECK(has(bad(&none.armature, inf, 0, 0, false), "armature[0][0]"));
  CHECK(has(bad(&none.armature, nan, 1, 3, true), "armature[1][3]"));
  why = bad(&none.q_lo, 1.5, 1, 2, true); // (above the table's q_hi = 1)
  CHECK(has(why, "q_lo[1][2] = 1.5") && has(why, "exceeds") && has(why, "q_hi[1][2] = 1"));
  CHECK(has(bad(&none.q_hi, -1.5, 0, 1, false), "q_lo[0][1] = -1 exceeds q_hi[0][1] = -1.5"));
  CHECK(has(bad(&none.q_lo, nan, 2, 0, true), "q_lo[2][0] is NaN"));
  CHECK(has(bad(&none.q_hi, nan, 0, 3, false), "q_hi[0][3] is NaN"));
  CHECK(bad(&none.q_lo, -inf, 0, 3, false).empty());
  smpc_joint_model_settings x = none;
  x.activation = -0.1;
  CHECK(has(check(x), "activation = -0.1"));
  x.activation = nan;
  CHECK(has(check(x), "activation"));
  x.activation = inf;
  CHECK(has(check(x), "activation"));
  x = none;
  x.stop_erp = 1.5;
  CHECK(has(check(x), "stop_erp = 1.5") && has(check(x), "[0, 1]"));
  x.stop_erp = -0.1;
  CHECK(has(check(x), "stop_erp = -0.1"));
  x.stop_erp = nan;
  CHECK(has(check(x), "stop_erp"));
  x = none;
  x.stops = 2;
  CHECK(has(check(x), "stops = 2"));
  x.stops = -1;
  CHECK(has(check(x), "stops = -1"));
  x = none;
  x.per_robot = 3;
  CHECK(has(check(x), "per_robot = 3"));
  // sizes: no 32-bit overflow for a large batch
  SimJointSizes z = sim_joint_sizes(3, 12);
  CHECK(z.array_bytes == 3 * 12 * 8 && z.tau_bytes == 3 * 12 * 8 && z.rows_bytes == 3 * 8 * 4 && z.lam_bytes == 3 * 8 * 8 && z.dropped_bytes == 3 * 4);
  z = sim_joint_sizes(1 << 27, 31);
  CHECK(z.array_bytes == (size_t)(1 << 27) * 31 * 8);
  std::printf("sim_joint_dims_check: ok\n");
  return 0;
}
