// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_body_dims.h (admission, layout and size of the simulator's per-robot body
// parameters), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/sim_body_dims_check.cpp -o sim_body_dims_check && ./sim_body_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_body_dims.h"
#include "../../simple-mpc_amd/csrc/smpc_robot_check.h"
#include "../../include/smpc_robots_builtin.h"
#include <limits>
#include <memory>
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
  const smpc_robot_model * go2 = &SMPC_ROBOT_GO2_LIKE;
  CHECK(robot_table_error(go2).empty());
  const int B = 3, nj = go2->njoints;
  CHECK(sim_body_bytes(B, nj) == (size_t)B * nj * 10 * sizeof(double) && sim_body_bytes(1, 32) == 2560);
  // heap arrays of exactly the admitted sizes, so that a read or a write past them is the sanitizer's to report
  std::vector<double> tab((size_t)nj * SIM_BODY_ROW, nan);
  sim_body_table_rows(go2, tab.data());
  for (int j = 0; j < nj; j++)
  {
    const double * r = &tab[(size_t)j * SIM_BODY_ROW];
    CHECK(r[0] == go2->mass[j] && r[1] == go2->com[j][0] && r[3] == go2->com[j][2] && r[4] == go2->inertia[j][0] && r[9] == go2->inertia[j][5]);
  }
  std::vector<double> good((size_t)B * nj * SIM_BODY_ROW);
  for (int i = 0; i < B; i++)
    for (size_t k = 0; k < tab.size(); k++)
      good[(size_t)i * tab.size() + k] = tab[k] * (k % SIM_BODY_ROW == 0 ? 1.0 + 0.1 * i : 1.0);
  // admitted: no parameters, the table's rows, scaled masses, negative products of inertia and centres of mass
  CHECK(sim_body_admission_error(B, nj, nullptr).empty());
  CHECK(sim_body_admission_error(B, nj, good.data()).empty());
  CHECK(sim_body_admission_error(1, nj, tab.data()).empty());
  {
    std::vector<double> a = good;
    a[(size_t)(1 * nj + 4) * SIM_BODY_ROW + 5] = -1e-3;
    a[(size_t)(1 * nj + 4) * SIM_BODY_ROW + 2] = -0.5;
    a[(size_t)(2 * nj + nj - 1) * SIM_BODY_ROW + 0] = 1e-300;
    CHECK(sim_body_admission_error(B, nj, a.data()).empty());
  }
  // refused: the field and the first offending [robot][joint]
  struct Case
  {
    int robot, joint, col;
    double value;
    const char * field;
  };
  const Case cases[] = {{1, 4, 0, 0.0, "mass[1][4]"},   {1, 4, 0, -2.0, "mass[1][4]"},  {1, 4, 0, nan, "mass[1][4]"},         {1, 4, 0, inf, "mass[1][4]"},
                        {0, 0, 1, nan, "com[0][0]"},    {2, 7, 3, -inf, "com[2][7]"},   {1, 4, 4, nan, "inertia[1][4]"},      {2, nj - 1, 9, inf, "inertia[2]"},
                        {0, nj - 1, 6, -inf, "inertia[0]"}};
  for (const Case & c : cases)
  {
    std::vector<double> a = good;
    a[(size_t)(c.robot * nj + c.joint) * SIM_BODY_ROW + c.col] = c.value;
    const std::string why = sim_body_admission_error(B, nj, a.data());
    CHECK(has(why, "body parameters") && has(why, c.field));
    // a row is admitted exactly when a robot table carrying it would be
    std::unique_ptr<smpc_robot_model> t(new smpc_robot_model(*go2));
    const double * r = &a[(size_t)(c.robot * nj + c.joint) * SIM_BODY_ROW];
    t->mass[c.joint] = r[0];
    for (int k = 0; k < 3; k++)
      t->com[c.joint][k] = r[1 + k];
    for (int k = 0; k < 6; k++)
      t->inertia[c.joint][k] = r[4 + k];
    CHECK(!robot_table_error(t.get()).empty());
  }
  // the first offender in [robot][joint] order is the one named
  {
    std::vector<double> a = good;
    a[(size_t)(2 * nj + 1) * SIM_BODY_ROW + 0] = -1.0;
    a[(size_t)(1 * nj + 9) * SIM_BODY_ROW + 8] = nan;
    a[(size_t)(1 * nj + 9) * SIM_BODY_ROW + 2] = inf;
    CHECK(has(sim_body_admission_error(B, nj, a.data()), "com[1][9]"));
    CHECK(sim_body_admission_error(1, nj, a.data()).empty()); // (robot 0 alone is fine)
  }
  // 32 joints: the bound of the per-robot array
  {
    std::vector<double> a((size_t)2 * 32 * SIM_BODY_ROW, 1.0);
    CHECK(sim_body_admission_error(2, 32, a.data()).empty());
    a.back() = nan;
    CHECK(has(sim_body_admission_error(2, 32, a.data()), "inertia[1][31]"));
  }
  std::printf("sim_body_dims_check: ok\n");
  return 0;
}
