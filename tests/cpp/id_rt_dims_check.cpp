// Stand-alone host check of simple-mpc_amd/csrc/smpc_id_rt_dims.h (sizes, dispatch, limit lengths, ancestor sets of the inverse-dynamics
// engine on a run-time joint tree), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/id_rt_dims_check.cpp -o id_rt_dims_check && ./id_rt_dims_check
#include "../../simple-mpc_amd/csrc/smpc_id_rt_dims.h"
#include <cstdlib>
#include <cstring>
#include <memory>

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

// a chain with two branches on the base: joints 1 .. nj - 1, every third one a child of the base
static void fill(smpc_robot_model & m, int nj, int nfeet)
{
  std::memset(&m, 0, sizeof(m));
  m.njoints = nj;
  m.nq = nj + 6;
  m.nv = nj + 5;
  m.nfeet = nfeet;
  m.parent[0] = -1;
  double msum = 0.0;
  for (int j = 0; j < nj; j++)
  {
    if (j > 0)
    {
      m.parent[j] = j % 3 == 1 ? 0 : j - 1;
      m.jtype[j] = 1 + j % 3;
    }
    m.mass[j] = 1.0 + 0.1 * j;
    msum += m.mass[j];
    m.jp_R[j][0] = m.jp_R[j][4] = m.jp_R[j][8] = 1.0;
  }
  m.total_mass = msum;
  m.q_ref[6] = 1.0;
  for (int f = 0; f < nfeet && f < SMPC_MAX_FEET; f++)
    m.foot_joint[f] = (f + 1) % nj;
}

int main()
{
  auto rm = std::make_unique<smpc_robot_model>();
  std::string why;
  // sizes: the two ends and quad_arm
  IdRtSizes s = id_rt_sizes(SMPC_MAX_JOINTS);
  CHECK(s.nv == ID_RT_MAX_NV && s.n == ID_RT_MAX_N && s.m == 114 && s.gr == ID_RT_MAX_GR && s.np == 64 && s.mp == 128);
  s = id_rt_sizes(19);
  CHECK(s.n == 36 && s.m == 88 && s.np == 48 && s.mp == 96 && s.na == 18);
  s = id_rt_sizes(2);
  CHECK(s.n == 19 && s.np == 32 && s.gr == 35);
  for (int nj = 2; nj <= SMPC_MAX_JOINTS; nj++)
  {
    s = id_rt_sizes(nj);
    CHECK(s.np == 32 || s.np == 48 || s.np == 64);
    CHECK(s.gr <= (s.np + 16 < ID_RT_MAX_GR ? s.np + 16 : ID_RT_MAX_GR) && s.n <= s.np && s.m <= s.mp);
  }
  // routes
  fill(*rm, 13, 4);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_GO2);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, true, why) == ID_ROUTE_RT && why.empty());
  fill(*rm, 23, 2);
  CHECK(id_route(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_TALOS);
  fill(*rm, 19, 2);
  CHECK(id_route(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("flat feet") != std::string::npos);
  fill(*rm, 19, 4);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_RT);
  fill(*rm, 19, 3);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("nfeet = 3") != std::string::npos);
  fill(*rm, 19, 4);
  rm->parent[5] = 7;
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("parent[5]") != std::string::npos);
  fill(*rm, 19, 4);
  rm->njoints = 1000; // nothing past the table's bounds is read
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("njoints") != std::string::npos);
  fill(*rm, 19, 4);
  rm->nfeet = -5;
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED);
  // limit vectors
  CHECK(id_limits_error(18, 18, 18, 18, 18).empty());
  CHECK(id_limits_error(18, 17, 18, 18, 18).find("effort_limit has 17") != std::string::npos);
  CHECK(id_limits_error(18, 18, 18, 18, 0).find("q_max") != std::string::npos);
  // ancestor sets
  fill(*rm, SMPC_MAX_JOINTS, 4);
  const std::vector<unsigned> anc = id_rt_ancestors(rm.get());
  CHECK(anc.size() == (size_t)SMPC_MAX_JOINTS && anc[0] == 1u);
  for (int j = 1; j < SMPC_MAX_JOINTS; j++)
  {
    CHECK((anc[j] & 1u) && ((anc[j] >> j) & 1u) && (anc[j] >> j) == 1u);
    CHECK(anc[j] == (anc[rm->parent[j]] | (1u << j)));
  }
  std::printf("id_rt_dims_check: ok\n");
  return 0;
}
