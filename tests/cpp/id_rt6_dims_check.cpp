// Stand-alone host check of the flat-foot half of simple-mpc_amd/csrc/smpc_id_rt_dims.h (id_rt6_sizes, id_route_any), meant to be built with
// -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/id_rt6_dims_check.cpp -o id_rt6_dims_check && ./id_rt6_dims_check
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
  std::string why, why0;
  // sizes: biped_legs, talos_like, tree32, the smallest table
  IdRt6Sizes s = id_rt6_sizes(13);
  CHECK(s.n == 42 && s.m == 106 && s.np == 48 && s.mp == 112 && s.na == 12 && s.dr == 30 && s.nf == 2);
  s = id_rt6_sizes(23);
  CHECK(s.n == 52 && s.m == 126 && s.np == 64 && s.mp == 128 && s.dr == 40);
  s = id_rt6_sizes(SMPC_MAX_JOINTS);
  CHECK(s.nv == ID_RT_MAX_NV && s.n == ID_RT6_MAX_N && s.n == 61 && s.m == 144 && s.np == 64 && s.mp == 144 && s.dr == ID_RT6_MAX_DR && s.dr == 49);
  s = id_rt6_sizes(2);
  CHECK(s.n == 31 && s.m == 84 && s.np == 32 && s.mp == 96 && s.dr == 19);
  for (int nj = 2; nj <= SMPC_MAX_JOINTS; nj++)
  {
    s = id_rt6_sizes(nj);
    CHECK(s.np == 32 || s.np == 48 || s.np == 64);
    CHECK(s.n <= s.np && s.m <= s.mp && s.dr <= 64 && s.fr == 34 && s.gr == s.dr + s.fr && s.m == s.n + 52 + s.na);
    CHECK(s.dr <= s.np - 12 && s.dr <= ID_RT6_MAX_DR); // what an instantiation of the solver holds in LDS
    CHECK(s.nq == nj + 6 && s.nv == nj + 5 && s.n == s.nv + 24);
  }
  // the point-foot sizes stay
  const IdRtSizes p = id_rt_sizes(19);
  CHECK(p.n == 36 && p.m == 88 && p.np == 48 && p.mp == 96 && p.na == 18);
  // routes of id_route_any: id_route's wherever id_route does not refuse for flat feet
  const int shapes[5][2] = {{13, 4}, {23, 2}, {19, 4}, {19, 3}, {13, 2}};
  for (int k = 0; k < 5; k++)
    for (int flat = 0; flat < 2; flat++)
      for (int force = 0; force < 2; force++)
      {
        fill(*rm, shapes[k][0], shapes[k][1]);
        const IdRoute r0 = id_route(rm.get(), flat != 0, 13, 4, 23, 2, force != 0, why0);
        const IdRoute r1 = id_route_any(rm.get(), flat != 0, 13, 4, 23, 2, force != 0, why);
        const bool flat_refusal = r0 == ID_ROUTE_REFUSED && flat && why0.find("flat feet") != std::string::npos;
        if (!flat_refusal && !(flat && force && r0 == ID_ROUTE_TALOS))
          CHECK(r1 == r0 && why == why0);
        CHECK(r0 != ID_ROUTE_RT6); // (id_route never answers with the new route)
      }
  fill(*rm, 13, 4);
  CHECK(id_route_any(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_GO2);
  CHECK(id_route_any(rm.get(), false, 13, 4, 23, 2, true, why) == ID_ROUTE_RT && why.empty());
  fill(*rm, 23, 2);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_TALOS);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, true, why) == ID_ROUTE_RT6 && why.empty());
  CHECK(id_route(rm.get(), true, 13, 4, 23, 2, true, why) == ID_ROUTE_TALOS); // (the debug switch does not reach flat feet through id_route)
  fill(*rm, 13, 2);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_RT6 && why.empty());
  fill(*rm, SMPC_MAX_JOINTS, 2);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_RT6);
  fill(*rm, 2, 2);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_RT6);
  fill(*rm, 19, 4);
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("nfeet = 4") != std::string::npos
        && why.find("built for 2 flat feet") != std::string::npos);
  fill(*rm, 19, 2);
  rm->parent[5] = 7;
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("parent[5]") != std::string::npos);
  fill(*rm, 19, 2);
  rm->njoints = 1000; // nothing past the table's bounds is read
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("njoints") != std::string::npos);
  fill(*rm, 19, 2);
  rm->nfeet = -5;
  CHECK(id_route_any(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED);
  // id_route itself: the sibling's cases, unchanged
  fill(*rm, 19, 2);
  CHECK(id_route(rm.get(), true, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("flat feet") != std::string::npos
        && why.find("instantiated for 13 joints / 4 point feet and for 23 joints / 2 flat feet") != std::string::npos);
  fill(*rm, 19, 4);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_RT);
  fill(*rm, 19, 3);
  CHECK(id_route(rm.get(), false, 13, 4, 23, 2, false, why) == ID_ROUTE_REFUSED && why.find("nfeet = 3") != std::string::npos);
  std::printf("id_rt6_dims_check: ok\n");
  return 0;
}
