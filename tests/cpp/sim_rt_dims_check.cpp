// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_rt_dims.h (sizes and admission of the rigid-body simulator on a run-time joint
// tree), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/sim_rt_dims_check.cpp -o sim_rt_dims_check && ./sim_rt_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_rt_dims.h"
#include <cstdlib>
#include <cstring>
#include <limits>
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
  for (int j = 0; j < nj && j < SMPC_MAX_JOINTS; j++)
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
static bool has(const std::string & s, const char * w) { return s.find(w) != std::string::npos; }

int main()
{
  auto rm = std::make_unique<smpc_robot_model>();
  // sizes: the bound of every array, quad_arm with point feet, a biped with flat feet
  SimRtSizes s = sim_rt_sizes(SMPC_MAX_JOINTS, 4, 3);
  CHECK(s.nq == 38 && s.nv == SIM_RT_MAX_NV && s.nx == 75 && s.na == 31 && s.nlam == SIM_RT_MAX_ROWS);
  s = sim_rt_sizes(19, 4, 3);
  CHECK(s.nq == 25 && s.nv == 24 && s.nx == 49 && s.na == 18 && s.nlam == 12 && s.fs == 3 && s.nfeet == 4);
  s = sim_rt_sizes(13, 2, 6);
  CHECK(s.nlam == 12 && s.na == 12);
  // admitted: every joint count with 1 .. 4 point feet and with 1 .. 2 flat feet -- never more than 12 contact rows
  for (int nj = 2; nj <= SMPC_MAX_JOINTS; nj++)
    for (int fs = 3; fs <= 6; fs += 3)
      for (int nf = 1; nf <= SMPC_MAX_FEET; nf++)
      {
        fill(*rm, nj, nf);
        const std::string why = sim_rt_admission_error(rm.get(), fs, 1);
        const bool ok = fs * nf <= SIM_RT_MAX_ROWS;
        CHECK(why.empty() == ok);
        if (!ok)
          CHECK(has(why, "nfeet = ") && has(why, "force_size 6"));
        else
          CHECK(sim_rt_sizes(nj, nf, fs).nlam <= SIM_RT_MAX_ROWS && sim_rt_sizes(nj, nf, fs).nv <= SIM_RT_MAX_NV);
      }
  // refused, each with the field in the message
  fill(*rm, 19, 4);
  CHECK(has(sim_rt_admission_error(rm.get(), 6, 1), "nfeet = 4"));
  CHECK(has(sim_rt_admission_error(rm.get(), 4, 1), "force_size = 4"));
  CHECK(has(sim_rt_admission_error(rm.get(), 0, 1), "force_size = 0"));
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 0), "batch = 0"));
  CHECK(has(sim_rt_admission_error(rm.get(), 3, -7), "batch = -7"));
  CHECK(sim_rt_admission_error(rm.get(), 3, 4096).empty());
  fill(*rm, 19, 0);
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "nfeet = 0"));
  fill(*rm, 19, 4);
  rm->nfeet = -5;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "nfeet = -5"));
  fill(*rm, 19, 4);
  rm->nfeet = 1000; // nothing past the table's bounds is read
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "nfeet = 1000"));
  fill(*rm, 33, 4);
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "njoints = 33"));
  fill(*rm, 1, 1);
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "njoints = 1"));
  fill(*rm, 19, 4);
  rm->njoints = 1000;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "njoints = 1000"));
  fill(*rm, 19, 4);
  rm->parent[5] = 7;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "parent[5]"));
  fill(*rm, 19, 4);
  rm->mass[4] = -1.0;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "mass[4]"));
  fill(*rm, 19, 4);
  rm->mass[4] = std::numeric_limits<double>::quiet_NaN();
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "mass[4]"));
  fill(*rm, 19, 4);
  rm->total_mass *= 1.001;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "total_mass"));
  fill(*rm, 19, 4);
  rm->foot_joint[2] = 19;
  CHECK(has(sim_rt_admission_error(rm.get(), 3, 1), "foot_joint[2]"));
  std::printf("sim_rt_dims_check: ok\n");
  return 0;
}
