// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_points_dims.h (the admission, the free slots, the band and the sizes of the
// simulator's body points), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/cpp/sim_points_dims_check.cpp -o sim_points_dims_check && ./sim_points_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_points_dims.h"
#include <climits>
#include <limits>

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

static smpc_body_points_settings good()
{
  smpc_body_points_settings s{};
  s.n = 16;
  for (int k = 0; k < 16; k++)
  {
    s.joint[k] = k % 13;
    s.offset[k][0] = 0.01 * k;
    s.offset[k][1] = -0.02;
    s.offset[k][2] = -0.2;
  }
  s.band = 0.03;
  return s;
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int nfeet = 4, P = 1, nj = 13;
  // ---- accepted: null, n = 0 (whatever else the struct holds), the full 16 points, band 0 (the default) ----
  CHECK(sim_points_admission_error(nfeet, P, nj, nullptr).empty());
  {
    smpc_body_points_settings s = good();
    CHECK(sim_points_admission_error(nfeet, P, nj, &s).empty());
    s.band = 0.0;
    CHECK(sim_points_admission_error(nfeet, P, nj, &s).empty());
    s.n = 0;
    s.joint[0] = -5;
    s.offset[3][1] = nan;
    s.band = -1.0;
    CHECK(sim_points_admission_error(nfeet, P, nj, &s).empty()); // (n = 0 clears: nothing else is read)
    CHECK(sim_points_admission_error(2, 4, nj, &s).empty());     // (also where no slot is free)
    s = good();
    s.n = 1;
    s.joint[1] = INT_MAX; // (beyond n: not read)
    s.offset[1][0] = inf;
    CHECK(sim_points_admission_error(nfeet, P, nj, &s).empty());
  }
  // ---- every refusal names the field and the first offending index ----
  {
    smpc_body_points_settings s = good();
    s.n = -1;
    std::string why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "body points") && has(why, "n = -1"));
    s.n = 17;
    why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "n = 17") && has(why, "[0, 16]"));
    s.n = INT_MAX;
    CHECK(!sim_points_admission_error(nfeet, P, nj, &s).empty());
    s.n = INT_MIN;
    CHECK(!sim_points_admission_error(nfeet, P, nj, &s).empty());
  }
  {
    smpc_body_points_settings s = good();
    s.joint[5] = nj;
    s.joint[9] = -1;
    std::string why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "joint[5] = 13") && has(why, "[0, 13)"));
    s.joint[5] = 0;
    why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "joint[9] = -1"));
    s.joint[9] = INT_MIN;
    CHECK(has(sim_points_admission_error(nfeet, P, nj, &s), "joint[9]"));
    s.joint[9] = INT_MAX;
    CHECK(has(sim_points_admission_error(nfeet, P, nj, &s), "joint[9]"));
    s.joint[9] = nj - 1;
    CHECK(sim_points_admission_error(nfeet, P, nj, &s).empty());
  }
  for (double bad : {nan, inf, -inf})
  {
    smpc_body_points_settings s = good();
    s.offset[15][2] = bad;
    s.offset[7][1] = bad;
    const std::string why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "offset[7][1]") && has(why, "finite"));
  }
  for (double bad : {nan, inf, -inf, -1e-300, -0.01})
  {
    smpc_body_points_settings s = good();
    s.band = bad;
    const std::string why = sim_points_admission_error(nfeet, P, nj, &s);
    CHECK(has(why, "band"));
  }
  {
    smpc_body_points_settings s = good(); // no free slot: 2 feet of 4 points, 4 feet of 2, 8 feet of 1
    for (int f : {2, 4, 8})
    {
      const std::string why = sim_points_admission_error(f, 8 / f, nj, &s);
      CHECK(has(why, "no free slot") && has(why, "= 8"));
    }
    CHECK(sim_points_admission_error(7, 1, nj, &s).empty());
  }
  // ---- the slots, the band and the sizes at their limits ----
  CHECK(sim_points_free_slots(4, 1) == 4 && sim_points_free_slots(2, 1) == 6 && sim_points_free_slots(2, 4) == 0 && sim_points_free_slots(1, 1) == 7);
  CHECK(sim_points_band(0.0) == SIM_POINTS_DEFAULT_BAND && sim_points_band(0.05) == 0.05 && sim_points_band(5e-324) == 5e-324);
  CHECK(sim_points_joint_bytes() == 64 && sim_points_offset_bytes() == 384);
  CHECK(sizeof(smpc_body_points_settings) == 4 + 64 + 4 + 384 + 8); // (the layout the Python mirror declares)
  CHECK(sim_points_slots_bytes(1) == 32 && sim_points_lam_bytes(1) == 192 && sim_points_gap_bytes(1) == 128 && sim_points_dropped_bytes(1) == 4
        && sim_points_touch_bytes(1) == 1);
  const int big = INT_MAX; // (size_t arithmetic: no overflow in int)
  CHECK(sim_points_lam_bytes(big) == (size_t)big * 192 && sim_points_gap_bytes(big) == (size_t)big * 128 && sim_points_slots_bytes(big) == (size_t)big * 32
        && sim_points_touch_bytes(big) == (size_t)big);
  std::printf("sim_points_dims_check: ok\n");
  return 0;
}
