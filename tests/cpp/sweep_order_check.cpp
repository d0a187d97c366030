// Host check of smpc_sweep_order.h: the walks of the slots of sweeps_kino_body for the shapes of tests/test_fused_sweeps.py (printed as
// strings of B / F per slot) and, for a range of (nslots, B), the properties the fused launch rests on: every instance below B is owned
// by exactly one slot, has its backward sweep exactly once and its forward sweep exactly once, the backward one first; no slot walks an
// instance at or beyond B; an even slot never has two backward sweeps in a row, an odd slot pairs them.
#include <cstdio>
#include <string>
#include <vector>
#include "smpc_sweep_order.h"

static int failures = 0;
#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);                                                       \
      failures++;                                                                                                      \
    }                                                                                                                  \
  } while (0)

static std::string walk(int s, int nslots, int B, std::vector<int> * state)
{
  using namespace smpc;
  const int m = sweeps_slot_count(s, nslots, B);
  std::string out;
  for (int k = 0; k < 2 * m; k++)
  {
    const SweepStep st = sweeps_slot_step(sweeps_slot_paired(s), m, k);
    const int inst = s + st.j * nslots;
    CHECK(st.j >= 0 && st.j < m && inst < B);
    if (inst < B && state)
    {
      // 0 untouched -> 1 backward done -> 2 forward done
      CHECK((*state)[inst] == (st.fwd ? 1 : 0));
      (*state)[inst]++;
    }
    out += st.fwd ? 'F' : 'B';
  }
  return out;
}

static std::string all(int nslots, int B)
{
  std::vector<int> state(B, 0);
  std::string out;
  for (int s = 0; s < nslots; s++)
    out += (s ? " / " : "") + walk(s, nslots, B, &state);
  for (int i = 0; i < B; i++)
    CHECK(state[i] == 2);
  return out;
}

int main()
{
  const int cases[5][2] = {{2, 3}, {2, 4}, {2, 7}, {3, 7}, {1, 3}};
  const char * want[5] = {"BFBF / BF", "BFBF / BBFF", "BFBFBFBF / BBFFBF", "BFBFBF / BBFF / BFBF", "BFBFBF"};
  for (int c = 0; c < 5; c++)
  {
    const std::string got = all(cases[c][0], cases[c][1]);
    std::printf("nslots %d, B %d: %s\n", cases[c][0], cases[c][1], got.c_str());
    CHECK(got == want[c]);
  }
  for (int nslots = 1; nslots <= 9; nslots++)
    for (int B = 1; B <= 40; B++)
    {
      all(nslots, B);
      for (int s = 0; s < nslots; s++)
      {
        const std::string w = walk(s, nslots, B, nullptr);
        if (s % 2 == 0)
          CHECK(w.find("BB") == std::string::npos && w.find("FF") == std::string::npos);
        else
          CHECK(w.find("BBB") == std::string::npos && w.find("FFF") == std::string::npos && (w.size() < 4 || w.substr(0, 4) == "BBFF"));
      }
    }
  // the grid of the headline shape: two instances per slot
  CHECK(walk(0, 2048, 4096, nullptr) == "BFBF" && walk(1, 2048, 4096, nullptr) == "BBFF" && walk(2047, 2048, 4096, nullptr) == "BBFF");
  if (failures)
    return 1;
  std::printf("sweep order check: OK\n");
  return 0;
}
