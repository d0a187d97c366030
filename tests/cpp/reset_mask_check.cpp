// Stand-alone host program for the host half of smpc_reset_instances (simple-mpc_amd/csrc/smpc_reset_mask.h): the instance list -> byte
// mask conversion and its index validation.  Built with -fsanitize=address,undefined by tests/test_reset_mask_host.py; the mask lives in a
// heap block of exactly B bytes, so that a write outside [0, B) is a sanitizer report and not a silent pass.
#include "smpc_reset_mask.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                                                    \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(cond))                                                                                                       \
    {                                                                                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                            \
      failures++;                                                                                                      \
    }                                                                                                                  \
  } while (0)

static std::vector<unsigned char> expect(int B, const std::vector<int> & idx)
{
  std::vector<unsigned char> m(B, 0);
  for (int i : idx)
    m[i] = 1;
  return m;
}

int main()
{
  using smpc::reset_mask_from_list;
  for (int B : {1, 3, 63, 64, 65, 66, 4096})
  {
    unsigned char * mask = (unsigned char *)std::malloc((size_t)B);
    auto same = [&](const std::vector<unsigned char> & want) {
      for (int b = 0; b < B; b++)
        if (mask[b] != want[b])
          return false;
      return true;
    };
    // both ends, unsorted, duplicates; a mask that held something else before
    for (int b = 0; b < B; b++)
      mask[b] = 0xAB;
    std::vector<int> idx = {B - 1, 0, B - 1, B / 2, 0};
    CHECK(reset_mask_from_list(idx.data(), (int)idx.size(), B, mask) == -1);
    CHECK(same(expect(B, idx)));
    // every instance, descending
    idx.clear();
    for (int b = B - 1; b >= 0; b--)
      idx.push_back(b);
    CHECK(reset_mask_from_list(idx.data(), B, B, mask) == -1);
    CHECK(same(std::vector<unsigned char>(B, 1)));
    // an empty list clears the mask (a null list is never read)
    CHECK(reset_mask_from_list(nullptr, 0, B, mask) == -1);
    CHECK(same(std::vector<unsigned char>(B, 0)));
    // an index outside [0, B), wherever it stands in the list: its position is returned and not one byte is written
    for (int bad : {B, -1, B + 1000000, -2147483647 - 1, 2147483647})
      for (int pos = 0; pos < 3; pos++)
      {
        for (int b = 0; b < B; b++)
          mask[b] = 0xCD;
        std::vector<int> l = {0, B - 1, 0};
        l[pos] = bad;
        CHECK(reset_mask_from_list(l.data(), 3, B, mask) == pos);
        CHECK(same(std::vector<unsigned char>(B, 0xCD)));
      }
    std::free(mask);
  }
  if (failures == 0)
    std::printf("reset mask check: OK\n");
  return failures == 0 ? 0 : 1;
}
