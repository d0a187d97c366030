// smpc_reset_mask.h -- host half of smpc_reset_instances: an instance list -> the byte mask [B] the reset kernel reads (smpc_reset.h).
// Plain C++ with no backend behind it, so that a stand-alone host program can exercise it (tests/cpp/reset_mask_check.cpp).
#pragma once

namespace smpc
{
  // mask[b] = 1 for every b in idx[0 .. n), 0 elsewhere.  The list may be unsorted and may name an instance more than once.  Returns -1,
  // or the position of the first index outside [0, B): the mask is then untouched (the list is checked before the first byte is written).
  inline int reset_mask_from_list(const int * idx, int n, int B, unsigned char * mask)
  {
    for (int i = 0; i < n; i++)
      if (idx[i] < 0 || idx[i] >= B)
        return i;
    for (int b = 0; b < B; b++)
      mask[b] = 0;
    for (int i = 0; i < n; i++)
      mask[idx[i]] = 1;
    return -1;
  }
} // namespace smpc
