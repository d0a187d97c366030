// smpc_sweep_order.h -- the order in which a block of sweeps_kino_body (smpc_riccati_kino.h) walks its instances: which slot owns
// which instances, and which (instance, phase) is step k of a slot's walk.  Plain constexpr C++ with no backend behind it (constexpr
// functions are callable from device code), so that a stand-alone host program can print and check the orders
// (tests/cpp/sweep_order_check.cpp).
//
// A grid of nslots blocks; slot s owns the instances s, s + nslots, s + 2 nslots, ... < B (its j-th is s + j nslots).  Phases of an
// instance: B = backward (Riccati) sweep, then F = forward sweep, which needs that instance's gains only.  Even slots walk  B F  per
// instance, odd slots walk pairs  B B F F  (a last unpaired instance as B F): once the first backward sweeps are over, the two kinds of
// slot are in opposite phases.
#pragma once

namespace smpc
{
  struct SweepStep
  {
    int j;    // the slot's j-th instance
    bool fwd; // false: backward sweep, true: forward sweep
  };
  // instances of slot s
  constexpr int sweeps_slot_count(int s, int nslots, int B) { return s < B ? (B - s + nslots - 1) / nslots : 0; }
  // kind of slot s: bit `shift` of s (0: even / odd slots.  Blocks s and s + 8 share an XCD, so with shift 0 the slots of one XCD are all
  // of one kind; shift 3 alternates the kinds inside every XCD)
  constexpr bool sweeps_slot_paired(int s, int shift = 0) { return ((s >> shift) & 1) != 0; }
  // step k = 0 .. 2 m - 1 of the walk of a slot that owns m instances
  constexpr SweepStep sweeps_slot_step(bool paired, int m, int k)
  {
    if (!paired)
      return SweepStep{k >> 1, (k & 1) != 0};
    const int q = k >> 2, r = k & 3; // pair q = the slot's instances 2 q and 2 q + 1: steps 4 q .. 4 q + 3
    if (2 * q + 1 < m)
      return SweepStep{2 * q + (r & 1), r >= 2};
    return SweepStep{2 * q, r != 0}; // the last, unpaired one: steps 4 q and 4 q + 1
  }
} // namespace smpc
