"""An instance's result must not depend on the batch around it: its position (lane, wave), the batch size (B = 1, < 64, = 64, a partial wave,
padding that changes per = ceil(B / 64) of compact_body), how many instances backtrack at once (more than the LS_SLOTS = 64 instance slots of the
list-mode launches: the list is walked in several strides) or the schedule (speculative / sequential line search, parts of the batch on streams of
their own).  tests/batch_check.py builds, per family, a pool of 150 distinct measured states on which THE ORACLE backtracks more than 64 instances
in the first iteration and in the final line search of control step 0, and solves it in several arrangements: every output a caller can read is
compared bit for bit, the in-order arrangement also with the oracle.  CPU tier: the emulated kernel bodies; -m gpu: the same on the device.

Pools (seed 3; counts of the oracle at control step 0 out of 150, max_iters = 1 / max_iters = 3; printed by every run):

  family         H = 20 (device)            CPU tier
  go2_kino       scale 16:   71 / 148       H = 20, the same pool.  At H = 6 the first iteration rejects alpha = 1 for at most 15 instances at any
                                            scale (2 / 5 / 7 / 10 / 11 / 15 / 14 at scales 12 / 16 / 20 / 24 / 32 / 48 / 64), 37 at H = 12
  go2_kino_ext   scale 1:    93 / 92        H = 6, scale 1: 123 / 125  (scale 2: 139 / 139, 4: 148 / 149, 8 and 16: 150 / 150 -- no instance left out)
  go2_full       scale 3:   141 / 116       H = 6, scale 6: 132 / 123  (H = 20: scale 4: 150 / 142, 6: 149 / 150; H = 6: scale 4: 71 / 58, 5: 112 / 84)
  talos_full     scale 3:   122 / 147       H = 6, scale 3: 107 / 144
  talos_kino6d   scale 4:    85 / 138       H = 6, scale 6: 100 / 147  (scale 4: 57 / 125)
  go2_cent       scale 2:   150 / 150       H = 6, scale 2: 150 / 150
  talos_cent     scale 6:   121 / 116       H = 6, scale 6: 118 / 113

"At least 3 instances do not backtrack" is asserted on the first iteration's list (the one the speculative scheme restores, backtracks and
re-derives in list mode); the final line search must leave at least one instance out (Go2 kinodynamics at scale 16: 148 of 150).
go2_cent: the point-foot centroidal oracle takes alpha < 1 for EVERY instance of the pool at control step 0 at every scale tried (0, 0.001, 0.01,
0.03, 0.1, 0.25, 0.5, 1, 2, 3, 6, 12: 150 / 150 each, all outputs finite), so "a proper subset" cannot be had there: its arrangements are kept with
that list of 150.  (The centroidal engines have no undecided list and no speculative scheme -- one fused kernel per control step and part,
lane per (instance, candidate) -- and do not read SMPC_NO_SPECULATIVE_LS: arrangement A4 holds for go2_cent by construction.)

Sizes on the device (B = 150, H = 20: 150 * 21 = 3150 (instance, stage) items; MI355X: 256 CUs):
  kinodynamics (Go2): the (instance, stage) kernels are launched as xcd_grid(150, 20) = 4096 blocks (8 tiles x 64 per group, smpc_kino_lane.h) on
    256 x 8 = 2048 resident wavefronts: the grid wraps; list mode: xcd_grid(64, 20) = 1536 blocks walking a list of up to 148 entries.  The
    sweeps themselves are one block per instance (150).
  fdyn_deriv_body (Talos, WIDE_DEV): sizeof(FullScratch<D, true>) = 40000 (full dynamics) / 40288 (kinodynamics, 6-D feet) bytes -> 4 blocks per
    CU, n_res = 1024 persistent blocks < 3150 items (3 or 4 items per block); list mode: 64 * 21 = 1344 slot items > 1024, and the (list entry,
    stage) pairs of a list of up to 147 entries (3087 pairs) dealt round-robin over 1024 blocks.
  Go2 full dynamics (WIDE_DEV = false): no persistent grid, 3150 blocks; list mode 1344 blocks walking the list in strides of 64.

Parity with the oracle at control step 0: decisions by S.alphas_agree and identical for >= 90 % of the instances; xs and us of the instances with
identical decisions at TOL = 1e-4, the bar of each family's own parity test of a backtracking scenario (test_gpu_parity.py::
test_line_search_backtracking_matches, test_fulldynamics_mpc.py::test_hip_unusual_horizon_and_backtracking, test_talos_*.py, test_centroidal_mpc.py::
test_gpu_active_friction_cones).  One instance of one pool is gated at 10 x the oracle's own disagreement instead: batch_check.SENSITIVE."""
import numpy as np
import pytest

import batch_check as BC
import mpc_setup as S
import oracle_lib as O

FAMILIES = list(BC.FAMILIES)
# CPU tier: the emulated lanes are sequential, so the horizon is 6 where the pool conditions can be met there (module docstring).  Every arrangement
# runs for every family (the slowest, Talos full dynamics, takes 40 s)
CPU_H = dict(go2_kino=20, go2_kino_ext=6, go2_full=6, talos_full=6, talos_kino6d=6, go2_cent=6, talos_cent=6)


def _calls(gm, slot):
    return gm.kernel_times()[slot][1]


def _case(family, lib, horizon, seq_lib):
    fam = BC.FAMILIES[family]
    p = BC.pool(family, horizon)
    BC.check_pool(p, family)
    X0, rb = p["X"], p["rb"]
    a0 = BC.run(family, [(BC.make_handle(family, BC.N, lib, horizon), np.arange(BC.N))], X0, rb)
    BC.check_parity(family, horizon, p, a0[0])
    n_own = [BC.backtracked(r["info"]) for r in a0]
    print("%s: the handle backtracks %s of %d instances in the final line search of control steps 0, 1" % (family, n_own, BC.N))
    for name, pieces in BC.arrangements(family).items():
        handles = [(BC.make_handle(family, B, lib, horizon, env), idx) for B, idx, env in pieces]
        BC.same_bits(a0, BC.run(family, handles, X0, rb), "%s, %s" % (family, name))
    if fam["sequential"]:
        # A4: the sequential line search of a cross-check build against its speculative scheme (bit identity: the claim of
        # test_kernel_bodies_emu.py::test_speculative_line_search_is_the_sequential_algorithm at B = 6).  Two host schedules
        # (StageEngine::run_iteration / speculative_step): every output bit for bit, of info the solver's scalars -- its column 12 is the
        # speculative scheme's own scratch (BC.INFO_SOLVER), 1e-9 / 3 there and never written by the sequential scheme
        base = a0 if seq_lib is lib else BC.run(family, [(BC.make_handle(family, BC.N, seq_lib, horizon), np.arange(BC.N))], X0, rb)
        seq_env = {"SMPC_NO_SPECULATIVE_LS": "1"}
        seq = BC.run(family, [(BC.make_handle(family, BC.N, seq_lib, horizon, seq_env), np.arange(BC.N))], X0, rb)
        BC.same_bits(base, seq, "%s, A4 sequential scheme" % family, info_cols=BC.INFO_SOLVER)
        if family == "go2_kino":  # the switch must have selected the other schedule: an explicit alpha = 1 trial in every iteration
            pair = [BC.make_handle(family, 2, seq_lib, horizon, env) for env in (None, seq_env)]
            for g in pair:
                g.iterate(X0[:2])
            assert _calls(pair[1], "trial") > _calls(pair[0], "trial"), "SMPC_NO_SPECULATIVE_LS did not select the sequential scheme"


@pytest.mark.parametrize("family", FAMILIES)
def test_emulated_batch_independence(built, family):
    lib = S.emu_lib()
    _case(family, lib, CPU_H[family], lib)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_hip_batch_independence(built, family):
    _case(family, None, 20, S.xcheck_lib() if BC.FAMILIES[family]["sequential"] else None)


def _gains_of_parts(lib):
    """The feedback gains a caller reads (K0, Ks, the K0 block of gatherOutputs) of a kinodynamics batch run as two parts (SMPC_STREAMS = 2) are
    those of the one-part handle.  The view of part 1 used to start max(G_STRIDE, GainsK::STRIDE) = 2224 doubles per (instance, stage) into the
    gains buffer while the read-out kernels index the whole buffer by the structured sweep's GainsK::STRIDE = 1592: xs and us were right (sweeps
    of a part write and read through the same view), the gains of every instance of part 1 were read from the wrong place.  B = 128: the smallest
    batch that runs as two parts (B >= 64 per part)."""
    B, H = 128, 6
    got = []
    for env in (None, {"SMPC_STREAMS": "2"}):
        gm = BC.make_handle("go2_kino", B, lib, H, env)
        gm.iterate(S.random_states(O.Robot("go2_like"), B, seed=BC.SEED))
        rows = np.zeros((B, gm.nx + gm.nu + gm.nu * gm.ndx))
        gm.gatherOutputs(rows)
        gm.wait()
        got.append(dict(xs=gm.xs, us=gm.us, K0=gm.K0, Ks=gm.Ks, rows=rows))
    assert np.all(np.isfinite(got[0]["Ks"])) and np.array_equal(got[0]["Ks"][:, 0], got[0]["K0"])
    assert np.array_equal(got[0]["rows"][:, gm.nx + gm.nu:].reshape(B, gm.nu, gm.ndx), got[0]["K0"])
    for name in got[0]:
        assert np.array_equal(got[0][name], got[1][name]), "%s of the batch in two parts differs from the one-part handle's" % name


def test_emulated_gains_of_a_batch_in_parts(built):
    _gains_of_parts(S.emu_lib())


@pytest.mark.gpu
def test_hip_gains_of_a_batch_in_parts(built):
    _gains_of_parts(None)
