"""smpc_reset_instances / smpc_reset_instances_device: single instances of a batched handle go back to the constructor's cold start
(solver state restored, problem data untouched; DESIGN.md "Resetting single instances").  CPU tier: every scenario on the
sequential-lane test build of the kernel bodies; tests/test_reset_instances_gpu.py runs the same scenarios on the HIP library.

All comparisons are bitwise (np.array_equal): a reset copies the retained cold solution, and the kernels see the same values at whatever
ring slot they stand."""
import ctypes as C

import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O

H = 10
QUICK_TROT = dict(T_ds=2, T_ss=6)  # contact switches inside a 6-step closed loop at H = 10


def _go2_states(rb, B, seed=20240529):
    return S.random_states(rb, B, seed=seed, scale=0.5)


def _talos_states(rb, B, seed=20240529):
    return S.talos_random_states(rb, B, seed=seed, scale=0.3)


# kind -> (maker, family, gait cycle, measured states, xs are multibody states)
KINDS = {
    "go2_kino": (S.make_product, "kino", lambda: O.trot_cycle(**QUICK_TROT), _go2_states, True),
    "go2_full": (S.make_full_product, "full", lambda: O.trot_cycle(**QUICK_TROT), _go2_states, True),
    "talos_full": (S.make_talos_product, "full", lambda: O.walk_cycle(**QUICK_TROT), _talos_states, True),
    "talos_kino": (S.make_talos_kino_product, "kino", lambda: O.walk_cycle(**QUICK_TROT), _talos_states, True),
    "go2_cent": (S.make_cent_product, "cent", lambda: O.trot_cycle(**QUICK_TROT), _go2_states, False),
    "talos_cent": (S.make_talos_cent_product, "cent", lambda: O.walk_cycle(**QUICK_TROT), _talos_states, False),
}
ALL_KINDS = list(KINDS)
BATCH = {"go2_kino": 66}  # lane_tree_body: 64 consecutive instances per wavefront
SUBSET = {"go2_kino": [0, 63, 64, 65]}  # both ends of a wavefront and across its boundary


def batch_of(kind):
    return BATCH.get(kind, 3)


def subset_of(kind):
    return SUBSET.get(kind, [1])


def make(kind, lib, walk=True, B=None):
    maker, _, cycle, states, _ = KINDS[kind]
    B = B or batch_of(kind)
    gm, rb, _, _ = maker(B, max_iters=1, lib=lib, horizon=H)
    gm.generateCycleHorizon(cycle())
    if walk:
        gm.switchToWalk(np.array([0.2, 0, 0, 0, 0, 0.1]))
        V = np.zeros((B, 6))
        V[:, 0] = np.linspace(0.1, 0.3, B)
        V[:, 5] = np.linspace(-0.1, 0.1, B)
        gm.setVelocityBaseBatched(V)  # one command per instance
    else:
        gm.switchToStand()
    return gm, rb, states(rb, B)


def snapshot(gm, names=("xs", "us", "vs", "lams", "Ks", "info", "status")):
    return {n: np.array(getattr(gm, n)) for n in names}


def assert_same(a, b, rows=None, what=""):
    for n in a:
        u, v = (a[n], b[n]) if rows is None else (a[n][rows], b[n][rows])
        assert np.array_equal(u, v, equal_nan=True), (what, n, float(np.nanmax(np.abs(u - v))))


def next_states(kind, gm, X0, k):
    """Closed loop: the solver's own prediction (a centroidal handle's xs are centroidal states: a shifted measured state instead)."""
    if KINDS[kind][4]:
        return gm.xs[:, 1, :].copy()
    X = X0.copy()
    X[:, 0] += 1e-3 * (k + 1)
    return X


# ---------------------------------------------------------------------------------------------------------------------------------
def cold_start_bitwise(kind, lib):
    """A reset of every instance before the first iterate changes nothing, and nothing of what the first iterate computes."""
    B = batch_of(kind)
    a, rb, X = make(kind, lib)
    b, _, _ = make(kind, lib)
    a.resetInstances(range(B))
    a.wait()
    assert_same(snapshot(a), snapshot(b), what="before iterate")
    a.iterate(X)
    b.iterate(X)
    assert_same(snapshot(a), snapshot(b), what="after iterate")


def isolation_while_walking(kind, lib):
    """Twins in closed loop on the walking gait with per-instance commands; a reset of a subset of A at step 3 leaves every other instance
    of A bit for bit what it is in B, at every later step."""
    B, sub = batch_of(kind), subset_of(kind)
    keep = np.setdiff1d(np.arange(B), sub)
    a, rb, X0 = make(kind, lib)
    b, _, _ = make(kind, lib)
    X = X0.copy()
    names = ("xs", "us", "Ks", "info")
    changed = False
    for k in range(6):
        if k == 3:
            a.resetInstances(sub)
        a.iterate(X)
        b.iterate(X)
        sa, sb = snapshot(a, names), snapshot(b, names)
        assert_same(sa, sb, rows=keep if k >= 3 else None, what="step %d" % k)
        if k >= 3:
            changed = changed or not np.array_equal(sa["us"][sub], sb["us"][sub])
        X = next_states(kind, b, X0, k)
    assert changed  # (the reset did something: the warm start of the subset is gone)


def equals_fresh_handle(kind, lib):
    """Standing (the stage list is the constructor's): after 4 control steps, a reset instance that iterates once is the instance of a
    fresh handle that iterates once on the same measured state -- every buffer the iterate reads was restored or is rewritten."""
    B = 3
    j = 1
    a, rb, X0 = make(kind, lib, walk=False, B=B)
    X = X0.copy()
    for k in range(4):
        a.iterate(X)
        X = next_states(kind, a, X0, k)
    a.resetInstances([j])
    a.iterate(X)
    c, _, _ = make(kind, lib, walk=False, B=B)
    Xc = X0.copy()
    Xc[j] = X[j]
    c.iterate(Xc)
    names = ("xs", "us", "vs", "lams", "K0", "info")
    sa, sc = snapshot(a, names), snapshot(c, names)
    sa["poses"], sc["poses"] = a.getReferencePoses(), c.getReferencePoses()
    assert_same(sa, sc, rows=[j], what="instance %d" % j)


def recovery(kind, lib):
    """A NaN measurement poisons one instance for good; a reset repairs it, and the others never notice either."""
    a, rb, X0 = make(kind, lib, B=3)
    b, _, _ = make(kind, lib, B=3)
    a.iterate(X0)
    b.iterate(X0)
    X = next_states(kind, b, X0, 0)
    Xn = X.copy()
    Xn[1, 9] = np.nan
    a.iterate(Xn)
    b.iterate(X)
    assert a.status[1] & 1
    X = next_states(kind, b, X0, 1)
    a.resetInstances([1])
    a.iterate(X)
    b.iterate(X)
    assert np.array_equal(a.status, [0, 0, 0])
    sa, sb = snapshot(a), snapshot(b)
    for n, v in sa.items():
        assert np.all(np.isfinite(v)), n
    assert sa["info"][1, 2] > 0  # the line search of the repaired instance accepted a step
    assert_same(sa, sb, rows=[0, 2], what="healthy instances")


def device_mask(kind, lib, to_device):
    """The mask form equals the host-list form.  to_device(mask uint8 [B]) -> (pointer, keep-alive)."""
    B, sub = batch_of(kind), subset_of(kind)
    a, rb, X0 = make(kind, lib)
    b, _, _ = make(kind, lib)
    X = X0.copy()
    for k in range(2):
        a.iterate(X)
        b.iterate(X)
        X = next_states(kind, b, X0, k)
    m = np.zeros(B, np.uint8)
    m[sub] = 1
    ptr, keep = to_device(m)
    a.reset_instances_device(ptr)
    a.wait()
    b.resetInstances(sub[::-1] + sub)  # unsorted, duplicates
    assert_same(snapshot(a), snapshot(b), what="after reset")
    assert a.save_state() == b.save_state()
    a.iterate(X)
    b.iterate(X)
    assert_same(snapshot(a), snapshot(b), what="after iterate")
    del keep


def checkpoint_interplay(kind, lib):
    sub = subset_of(kind)
    a, rb, X0 = make(kind, lib)
    d, _, _ = make(kind, lib)
    X = X0.copy()
    for k in range(2):
        a.iterate(X)
        X = next_states(kind, a, X0, k)
    before = snapshot(a)
    blob = a.save_state()
    a.resetInstances(sub)
    assert a.save_state() != blob
    a.load_state(blob)  # save, reset, load: the state from before the reset
    assert a.save_state() == blob
    assert_same(snapshot(a), before, what="save / reset / load")
    # the cold solution is not part of the checkpoint: a handle that loaded resets with its own constructor's copy
    d.load_state(blob)
    d.resetInstances(sub)
    a.resetInstances(sub)
    assert d.save_state() == a.save_state()
    a.iterate(X)
    d.iterate(X)
    assert_same(snapshot(a), snapshot(d), what="load / reset against reset")


def retained_derivatives(kind, lib):
    a, rb, X0 = make(kind, lib, B=3)
    a.setRetainStateDerivatives(True)
    a.iterate(X0)
    assert np.all(np.isfinite(a.getStateDerivative(2)))
    a.resetInstances([1])
    with pytest.raises(RuntimeError, match="smpc_reset_instances has run"):
        a.getStateDerivative(2)
    assert a.getStateDerivative(0).shape[0] == 3  # (stages 0, 1 are solver state: restored, always readable)
    a.iterate(X0)
    assert np.all(np.isfinite(a.getStateDerivative(2)))


def _host_mask(m):
    return m.ctypes.data, m


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_cold_start_bitwise(built, kind):
    cold_start_bitwise(kind, S.emu_lib())


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_isolation_while_walking(built, kind):
    isolation_while_walking(kind, S.emu_lib())


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_equals_fresh_handle(built, kind):
    equals_fresh_handle(kind, S.emu_lib())


@pytest.mark.parametrize("kind", ["go2_kino", "go2_full", "go2_cent"])
def test_recovery_from_a_nan_measurement(built, kind):
    recovery(kind, S.emu_lib())


@pytest.mark.parametrize("kind", ["go2_kino", "talos_full", "go2_cent"])
def test_device_mask_equals_host_list(built, kind):
    device_mask(kind, S.emu_lib(), _host_mask)


@pytest.mark.parametrize("kind", ["go2_kino", "go2_full", "talos_cent"])
def test_checkpoint_interplay(built, kind):
    checkpoint_interplay(kind, S.emu_lib())


@pytest.mark.parametrize("kind", ["go2_kino", "go2_cent"])
def test_retained_derivatives_refuse_until_the_next_iterate(built, kind):
    retained_derivatives(kind, S.emu_lib())


def test_argument_handling(built):
    """Raw C ABI: null arguments and indices outside [0, B) are SMPC_ERR_INVALID and change nothing; duplicates, unsorted lists and n = 0
    are accepted."""
    lib = S.emu_lib()
    R = C.CDLL(S.EMU_LIB)
    R.smpc_last_error.restype = C.c_char_p
    INVALID = -1
    B = 3
    gm, rb, X = make("go2_kino", lib, B=B)
    gm.iterate(X)
    h = C.c_void_p(gm._h.value if hasattr(gm._h, "value") else gm._h)
    before, blob = snapshot(gm), gm.save_state()

    def ints(*v):
        return (C.c_int * len(v))(*v)

    assert R.smpc_reset_instances(None, ints(0), 1) == INVALID and b"null argument" in R.smpc_last_error()
    assert R.smpc_reset_instances(h, None, 1) == INVALID and b"null argument" in R.smpc_last_error()
    assert R.smpc_reset_instances_device(None, ints(0)) == INVALID and b"null argument" in R.smpc_last_error()
    assert R.smpc_reset_instances_device(h, None) == INVALID and b"null argument" in R.smpc_last_error()
    for bad in (B, -1):
        assert R.smpc_reset_instances(h, ints(0, bad, 1), 3) == INVALID and b"out of range" in R.smpc_last_error()
        assert_same(snapshot(gm), before, what="index %d" % bad)
        assert gm.save_state() == blob
    assert R.smpc_reset_instances(h, ints(0), -1) == INVALID
    assert R.smpc_reset_instances(h, None, 0) == 0 and R.smpc_reset_instances(h, ints(0), 0) == 0  # n = 0: a no-op that succeeds
    assert gm.save_state() == blob
    assert R.smpc_reset_instances(h, ints(2, 0, 2, 2, 0), 5) == 0  # unsorted, duplicates
    after = snapshot(gm)
    assert np.array_equal(after["xs"][1], before["xs"][1]) and not np.array_equal(after["xs"][0], before["xs"][0])
    twin, _, _ = make("go2_kino", lib, B=B)
    twin.iterate(X)
    twin.resetInstances([0, 2])
    assert twin.save_state() == gm.save_state()
    with pytest.raises(RuntimeError, match="out of range"):
        gm.resetInstances([B])
