"""GPU tier of tests/test_id_flat_any_robot.py: the same helpers on the HIP library (B = 3), block independence at B = 65 / 64 / 1,
replicas, and a NaN state that stays in its own robot."""
import numpy as np
import pytest

import robot_tables as RT
import test_id_flat_any_robot as T

pytestmark = pytest.mark.gpu


def test_refusal_is_gone(built):
    T.refusal_is_gone(None)


@pytest.mark.parametrize("centroidal", [False, True])
@pytest.mark.parametrize("name", T.ROBOTS)
def test_quantities_qp_and_solution(built, name, centroidal):
    T.pieces(name, None, centroidal)


@pytest.mark.parametrize("variant", [dict(contact_motion_equality=True), dict(tsid_joint_bounds=True), dict(contact_motion_equality=True, tsid_joint_bounds=True),
                                     dict(base_reference_as_coded=True)])
def test_qp_variants(built, variant):
    T.pieces("biped_legs", None, False, **variant)
    T.pieces("tree32", None, True, **variant)


@pytest.mark.parametrize("centroidal", [False, True])
@pytest.mark.parametrize("name", T.ROBOTS)
def test_solution_at_fixed_work(built, name, centroidal):
    T.pieces(name, None, centroidal, solution=True)


@pytest.mark.parametrize("name", T.ROBOTS)
def test_warm_started_ticks(built, name):
    T.standing_loop(name, None, 20, 1e-5, **T.KINO)


@pytest.mark.parametrize("name,ticks", [("biped_legs", 40), ("tree32", 20)])
def test_default_stopping_rule(built, name, ticks):
    """The early exit, the residual of the checked iterate and the rho re-factorisation on the device."""
    T.standing_loop(name, None, ticks, 1e-4, resid_bars=True, admm_iters=400, admm_tol=1e-7, **dict(T.KINO, contact_motion_equality=True))


@pytest.mark.parametrize("centroidal", [False, True])
def test_run_time_engine_against_templated_engine(built, centroidal):
    w = T.rt_vs_templated(None, centroidal)
    assert w["quant"] < 1e-11 and w["qp"] < 1e-11 and w["tau"] < 1e-8, w


def test_targets_from_run_time_centroidal_mpc(built):
    T.resident_targets(None)


@pytest.mark.parametrize("name", T.ROBOTS)
def test_blocks_are_independent(built, name):
    """B = 65 against handles of B = 64 and B = 1 holding the same robots, bitwise; replicas inside a batch are bit-identical."""
    tab = RT.table(name)
    X = RT.random_states(tab, 65, seed=41, tilt=0.3, spread=0.5)
    X[7] = X[3]
    X[64] = X[3]
    out = []
    for B, rows in ((65, slice(0, 65)), (64, slice(0, 64)), (1, slice(64, 65))):
        rb, _, gk = T.make(name, None, B, admm_iters=40, oracle=False, **T.KINO)
        tau = gk.solve(0.0, X[rows, : rb.nq], X[rows, rb.nq:])
        tau = gk.solve(0.0, X[rows, : rb.nq], X[rows, rb.nq:])  # (warm-started)
        out.append((tau.copy(), gk.getAccelerations().copy(), gk.getContactForces().copy()))
    for a, b, c in zip(*out):
        assert np.array_equal(a[:64], b) and np.array_equal(a[64:].reshape(-1), c.reshape(-1))  # (a handle of one robot returns vectors)
    tau = out[0][0]
    assert np.isfinite(tau).all()
    assert np.array_equal(tau[3], tau[7]) and np.array_equal(tau[3], tau[64]) and np.abs(tau[0] - tau[1]).max() > 1e-6


def test_nan_state_stays_in_its_robot(built):
    rb, _, gk = T.make("biped_legs", None, 3, oracle=False, **T.KINO)
    _, _, ref = T.make("biped_legs", None, 3, oracle=False, **T.KINO)
    X = RT.near_reference_states(rb, 3, seed=51, scale=0.3)
    want = ref.solve(0.0, X[:, : rb.nq], X[:, rb.nq:]).copy()
    Xn = X.copy()
    Xn[1, 9] = np.nan
    gk.solve(0.0, Xn[:, : rb.nq], Xn[:, rb.nq:])
    r = gk.getResiduals()
    assert not np.isfinite(r[1]) and np.isfinite(r[0]) and np.isfinite(r[2])
    gk.reset(1)
    tau = gk.solve(0.0, X[:, : rb.nq], X[:, rb.nq:])
    assert np.isfinite(gk.getResiduals()).all() and np.array_equal(tau[1], want[1])
