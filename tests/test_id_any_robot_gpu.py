"""GPU tier of tests/test_id_any_robot.py: the same cases on the HIP library (B = 3), block independence at B = 65 / 64 / 1, replicas,
and a NaN state that stays in its own robot."""
import numpy as np
import pytest

import robot_tables as RT
import test_id_any_robot as T
from test_oracle_id import static_forces

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("centroidal", [False, True])
@pytest.mark.parametrize("name", T.ROBOTS)
def test_quantities_qp_and_solution(built, name, centroidal):
    T.pieces(name, None, centroidal)


@pytest.mark.parametrize("variant", [dict(contact_motion_equality=True), dict(tsid_joint_bounds=True), dict(contact_motion_equality=True, tsid_joint_bounds=True),
                                     dict(base_reference_as_coded=True)])
def test_qp_variants(built, variant):
    """(contact_motion_equality / tsid_joint_bounds off: test_quantities_qp_and_solution)"""
    T.pieces("quad_arm", None, False, **variant)
    T.pieces("tree32p", None, True, **variant)


def test_closed_loop_fixed_iterations(built):
    T.closed_loop("quad_arm", None, 200, 1e-7, B=3)


def test_closed_loop_tree32p(built):
    T.closed_loop("tree32p", None, 40, 1e-7, B=3)


def test_closed_loop_default_stopping_rule(built):
    """The early exit, the residual of the checked iterate and the rho re-factorisation on the device."""
    T.closed_loop("quad_arm", None, 40, 1e-5, B=3, admm_iters=400, admm_tol=1e-7)
    T.closed_loop("tree32p", None, 20, 1e-5, B=3, admm_iters=400, admm_tol=1e-7)


def test_targets_from_run_time_centroidal_mpc(built):
    T.resident_targets(None)


def test_run_time_engine_against_templated_engine(built):
    T.rt_vs_templated(None)


@pytest.mark.parametrize("name", ["quad_arm", "tree32p"])
def test_blocks_are_independent(built, name):
    """B = 65 against handles of B = 64 and B = 1 holding the same robots, bitwise; replicas inside a batch are bit-identical."""
    tab = T.table(name)
    X = RT.random_states(tab, 65, seed=41, tilt=0.3, spread=0.5)
    X[7] = X[3]
    X[64] = X[3]
    out = []
    for B, rows in ((65, slice(0, 65)), (64, slice(0, 64)), (1, slice(64, 65))):
        rb, _, gk = T.make(name, None, B, admm_iters=40, **T.ALL)
        tau = gk.solve(0.0, X[rows, : rb.nq], X[rows, rb.nq:])
        tau = gk.solve(0.0, X[rows, : rb.nq], X[rows, rb.nq:])  # (warm-started)
        out.append((tau.copy(), gk.getAccelerations().copy(), gk.getContactForces().copy()))
    for a, b, c in zip(*out):
        assert np.array_equal(a[:64], b) and np.array_equal(a[64:].reshape(-1), c.reshape(-1))  # (a handle of one robot returns vectors)
    tau = out[0][0]
    assert np.array_equal(tau[3], tau[7]) and np.array_equal(tau[3], tau[64]) and np.abs(tau[0] - tau[1]).max() > 1e-6


def test_nan_state_stays_in_its_robot(built):
    rb, _, gk = T.make("quad_arm", None, 3, **T.ALL)
    _, _, ref = T.make("quad_arm", None, 3, **T.ALL)
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
