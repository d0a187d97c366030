"""GPU tier of tests/test_reframed_robots.py: the HIP kernels on re-framed and renumbered robot tables (dense rotations in every joint
placement, another topological order of the joints), through the same helpers with lib = None.  The per-lane LDS joint records, the level
schedule of the run-time trees and the gfx950-only paths are what the emulated tier cannot see.  Every case is small: B <= 3 for dynamics
and QP pieces, B = 2 and H <= 20 for MPC knots and closed loops.  The table of tests and the kernel files they reach is in the header of
tests/test_reframed_robots.py; the test names are the same here."""
import pytest

import mpc_setup as S
import test_centroidal_any_robot as TC
import test_id_any_robot as TP
import test_id_flat_any_robot as TF
import test_reframed_robots as T
import test_robot_sim_any_robot as TS

pytestmark = pytest.mark.gpu
SHORT = T.SHORT


# ------------------------------------------------------------------------------------------------------------------------ run-time kernels
@pytest.mark.parametrize("name,fs", [("quad_arm_rn", 3), ("tree32p_rn", 3), ("biped_legs_rn", 6), ("tree32_rn", 6), ("biped_legs_rn", 3), ("tree32_rn", 3)])
def test_simulator_forward_dynamics(built, name, fs):
    TS.fd_against_oracle(name, fs, None)


@pytest.mark.parametrize("name", ["quad_arm_rn", "biped_legs_rn", "tree32_rn"])
def test_centroidal_on_run_time_tree(built, name):
    TC.frontend_vs_oracle(name, None, B=3)
    TC.closed_loop(name, None, 1, 1e-4, B=2)


@pytest.mark.parametrize("centroidal", [False, True])
@pytest.mark.parametrize("name", ["quad_arm_rn", "tree32p_rn"])
def test_point_foot_id_pieces(built, name, centroidal):
    TP.pieces(name, None, centroidal)


@pytest.mark.parametrize("centroidal", [False, True])
@pytest.mark.parametrize("name", ["biped_legs_rn", "tree32_rn"])
def test_flat_foot_id_pieces(built, name, centroidal):
    T.flat_foot_id_pieces(name, None, centroidal)


# ----------------------------------------------------------------------------------------- templated kernels on go2_like_rf / talos_like_rf
def test_templated_front_ends(built):
    import test_frontend as F

    with S.robots(**T.GO2, **T.TALOS):
        F._check(None)  # frontend_body (kinodynamics handle)
        F._check_all_handles(None)  # frontend_body / frontend_full_body behind the other five handles, H = 10


def test_constraint_dynamics(built):
    import test_constraint_dynamics as F

    with S.robots(**T.GO2, **T.TALOS):
        F._check(None, n=6, seed=9, Kp=(0, 0, 50.0), Kd=(100.0, 100.0, 100.0))  # full_fd_body
        F._check_full_handles(None)  # fdyn_fd_body, 3-D and 6-D contacts


def test_go2_kinodynamics_knots(built):
    T.go2_kinodynamics_knots(None)


def test_go2_kinodynamics_closed_loop(built):
    T.go2_kinodynamics_closed_loop(None)


def test_go2_full_dynamics_knots(built):
    T.go2_full_dynamics_knots(None)


def test_talos_kinodynamics_knots(built):
    T.talos_kinodynamics_knots(None)


def test_talos_full_dynamics_knots(built):
    T.talos_full_dynamics_knots(None)


def test_talos_centroidal(built):
    import test_talos_centroidal as F

    om, gm, rb = S.make_talos_cent_pair(2, max_iters=2, robot="talos_like_rf", **SHORT)
    F._loop(om, gm, rb, 1)


# ------------------------------------------------------------------------------------------------------------------ product against product
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("family", ["go2 kinodynamics", "talos full dynamics"])
def test_product_pair(built, family, iters):
    T.product_pair(family, None, iters)
