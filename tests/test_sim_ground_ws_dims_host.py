"""Host half of the warm-started ground contact solve (smpc_sim_ground_ws_dims.h: the admission behind smpc_robot_sim_set_ground_solver and
smpc_robot_sim_ground_solve_dynamics, the settings as the kernel reads them, buffer sizes, and the reset list behind
smpc_robot_sim_reset_ground_warm_start) as a stand-alone C++ program with its own main, compiled with -fsanitize=address,undefined.  CPU
tier only: host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_ground_ws_dims_check.cpp")


def test_admission_sizes_and_reset_lists_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "sim_ground_ws_dims_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sim_ground_ws_dims_check: ok" in out.stdout
