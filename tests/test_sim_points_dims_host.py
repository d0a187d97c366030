"""Host half of the simulator's body points (smpc_sim_points_dims.h: the admission behind smpc_robot_sim_set_body_points and
smpc_robot_sim_ground_points_dynamics, the free slots, the band and the sizes) as a stand-alone C++ program with its own main, compiled
with -fsanitize=address,undefined.  CPU tier only: host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_points_dims_check.cpp")


def test_admission_and_sizes_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "sim_points_dims_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sim_points_dims_check: ok" in out.stdout
