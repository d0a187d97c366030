"""Host half of the rigid-body simulator on a run-time joint tree (smpc_sim_rt_dims.h: buffer sizes and the admission behind
smpc_robot_sim_create -- contact size, foot count per contact size, batch, the robot table) as a stand-alone C++ program with its own main,
compiled with -fsanitize=address,undefined.  CPU tier only: host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_rt_dims_check.cpp")


def test_sizes_and_admission_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "sim_rt_dims_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sim_rt_dims_check: ok" in out.stdout
