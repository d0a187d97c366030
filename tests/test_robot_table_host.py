"""Validation of caller-filled robot tables (smpc_robot_check.h: what smpc_create_centroidal checks before it allocates anything for a robot
with a run-time joint tree) as a stand-alone C++ program with its own main, compiled with -fsanitize=address,undefined.  CPU tier only:
host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "robot_table_check.cpp")


def test_table_validation_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "robot_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "simple-mpc_amd", "csrc"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "robot table check: OK" in out.stdout
