"""Host half of smpc_reset_instances (smpc_reset_mask.h: instance list -> byte mask, index validation) as a stand-alone C++ program
with its own main, compiled with -fsanitize=address,undefined.  CPU tier only: host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "reset_mask_check.cpp")


def test_list_to_mask_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "reset_mask_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "simple-mpc_amd", "csrc"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reset mask check: OK" in out.stdout
