"""Host half of the flat-foot inverse-dynamics engine on a run-time joint tree (smpc_id_rt_dims.h: id_rt6_sizes, id_route_any -- the routing
behind smpc_id_create_any -- and id_route unchanged beside it) as a stand-alone C++ program with its own main, compiled with
-fsanitize=address,undefined.  CPU tier only: host code, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "id_rt6_dims_check.cpp")


def test_flat_foot_sizes_and_routes_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "id_rt6_dims_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "id_rt6_dims_check: ok" in out.stdout
