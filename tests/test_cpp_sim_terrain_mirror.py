"""The terrain of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setTerrain, clearTerrain, terrainDevicePointers,
lastTerrainNormals, lastTerrainHeights, groundTerrainDynamics, terrain_height, terrain_from_function) exercised by a C++ program
(tests/cpp/batched_sim_terrain_check.cpp: the mirror against the C ABI called directly with equal bits in the host-buffer solve and over 30
steps on a rough tile, a flat tile against the kernels on the plane, clearing, setGround, refusals).  CPU tier: linked against the
sequential-lane test build of the kernel bodies; GPU tier: against libsmpc_hip.so, states and torques in hipMalloc'ed memory."""
import os
import subprocess

import pytest

import mpc_setup as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "batched_sim_terrain_check.cpp")
HIP_LIB = os.path.join(ROOT, "simple-mpc_amd", "csrc", "libsmpc_hip.so")


def _build_and_run(lib_path, exe, hip):
    libdir, libname = os.path.split(lib_path)
    cmd = ["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + libdir, "-l:" + libname, "-Wl,-rpath," + libdir]
    if hip:
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        cmd += ["-DSMPC_CHECK_HIP", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                "-Wl,-rpath," + os.path.join(rocm, "lib")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batched sim terrain mirror: OK" in out.stdout


def test_cpp_program_against_the_cpu_test_build(built, tmp_path):
    S.emu_lib()
    _build_and_run(S.EMU_LIB, str(tmp_path / "batched_sim_terrain_emu"), False)


@pytest.mark.gpu
def test_cpp_program_against_the_hip_library(built, tmp_path):
    _build_and_run(HIP_LIB, str(tmp_path / "batched_sim_terrain_hip"), True)
