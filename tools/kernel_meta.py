"""Registers, LDS, scratch and spill counts of every kernel of a built library, from the metadata of its gfx950 code object, and the
comparison of two libraries symbol by symbol (how DESIGN 3.26 checks that a pull request leaves the existing kernels' resources alone):

    python3 tools/kernel_meta.py <lib.so> [name filter]
    python3 tools/kernel_meta.py diff <parent lib.so> <new lib.so>

The code object is taken out of the library's .hip_fatbin section with llvm-objcopy and clang-offload-bundler and read with
llvm-readelf --notes (ROCM_PATH, default /opt/rocm).  `diff` lists the symbols that only one library has and those whose counts differ, and
exits with 1 if a symbol of the first library is missing from the second or has other counts there."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def kernels(lib):
    """{symbol: (VGPR, SGPR, LDS bytes, scratch bytes, VGPR spills, SGPR spills)}"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        out[g("name")] = tuple(int(g(k)) for k in FIELDS)
    return out


if __name__ == "__main__":
    if sys.argv[1] == "diff":
        a, b = kernels(sys.argv[2]), kernels(sys.argv[3])
        gone = sorted(set(a) - set(b))
        changed = sorted(k for k in a if k in b and a[k] != b[k])
        for k in gone:
            print("only in the first:", k, a[k])
        for k in changed:
            print("changed:", k, a[k], "->", b[k])
        for k in sorted(set(b) - set(a)):
            print("only in the second:", k, b[k])
        print("%d kernels in the first library, %d in the second; %d missing from the second, %d with other counts" % (len(a), len(b), len(gone), len(changed)))
        sys.exit(1 if gone or changed else 0)
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    print("VGPR SGPR LDS scratch VGPR-spills SGPR-spills  symbol")
    for k, v in sorted(kernels(sys.argv[1]).items()):
        if flt in k:
            print("%4d %4d %6d %5d %3d %3d  %s" % (v + (k,)))
