"""orbx_stage.h, the one place where the matchers' host entry points lay
their arrays out in the context scratch: every region on a 256-byte
boundary, no two regions at one address (empty ones included), `total` the
end of the last region, and put / fill / get through a region handle touching
exactly count * sizeof(T) bytes.

The checks are in stage_layout_main.cpp, a stand-alone program that includes
the header and makes no HIP call; it is built with AddressSanitizer and
UndefinedBehaviorSanitizer with the flags build.py gives .cpp files, and run."""
import shutil
import subprocess
from pathlib import Path

from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


def test_stage_layout(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    rocm = Path(build.hipcc()).resolve().parent.parent
    exe = tmp_path / "stage_layout"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", f"-I{rocm / 'include'}", f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}",
           str(HERE / "stage_layout_main.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0 and "hip" in p.stderr and "undefined reference" in p.stderr:
        # the header's inline transports were emitted: link the runtime (still no HIP call)
        p = subprocess.run(cmd + [f"-L{rocm / 'lib'}", "-lamdhip64", f"-Wl,-rpath,{rocm / 'lib'}"],
                           capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
