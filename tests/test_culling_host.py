"""The culling additions to orbx_covis_host.h: the per-keyframe "octaves set"
flags, the argument checks of orbx_covis_cull_keyframes and
orbx_covis_cull_points, the shadow after a cull record (the culled rows gone,
the observer lists in step, the bad points erased), all or none on a capacity
error, and the layout of orbx_covis_cull_args.

The checks are in culling_host_check.cpp, a stand-alone program that includes
the header; it is built with AddressSanitizer and UndefinedBehaviorSanitizer
and run, with nothing preloaded and no GPU."""
import shutil
import subprocess
from pathlib import Path

from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


def test_culling_host_bookkeeping(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    exe = tmp_path / "culling_host_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}", str(HERE / "culling_host_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
