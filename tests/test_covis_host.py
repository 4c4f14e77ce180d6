"""orbx_covis_host.h, the host bookkeeping of the device covisibility map: the
id table (range, in use, never reused after erase), key uniqueness and the
ranks that stand for the keys' order, the checks of rows (a point twice,
ranges), the edits on the shadow (in order, all or none, with the observer
lists kept in step), and the layout of orbx_covis_reference_args as the Python
binding mirrors it.

The checks are in covis_host_check.cpp, a stand-alone program that includes
the header; it is built with AddressSanitizer and UndefinedBehaviorSanitizer
and run, with nothing preloaded and no GPU."""
import shutil
import subprocess
from pathlib import Path

from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


def test_covis_host_bookkeeping(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    exe = tmp_path / "covis_host_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}", str(HERE / "covis_host_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
