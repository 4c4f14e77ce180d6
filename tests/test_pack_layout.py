"""orbx_pack.h, the one place where the batched solver entry points state the
sizes of what they stage: regions on 16-byte boundaries in take order without
overlap, `total` the sum of the rounded sizes, every source byte for byte at
its offset in a blob that is zero everywhere else, the device pointer base
plus offset, empty regions with a null source accepted.

The checks are in pack_check.cpp, a stand-alone program that includes the
header (standard headers only) and the C ABI's structs; it is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run, with nothing
preloaded and no GPU."""
import shutil
import subprocess
from pathlib import Path

from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


def test_pack_layout(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    exe = tmp_path / "pack_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}", str(HERE / "pack_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
