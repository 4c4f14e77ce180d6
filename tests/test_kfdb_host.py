"""orbx_kfdb_host.h, the host bookkeeping of the device keyframe database:
the id table (range, in use, free again after erase), the add counter that
orders the inverted-file lists (kept over erase, reset by clear, refused when
exhausted), the capacity bounds, the checks of id lists and BowVectors, and
the layout of orbx_kfdb_query_args as the Python binding mirrors it.

The checks are in kfdb_host_check.cpp, a stand-alone program that includes the
header; it is built with AddressSanitizer and UndefinedBehaviorSanitizer and
run, with nothing preloaded and no GPU."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import orb_slam_amd as ox
from orb_slam_amd import build

HERE = Path(__file__).resolve().parent


def test_kfdb_host_bookkeeping(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or build.hipcc()
    exe = tmp_path / "kfdb_host_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{build.PKG.parent / 'include'}", f"-I{build.CSRC}", str(HERE / "kfdb_host_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_query_struct_mirrors_the_header():
    assert ctypes.sizeof(ox.KfdbQuery) == 136
    assert ox.KfdbQuery.words.offset == 16 and ox.KfdbQuery.candidates.offset == 64
    assert ox.KfdbQuery.tap_words.offset == 96


def test_abi_exports_the_database():
    """Revision 12 of the ABI: every orbx_kfdb_* entry point is exported, and
    each refuses a null context or database before touching a device."""
    lib = ox.lib()
    assert lib.orbx_abi_version() >= 12
    out = ctypes.c_void_p()
    assert lib.orbx_kfdb_create(None, 8, 8, ctypes.byref(out)) == -1
    assert lib.orbx_kfdb_size(None) == -1
    assert lib.orbx_kfdb_clear(None, None) == -1
    assert lib.orbx_kfdb_add(None, None, 0, 0, None, None) == -1
    assert lib.orbx_kfdb_add_slot(None, None, 0, 0) == -1
    assert lib.orbx_kfdb_erase(None, None, 0) == -1
    assert lib.orbx_kfdb_set_neighbours(None, None, 0, None, None) == -1
    assert lib.orbx_kfdb_query(None, None, None) == -1
    assert lib.orbx_kfdb_score(None, None, -1, 0, None, None, 0, None, None) == -1
    lib.orbx_kfdb_destroy(None)   # no-op
