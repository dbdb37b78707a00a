"""pr::Arena (csrc/arena.hpp, included by handle_core.hpp) is the one layout rule of the resident handle families: take(bytes) returns the running total and adds
bytes rounded up to a multiple of 16.  tests/native/arena_check.cpp checks the rule on the host with a plain compiler (no HIP), and rebuilds
the layouts of two families from the part lists of include/place_recognition.h; here those totals are compared with what the library's
pr_gate_scratch_bytes / pr_mapgrow_scratch_bytes return, at the sizes test_gate_cpu.py and test_mapgrow_cpu.py use."""
import os
import shutil
import subprocess

import pytest

from so_dso_place_recognition_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("arena") / "arena_check")
    r = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "native", "arena_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def total(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:]
    return int(r.stdout)


def test_arena_rule(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("arena ok"), r.stdout[-2000:]


def test_arena_rebuilds_the_gate_layout(exe):
    lib = _lib.load()
    for nc, ec, mg in ((40, 600, 6), (1, 1, 0), (1 << 20, 65536, 65535), (16, 8, 2), (3475, 173, 40), (44, 257, 5), (8, 4097, 17)):
        assert lib.pr_gate_scratch_bytes(nc, ec, mg) == total(exe, "gate", ec, mg + 1) > 0, (nc, ec, mg)


def test_arena_rebuilds_the_mapgrow_layout(exe):
    lib = _lib.load()
    for m in (1, 16, 255, 256, 257, 513, 9000, 1 << 26):
        assert lib.pr_mapgrow_scratch_bytes(m) == total(exe, "mapgrow", m) > 0, m
