"""The world map (pr_worldmap) without a device: the ABI surface, the argument errors that are returned before any device
is touched, what the Python class refuses before it calls the library, and properties of the NumPy restatement the GPU tests compare
the kernels with (worldmap_np.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_worldmap_create", "pr_worldmap_destroy", "pr_worldmap_scratch_bytes", "pr_worldmap_count", "pr_worldmap_fuse_dev",
         "pr_worldmap_fuse")


def test_worldmap_symbols_records_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_worldmap_")) == sorted(NAMES)
    flags = re.search(r"enum \{ PR_WORLDMAP_OVERFLOW = 1, PR_WORLDMAP_SKIPPED = 2, PR_WORLDMAP_RANGE = 4, PR_WORLDMAP_TABLE = 8 \};", code)
    assert flags and (_lib.WORLDMAP_OVERFLOW, _lib.WORLDMAP_SKIPPED, _lib.WORLDMAP_RANGE, _lib.WORLDMAP_TABLE) == (1, 2, 4, 8)
    assert (wnp.OVERFLOW, wnp.SKIPPED, wnp.RANGE, wnp.TABLE) == (1, 2, 4, 8)
    assert "typedef struct pr_worldmap pr_worldmap;" in code
    fields = re.search(r"typedef struct pr_worldmap_buffers \{(.*?)\} pr_worldmap_buffers;", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*;", fields)) == tuple(n for n, _ in _lib.WorldMapBuffers._fields_) == api.WorldMap.NAMES
    assert C.sizeof(_lib.WorldMapBuffers) == 6 * C.sizeof(C.c_void_p)
    for m in ("fuse_torch", "fuse", "write_ply", "rows", "count_rows", "close"):
        assert hasattr(api.WorldMap, m), m
    for words in ("pr_worldmap", "DESIGN.md 4.19", "tests/worldmap_np.py", "(R[0][a] d0 + R[1][a] d1) + R[2][a] d2", "floor(w_a / cell)",
                  "[-2^20, 2^20)", "compared as a double", "PR_WORLDMAP_TABLE"):
        assert words in txt, words
    hip = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "worldmap.hip")).read()
    assert "(q[a] * d0 + q[4 + a] * d1) + q[8 + a] * d2" in hip and "step < T" in hip
    mk = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "Makefile")).read()
    assert re.search(r"worldmap\.o: worldmap\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "-ffp-contract=off" in mk


def test_worldmap_scratch_size_formula():
    """20 T + 4 point_capacity + 8 nblk4 + 96 keyframe_capacity + 64 bytes, each part rounded up to 16; T = 64 and 2048 at the capacities
    the GPU tests use."""
    lib = _lib.load()
    up = lambda b: (b + 15) & ~15
    for kcap, pcap in ((4, 32), (4, 600), (1, 1), (112, 1 << 20), (7, 257), (3, 1025)):
        T = 1 << wnp.log2T(pcap)
        assert T >= 64 and T >= 2 * pcap and (T == 64 or T < 4 * pcap)
        nblk4 = (((pcap + 255) // 256) + 3) & ~3
        want = 16 * T + up(4 * T + 16) + up(4 * pcap) + up(8 * nblk4) + up(96 * kcap) + 16 + 32
        assert lib.pr_worldmap_scratch_bytes(kcap, pcap) == want, (kcap, pcap)
    assert 1 << wnp.log2T(32) == 64 and 1 << wnp.log2T(600) == 2048
    assert lib.pr_worldmap_scratch_bytes(0, 8) == 0 and lib.pr_worldmap_scratch_bytes(8, 0) == 0
    assert lib.pr_worldmap_scratch_bytes(8, (1 << 29) + 1) == 0 and lib.pr_worldmap_scratch_bytes(8, 1 << 29) > 20 << 30


def _bufs(null=None):
    """a pr_worldmap_buffers of non-NULL addresses that are never dereferenced (every case below fails before the device is touched)"""
    store = (C.c_double * 8)()
    b = _lib.WorldMapBuffers(*([C.addressof(store)] * 6))
    if null:
        setattr(b, null, None)
    return b, store


def test_worldmap_create_argument_errors():
    """Value checks come before anything touches a device; the NULL map and the NULL context are the last two."""
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    b, keep = _bufs()
    fake_map = C.c_void_p(C.addressof(keep))
    h = C.c_void_p(1)
    assert lib.pr_worldmap_create(None, fake_map, C.byref(b), 8, None) == _lib.PR_EINVAL and "out is NULL" in err()
    assert lib.pr_worldmap_create(None, fake_map, None, 8, C.byref(h)) == _lib.PR_EINVAL and "buffers is NULL" in err() and not h.value
    for oc in (0, -1):
        h = C.c_void_p(1)
        assert lib.pr_worldmap_create(None, fake_map, C.byref(b), oc, C.byref(h)) == _lib.PR_EINVAL and not h.value
        assert "pr_worldmap_create: out_capacity=%d is below 1" % oc in err()
    h = C.c_void_p(1)
    assert lib.pr_worldmap_create(None, None, C.byref(b), 8, C.byref(h)) == _lib.PR_EINVAL and "map is NULL" in err() and not h.value
    assert lib.pr_worldmap_create(None, fake_map, C.byref(b), 8, C.byref(h)) == _lib.PR_EINVAL and "ctx is NULL" in err() and not h.value


@pytest.mark.parametrize("name", api.WorldMap.NAMES)
def test_worldmap_create_null_buffer(name):
    lib = _lib.load()
    b, keep = _bufs(null=name)
    h = C.c_void_p(1)
    assert lib.pr_worldmap_create(None, C.c_void_p(C.addressof(keep)), C.byref(b), 8, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert b"a buffer is NULL" in lib.pr_last_error(None)


def test_worldmap_null_handles_and_values():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    r, f = C.c_int64(7), C.c_int32(7)
    err = lambda: lib.pr_last_error(None)
    assert lib.pr_worldmap_count(None, C.byref(r), C.byref(f)) == _lib.PR_EINVAL and b"pr_worldmap_count: world map is NULL" in err()
    forms = (("pr_worldmap_fuse_dev", lambda cell, mc, k: lib.pr_worldmap_fuse_dev(None, buf, buf, cell, mc, k, buf)),
             ("pr_worldmap_fuse", lambda cell, mc, k: lib.pr_worldmap_fuse(None, buf, buf, cell, mc, k, buf, buf, buf, buf, buf, buf)))
    for name, fuse in forms:
        who = name.encode()
        assert fuse(0.2, 1, 0) == _lib.PR_EINVAL and who + b": world map is NULL" in err()
        for cell in (0.0, -0.2, -0.0, float("nan"), float("inf"), -float("inf")):
            assert fuse(cell, 1, 0) == _lib.PR_EINVAL and who + b": cell must be finite and positive" in err(), cell
        for mc in (0, -1):
            assert fuse(0.2, mc, 0) == _lib.PR_EINVAL and who + b": min_count=%d is below 1" % mc in err()
        for k in (-1, 2, 7):
            assert fuse(0.2, 1, k) == _lib.PR_EINVAL and who + b": keep=%d is neither" % k in err()
    lib.pr_worldmap_destroy(None)                      # a no-op


def test_world_map_refuses_before_the_library():
    import torch

    class Fake:
        pass
    km = Fake(); km.ctx, km.keyframe_capacity, km.h = object(), 8, None
    with pytest.raises(ValueError, match="share one context"):
        api.WorldMap(object(), km, 16)                 # a map of another context: refused before any handle exists
    wm = api.WorldMap.__new__(api.WorldMap)            # no handle, no library call: the checks are the first thing fuse_torch does
    wm.ctx, wm.km, wm.h, wm.out_capacity = km.ctx, km, None, 16
    wm.state = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="keep is 'first' or 'last'"):
        wm.fuse_torch(keep="newest")
    with pytest.raises(ValueError, match="keep is 'first' or 'last'"):
        wm.fuse(keep=1)
    for poses in (torch.zeros((8, 12), dtype=torch.float64), torch.zeros((9, 12), dtype=torch.float64), torch.zeros((8, 12), dtype=torch.float32)):
        with pytest.raises(ValueError, match="poses must be"):
            wm.fuse_torch(poses=poses)                 # not on the device / another capacity / another dtype
    with pytest.raises(ValueError, match="n must be"):
        wm.fuse_torch(n=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="info must be"):
        wm.fuse_torch(info=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"poses must be \[keyframe_capacity, 12\]"):
        wm.fuse(poses=np.zeros((9, 12)))


# ------------------------------------------------------------------------------------------------ the restatement
def _map(seed, sizes, spread=3.0, kcap=None, pcap=None):
    rng = np.random.default_rng(seed)
    kcap = len(sizes) if kcap is None else kcap
    offs = np.zeros(kcap + 1, np.int64)
    offs[1:len(sizes) + 1] = np.cumsum(sizes)
    offs[len(sizes) + 1:] = offs[len(sizes)]
    P = int(offs[-1])
    pcap = P if pcap is None else pcap
    xyz = np.zeros((pcap, 3)); xyz[:P] = rng.normal(0, spread, (P, 3))
    inten = np.zeros(pcap, np.float32); inten[:P] = rng.random(P).astype(np.float32)
    poses = np.zeros((kcap, 12))
    for r in range(kcap):
        q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        poses[r] = np.concatenate([q, rng.normal(0, 2, (3, 1))], 1).reshape(12)
    return xyz, inten, offs, poses


def test_fusing_the_own_output_under_the_identity_returns_it():
    xyz, inten, offs, poses = _map(1, [200, 0, 300, 150])
    a = wnp.fuse(xyz, inten, offs, poses, 4, 0.5)
    r = int(a["state"][0])
    assert 100 < r < 650 and a["info"].tolist() == [r, r, 650, 0]
    b = wnp.fuse(a["xyz"], a["inten"], np.array([0, r], np.int64), wnp.identity_poses(1), 1, 0.5)
    assert b["xyz"].tobytes() == a["xyz"].tobytes() and b["inten"].tobytes() == a["inten"].tobytes()
    assert b["src"].tolist() == list(range(r)) and not b["row"].any() and (b["count"] == 1).all() and b["info"].tolist() == [r, r, r, 0]


@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_first_and_last_select_the_same_voxels_and_counts(min_count):
    xyz, inten, offs, poses = _map(2, [300, 300, 300], spread=1.5)
    a = wnp.fuse(xyz, inten, offs, poses, 3, 0.5, min_count, "first")
    b = wnp.fuse(xyz, inten, offs, poses, 3, 0.5, min_count, "last")
    cells = lambda o: sorted(zip(map(tuple, np.floor(o["xyz"] / 0.5).astype(int).tolist()), o["count"].tolist()))
    assert cells(a) == cells(b) and a["info"].tolist() == b["info"].tolist() and len(a["src"]) > 10
    assert (a["src"] <= np.sort(b["src"])).all() and (a["src"] != b["src"]).any() == bool((a["count"] > 1).any())
    assert (np.diff(a["src"]) > 0).all() and (np.diff(b["src"]) > 0).all()          # a subsequence of the map in map order
    assert (a["count"] >= min_count).all()
    if min_count == 1:
        assert len(a["src"]) == len(a["keys"]) and a["count"].sum() == a["info"][2] == 900     # rows = distinct keys


def test_exact_cell_boundaries_and_negative_coordinates_land_in_the_floor_cell():
    """cell = 0.25 (a power of two: every quotient below is exact).  Under the identity pose a coordinate k * cell sits in cell k, just
    below it in cell k - 1, and negative coordinates round toward minus infinity, not toward zero."""
    cell = 0.25
    xs = np.array([0.0, -0.0, 0.25, -0.25, np.nextafter(0.25, 0), np.nextafter(-0.25, -1), -0.125, 0.125, 3 * cell, -3 * cell, -1e-300])
    want = [0, 0, 1, -1, 0, -2, -1, 0, 3, -3, -1]
    xyz = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], 1)
    o = wnp.fuse(xyz, np.zeros(len(xs), np.float32), np.array([0, len(xs)], np.int64), wnp.identity_poses(1), 1, cell)
    by_cell = {}
    for i, k in enumerate(want):
        by_cell.setdefault(k, []).append(i)
    assert sorted(o["src"].tolist()) == sorted(v[0] for v in by_cell.values())
    assert {(k, 0, 0) for k in by_cell} == o["keys"]
    assert dict(zip(o["src"].tolist(), o["count"].tolist())) == {v[0]: len(v) for v in by_cell.values()}
    assert np.signbit(o["xyz"][list(o["src"]).index(0), 0]) == False and o["info"].tolist() == [6, 6, 11, 0]   # noqa: E712


def test_range_skips_clamps_and_overflow_of_the_restatement():
    cell = 1.0
    lim = float(1 << 20)
    xs = np.array([lim, lim - 1, -lim, -lim - 1, np.nan, np.nextafter(lim, 0), 5.0])
    xyz = np.stack([np.zeros_like(xs), xs, np.zeros_like(xs)], 1)
    offs = np.array([0, len(xs), len(xs), len(xs)], np.int64)
    o = wnp.fuse(xyz, np.arange(len(xs), dtype=np.float32), offs, wnp.identity_poses(3), 1, cell)
    assert o["src"].tolist() == [1, 2, 6] and o["info"].tolist() == [3, 3, 4, wnp.SKIPPED | wnp.RANGE] and o["count"].tolist() == [2, 1, 1]
    o = wnp.fuse(xyz, np.arange(len(xs), dtype=np.float32), offs, wnp.identity_poses(3), 99, cell, out_capacity=2)       # n is clamped
    assert o["src"].tolist() == [1, 2] and o["info"].tolist() == [2, 3, 4, wnp.SKIPPED | wnp.RANGE | wnp.OVERFLOW]
    for n in (0, -4):
        o = wnp.fuse(xyz, np.arange(len(xs), dtype=np.float32), offs, wnp.identity_poses(3), n, cell)
        assert o["info"].tolist() == [0, 0, 0, 0] and len(o["src"]) == 0
    poses = wnp.identity_poses(3); poses[0, 7] = np.inf
    o = wnp.fuse(xyz, np.arange(len(xs), dtype=np.float32), offs, poses, 3, cell)
    assert o["info"].tolist() == [0, 0, 0, wnp.SKIPPED]


def test_the_committed_colliding_cells_collide():
    """what test_gpu_worldmap.py relies on at T = 64: 32 distinct keys, at least 8 with one home slot, and a chain across slot 63 -> 0"""
    cells = wnp.COLLIDING_CELLS
    keys = [wnp.key_of(c) for c in cells]
    assert len(cells) == 32 == len(set(keys)) and all(0 <= k < 1 << 63 for k in keys)
    homes = [wnp.home_slot(k, 6) for k in keys]
    assert all(0 <= h < 64 for h in homes)
    assert homes.count(62) >= 8                        # slots 62, 63 and then 0, 1, ...: the chain crosses the table's end
    table = [None] * 64                                # linear probing in list order
    wrapped = 0
    for k, h in zip(keys, homes):
        at = h
        while table[at] is not None:
            wrapped += at == 63
            at = (at + 1) & 63
        table[at] = k
    assert wrapped >= 1 and table[62] is not None and table[63] is not None and table[0] is not None
    assert wnp.key_of((-wnp.LIM, -wnp.LIM, -wnp.LIM)) == 0 and wnp.key_of((wnp.LIM - 1,) * 3) == (1 << 63) - 1
