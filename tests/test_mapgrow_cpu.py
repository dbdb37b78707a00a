"""The incremental world map (pr_mapgrow) without a device: the ABI surface and the header's rule text, the scratch
formula, the argument errors returned before any device is touched, what the Python class refuses before it calls the library, and the
identity the feature rests on - the restatement (mapgrow_np.py) applied row by row equals the committed restatements of the rebuild
(worldmap_np.fuse, maploc_np.index, mapplane_np.normals) after every keyframe, the overflow in the middle of a cloud and a cloud entirely
inside known voxels included; the three refusals and the switched-off call leave the model unchanged."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import maploc_np as mnp
import mapgrow_np as gnp
import mapplane_np as pnp
import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_mapgrow_create", "pr_mapgrow_destroy", "pr_mapgrow_scratch_bytes", "pr_mapgrow_sync_dev", "pr_mapgrow_extend_dev",
         "pr_mapgrow_normals_dev", "pr_mapgrow_extend", "pr_mapgrow_normals", "pr_mapgrow_count")


def test_mapgrow_symbols_rule_text_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_mapgrow_")) == sorted(NAMES)
    assert "typedef struct pr_mapgrow pr_mapgrow;" in code
    assert re.search(r"enum \{ PR_MAPGROW_ORDER = 16, PR_MAPGROW_STALE = 32, PR_MAPGROW_FULL = 64 \};", code)
    assert (_lib.MAPGROW_ORDER, _lib.MAPGROW_STALE, _lib.MAPGROW_FULL) == (gnp.ORDER, gnp.STALE, gnp.FULL) == (16, 32, 64)
    assert re.search(r"pr_mapgrow_create\(pr_ctx\* ctx, pr_worldmap\* wm, pr_maploc\* ml, pr_mapgrow\*\* out\)", code)
    for m in ("sync_torch", "extend_torch", "normals_torch", "rebuild_torch", "extend", "normals", "count", "close"):
        assert hasattr(api.MapGrower, m), m
    for words in ("pr_mapgrow", "DESIGN.md 4.24", "THE REBUILD'S", "r != fused or r >= n", "R != rows_seen", "PR_MAPGROW_FULL",
                  "the call is off", "count[j] += 1", "the smallest g", "R' = min(R + new voxels, ocap)", "[a, b) = [R, R')",
                  "a lookup returns \"no row\"", "keys around that row's voxel", "they store equal bytes", "648 mcp",
                  "keep = 1 and min_count > 1", "after a relaxation the caller rebuilds and syncs",
                  "turns the call into a refusal with PR_WORLDMAP_TABLE"):
        assert words in txt, words
    # the rebuild and the incremental path run ONE copy of the position, the key and the per-row normal
    wc = open(os.path.join(CSRC, "worldmap_common.hpp")).read()
    nh = open(os.path.join(CSRC, "mapplane_normal.hpp")).read()
    assert "(q[a] * d0 + q[4 + a] * d1) + q[8 + a] * d2" in wc and "floor(w[0] / cell)" in wc
    assert "step < Tn" in nh and "row >= (u64)v.ocap" in nh and "MP_SWEEPS = %d" % pnp.SWEEPS in nh
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    for name, incs in (("worldmap.hip", ("worldmap_common.hpp",)), ("mapplane.hip", ("mapplane_normal.hpp",)),
                       ("mapgrow.hip", ("worldmap_common.hpp", "mapplane_normal.hpp"))):
        src = strip(open(os.path.join(CSRC, name)).read())
        for inc in incs:
            assert '#include "%s"' % inc in src, (name, inc)
        assert "q[8 + a] * d2" not in src and "sqrt(theta" not in src, name        # no second copy of either
    hip = strip(open(os.path.join(CSRC, "mapgrow.hip")).read())
    assert "world_of(" in hip and "key_of(" in hip and "row_normal(" in hip and "step < T" in hip
    assert "while" not in hip and "atomicAdd(&v.w.count[j], 1)" in hip
    for a in re.findall(r"atomic\w+", hip):
        assert a in ("atomicCAS", "atomicMin", "atomicAdd", "atomicOr"), a
    assert not re.search(r"atomicAdd\([^;]*(double|float)", hip)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"mapgrow\.o: mapgrow\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "-ffp-contract=off" in mk
    assert "mapgrow.o mapgrow_host.o" in mk


def test_mapgrow_scratch_size_formula():
    lib = _lib.load()
    for m in (1, 16, 255, 256, 257, 513, 9000, 1 << 26):
        want = gnp.scratch_bytes(m)
        assert want > 0 and want % 16 == 0 and lib.pr_mapgrow_scratch_bytes(m) == want, m
    for bad in (0, -1, (1 << 26) + 1):
        assert lib.pr_mapgrow_scratch_bytes(bad) == 0 and gnp.scratch_bytes(bad) == 0, bad


def test_mapgrow_argument_errors_before_any_device():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    err = lambda: lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_mapgrow_create(None, buf, buf, None) == _lib.PR_EINVAL and b"out is NULL" in err()
    assert lib.pr_mapgrow_create(None, None, buf, C.byref(h)) == _lib.PR_EINVAL and b"world map is NULL" in err() and not h.value
    h = C.c_void_p(1)
    assert lib.pr_mapgrow_create(None, buf, None, C.byref(h)) == _lib.PR_EINVAL and b"localiser is NULL" in err() and not h.value
    assert lib.pr_mapgrow_create(None, buf, buf, C.byref(h)) == _lib.PR_EINVAL and b"ctx is NULL" in err()
    lib.pr_mapgrow_destroy(None)                       # a no-op
    assert lib.pr_mapgrow_sync_dev(None, buf) == _lib.PR_EINVAL and b"pr_mapgrow_sync_dev: grower is NULL" in err()
    assert lib.pr_mapgrow_extend_dev(None, buf, None, buf) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
    assert lib.pr_mapgrow_extend_dev(None, buf, buf, None) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
    assert lib.pr_mapgrow_extend_dev(None, None, buf, buf) == _lib.PR_EINVAL and b"pr_mapgrow_extend_dev: grower is NULL" in err()
    assert lib.pr_mapgrow_extend(None, buf, 0, None) == _lib.PR_EINVAL and b"info is NULL" in err()
    assert lib.pr_mapgrow_extend(None, None, 0, buf) == _lib.PR_EINVAL and b"pr_mapgrow_extend: grower is NULL" in err()
    f, r, fl = C.c_int32(7), C.c_int64(7), C.c_int32(7)
    assert lib.pr_mapgrow_count(None, C.byref(f), C.byref(r), C.byref(fl)) == _lib.PR_EINVAL and b"pr_mapgrow_count: grower is NULL" in err()
    for name in ("pr_mapgrow_normals_dev", "pr_mapgrow_normals"):                # pr_mapplane_normals_dev's refusals
        fn, who = getattr(lib, name), name.encode()
        assert fn(None, 0.4, 5, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": grower is NULL" in err()
        for rad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert fn(None, rad, 5, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": radius=" in err(), rad
        for mn in (2, 0, -1, 28):
            assert fn(None, 0.4, mn, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": min_nbrs=%d outside 3 .. 27" % mn in err()
        for mr in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
            assert fn(None, 0.4, 5, mr, buf, buf) == _lib.PR_EINVAL and who + b": max_ratio=" in err(), mr
        assert fn(None, 0.4, 3, 1.0, buf, buf) == _lib.PR_EINVAL and b"grower is NULL" in err()               # 3, 27 and 1.0 are inside
        assert fn(None, 0.4, 27, 1.0, None, buf) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
        assert fn(None, 0.4, 27, 1.0, buf, None) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()


def test_map_grower_refuses_before_the_library():
    import torch

    class Fake:
        pass
    ctx = object()
    wm, ml = Fake(), Fake()
    wm.ctx, ml.ctx, ml.wm = ctx, object(), wm
    with pytest.raises(ValueError, match="share one context"):
        api.MapGrower(ctx, wm, ml)                     # a localiser of another context: refused before any handle exists
    ml.ctx, ml.wm = ctx, Fake()
    with pytest.raises(ValueError, match="created over this world map"):
        api.MapGrower(ctx, wm, ml)
    wm.state, wm.out_capacity, wm.km = torch.zeros(4, dtype=torch.int32), 16, Fake()
    wm.km.keyframe_capacity = 4
    mg = api.MapGrower.__new__(api.MapGrower)
    mg.ctx, mg.wm, mg.ml, mg.h = ctx, wm, ml, None
    row, n, i = torch.zeros(1, dtype=torch.int32), torch.zeros((16, 3), dtype=torch.float64), torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError, match="row must be a contiguous CUDA tensor"):
        mg.extend_torch(row)                           # not on the device
    with pytest.raises(ValueError, match="n must be a contiguous CUDA tensor"):
        mg.sync_torch(row)
    with pytest.raises(ValueError, match="normals must be a contiguous CUDA tensor"):
        mg.normals_torch(0.4, 5, 0.1, n, i)
    with pytest.raises(ValueError, match=r"poses must be \[keyframe_capacity, 12\]"):
        mg.extend(0, np.zeros((3, 12)))
    with pytest.raises(ValueError, match="normals must be a contiguous f64"):
        mg.normals(0.4, 5, 0.1, np.zeros((15, 3)), i.numpy())
    pl = Fake(); pl.ml = Fake()
    with pytest.raises(ValueError, match="over this grower's localiser"):
        mg.rebuild_torch(pl)


# ------------------------------------------------------------------------------------------------ the identity
def assert_model_is_the_rebuild(M, D, n, what, normals=True):
    """the model after its extends against worldmap_np.fuse / maploc_np.index / mapplane_np.normals at the count n"""
    w = wnp.fuse(D["m_xyz"], D["m_inten"], D["m_offs"], D["poses"], n, M.cell, 1, "first", out_capacity=M.ocap)
    R = int(w["state"][0])
    assert M.state.tobytes() == w["state"].tobytes(), (what, M.state, w["state"])
    for name in ("xyz", "inten", "src", "row", "count"):
        assert getattr(M, name)[:R].tobytes() == w[name].tobytes(), (what, name)
    ix = mnp.index(M.xyz, R, M.cell, M.ocap)
    assert ix["flags"] == 0 and M.first == ix["first"], what
    if normals:
        wn, wi = pnp.normals(ix, M.xyz, out_capacity=M.ocap, **gnp.NORMALS)
        assert M.ninfo.tolist() == wi.tolist() and M.normals_.tobytes() == wn.tobytes(), what
    return w


@pytest.mark.parametrize("ocap", (2048, 300))
def test_row_by_row_equals_the_rebuild_at_every_n(ocap):
    D = gnp.drive()
    assert D["sizes"] == gnp.SIZES
    M = gnp.Model(D["m_xyz"], D["m_inten"], D["m_offs"], ocap, D["cell"], 600)
    M.rebuild(D["poses"], 0, gnp.NORMALS)
    assert M.rows() == 0 and M.fused == 0
    saw_overflow = saw_valid = False
    for r in range(D["n"]):
        before = M.rows()
        info = M.extend(D["poses"], r, D["n"])
        if info[3] & gnp.FULL:                                     # the call after the overflow: refused, nothing changed
            assert saw_overflow and info.tolist() == [0, before, 0, gnp.FULL] and M.fused < r + 1
            break
        M.normals(**gnp.NORMALS)
        w = assert_model_is_the_rebuild(M, D, r + 1, (ocap, r))
        assert info.tolist() == [int(w["info"][0]) - before, int(w["info"][0]), info[2], info[3]] and info[3] == (info[3] & 15)
        assert (M.fused, M.rows_seen, M.a, M.b) == (r + 1, M.rows(), before, M.rows())
        if D["sizes"][r] == 0:
            assert info.tolist() == [0, before, 0, 0]
        if r == D["n"] - 1:                                         # the cloud inside known voxels: counts only
            assert info.tolist() == [0, before, D["sizes"][r], 0] and M.dirty_rows() == set()
        saw_overflow |= bool(info[3] & wnp.OVERFLOW)
        saw_valid |= bool((M.ninfo > 0).any())
    assert saw_valid
    if ocap == 300:
        assert saw_overflow and M.rows() == 300 and int(M.state[1]) & wnp.OVERFLOW     # reached in the middle of a cloud
        at = [wnp.fuse(D["m_xyz"], D["m_inten"], D["m_offs"], D["poses"], n, M.cell, 1, "first", out_capacity=ocap)["info"][1] for n in (M.fused - 1, M.fused)]
        assert at[0] < 300 < at[1]                                  # the cloud brings rows below the capacity and voxels past it
    else:
        assert not saw_overflow and M.fused == D["n"]


def test_a_rebuild_in_the_middle_and_a_growing_neighbourhood():
    """extends behind a rebuild at n = 3 equal the rebuild at 4 .. ; a normal flips from invalid to valid when the row that completes
    its neighbourhood arrives (k = min_nbrs - 1 -> min_nbrs)"""
    D = gnp.drive()
    M = gnp.Model(D["m_xyz"], D["m_inten"], D["m_offs"], 2048, D["cell"], 600)
    M.rebuild(D["poses"], 3, gnp.NORMALS)
    assert M.fused == 3 and M.a == M.b == M.rows() and M.dirty_rows() == set()
    for r in range(3, 6):
        M.extend(D["poses"], r, D["n"])
        M.normals(**gnp.NORMALS)
        assert_model_is_the_rebuild(M, D, r + 1, ("from 3", r))
    M = gnp.Model(gnp.FLIP[0], np.zeros(8, np.float32), gnp.FLIP[1], 32, 1.0, 8)
    poses = wnp.identity_poses(3)
    kw = gnp.FLIP[2]
    M.rebuild(poses, 1, kw)
    assert M.ninfo[:3].tolist() == [-3, -2, -2]                    # row 0 has itself and two neighbours within the radius: one short
    assert M.extend(poses, 1, 2).tolist() == [1, 4, 1, 0]
    assert M.dirty_rows() == {0, 2, 3}                             # row 1's voxel (1, 0, 0) is two away from the new (-1, 0, 0)
    M.normals(**kw)
    assert M.ninfo[:4].tolist() == [4, -2, -2, -2] and (M.ninfo[4:] == 0).all() and M.normals_[0, 2] > 0.99
    ix = mnp.index(M.xyz, 4, 1.0, 32)
    wn, wi = pnp.normals(ix, M.xyz, out_capacity=32, **kw)
    assert wi.tolist() == M.ninfo.tolist() and wn.tobytes() == M.normals_.tobytes()


def test_refusals_and_the_switched_off_call_leave_the_model_unchanged():
    D = gnp.drive()
    M = gnp.Model(D["m_xyz"], D["m_inten"], D["m_offs"], 300, D["cell"], 600)
    M.rebuild(D["poses"], 2, gnp.NORMALS)
    R = M.rows()
    for r, map_n, want in ((-1, 8, 0), (-5, 8, 0), (1, 8, gnp.ORDER), (3, 8, gnp.ORDER), (2, 2, gnp.ORDER), (1 << 30, 8, gnp.ORDER)):
        snap = M.snapshot()
        assert M.extend(D["poses"], r, map_n).tolist() == [0, R, 0, want], (r, map_n)
        assert M.snapshot() == snap, (r, map_n)
    M.state[0] = R - 1                                             # somebody fused without a sync
    snap = M.snapshot()
    assert M.extend(D["poses"], 2, 8).tolist() == [0, R - 1, 0, gnp.STALE] and M.snapshot() == snap
    assert M.extend(D["poses"], 1, 8).tolist() == [0, R - 1, 0, gnp.STALE | gnp.ORDER] and M.snapshot() == snap
    M.state[0] = R
    M.state[1] |= wnp.OVERFLOW
    snap = M.snapshot()
    assert M.extend(D["poses"], 2, 8).tolist() == [0, R, 0, gnp.FULL] and M.snapshot() == snap
    M.state[1] = 0
    assert M.extend(D["poses"], 2, 8)[3] == 0 and M.fused == 3     # and the accepted call goes through
    # a pose row with a NaN: every point skipped, fused advances, nothing stored; the rebuild says the same
    bad = D["poses"].copy()
    bad[3, 7] = np.nan
    R = M.rows()
    assert M.extend(bad, 3, 8).tolist() == [0, R, 0, wnp.SKIPPED] and M.fused == 4
    w = wnp.fuse(D["m_xyz"], D["m_inten"], D["m_offs"], bad, 4, M.cell, 1, "first", out_capacity=300)
    assert w["state"].tobytes() == M.state.tobytes()
