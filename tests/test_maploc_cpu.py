"""The map localiser (pr_maploc) without a device: the ABI surface, the scratch formula, the argument errors that are
returned before any device is touched, what the Python class refuses before it calls the library, and properties of the NumPy
restatement the GPU tests compare the kernels with (maploc_np.py): its voxel walk is the plain brute-force scan, the containment claim at
the radius, the seed rule against posegraph_np, and the committed colliding keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import maploc_np as mnp
import posegraph_np as pg
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_maploc_create", "pr_maploc_destroy", "pr_maploc_scratch_bytes", "pr_maploc_count", "pr_maploc_index_dev", "pr_maploc_seed_dev",
         "pr_maploc_nn_dev", "pr_maploc_refine_dev", "pr_maploc_index", "pr_maploc_nn", "pr_maploc_refine")


def test_maploc_symbols_records_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_maploc_")) == sorted(NAMES)
    assert re.search(r"enum \{ PR_MAPLOC_SKIPPED = 1, PR_MAPLOC_RANGE = 2, PR_MAPLOC_DUPLICATE = 4, PR_MAPLOC_TABLE = 8 \};", code)
    assert (_lib.MAPLOC_SKIPPED, _lib.MAPLOC_RANGE, _lib.MAPLOC_DUPLICATE, _lib.MAPLOC_TABLE) == (1, 2, 4, 8)
    assert (mnp.SKIPPED, mnp.RANGE, mnp.DUPLICATE, mnp.TABLE) == (1, 2, 4, 8)
    assert "typedef struct pr_maploc pr_maploc;" in code
    assert re.search(r"pr_maploc_create\(pr_ctx\* ctx, const pr_worldmap_buffers\* world,", code)      # the record, not the pr_worldmap handle
    assert C.sizeof(_lib.WorldMapBuffers) == 6 * C.sizeof(C.c_void_p)
    for m in ("index_torch", "seed_torch", "nn_torch", "refine_torch", "localize_torch", "index", "nn", "refine", "count", "close"):
        assert hasattr(api.MapLocalizer, m), m
    for words in ("pr_maploc", "DESIGN.md 4.20", "floor(x_a / cell)", "[-2^20, 2^20)", "[-2^20 - 1, 2^20 + 1)", "compared as a double",
                  "smaller d2, then smaller j", "max_corr (1 + 2^-10)", "PR_MAPLOC_TABLE", "tinv_a = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2)",
                  "(Rinv[a][0] Rr[0][b] +"):
        assert words in txt, words
    hip = open(os.path.join(CSRC, "maploc.hip")).read()
    assert "step < T" in hip and "step < Tn" in hip and "0x9E3779B97F4A7C15ull" in hip
    assert "chunk_sums(A, S, T, pair, i, i < S.ns, bd, bj, mc2, red," in hip and '#include "icp_common.hpp"' in hip
    assert "-((P[a] * P[3] + P[4 + a] * P[7]) + P[8 + a] * P[11])" in hip
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"maploc\.o: maploc\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "-ffp-contract=off" in mk


def test_maploc_scratch_size_formula():
    lib = _lib.load()
    for ocap, pc, ms in ((32, 8, 513), (600, 5, 257), (1, 1, 0), (1 << 20, 64, 4096), (257, 3, 1), (1025, 65535, 256), (8, 2, 255)):
        T = 1 << mnp.log2T(ocap)
        assert T >= 64 and T >= 2 * ocap and (T == 64 or T < 4 * ocap)
        want = mnp.scratch_bytes(ocap, pc, ms)
        assert want > 16 * T and lib.pr_maploc_scratch_bytes(ocap, pc, ms) == want, (ocap, pc, ms)
    assert 1 << mnp.log2T(32) == 64 and 1 << mnp.log2T(600) == 2048
    for bad in ((0, 1, 1), ((1 << 29) + 1, 1, 1), (8, 0, 1), (8, 65536, 1), (8, 1, -1), (8, 1, (1 << 26) + 1)):
        assert lib.pr_maploc_scratch_bytes(*bad) == 0 and mnp.scratch_bytes(*bad) == 0, bad
    assert lib.pr_maploc_scratch_bytes(1 << 29, 1, 0) > 16 << 30


def _bufs(null=None):
    """a pr_worldmap_buffers of non-NULL addresses that are never dereferenced (every case below fails before the device is touched)"""
    store = (C.c_double * 8)()
    b = _lib.WorldMapBuffers(*([C.addressof(store)] * 6))
    if null:
        setattr(b, null, None)
    return b, store


def test_maploc_create_argument_errors():
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    b, keep = _bufs()

    def create(world=b, ocap=8, cell=1.0, pc=4, ms=16, out=True):
        h = C.c_void_p(1)
        rc = lib.pr_maploc_create(None, C.byref(world) if world is not None else None, ocap, cell, pc, ms, C.byref(h) if out else None)
        assert rc == _lib.PR_EINVAL and (not out or not h.value)
        return err()

    assert "out is NULL" in create(out=False)
    assert "world is NULL" in create(world=None)
    for name in ("xyz", "row", "state"):
        assert "a buffer is NULL" in create(world=_bufs(null=name)[0]), name
    for oc in (0, -1, (1 << 29) + 1):
        assert "out_capacity=%d outside" % oc in create(ocap=oc)
    for cell in (0.0, -0.2, -0.0, float("nan"), float("inf"), -float("inf")):
        assert "cell must be finite and positive" in create(cell=cell), cell
    for pc in (0, -1, 65536):
        assert "pair_capacity=%d outside" % pc in create(pc=pc)
    for ms in (-1, (1 << 26) + 1):
        assert "max_src_pts=%d outside" % ms in create(ms=ms)
    assert "ctx is NULL" in create()                   # the last check: everything else was in order
    for unused in ("inten", "src", "count"):           # members the localiser does not read may be NULL
        assert "ctx is NULL" in create(world=_bufs(null=unused)[0]), unused


def test_maploc_null_handles_and_values():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    r, f = C.c_int64(7), C.c_int32(7)
    err = lambda: lib.pr_last_error(None)
    assert lib.pr_maploc_count(None, C.byref(r), C.byref(f)) == _lib.PR_EINVAL and b"pr_maploc_count: localiser is NULL" in err()
    assert lib.pr_maploc_index_dev(None, buf) == _lib.PR_EINVAL and b"pr_maploc_index_dev: localiser is NULL" in err()
    assert lib.pr_maploc_index(None, buf) == _lib.PR_EINVAL and b"pr_maploc_index: localiser is NULL" in err()
    assert lib.pr_maploc_seed_dev(None, buf, buf, 8, buf, None, None, None, 1, buf, buf) == _lib.PR_EINVAL and b"localiser is NULL" in err()
    for kcap in (0, -4):
        assert lib.pr_maploc_seed_dev(None, buf, buf, kcap, buf, None, None, None, 1, buf, buf) == _lib.PR_EINVAL
        assert b"pr_maploc_seed_dev: keyframe_capacity=%d is below 1" % kcap in err()
    forms = (("pr_maploc_nn_dev", lambda mc, **kw: lib.pr_maploc_nn_dev(None, buf, buf, 1, buf, 1, buf, None, mc, buf, buf, buf)),
             ("pr_maploc_nn", lambda mc, **kw: lib.pr_maploc_nn(None, buf, buf, 1, buf, 1, buf, None, mc, buf, buf, buf)),
             ("pr_maploc_refine_dev", lambda mc, it=5, tr=1e-6, tf=1e-6, mi=3:
              lib.pr_maploc_refine_dev(None, buf, buf, 1, buf, 1, buf, None, it, mc, tr, tf, mi, buf, buf)),
             ("pr_maploc_refine", lambda mc, it=5, tr=1e-6, tf=1e-6, mi=3:
              lib.pr_maploc_refine(None, buf, buf, 1, buf, 1, buf, None, it, mc, tr, tf, mi, buf, buf)))
    for name, call in forms:
        who = name.encode()
        assert call(0.5) == _lib.PR_EINVAL and who + b": localiser is NULL" in err()
        for mc in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(mc) == _lib.PR_EINVAL and who + b": max_corr=" in err(), (name, mc)
        if "refine" in name:                           # the checks of check_params in icp.cpp
            assert call(0.5, it=-1) == _lib.PR_EINVAL and who + b": max_iter=-1 < 0" in err()
            assert call(0.5, mi=2) == _lib.PR_EINVAL and who + b": min_inliers=2 < 3" in err()
            assert call(0.5, tr=float("nan")) == _lib.PR_EINVAL and b"is NaN" in err()
            assert call(0.5, tf=float("nan")) == _lib.PR_EINVAL and b"is NaN" in err()
    lib.pr_maploc_destroy(None)                        # a no-op


def test_map_localizer_refuses_before_the_library():
    import torch

    class Fake:
        pass
    wm = Fake(); wm.ctx, wm.out_capacity, wm.NAMES = object(), 16, api.WorldMap.NAMES
    with pytest.raises(ValueError, match="share one context"):
        api.MapLocalizer(object(), wm, 1.0, 4, 16)     # a world map of another context: refused before any handle exists
    ml = api.MapLocalizer.__new__(api.MapLocalizer)    # no handle, no library call: the checks are the first thing a method does
    wm.state = torch.zeros(4, dtype=torch.int32)
    ml.ctx, ml.wm, ml.h, ml.cell, ml.pair_capacity, ml.max_src_pts = wm.ctx, wm, None, 1.0, 4, 16
    x, o, ps, T = torch.zeros((8, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 3, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="info must be"):
        ml.index_torch(info=torch.zeros(4, dtype=torch.int32))
    for call in (ml.nn_torch, ml.refine_torch):
        with pytest.raises(ValueError, match="xyz_q must be a contiguous CUDA tensor"):
            call(x, o, ps, T)                          # not on the device
        with pytest.raises(ValueError, match="xyz_q must be"):
            call(x.float(), o, ps, T)
    with pytest.raises(ValueError, match="poses must be"):
        ml.seed_torch(torch.zeros((8, 12), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), ps)
    with pytest.raises(ValueError, match="CSR set"):
        ml.nn(np.zeros((8, 3)), [0, 4], [0], np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match=r"T must be \[c, 3, 4\]"):
        ml.refine(np.zeros((8, 3)), [0, 8], [0, 0], np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match=r"excl must be \[c, 2\]"):
        ml.nn(np.zeros((8, 3)), [0, 8], [0], np.zeros((1, 3, 4)), excl=[1, 2, 3])


# ------------------------------------------------------------------------------------------------ the restatement
def _world(seed, rows, spread=6.0, cell=1.0):
    """rows world points, one per voxel (as a fuse at `cell` leaves them), their keyframe rows ascending"""
    rng = np.random.default_rng(seed)
    seen, pts = set(), []
    while len(pts) < rows:
        p = rng.normal(0, spread, 3)
        k = tuple(np.floor(p / cell).astype(int))
        if k not in seen:
            seen.add(k); pts.append(p)
    return np.array(pts).reshape(-1, 3), np.sort(rng.integers(0, 6, rows)).astype(np.int32)


def test_the_voxel_walk_is_the_brute_force_scan_over_its_candidate_set():
    """maploc_np.nn (27 voxels) against maploc_np.nn_brute (every indexed, non-excluded row, masked): with and without exclusion
    windows, with NaN / Inf rows and sources, duplicates of a coarser index, and the largest max_corr the cell allows."""
    xyz, row = _world(1, 700)
    xyz[13] = (np.nan, 0, 0); xyz[99] = (0, np.inf, 0)
    rng = np.random.default_rng(2)
    P = xyz[rng.integers(0, 700, 900)] + rng.normal(0, 0.4, (900, 3))
    P[5] = (np.nan, 1, 1); P[6] = (1, -np.inf, 1); P[7] = (1e300, 0, 0); P[8] = P[9]
    for cell, mc in ((1.0, 1.0 / mnp.SLACK), (1.0, 0.5), (2.0, 1.5)):
        ix = mnp.index(xyz, 700, cell)
        assert ix["flags"] & mnp.SKIPPED and bool(ix["flags"] & mnp.DUPLICATE) == (cell == 2.0) and ix["info"][1] == 700
        assert len(ix["rows"]) == len(ix["first"]) == ix["info"][0] and (cell == 2.0 or ix["info"][0] == 698)
        for excl in (None, (2, 3), (0, 5), (4, 1)):
            a = mnp.nn(ix, xyz, row, P, mc, excl)
            b = mnp.nn_brute(ix, xyz, row, P, mc, excl)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (cell, mc, excl)
            assert a[0][5] == a[0][6] == a[0][7] == -1 and ((a[0] >= 0).any() or excl == (0, 5)) and not (excl == (0, 5) and (a[0] >= 0).any())
            if excl is not None and excl[0] <= excl[1]:
                hit = a[0][a[0] >= 0]
                assert not ((row[hit] >= excl[0]) & (row[hit] <= excl[1])).any()
    assert mnp.index(xyz, 1 << 30, 1.0)["R"] == 700 and mnp.index(xyz, -3, 1.0)["info"].tolist() == [0, 0, 0, 0]


def test_voxel_formulas_restate_the_source_text():
    hip = open(os.path.join(CSRC, "maploc.hip")).read()
    hpp = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert re.search(r"constexpr double MAPLOC_SLACK = 1\.0 \+ 0x1p-10;", hpp) and mnp.SLACK == 1.0 + 2.0 ** -10
    quot = re.search(r"double voxel_quot\(double x, double cell\) \{ return (.*?); \}", hip).group(1)
    coord = re.search(r"double voxel_coord\(double x, double cell\) \{ return (.*?); \}", hip).group(1)
    assert quot == mnp.voxel_quot.__doc__ and coord == mnp.voxel_coord.__doc__
    code = re.sub(r"//[^\n]*", "", hip)
    assert code.count("voxel_quot(") == 3 and "voxel_quot(p[a], v.cell)" in code  # its definition, voxel_coord and the probe: one division
    assert code.count("voxel_coord(") == 4                                        # its definition and the index's three axes
    assert code.count("floor(") == 2 and "(int)floor(t)" in code                  # voxel_coord's and the probe's floor of the same quotient
    assert "max_corr * pr::MAPLOC_SLACK > ml->v.cell" in open(os.path.join(CSRC, "maploc.cpp")).read()


def test_containment_margin_at_the_radius():
    """4 x 10^5 (target, source) coordinate pairs: cell = max_corr (1 + 2^-10) exactly, targets in voxels up to +-2^20, the source a few
    ulps either side of max_corr away.  Whenever d2 < fl(max_corr^2) - on the rounded values, as the kernels form it - the two voxel
    indices differ by at most 1 and the probe's range test keeps the source, so the source's 27 voxels hold the target."""
    rng = np.random.default_rng(11)
    n = 100000
    seen_in = seen_out = 0
    for trial in range(4):
        with np.errstate(all="ignore"):
            if trial == 3:                              # unit cell (a cell that is no multiple of max_corr's slack), lattice-like targets
                cell = np.ones(n); mc = np.nextafter(cell / mnp.SLACK, 0.0)
                while np.any(mc * mnp.SLACK > cell):
                    mc = np.where(mc * mnp.SLACK > cell, np.nextafter(mc, 0.0), mc)
            else:
                mc = np.ldexp(1.0 + rng.random(n), rng.integers(-30, 30, n))
                cell = mc * mnp.SLACK                   # exactly the smallest cell the check admits
            assert np.all(mc * mnp.SLACK <= cell)
            if trial == 0:                              # voxel indices over the whole 21-bit range
                vox = rng.integers(-mnp.LIM, mnp.LIM, n).astype(np.float64)
            elif trial == 1:                            # at the range's two ends
                vox = np.where(rng.random(n) < 0.5, -mnp.LIM + rng.integers(0, 3, n), mnp.LIM - 1 - rng.integers(0, 3, n)).astype(np.float64)
            else:                                       # around the origin (both signs, -0.0 included)
                vox = rng.integers(-4, 4, n).astype(np.float64)
            frac = rng.choice([0.0, 1.0, -1.0], n) * np.ldexp(1.0, -rng.integers(1, 53, n)) + rng.choice([0.0, 0.5, 1.0], n)
            q = (vox + np.clip(frac, 0.0, 1.0)) * cell
            q = np.where(rng.random(n) < 0.2, np.round(q), q) if trial == 3 else q
            cq = mnp.voxel_coord(q, cell)
            indexed = (cq >= -mnp.LIM) & (cq < mnp.LIM)                # the target is in the index at all
            p = q + mc * rng.choice([-1.0, 1.0], n)
            for _ in range(3):                          # 0 .. 3 ulps, towards the target or away from it
                step = np.nextafter(p, np.where(rng.random(n) < 0.5, q, np.where(p > q, np.inf, -np.inf)))
                p = np.where(rng.random(n) < 0.6, step, p)
            dx = p - q
            d2 = ((dx * dx) + 0.0 * 0.0) + 0.0 * 0.0
            inl = indexed & (d2 < mc * mc)
            t = mnp.voxel_quot(p, cell)
            cp = np.floor(t)
        assert np.all(np.abs(cp[inl] - cq[inl]) <= 1), np.flatnonzero(inl & ~(np.abs(cp - cq) <= 1))[:5]
        assert np.all((t[inl] >= -(mnp.LIM + 1.0)) & (t[inl] < mnp.LIM + 1.0))       # the probe's range test keeps every inlier's source
        seen_in += int(inl.sum()); seen_out += int((indexed & ~inl).sum())
    assert seen_in > 50000 and seen_out > 50000 and seen_in + seen_out >= 390000


def test_seed_rule_against_posegraph_np():
    """T0 = inv(P_idx) o T_rel to a few roundings of posegraph_np's inv / mul; the OFF rules; the exact bits of the plain inverse."""
    rng = np.random.default_rng(5)
    kcap = 6
    poses = np.zeros((kcap, 3, 4))
    for r in range(kcap):
        poses[r, :, :3] = pg.exp_so3(rng.normal(0, 1.0, 3)); poses[r, :, 3] = rng.normal(0, 30.0, 3)
    poses[4, 1, 2] = np.nan
    T_rel = np.zeros((8, 3, 4))
    for p in range(8):
        T_rel[p, :, :3] = pg.exp_so3(rng.normal(0, 0.3, 3)); T_rel[p, :, 3] = rng.normal(0, 2.0, 3)
    T_rel[6, 0, 3] = np.inf
    idx = np.array([0, 3, -1, 5, 4, 2, 1, 5], np.int32)
    acc = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.uint8)
    src = np.arange(8, dtype=np.int32)[::-1].copy()
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    T0, ps = mnp.seed(poses, 5, idx, acc, T_rel, src)
    on = [True, True, False, False, False, True, False, False]       # idx -1 | not accepted | NaN pose | Inf T_rel | idx 5 >= n = 5
    assert ps.tolist() == [int(src[p]) if on[p] else -1 for p in range(8)]
    for p in range(8):
        if not on[p]:
            assert T0[p].tobytes() == eye.tobytes()
        else:
            want = pg.mul(pg.inv(poses[idx[p]]), T_rel[p])
            assert np.abs(T0[p] - want).max() <= 8 * np.finfo(float).eps * 64.0, p      # translations of ~ 50 m: a few roundings of them
    T0, ps = mnp.seed(poses, 99, idx, None, None, None)                # n beyond the capacity: clamped to it; no accepted, no T_rel, no src
    assert ps.tolist() == [0, 1, -1, 3, -1, 5, 6, 7]
    for p in (0, 1, 3, 5, 6, 7):
        P = poses[idx[p]]
        assert T0[p][:, :3].tobytes() == np.ascontiguousarray(P[:, :3].T).tobytes()
        assert np.abs(T0[p] - pg.inv(P)).max() <= 8 * np.finfo(float).eps * 64.0
    assert mnp.seed(poses, 0, idx)[1].tolist() == [-1] * 8 and mnp.seed(poses, -7, idx)[1].tolist() == [-1] * 8


def test_committed_colliding_keys():
    """ten keys share the home slot 62 of a T = 64 table - their chain wraps the table's end - and the other 22 are spread"""
    cells = mnp.COLLIDING_CELLS
    assert len(cells) == len(set(cells)) == 32 and mnp.log2T(32) == 6
    homes = [mnp.home_slot(mnp.key_of(c), 6) for c in cells]
    assert homes[:10] == [62] * 10 and len(set(homes[10:])) >= 12 and 62 not in homes[10:] and 63 not in homes[10:]
    assert all(0 <= mnp.key_of(c) < 1 << 63 for c in cells)
    assert mnp.key_of((-mnp.LIM, -mnp.LIM, -mnp.LIM)) == 0 and mnp.key_of((mnp.LIM - 1,) * 3) == (1 << 63) - 1
    assert mnp.key_of((1, 2, 3)) == ((mnp.LIM + 1) << 42) | ((mnp.LIM + 2) << 21) | (mnp.LIM + 3)      # c_0 highest, as the world map packs it


def test_the_boxed_refinement_is_the_full_scan_bit_for_bit():
    """maploc_np.icp scans, per pass, only the candidates inside the box of the transformed points widened by the radius; the result is
    icp_grid_np.icp_masked over every candidate, bit for bit, with and without an exclusion window."""
    import icp_grid_np
    xyz, row = _world(3, 900, spread=5.0)
    ix = mnp.index(xyz, 900, 1.0)
    rng = np.random.default_rng(4)
    R = pg.exp_so3(np.array([0.02, -0.03, 0.04]))
    P = (xyz[rng.permutation(900)[:250]] - np.array([0.2, -0.1, 0.15])) @ R            # T = [R | t] brings it back
    T0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    for excl in (None, (1, 2)):
        a = mnp.icp(ix, xyz, row, P, T0, excl, max_corr=0.9, max_iter=30)
        b = icp_grid_np.icp_masked(P, xyz[mnp.candidates(ix, row, excl)], T0, max_corr=0.9, max_iter=30)
        assert a["T"].tobytes() == b["T"].tobytes() and all(a[k] == b[k] for k in ("status", "iters", "n_inl", "fitness", "rmse")), excl
        assert a["n_inl"] > 100 and a["iters"] >= 2
