"""The local submaps without a device (pr_submap): the header's rule text, the exported and bound symbols, the scratch
formula, every refusal that comes before a device is touched, the NumPy restatement (submap_np.py) against hand-written lists and a
five-row model, its transform against posegraph_np, and the corner scene on the restatements (icp_np.py): single-cloud ICP of the revisit
pair is rejected, the w = 3 submap pair is accepted and recovers the planted pose."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import icp_np
import posegraph_np as pg
import submap_cases as cases
import submap_np as sn
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_submap_create", "pr_submap_destroy", "pr_submap_scratch_bytes", "pr_submap_build_dev", "pr_submap_build")
IMAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ 1. header, symbols, formula, refusals
def test_header_carries_the_rule_and_the_symbols_are_bound():
    h = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for phrase in ("tests/submap_np.py", "r_0 = centre, then centre - 1, centre + 1, centre - 2, centre + 2", "With past_only != 0 only rows <= centre",
                   "|r - avoid[p]| > avoid_gap", "the centre is exempt", "no address is formed from it", "a submap never holds part of a cloud",
                   "centre < 0 switches the slot off", "PR_SUBMAP_NO_CENTER", "a slot is never partial", "entries c + 1 .. slot_capacity are set to out_offs[c]",
                   "Rows of out_xyz at or behind out_offs[c] are not written", "copied bit for bit", "y = R_c (R_r^T (x - t_r)) + t_c",
                   "u_k = (R_r[0][k] d_0 + R_r[1][k] d_1) +", "y_k = v_k + t_c[k]", "no voxel de-duplication",
                   "enum { PR_SUBMAP_TRUNCATED = 1, PR_SUBMAP_NO_CENTER = 2, PR_SUBMAP_OVERFLOW = 4 }"):
        assert phrase in h, phrase
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert C.sizeof(_lib.SubmapParams) == 16 and [n for n, _ in _lib.SubmapParams._fields_] == ["half_window", "past_only", "avoid_gap", "max_pts"]
    assert (_lib.SUBMAP_TRUNCATED, _lib.SUBMAP_NO_CENTER, _lib.SUBMAP_OVERFLOW) == (sn.TRUNCATED, sn.NO_CENTER, sn.OVERFLOW) == (1, 2, 4)
    mk = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "Makefile")).read()
    assert "submap.o: submap.hip submap.hpp trajeval.hpp\n\t$(HIPCC) $(GENFLAGS)" in mk          # GENFLAGS carries -ffp-contract=off


def r16(x):
    return (x + 15) & ~15


@pytest.mark.parametrize("S,w", [(1, 0), (3, 1), (65, 2), (1024, 5), (65535, 31), (7, 31)])
def test_scratch_formula(S, w):
    L = 2 * w + 1
    want = 3 * r16(4 * S * L) + r16(8 * S * L) + 3 * r16(4 * S) + r16(8 * S)
    assert _lib.load().pr_submap_scratch_bytes(S, w) == want


@pytest.mark.parametrize("S,w,P,M,K,word", [(0, 1, 10, 10, 10, "slot_capacity"), (65536, 1, 10, 10, 10, "slot_capacity"), (4, -1, 10, 10, 10, "w_max"),
                                            (4, 32, 10, 10, 10, "w_max"), (4, 1, 0, 10, 10, "point_capacity"), (4, 1, (1 << 40) + 1, 10, 10, "point_capacity"),
                                            (4, 1, 10, 0, 10, "max_cloud_points"), (4, 1, 10, (1 << 26) + 1, 10, "max_cloud_points"),
                                            (4, 1, 10, 10, 0, "keyframe_capacity"), (4, 1, 10, 10, (1 << 24) + 1, "keyframe_capacity")])
def test_bad_sizes_are_refused_before_a_device_is_touched(S, w, P, M, K, word):
    lib = _lib.load()
    h = C.c_void_p(5)
    assert lib.pr_submap_create(None, S, w, P, M, K, C.byref(h)) == _lib.PR_EINVAL and not h
    assert word in lib.pr_last_error(None).decode()
    if word in ("slot_capacity", "w_max"):
        assert lib.pr_submap_scratch_bytes(S, w) == 0


def prm(**kw):
    d = dict(half_window=1, past_only=0, avoid_gap=0, max_pts=100)
    d.update(kw)
    return _lib.SubmapParams(*(d[n] for n, _ in _lib.SubmapParams._fields_))


@pytest.mark.parametrize("c,kw,word", [(-1, {}, "c=-1"), (65536, {}, "c=65536"), (1, dict(half_window=-1), "half_window=-1"),
                                       (1, dict(half_window=32), "half_window=32"), (1, dict(max_pts=0), "max_pts=0"), (1, dict(max_pts=-5), "max_pts=-5"),
                                       (1, dict(avoid_gap=-1), "avoid_gap=-1"), (1, None, "params is NULL"), (0, {}, "handle is NULL"),
                                       (1, {}, "handle is NULL")])
def test_bad_build_arguments_are_refused_before_a_device_is_touched(c, kw, word):
    """without a handle the limits are create's widest; with one (test_gpu_submap.py) they are the handle's"""
    lib = _lib.load()
    p = None if kw is None else prm(**kw)
    for fn, who in ((lib.pr_submap_build_dev, "pr_submap_build_dev: "), (lib.pr_submap_build, "pr_submap_build: ")):
        assert fn(None, None, None, None, None, None, c, None if p is None else C.byref(p), None, None, None, None) == _lib.PR_EINVAL
        msg = lib.pr_last_error(None).decode()
        assert msg.startswith(who) and word in msg, msg


def test_create_and_destroy_refusals():
    lib = _lib.load()
    out = C.c_void_p()
    assert lib.pr_submap_create(None, 4, 1, 10, 10, 10, None) == _lib.PR_EINVAL and "out is NULL" in lib.pr_last_error(None).decode()
    assert lib.pr_submap_create(None, 4, 1, 10, 10, 10, C.byref(out)) == _lib.PR_EINVAL and "ctx is NULL" in lib.pr_last_error(None).decode()
    lib.pr_submap_destroy(None)


def test_the_class_refuses_a_foreign_map_before_the_library():
    sb = api.SubmapBuilder.__new__(api.SubmapBuilder)
    ctx = types.SimpleNamespace(device=0)
    sb.ctx, sb.h, sb.lib, sb.slot_capacity, sb.w_max, sb.point_capacity, sb.max_cloud_points, sb.keyframe_capacity = ctx, None, None, 4, 2, 100, 10, 8
    foreign = types.SimpleNamespace(ctx=object(), keyframe_capacity=8)
    other = types.SimpleNamespace(ctx=ctx, keyframe_capacity=9)
    for fn in (sb.build_torch, sb.build):
        with pytest.raises(ValueError, match="share one context"):
            fn(foreign, np.zeros(1, np.int32), w=1)
        with pytest.raises(ValueError, match="keyframe_capacity"):
            fn(other, np.zeros(1, np.int32), w=1)
    sb.out = None
    with pytest.raises(ValueError, match="share one context"):
        sb.pair_torch(foreign, types.SimpleNamespace(numel=lambda: 1), None, w=1, out=(None, None))
    mine = types.SimpleNamespace(ctx=ctx, keyframe_capacity=8)
    with pytest.raises(ValueError, match="w must lie in 0 .. w_max"):
        sb.build(mine, np.zeros(1, np.int32), w=3)
    with pytest.raises(ValueError, match="0 .. slot_capacity"):
        sb.build(mine, np.zeros(5, np.int32), w=1)


# ------------------------------------------------------------------------------------------------ 2. the restatement's walk
def test_walk_order_against_hand_written_lists():
    n = 9
    assert sn.walk(0, 2) == [0, -1, 1, -2, 2]
    assert sn.walk(1, 2) == [1, 0, 2, -1, 3]
    assert sn.walk(n - 1, 2) == [8, 7, 9, 6, 10]
    assert sn.walk(4, 0) == [4] and sn.walk(IMAX, 1) == [IMAX, IMAX - 1, IMAX + 1]
    assert sn.walk(4, 2, past_only=True) == [4, 3, 2] and sn.walk(0, 2, past_only=True) == [0, -1, -2]


def model(sizes=(2, 3, 0, 4, 1)):
    xyz, offs, poses = cases.random_map(sizes, seed=11)
    return xyz, offs, poses


def taken(offs, poses, n, centre, avoid=None, **kw):
    d = dict(w=2, past_only=False, avoid_gap=0, max_pts=1000, max_cloud_points=100)
    d.update(kw)
    entries, flags = sn.plan_slot(offs, poses, n, centre, avoid, **d)
    return [e[0] for e in entries], flags


def test_the_walk_is_cut_at_both_ends_of_the_map_and_by_past_only():
    xyz, offs, poses = model()
    assert taken(offs, poses, 5, 0) == ([0, 1, 2], 0)
    assert taken(offs, poses, 5, 1) == ([1, 0, 2, 3], 0)
    assert taken(offs, poses, 5, 4) == ([4, 3, 2], 0)
    assert taken(offs, poses, 3, 2) == ([2, 1, 0], 0)                # rows >= n are not there
    assert taken(offs, poses, 5, 2, past_only=True) == ([2, 1, 0], 0)
    assert taken(offs, poses, 5, 0, past_only=True) == ([0], 0)
    assert taken(offs, poses, 5, -1) == ([], 0)                      # switched off: no flag
    assert taken(offs, poses, 5, 5) == ([], sn.NO_CENTER) and taken(offs, poses, 5, IMAX) == ([], sn.NO_CENTER)
    bad = poses.copy(); bad[2, 7] = np.nan
    assert taken(offs, bad, 5, 2) == ([], sn.NO_CENTER)
    assert taken(offs, bad, 5, 3) == ([3, 4, 1], 0)                  # a neighbour's pose: the row is skipped, the walk goes on
    bad[2, 7] = np.inf
    assert taken(offs, bad, 5, 1) == ([1, 0, 3], 0)


def test_the_avoid_band():
    xyz, offs, poses = model()
    assert taken(offs, poses, 5, 2, avoid=3, avoid_gap=0) == ([2, 1, 0, 4], 0)        # gap 0: the row itself only
    assert taken(offs, poses, 5, 2, avoid=3, avoid_gap=1) == ([2, 1, 0], 0)           # the centre is exempt although |2 - 3| <= 1
    assert taken(offs, poses, 5, 2, avoid=2, avoid_gap=0) == ([2, 1, 3, 0, 4], 0)     # avoid == centre: exempt
    assert taken(offs, poses, 5, 2, avoid=40, avoid_gap=3) == ([2, 1, 3, 0, 4], 0)
    for av in (0, 3, IMAX):                                                            # the largest gap: nothing but the centre
        assert taken(offs, poses, 5, 2, avoid=av, avoid_gap=IMAX) == ([2], 0)
    # |r + 2^31| = 2^31 + r exceeds the largest i32: every row is eligible - in 32-bit arithmetic the difference would wrap
    assert taken(offs, poses, 5, 2, avoid=-2 ** 31, avoid_gap=IMAX) == ([2, 1, 3, 0, 4], 0)


def test_whole_row_and_whole_slot_capacity_on_the_five_row_model():
    xyz, offs, poses = model()                                       # lengths 2, 3, 0, 4, 1; walk of centre 2: rows 2, 1, 3, 0, 4
    assert taken(offs, poses, 5, 2, max_pts=10) == ([2, 1, 3, 0, 4], 0)               # met exactly
    assert taken(offs, poses, 5, 2, max_pts=9) == ([2, 1, 3, 0], sn.TRUNCATED)         # exceeded by one point: row 4 ends the walk
    assert taken(offs, poses, 5, 2, max_pts=6) == ([2, 1], sn.TRUNCATED)               # row 3 does not fit: rows 0 and 4 are not tried
    assert taken(offs, poses, 5, 3, max_pts=3) == ([], sn.TRUNCATED)                   # the centre itself
    assert taken(offs, poses, 5, 2, max_cloud_points=3) == ([2, 1, 0, 4], 0)           # a row above max_cloud_points is skipped
    scr = offs.copy(); scr[2] = offs[1] - 1                                            # row 1: negative length; row 2: 4 points
    assert taken(scr, poses, 5, 2, max_cloud_points=3) == ([0, 4], 0)                  # a centre that fails only the length test is skipped
    assert taken(scr, poses, 5, 2, max_cloud_points=4) == ([2, 3, 0, 4], 0)
    scr[0] = -1                                                                        # a negative start: row 0 forms no address
    assert taken(scr, poses, 5, 2, max_cloud_points=4) == ([2, 3, 4], 0)
    kw = dict(slot_capacity=4, max_cloud_points=100, keyframe_capacity=5, w=1, max_pts=100)
    full = sn.build(xyz, offs, poses, 5, [0, 3, 1], point_capacity=100, **kw)          # slots of 5, 5 and 5 points
    assert full["offs"].tolist() == [0, 5, 10, 15, 15] and full["rows"].tolist() == [[2, 0], [3, 0], [3, 0], [0, 0]] and full["info"].tolist() == [3, 15, 0, 0]
    cut = sn.build(xyz, offs, poses, 5, [0, 3, 4], point_capacity=9, **kw)             # slot 1 (5 points) does not fit behind slot 0, slot 2 (1 + 4) does not either
    assert cut["offs"].tolist() == [0, 5, 5, 5, 5] and cut["rows"].tolist() == [[2, 0], [0, 4], [0, 4], [0, 0]]
    cut = sn.build(xyz, offs, poses, 5, [0, 3, 2], point_capacity=9, **dict(kw, w=0))  # slots of 2, 4, 0 points: all fit
    assert cut["offs"].tolist() == [0, 2, 6, 6, 6] and cut["info"].tolist() == [3, 6, 0, 0]
    cut = sn.build(xyz, offs, poses, 5, [1, 3, 0], point_capacity=6, **dict(kw, w=0))  # 3, then 4 overflows, then 2 goes behind slot 0
    assert cut["offs"].tolist() == [0, 3, 3, 5, 5] and cut["rows"].tolist() == [[1, 0], [0, 4], [1, 0], [0, 0]] and cut["info"].tolist() == [2, 5, 0, 4]
    assert cut["xyz"].tobytes() == np.concatenate([xyz[2:5], xyz[0:2]]).tobytes()      # the centre rows, bit for bit


# ------------------------------------------------------------------------------------------------ 3. the transform
@pytest.mark.parametrize("shift", [0.0, 5.0e6])
def test_transform_against_posegraph_np(shift):
    """y = R_c (R_r^T (x - t_r)) + t_c against T x with T = posegraph_np.mul(P_c, inv(P_r)).  Every intermediate of either form is at most
    M = |x| + |t_r| + |t_c| in norm (rotations keep norms).  The rule rounds 12 times per component (1 difference, 5 + 5 in the two dot
    products, 1 sum); the reference about 17 (5 per entry of R_c R_r^T, 6 for its translation, 6 to apply it); every rounding is at most
    2^-53 of an intermediate, so the two differ by at most 29 x 2^-53 M < 2^-48 M per component."""
    xyz, offs, poses = cases.random_map((40, 40, 40), seed=3, shift=shift)
    for r, c in ((0, 1), (2, 0), (1, 2)):
        x = xyz[offs[r]:offs[r + 1]]
        y = sn.transform(x, poses[r], poses[c])
        T = pg.mul(poses[c], pg.inv(poses[r]))
        ref = x @ T[:, :3].T + T[:, 3]
        M = np.linalg.norm(x, axis=1) + np.linalg.norm(poses[r].reshape(3, 4)[:, 3]) + np.linalg.norm(poses[c].reshape(3, 4)[:, 3])
        assert (np.abs(y - ref).max(axis=1) <= 2.0 ** -48 * M).all(), (shift, r, c, np.abs(y - ref).max())
    assert sn.transform(np.zeros((0, 3)), poses[0], poses[1]).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 4. the scene that shows the point
def test_corner_scene_on_the_restatements():
    """single-cloud ICP of the revisit pair is rejected (too few inliers: two keyframes share two landmarks), the w = 3 submap pair is
    accepted and moves the seed's error (0.035 rad, 0.116 m) to the noise level; the decisions are far from their thresholds, so a
    device that sums in another order takes the same ones"""
    sc, K = cases.corner_scene(), cases.CORNER
    res = {}
    for w in (0, K["w"]):
        q, db = cases.corner_sets(sc, w)
        assert len(q) == K["per_keyframe"] * (w + 1) and len(db) == K["per_keyframe"] * (2 * w + 1)
        res[w] = icp_np.icp(q, db, sc["T0"], **K["icp"])
    single, sub = res[0], res[K["w"]]
    ok = lambda r: r["status"] in (icp_np.CONVERGED, icp_np.MAX_ITER) and r["fitness"] >= K["min_fitness"] and r["rmse"] <= K["max_rmse"]
    assert single["status"] == icp_np.TOO_FEW and not ok(single)
    assert ok(sub) and sub["n_inl"] >= 2 * K["icp"]["min_inliers"]
    seed, got = cases.pose_error(sc["T0"], sc["T_true"]), cases.pose_error(sub["T"], sc["T_true"])
    print(f"   corner scene: seed error {seed}, w = 3 submaps {got}, fitness {sub['fitness']:.3f}, rmse {sub['rmse']:.4f}, n_inl {sub['n_inl']}")
    assert got[0] < seed[0] / 10 and got[1] < seed[1] / 10
    assert min(sub["nn_margin"]) > 1e-6 and min(sub["corr_margin"]) > 1e-6 and sub["stop_margin"] > 1e-3
    assert min(single["corr_margin"]) > 1e-6
