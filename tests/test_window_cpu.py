"""The resident point window (pr_window) without a device: the ABI surface, its argument errors, the cursor rule
(api.split_points_by_pose) and - against the oracle - that pushing the split delivers what the reference's file loop appends."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
import oracle_lib
import window_model
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_window_create", "pr_window_destroy", "pr_window_reset", "pr_window_count", "pr_window_push_dev", "pr_window_push")


def test_window_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert "PR_WINDOW_OVERFLOW = 1" in txt and _lib.WINDOW_OVERFLOW == 1
    assert all(hasattr(api.CloudWindow, m) for m in ("push", "push_torch", "reset", "count", "close"))


@pytest.mark.parametrize("args,word", [
    ((45.0, 0, 0, 1, 1), "capacities"), ((45.0, 0, 10, 0, 1), "capacities"), ((45.0, 0, 10, 1, -3), "capacities"),
    ((45.0, 0, 10, 11, 5), "max_new_points"), ((45.0, 2, 10, 5, 5), "polar"), ((45.0, -1, 10, 5, 5), "polar"),
    ((0.0, 0, 10, 5, 5), "lidarRange"), ((-45.0, 1, 10, 5, 5), "lidarRange"), ((float("nan"), 0, 10, 5, 5), "lidarRange"),
    ((float("inf"), 0, 10, 5, 5), "lidarRange"), ((45.0, 1, 10, 5, 5), "ctx is NULL")])
def test_window_argument_errors(args, word):
    """Value checks come before anything touches a device, so they are testable here: PR_EINVAL and a message that names the argument.
    (The NULL context is the last check: a valid argument set reaches it.)"""
    lib = _lib.load()
    h = C.c_void_p(1)
    rc = lib.pr_window_create(None, *args, C.byref(h))
    assert rc == _lib.PR_EINVAL and not h.value
    msg = lib.pr_last_error(None).decode()
    assert "pr_window_create" in msg and word in msg, msg


def test_window_null_handles():
    lib = _lib.load()
    n = C.c_int32(7)
    buf = (C.c_double * 64)()
    assert lib.pr_window_create(None, 45.0, 0, 10, 5, 5, None) == _lib.PR_EINVAL and b"out is NULL" in lib.pr_last_error(None)
    assert lib.pr_window_reset(None) == _lib.PR_EINVAL and b"pr_window_reset" in lib.pr_last_error(None)
    assert lib.pr_window_count(None, C.byref(n)) == _lib.PR_EINVAL and b"pr_window_count" in lib.pr_last_error(None)
    assert lib.pr_window_push_dev(None, buf, buf, buf, buf, 1, buf, buf, buf, buf, buf) == _lib.PR_EINVAL
    assert b"pr_window_push_dev" in lib.pr_last_error(None)
    assert lib.pr_window_push(None, buf, buf, buf, 0, buf, buf, C.byref(n), buf, buf) == _lib.PR_EINVAL
    assert b"pr_window_push" in lib.pr_last_error(None)
    lib.pr_window_destroy(None)                     # a no-op


def _ten_lines(pose_ids, point_ids):
    return window_model.cursor_cuts(list(pose_ids), list(point_ids))


def test_split_points_by_pose_is_the_cursor_rule():
    rng = np.random.default_rng(2)
    poses = np.arange(3, 60, 2)
    sorted_ids = np.sort(rng.integers(0, 58, 400))
    cases = [(poses, sorted_ids)]
    wait = sorted_ids.copy(); wait[30], wait[300] = wait[300], wait[30]          # an out-of-order id: the cursor waits behind it
    cases.append((poses, wait))
    cases.append((poses, np.concatenate([sorted_ids, [70, 71, 99]])))              # ids above the last pose: never delivered
    cases.append((poses, np.concatenate([[1000], sorted_ids])))                    # ... in front: nothing is ever delivered
    cases.append((poses[::-1].copy(), sorted_ids))                                 # descending pose ids: the cursor does not go back
    cases.append((poses, np.zeros(0, np.int64))); cases.append((np.zeros(0, np.int64), sorted_ids))
    cases.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
    for k in range(20):
        cases.append((np.sort(rng.integers(0, 50, 25)), rng.integers(0, 60, 200)))
    for pid, qid in cases:
        got = api.split_points_by_pose(pid, qid)
        want = _ten_lines(pid, qid)
        assert got.dtype == np.int64 and np.array_equal(got, want), (pid, qid)
        assert got[0] == 0 and np.all(np.diff(got) >= 0) and got[-1] <= len(qid)
    assert api.split_points_by_pose(poses, np.concatenate([[1000], sorted_ids]))[-1] == 0
    g = api.split_points_by_pose(poses, np.concatenate([sorted_ids, [70, 71, 99]]))
    assert g[-1] == len(sorted_ids)


@pytest.mark.parametrize("swap", [False, True])
def test_pushing_the_split_reproduces_the_file_loops_appends(golden_dir, tmp_path, swap):
    """The reference's loop appends points by its cursor; the window is pushed api.split_points_by_pose's slices.  With the oracle: the set
    that results from pushing the slices (window_model.replay: append, range test, prune - the reference's expressions) holds, at every
    emitting pose, every point of the oracle's cloud, and the cloud has one point per occupied voxel cell of that set."""
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    lines = [l for l in open(poses).read().split("\n") if l.strip()][:60]
    pf = str(tmp_path / "poses.txt"); open(pf, "w").write("\n".join(lines) + "\n")
    pts = str(tmp_path / "pts.txt")
    helpers.write_synthetic_points(pf, pts, per_pose=40)
    if swap:
        rows = open(pts).read().strip().split("\n")
        rows[50], rows[1500] = rows[1500], rows[50]
        open(pts, "w").write("\n".join(rows) + "\n")
    pid, w, qid, xyz, it = api.read_poses_points(pf, pts)
    cuts = api.split_points_by_pose(pid, qid)
    assert np.array_equal(cuts, _ten_lines(pid, qid))
    slices = [np.arange(cuts[p], cuts[p + 1]) for p in range(len(pid))]
    assert np.array_equal(np.concatenate(slices), np.arange(cuts[-1]))            # the splits concatenate to the consumed prefix
    assert cuts[-1] == len(qid) and (not swap or cuts[10] == 50)                    # (the swapped-in late id makes the cursor wait for its pose)
    ox, oi, oo, oid = oracle_lib.pts_preprocess(pf, pts, None, 45.0, False)
    steps = [s for s in window_model.replay(w, cuts, xyz, 45.0) if s["emit"]]
    assert len(steps) == len(oid) == 30
    for e, s in enumerate(steps):
        cloud = ox[oo[e]:oo[e + 1]]
        have = {r.tobytes() for r in s["cam"]}
        assert all(r.tobytes() in have for r in cloud), e
        cell = np.floor((s["cam"] + 45.0) * (1.0 / (45.0 / np.array([30.0, 60.0, 30.0])))).astype(np.int64)
        assert len(cloud) == len(np.unique(cell, axis=0)), e
    assert oo[-1] > 1000
