"""The resident point window on the device (pr_window, window.hip): a drive replayed keyframe by keyframe equals the batch
pre-stage bit for bit - points, ORDER, frame, float intensity average - through resets, short ranges, unsorted ids, the shapes at which the
kernels take another path, overflow, graph capture, and on into the generators and one online match / append step.
Everything here is equality of bits; the yardsticks are the host pre-stage (pinned to the oracle by test_prestage.py) and pr_cloud_frames_dev."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers
import window_model
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import Matcher, _stream_context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERFLOW, ORDER_GLOBAL = _lib.WINDOW_OVERFLOW, _lib.WINDOW_ORDER_GLOBAL


def same(a, b):
    return (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
            and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


@pytest.fixture(scope="module")
def seq07(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("seq07w")
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    pts = str(d / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
    short = str(d / "poses140.txt")                                # the 140 poses the points were made for (the drive of cases 4 - 7)
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    return poses, pts, d, short


@pytest.fixture(scope="module")
def drive(seq07):
    """the first 140 poses of the case-1 files as arrays, cut into pushes"""
    poses, pts, d, short = seq07
    pid, w, qid, xyz, it = api.read_poses_points(short, pts)
    return dict(pid=pid, w=w, xyz=xyz, it=it, cuts=api.split_points_by_pose(pid, qid))


# ------------------------------------------------------------------------------------------------ 1. replay == host form
@pytest.mark.parametrize("polar", [False, True])
def test_replay_equals_the_host_form(seq07, polar):
    poses, pts, d, _ = seq07
    idh = str(d / f"ids_h_{polar}.txt"); ids_ = str(d / f"ids_s_{polar}.txt")
    h = api.pts_preprocess(poses, pts, idh, 45.0, polar)
    s = api._pts_preprocess_stream(poses, pts, ids_, 45.0, polar, api.default_context(), return_frames=True)
    g = api.pts_preprocess(poses, pts, ids_, 45.0, polar, gpu="stream")
    assert len(h[3]) == 693 and h[2][-1] > 10000                   # (the whole pose file: 723 poses, points for the first 140)
    assert same(s[:4], h) and same(g, h)
    assert open(ids_, "rb").read() == open(idh, "rb").read()
    fr = api.cloud_frames(h[0], h[1], h[2])                      # pr_cloud_frames_dev over every push's cloud: moments pass + average chain
    assert fr.shape == s[4].shape and np.array_equal(fr.view(np.uint64), s[4].view(np.uint64))
    assert np.all(s[4][:, 15] == 1.0) and np.array_equal(s[4][:, 13], np.diff(h[2]).astype(np.float64))


# ------------------------------------------------------------------------------------------------ 2. resets, ranges, cursor
def test_resets_ranges_cursor_and_empty_inputs(golden_dir, tmp_path):
    full = open(os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")).read().split("\n")
    lines = [l for l in full[:90] if l.strip()]
    second = []
    for k, l in enumerate(lines[:70]):                             # same trajectory again with later ids: |t| < 1 -> reset
        t = l.split(); t[0] = str(int(lines[-1].split()[0]) + 1 + k); second.append(" ".join(t) + " ")
    poses = str(tmp_path / "poses.txt"); open(poses, "w").write("\n".join(lines + second) + "\n")
    pts = str(tmp_path / "pts.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=50)
    rows = open(pts).read().strip().split("\n")
    rows[100], rows[4000] = rows[4000], rows[100]                  # an out-of-order id: the cursor waits behind it
    open(pts, "w").write("\n".join(rows) + "\n")
    for polar, rng_ in ((False, 45.0), (True, 45.0), (False, 20.0), (True, 12.5)):
        h = api.pts_preprocess(poses, pts, None, rng_, polar)
        g = api.pts_preprocess(poses, pts, None, rng_, polar, gpu="stream")
        assert len(h[3]) == 100 and same(g, h), (polar, rng_)
    empty = str(tmp_path / "empty.txt"); open(empty, "w").write("")
    g = api.pts_preprocess(poses, empty, None, 45.0, False, gpu="stream")
    h = api.pts_preprocess(poses, empty, None, 45.0, False)
    assert same(g, h) and g[0].shape == (0, 3) and len(g[3]) == 100
    g = api.pts_preprocess(empty, empty, None, 45.0, True, gpu="stream")
    assert len(g[3]) == 0 and list(g[2]) == [0] and g[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 3. shapes
T2 = [1, 0, 0, 2, 0, 1, 0, 0, 0, 0, 1, 0]          # identity rotation, camera = world + (2, 0, 0): |t| >= 1, no reset


def T(tx):
    w = list(T2); w[3] = tx
    return w


def hand_made(tmp_path, name, pushes, lidar_range=45.0, polars=(False, True)):
    """30 empty warm-up poses, then `pushes` = [(w2c [12], xyz [n, 3], inten [n])]: written to files with 17 significant digits (the
    parser is strtod: every bit survives), the host form against the window.  Returns {polar: host result}."""
    P = [(T2, np.zeros((0, 3)), np.zeros(0, np.float32))] * 30 + list(pushes)
    pf, qf = str(tmp_path / f"{name}_poses.txt"), str(tmp_path / f"{name}_pts.txt")
    with open(pf, "w") as f:
        for i, (w, _, _) in enumerate(P):
            f.write("%d " % (i + 1) + "".join("%.17g " % v for v in w) + "\n")
    with open(qf, "w") as f:
        for i, (_, x, it) in enumerate(P):
            for r, v in zip(np.asarray(x, np.float64).reshape(-1, 3), np.asarray(it, np.float32).reshape(-1)):
                f.write("%d %.17g %.17g %.17g %.9g\n" % (i + 1, r[0], r[1], r[2], v))
    out = {}
    for polar in polars:
        h = api.pts_preprocess(pf, qf, None, lidar_range, polar)
        g = api.pts_preprocess(pf, qf, None, lidar_range, polar, gpu="stream")
        assert len(h[3]) == len(pushes) and same(g, h), (name, polar)
        out[polar] = h
    return out


def own_cells(K, seed=0):
    """K points, each in a voxel cell of its own (cells of 1.5 x 0.75 x 1.5 m at range 45), camera frame, well inside the range"""
    rng = np.random.default_rng(seed)
    ix, iy, iz = np.meshgrid(np.arange(61), np.arange(121), np.arange(61), indexing="ij")
    c = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1)
    centre = (c + 0.5) * np.array([1.5, 0.75, 1.5]) - 45.0
    centre = centre[np.linalg.norm(centre, axis=1) < 40.0]
    assert len(centre) >= K
    p = centre[rng.permutation(len(centre))[:K]] + rng.uniform(-0.2, 0.2, (K, 3))
    return p - np.array([2.0, 0, 0]), rng.uniform(0, 255, K).astype(np.float32)           # world points under T2


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_alive_counts_around_the_scan_blocks(tmp_path, n):
    x, it = own_cells(n, seed=n)
    r = hand_made(tmp_path, "alive", [(T2, x, it), (T2, np.zeros((0, 3)), np.zeros(0, np.float32))])     # (n_new = 0 on an emitting pose)
    assert list(r[False][2]) == [0, n, 2 * n]


def test_all_points_in_one_cell(tmp_path):
    rng = np.random.default_rng(3)
    x = np.array([10.2, 0.2, 10.2]) + rng.uniform(0, 0.1, (700, 3))
    r = hand_made(tmp_path, "one", [(T2, x, rng.uniform(0, 9, 700).astype(np.float32))], polars=(False,))
    assert list(r[False][2]) == [0, 1]


@pytest.mark.parametrize("K", [12, 13, 14, 29, 30, 59, 60, 61])
def test_every_point_in_its_own_cell_at_the_rehash_thresholds(tmp_path, K):
    x, it = own_cells(K, seed=K)
    r = hand_made(tmp_path, "own", [(T2, x, it)])
    assert list(r[False][2]) == [0, K]


def lds_limit():
    src = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "kernels.hpp")).read()
    return int(re.search(r"WIN_ORDER_LDS_INTS\s*=\s*(\d+)", src).group(1))


def test_order_scratch_in_lds_and_in_global_memory(tmp_path):
    """The order kernel keeps next[K] + bkt[bucket count] in LDS while K + bucket count <= WIN_ORDER_LDS_INTS.  libstdc++ keeps the load
    factor <= 1 (bucket count >= K), so K = limit / 2 + 1 cannot fit and runs the global-scratch path; K = 61 fits.  info[3] says which."""
    L = lds_limit()
    assert L * 4 <= 160 * 1024
    K = L // 2 + 1
    x, it = own_cells(K, seed=5)
    r = hand_made(tmp_path, "big", [(T2, x, it)], polars=(False,))
    assert list(r[False][2]) == [0, K]
    ctx = api.default_context()
    for k, want in ((61, 0), (K, ORDER_GLOBAL)):
        win = api.CloudWindow(ctx, 45.0, False, K, K, K)
        for _ in range(30):
            win.push(T2, np.zeros((0, 3)), np.zeros(0, np.float32))
        ox, oi, fr, info = win.push(T2, x[:k], it[:k])
        assert info[0] == 1 and info[1] == k and (info[3] & ORDER_GLOBAL) == want and not (info[3] & OVERFLOW)
        assert np.array_equal(ox.view(np.uint64), r[False][0][:k].view(np.uint64)) or k != K
        win.close()


def test_exact_ties_go_to_the_earlier_point(tmp_path):
    x, _ = own_cells(40, seed=7)
    x3 = np.concatenate([x, x, x[::-1]])                           # every cell three times, identical coordinates
    it = np.arange(120, dtype=np.float32)
    r = hand_made(tmp_path, "ties", [(T2, x3, it)])
    for polar in (False, True):
        assert r[polar][2][-1] == 40 and sorted(r[polar][1]) == list(range(40))    # the first copy's intensity survives


def test_range_edge_and_no_return(tmp_path):
    inside = np.nextafter(43.0, 0.0)
    x = np.array([[43.0, 0, 0], [inside, 0, 0], [0, 43.0, 0], [1.0, 2.0, 3.0]])     # camera (45, 0, 0): |p| == range is out (strict)
    it = np.array([1, 2, 3, 4], np.float32)
    r = hand_made(tmp_path, "edge", [(T2, x, it)], polars=(False,))
    assert sorted(r[False][1]) == [2.0, 3.0, 4.0]
    # camera x = 44 (in), 46 (out: leaves for good), 44 again two poses later: must stay gone
    x = np.array([[42.0, 0, 0], [5.0, 1.0, 1.0]]); it = np.array([1, 2], np.float32)
    none = (np.zeros((0, 3)), np.zeros(0, np.float32))
    r = hand_made(tmp_path, "gone", [(T(2.0), x, it), (T(4.0),) + none, (T(3.0),) + none, (T(2.0),) + none])
    for polar in (False, True):
        assert list(np.diff(r[polar][2])) == [2, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ 4. overflow
def test_overflow_flag(drive):
    ctx = api.default_context()
    steps = window_model.replay(drive["w"], drive["cuts"], drive["xyz"], 45.0)
    need = np.array([s["need"] for s in steps])
    cap = int(need.max()) - 1                                      # one short of what the drive needs
    first = int(np.argmax(need > cap))
    assert first > 40 and steps[first]["emit"]
    win = api.CloudWindow(ctx, 45.0, False, cap, 60, cap)
    cuts = drive["cuts"]
    try:
        for p in range(first + 4):
            ox, oi, fr, info = win.push(drive["w"][p], drive["xyz"][cuts[p]:cuts[p + 1]], drive["it"][cuts[p]:cuts[p + 1]])
            assert bool(info[3] & OVERFLOW) == (p >= first), p      # set on exactly the predicted push, and it stays
            if p < first:
                assert info[2] == steps[p]["alive"]
        assert win.count() <= cap
        ox, oi, fr, info = win.push(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.5]), np.zeros((0, 3)), np.zeros(0, np.float32))   # |t| < 1
        assert info[0] == 0 and info[2] == 0 and not (info[3] & OVERFLOW) and win.count() == 0
    finally:
        win.close()


def test_nothing_is_written_past_max_out_points(drive):
    max_out, G = 7, 16
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        win = api.CloudWindow(ctx, 45.0, True, 4000, 60, max_out)
        full = api.CloudWindow(ctx, 45.0, True, 4000, 60, 4000)
        big = dict(xyz=torch.full(((max_out + G) * 3,), -7.0, dtype=torch.float64, device="cuda"),
                   inten=torch.full((max_out + G,), -7.0, dtype=torch.float32, device="cuda"),
                   offs=torch.full((2 + G,), -7, dtype=torch.int64, device="cuda"), frame=torch.full((16 + G,), -7.0, dtype=torch.float64, device="cuda"),
                   info=torch.full((4 + G,), -7, dtype=torch.int32, device="cuda"))
        out = dict(xyz=big["xyz"][:max_out * 3].view(max_out, 3), inten=big["inten"][:max_out], offs=big["offs"][:2], frame=big["frame"][:16],
                   info=big["info"][:4])
        cuts = drive["cuts"]
        for p in range(33):
            x = torch.from_numpy(np.ascontiguousarray(np.resize(drive["xyz"][cuts[p]:cuts[p + 1]], (60, 3)))).cuda()
            it = torch.from_numpy(np.ascontiguousarray(np.resize(drive["it"][cuts[p]:cuts[p + 1]], 60))).cuda()
            w = torch.from_numpy(drive["w"][p].copy()).cuda()
            n = torch.tensor([cuts[p + 1] - cuts[p]], dtype=torch.int32, device="cuda")
            win.push_torch(w, x, it, n, out=out)
            ref = full.push_torch(w, x, it, n)
            st.synchronize()
            info, rinfo = out["info"].cpu().numpy(), ref["info"].cpu().numpy()
            assert info[0] == rinfo[0] == int(p >= 30) and info[2] == rinfo[2]
            if p >= 30:
                assert rinfo[1] > 100 and info[1] == max_out and (info[3] & OVERFLOW) and not (rinfo[3] & OVERFLOW)
                assert list(out["offs"].cpu().numpy()) == [0, max_out]
                assert torch.equal(out["xyz"], ref["xyz"][:max_out]) and torch.equal(out["inten"], ref["inten"][:max_out])
            for k, used in (("xyz", max_out * 3), ("inten", max_out), ("offs", 2), ("frame", 16), ("info", 4)):
                assert bool((big[k][used:] == -7).all()), (p, k)    # the guard words behind every buffer
        win.close(); full.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. capture
def test_capture_and_replay(drive):
    P, cuts = 60, drive["cuts"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
        it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")

        def load(p):
            k = int(cuts[p + 1] - cuts[p])
            pose.copy_(torch.from_numpy(drive["w"][p].copy()))
            x[:k].copy_(torch.from_numpy(drive["xyz"][cuts[p]:cuts[p + 1]].copy())); it[:k].copy_(torch.from_numpy(drive["it"][cuts[p]:cuts[p + 1]].copy()))
            n.fill_(k)

        def take(out):
            st.synchronize()
            info = out["info"].cpu().numpy().copy()
            k = int(info[1])
            return (info.tobytes(), out["offs"].cpu().numpy().tobytes(), out["xyz"][:k].cpu().numpy().tobytes(),
                    out["inten"][:k].cpu().numpy().tobytes(), out["frame"].cpu().numpy().tobytes())

        eager_win = api.CloudWindow(ctx, 45.0, False, 4000, 60, 4000)
        eager = []
        for p in range(P):
            load(p)
            eager.append(take(eager_win.push_torch(pose, x, it, n)))
        eager_win.close()
        assert sum(np.frombuffer(e[0], np.int32)[0] for e in eager) == 30 and np.frombuffer(eager[-1][0], np.int32)[1] > 500

        win = api.CloudWindow(ctx, 45.0, False, 4000, 60, 4000)
        out = win.empty_out()
        load(0)
        win.push_torch(pose, x, it, n, out=out)                    # one eager push, then the capture
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            win.push_torch(pose, x, it, n, out=out)
        for p in range(1, P):
            load(p)
            g.replay()
            assert take(out) == eager[p], p
        runs = []
        for _ in range(2):                                          # the whole drive twice through the graph
            win.reset()
            runs.append([])
            for p in range(P):
                load(p)
                g.replay()
                runs[-1].append(take(out))
        assert runs[0] == runs[1] and runs[0] == eager
        del g
        win.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. into the generators
def _batch_rows(ctx, lib, poses, pts, polar, type_, rows, cols):
    h = C.c_void_p()
    ctx.check(lib.pr_pts_preprocess_gpu(ctx.h, poses.encode(), pts.encode(), None, 45.0, int(polar), 0, C.byref(h)))
    try:
        N = lib.pr_clouds_count(h)
        got = np.empty((rows * N, cols))
        ctx.check(lib.pr_generate_clouds(ctx.h, type_, h, 45.0, got.ctypes.data))
    finally:
        lib.pr_clouds_free(h)
    return got.reshape(N, rows, cols)


def _push_all(ctx, drive, polar, each):
    """the drive through push_torch on ctx's stream (= torch's current one); each(e, out) after every emitting push"""
    cuts = drive["cuts"]
    win = api.CloudWindow(ctx, 45.0, polar, 9000, 60, 9000)
    out = win.empty_out()
    e = 0
    for p in range(len(drive["pid"])):
        k = int(cuts[p + 1] - cuts[p])
        x = torch.zeros((60, 3), dtype=torch.float64, device="cuda"); it = torch.zeros(60, dtype=torch.float32, device="cuda")
        x[:k] = torch.from_numpy(drive["xyz"][cuts[p]:cuts[p + 1]].copy()).cuda(); it[:k] = torch.from_numpy(drive["it"][cuts[p]:cuts[p + 1]].copy()).cuda()
        win.push_torch(torch.from_numpy(drive["w"][p].copy()).cuda(), x, it, torch.tensor([k], dtype=torch.int32, device="cuda"), out=out)
        if p >= 30:                                                # (no reset in this drive: every pose from the 31st on emits)
            each(e, out)
            e += 1
    win.close()
    return e


@pytest.mark.parametrize("type_", ["sc", "m2dp", "delight"])
def test_a_push_feeds_the_generators(seq07, drive, type_):
    _, pts, d, poses = seq07
    lib = _lib.load()
    tid, rows, cols, polar = {"sc": (0, 1, 2400, False), "m2dp": (1, 4, 384, True), "delight": (2, 16, 256, True)}[type_]
    ctx = _stream_context(0)
    want = _batch_rows(ctx, lib, poses, pts, polar, tid, rows, cols)
    sig = torch.empty((rows, cols), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    seen = []

    def each(e, out):
        if e not in (0, 37, 109):
            return
        if type_ == "delight":
            ctx.check(lib.pr_delight_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, p(out["frame"]), p(sig)))
        else:
            fn = lib.pr_sc_generate_frames_dev if type_ == "sc" else lib.pr_m2dp_generate_frames_dev
            ctx.check(fn(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig)))
        ctx.sync()
        assert np.array_equal(sig.cpu().numpy().view(np.uint64), want[e].view(np.uint64)), (type_, e)
        seen.append(e)

    assert _push_all(ctx, drive, polar, each) == len(want) == 110 and seen == [0, 37, 109]
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. one online step, end to end
def test_online_chain_push_generate_match_append(seq07, drive):
    """push -> SC row -> Matcher.match(1) -> append_database over the drive, against the same causal loop over the batch-generated rows."""
    _, pts, d, poses = seq07
    lib = _lib.load()
    ctx = _stream_context(0)
    batch = _batch_rows(ctx, lib, poses, pts, False, 0, 1, 2400)[:, 0, :]
    N = len(batch)
    p = lambda t: C.c_void_p(t.data_ptr())

    def online(row_of):
        mt = Matcher("sc", 1, N, ctx=ctx)
        mt.reserve_database()
        res = []

        def step(e, out):
            row = row_of(e, out)
            if mt.n >= 3:
                idx, sc = mt.match(row, 0, 2.0, 1)
                res.append((idx.cpu().numpy().copy(), sc.cpu().numpy().copy()))
            mt.append_database(row)
        return mt, res, step

    rows_dev = torch.from_numpy(batch).cuda()
    mt, want, step = online(lambda e, out: rows_dev[e:e + 1].clone())
    for e in range(N):
        step(e, None)
    mt.close()

    sig = torch.empty((1, 2400), dtype=torch.float64, device="cuda")

    def from_push(e, out):
        ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig)))
        return sig.clone()

    mt, got, step = online(from_push)
    assert _push_all(ctx, drive, False, step) == N
    mt.close()
    assert len(got) == len(want) == N - 3
    for (gi, gs), (wi, ws) in zip(got, want):
        assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint64), ws.view(np.uint64))
    assert len({int(i[0, 0]) for i, _ in got}) > 5
    ctx.close()
