"""The resident keyframe map on the device (pr_map, map.hip): a drive pushed and appended keyframe by keyframe equals the
batch pre-stage's CSR set, the append rule equals its NumPy model (map_model.py) at the copy kernel's edges and through every kind of
overflow with guard words behind every buffer, a captured push + append replays, and verify_dev from the map returns the bytes of
verify_dev from concatenated tensors.  Everything is equality of bits except the pose errors of the online loop."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import icp_cases
import map_model
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import Matcher, _stream_context

pytestmark = pytest.mark.gpu

OVERFLOW, DROPPED = _lib.MAP_OVERFLOW, _lib.MAP_DROPPED
NAMES = api.KeyframeMap.NAMES


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(km):
    """the seven buffers of a map as host arrays (the caller has synchronised)"""
    return {n: getattr(km, n).cpu().numpy() for n in NAMES}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equals_model(km, model, what):
    got, want = host(km), model.arrays()
    for n in NAMES:
        assert same_bytes(got[n], want[n]), (what, n)


# ------------------------------------------------------------------------------------------------ the drive of test_gpu_window.py
@pytest.fixture(scope="module")
def seq07(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("seq07m")
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    pts = str(d / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
    short = str(d / "poses140.txt")
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    pid, w, qid, xyz, it = api.read_poses_points(short, pts)
    return dict(poses=short, pts=pts, pid=pid, w=w, xyz=xyz, it=it, cuts=api.split_points_by_pose(pid, qid))


def pose_inputs(drive, p):
    cuts = drive["cuts"]
    k = int(cuts[p + 1] - cuts[p])
    x = np.zeros((60, 3)); it = np.zeros(60, np.float32)
    x[:k] = drive["xyz"][cuts[p]:cuts[p + 1]]; it[:k] = drive["it"][cuts[p]:cuts[p + 1]]
    return drive["w"][p].reshape(12), x, it, k, int(drive["pid"][p])


KCAP, PCAP, MAXC = 112, 1 << 20, 9000


@pytest.fixture(scope="module")
def eager_map(seq07):
    """The 140 poses through push_torch -> append_push on one context (torch's current stream), the 30 warm-up pushes included: the host
    copy of the map and every append's info."""
    ctx = _stream_context(0)
    win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
    km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
    out = win.empty_out()
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    infos = []
    for p in range(len(seq07["pid"])):
        w, x, it, k, pid = pose_inputs(seq07, p)
        win.push_torch(dev(w), dev(x), dev(it, np.float32), torch.tensor([k], dtype=torch.int32, device="cuda"), out=out)
        km.append_push(out, pose=dev(w), id=torch.tensor([pid], dtype=torch.int32, device="cuda"), info=info)
        infos.append(info.cpu().numpy().copy())
    ctx.sync()
    res = dict(host=host(km), infos=np.array(infos), count=km.count())
    km.close(); win.close(); ctx.close()
    return res


# ------------------------------------------------------------------------------------------------ 1. drive = batch
def test_drive_equals_the_batch_prestage(seq07, eager_map):
    lib = _lib.load()
    ctx = api.Context(0)
    h = C.c_void_p()
    ctx.check(lib.pr_pts_preprocess_gpu(ctx.h, seq07["poses"].encode(), seq07["pts"].encode(), None, 45.0, 0, 0, C.byref(h)))
    try:
        N = int(lib.pr_clouds_count(h))
        T = int(np.ctypeslib.as_array(lib.pr_clouds_offs(h), (N + 1,))[-1])
        hip = C.CDLL("libamdhip64.so")

        def dev_array(ptr, shape, dtype):                  # a copy of library-owned device memory
            t = torch.empty(int(np.prod(shape)), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(t.numel() * t.element_size()), 3) == 0
            return t.reshape(shape).cpu().numpy()
        bx = dev_array(lib.pr_clouds_dev_xyz(h), (T, 3), torch.float64)
        bi = dev_array(lib.pr_clouds_dev_inten(h), (T,), torch.float32)
        bo = dev_array(lib.pr_clouds_dev_offs(h), (N + 1,), torch.int64)
        bf = dev_array(lib.pr_clouds_dev_frames(h), (N, 16), torch.float64)
    finally:
        lib.pr_clouds_free(h)
        ctx.close()
    m, infos = eager_map["host"], eager_map["infos"]
    assert N == 110 and eager_map["count"] == (110, T, 0) and list(m["state"]) == [110, 0, 0, 0] and 10000 < T <= PCAP
    assert same_bytes(m["offs"][:N + 1], bo) and same_bytes(m["xyz"][:T], bx) and same_bytes(m["inten"][:T], bi) and same_bytes(m["frames"][:N], bf)
    assert np.array_equal(m["ids"][:N], seq07["pid"][30:].astype(np.int32)) and same_bytes(m["poses"][:N], seq07["w"][30:].reshape(N, 12))
    assert not m["frames"][N:].any() and not m["offs"][N + 1:].any()             # the rows the map does not hold yet
    assert np.array_equal(infos[:30], np.tile([0, -1, 0, 0], (30, 1)))           # the warm-up pushes: switched off by emitted = info
    assert np.array_equal(infos[30:], np.stack([np.ones(N), np.arange(N), np.arange(N) + 1, np.zeros(N)], 1).astype(np.int32))


# ------------------------------------------------------------------------------------------------ 2. shapes
def clouds_of(sizes, seed, first=0):
    """CSR set of random clouds whose first point is `first` (the points in front are filler), with their frames"""
    rng = np.random.default_rng(seed)
    offs = first + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = rng.normal(0, 6, (int(offs[-1]), 3)); it = rng.random(int(offs[-1])).astype(np.float32)
    N = len(sizes)
    fr = api.cloud_frames(x, it, offs).reshape(N, 16)
    return x, it, offs, fr, rng.normal(0, 1, (N, 12)), rng.integers(0, 10000, N).astype(np.int32)


def append_both(km, model, c, emitted=None, max_points=None, what=None):
    x, it, offs, fr, po, ids = c
    e = None if emitted is None else torch.tensor([emitted], dtype=torch.int32, device="cuda")
    info = km.append_torch(dev(x), dev(it, np.float32), dev(offs, np.int64), dev(fr), poses=dev(po), ids=dev(ids, np.int32), emitted=e,
                           max_points=max_points)
    want = model.append(x, it, offs, fr, poses=po, ids=ids, emitted=None if emitted is None else [emitted], max_points=max_points)
    km.ctx.sync()
    got = info.cpu().numpy()
    assert list(got) == list(want), (what, got, want)
    assert_equals_model(km, model, what)
    return got


def test_shapes_at_the_copy_kernels_edges():
    ctx = _stream_context(0)
    km = api.KeyframeMap(ctx, 16, 4096, 600, max_append=5)
    model = map_model.MapModel(16, 4096, 600, max_append=5)
    for n in (0, 1, 2, 3, 255, 256, 257, 511, 512, 513):
        got = append_both(km, model, clouds_of([n], 100 + n), what=n)
        assert got[0] == 1 and got[3] == 0
    got = append_both(km, model, clouds_of([0, 257, 1, 0, 256], 7, first=7), what="N = 5")
    assert list(got) == [5, 10, 15, 0] and km.count() == (15, 2310 + 514, 0)
    before = host(km)
    got = append_both(km, model, clouds_of([40], 8), emitted=0, what="emitted = 0")
    assert list(got) == [0, -1, 15, 0]
    after = host(km)
    for n in NAMES:
        assert same_bytes(before[n], after[n]), n                      # no byte of any buffer changed (the frame of an empty cloud is NaN)
    x, it, offs, fr, po, ids = clouds_of([3, 3, 3, 3, 3, 3], 9)
    with pytest.raises(_lib.PRError, match="max_append"):
        km.append_torch(dev(x), dev(it, np.float32), dev(offs, np.int64), dev(fr))
    x, it, offs, fr, po, ids = clouds_of([77], 10, first=5)            # the host form, into the last row
    want = model.append(x, it, offs, fr, poses=po, ids=ids)
    assert list(km.append(x, it, offs, fr, poses=po, ids=ids)) == list(want) == [1, 15, 16, 0]
    assert_equals_model(km, model, "host form")
    x, it, offs, fr, po, ids = clouds_of([5], 11)                      # NULL poses / ids, no row left
    want = model.append(x, it, offs, fr)
    assert list(km.append(x, it, offs, fr)) == list(want) == [0, -1, 16, OVERFLOW]
    assert_equals_model(km, model, "full")
    km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. overflow
GUARD = -7


def guarded_map(ctx, kcap, pcap, maxc):
    """a map over buffers one row / 64 points longer than stated, the excess filled with a guard pattern"""
    shapes = dict(xyz=(pcap * 3, 64 * 3, torch.float64), inten=(pcap, 64, torch.float32), offs=(kcap + 1, 1, torch.int64),
                  frames=(kcap * 16, 16, torch.float64), poses=(kcap * 12, 12, torch.float64), ids=(kcap, 1, torch.int32), state=(4, 4, torch.int32))
    big, bufs = {}, {}
    for n, (used, extra, dt) in shapes.items():
        big[n] = torch.zeros(used + extra, dtype=dt, device="cuda")
        big[n][used:] = GUARD
        bufs[n] = big[n][:used]
    bufs["xyz"] = bufs["xyz"].view(pcap, 3); bufs["frames"] = bufs["frames"].view(kcap, 16); bufs["poses"] = bufs["poses"].view(kcap, 12)
    km = api.KeyframeMap(ctx, kcap, pcap, maxc, buffers=bufs)

    def intact():
        for n, (used, extra, dt) in shapes.items():
            assert bool((big[n][used:] == GUARD).all()), n
    return km, intact


# per map: (sizes of the single-cloud appends, max_points of each or None, expected flags in info[3], expected clouds appended)
SEQUENCES = {
    "a cloud of 301 points": ([301, 10], [None, None], [OVERFLOW | DROPPED, OVERFLOW], [1, 1]),
    "beyond the call's max_points": ([200, 200], [100, 200], [OVERFLOW | DROPPED, OVERFLOW], [1, 1]),
    "does not fit point_capacity": ([300, 300, 1], [None, None, None], [0, 0, OVERFLOW | DROPPED], [1, 1, 1]),
    "a fourth keyframe": ([10, 10, 10, 10], [None] * 4, [0, 0, 0, OVERFLOW], [1, 1, 1, 0]),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_overflow_flags_dropped_rows_and_guards(name):
    sizes, mps, flags, napp = SEQUENCES[name]
    ctx = _stream_context(0)
    km, intact = guarded_map(ctx, 3, 600, 300)
    model = map_model.MapModel(3, 600, 300)
    sets = [clouds_of([n], 40 + j) for j, n in enumerate(sizes)]
    for j, c in enumerate(sets):
        got = append_both(km, model, c, max_points=mps[j], what=(name, j))
        assert got[3] == flags[j] and got[0] == napp[j], (name, j, got)
        intact()
        if flags[j] & DROPPED:                                         # the row is there, empty, under a zero frame, with its pose and id
            r = int(got[1])
            m = host(km)
            assert m["offs"][r + 1] == m["offs"][r] and not m["frames"][r].any()
            assert same_bytes(m["poses"][r], c[4][0]) and m["ids"][r] == c[5][0]
    assert km.count()[2] == OVERFLOW
    km.reset(); model.reset()
    ctx.sync()
    m = host(km)
    assert not m["state"].any() and not m["offs"].any() and not m["frames"].any() and km.count() == (0, 0, 0)
    got = append_both(km, model, clouds_of([20], 60), what=(name, "after reset"))
    assert list(got) == [1, 0, 1, 0]
    intact()
    km.close()
    big = api.KeyframeMap(ctx, 8, 4096, 600)                           # the same appends succeed on a larger map
    bmodel = map_model.MapModel(8, 4096, 600)
    for j, c in enumerate(sets):
        got = append_both(big, bmodel, c, max_points=None if mps[j] is None else sizes[j], what=(name, "large", j))
        assert list(got) == [1, j, j + 1, 0]
    assert big.count() == (len(sizes), sum(sizes), 0)
    big.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. capture
def test_captured_push_and_append_replays(seq07, eager_map):
    P = 60
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
        it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda"); info = torch.zeros(4, dtype=torch.int32, device="cuda")

        def load(p):
            w, hx, hit, k, pid = pose_inputs(seq07, p)
            pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit))
            n.fill_(k); kid.fill_(pid)

        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        out = win.empty_out()
        load(0)
        win.push_torch(pose, x, it, n, out=out)                        # one eager push + append, then the capture of the pair
        km.append_push(out, pose=pose, id=kid, info=info)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            win.push_torch(pose, x, it, n, out=out)
            km.append_push(out, pose=pose, id=kid, info=info)
        for p in range(1, P):
            load(p)
            g.replay()
            st.synchronize()
            assert list(info.cpu().numpy()) == ([0, -1, 0, 0] if p < 30 else [1, p - 30, p - 29, 0]), p
        got, want = host(km), eager_map["host"]
        K = P - 30
        T = int(want["offs"][K])
        assert km.count() == (K, T, 0) and T > 1000
        assert same_bytes(got["offs"][:K + 1], want["offs"][:K + 1]) and same_bytes(got["xyz"][:T], want["xyz"][:T])
        assert same_bytes(got["inten"][:T], want["inten"][:T]) and same_bytes(got["frames"][:K], want["frames"][:K])
        assert same_bytes(got["poses"][:K], want["poses"][:K]) and same_bytes(got["ids"][:K], want["ids"][:K])
        assert not got["frames"][K:].any() and not got["offs"][K + 1:].any()
        del g
        km.close(); win.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. verify from the map = from tensors
def stats_host(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), api.ICP_STATS)


def test_verify_from_the_map_equals_verify_from_tensors():
    names = list(icp_cases.CASES)
    cs = [icp_cases.case(n) for n in names]
    n = len(cs)
    rng = np.random.default_rng(5)
    xq, oq = icp_cases.csr([c["P"] for c in cs]); xd, od = icp_cases.csr([c["Q"] for c in cs])
    iq, idn = rng.random(len(xq)).astype(np.float32), rng.random(len(xd)).astype(np.float32)
    sig_q, sig_d = api.sc_generate(xq, iq, oq), api.sc_generate(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    mt = Matcher("sc", n, n, ctx=api.Context(0, exact_statistics=True))
    mt.pack_database(dev(sig_d))
    mt.match(dev(sig_q), 0, 2.0, 1)
    MAXD = 2048
    ms = max(len(c["P"]) for c in cs)
    assert max(len(c["Q"]) for c in cs) <= MAXD
    km = api.KeyframeMap(mt.ctx, 8, len(xd) + 100, MAXD)
    parts = [(dev(xd[od[i]:od[i + 1]]), dev(idn[od[i]:od[i + 1]], np.float32), dev([0, od[i + 1] - od[i]], np.int64), dev(fd[i:i + 1]))
             for i in range(n)]
    cq, cd, dfq, dfd = (dev(xq), dev(oq, np.int64)), (dev(xd), dev(od, np.int64)), dev(fq), dev(fd)
    idx = dev(np.stack([np.arange(n), (np.arange(n) + 1) % n, np.full(n, -1), 6 + np.arange(n) % 2], 1), np.int32)
    torch.cuda.synchronize()                                           # the uploads (torch's stream) before the context's stream reads them
    for x, it, o, f in parts:                                          # the DB clouds one at a time
        km.append_torch(x, it, o, f)
    mt.ctx.sync()
    assert km.count() == (n, len(xd), 0)
    assert same_bytes(km.xyz[:len(xd)].cpu().numpy(), xd) and same_bytes(km.offs[:n + 1].cpu().numpy(), od) and same_bytes(km.frames[:n].cpu().numpy(), fd)
    kw = dict(max_corr=1.0, min_fitness=0.6, max_rmse=0.3, **{k: v for k, v in icp_cases.PARAMS.items() if k != "max_corr"})
    for H, search in ((1, None), (2, None), (1, "grid")):
        want = mt.verify_dev(idx, cq, cd, dfq, dfd, ms, MAXD, hypotheses=H, search=search, **kw)
        got = km.verify_dev(mt, idx, cq, dfq, ms, hypotheses=H, search=search, **kw)
        fwd = mt.verify_dev(idx, cq, km, dfq, None, ms, None, hypotheses=H, search=search, **kw)
        torch.cuda.synchronize()
        for a, b, c in zip(want, got, fwd):
            assert same_bytes(a.cpu().numpy(), b.cpu().numpy()) and same_bytes(a.cpu().numpy(), c.cpu().numpy()), (H, search)
        s = stats_host(got[1]).reshape(n, 4); acc = got[2].cpu().numpy()
        assert (s["status"][:, 2:] == _lib.ICP_NO_PAIR).all() and not acc[:, 2:].any()      # the -1 slot and the row >= keyframes
        assert (s["status"][:, 0] != _lib.ICP_NO_PAIR).all()
        print("   H", H, "search", search, "accepted:", acc.astype(int).tolist())
    with pytest.raises(ValueError):
        mt.verify_dev(idx, cq, km, dfq, dfd, ms, None, **kw)
    km.close(); mt.close()


# ------------------------------------------------------------------------------------------------ 6. the online loop
def test_online_loop_append_match_verify_on_a_generated_drive():
    """For each place of pose_drive.drive() in turn: its DB cloud into the map, its M2DP row into the growing database, then the query
    of that place is matched (k = 1) and verified from the map with the thresholds test_gpu_pose.py uses on this drive (min_fitness 0.6,
    max_rmse 0.3, max_corr 1.0).  From a database of 3 rows on, every query must be accepted with a pose error under 0.2 degrees and
    0.05 m.  The z-score fusion of a database of 3 - 5 rows need not rank the true row first (its row statistics are those of 3 - 5
    numbers): where it does not, idx = i is verified directly for that step - the thresholds are the same; with all 6 rows the top-1 must
    be the true row, as in test_m2dp_and_delight_match_verify_dev_on_a_generated_drive."""
    import pose_drive
    qs, ds, iq, idn, Rs, ts = pose_drive.drive()
    c = len(qs)
    xq, oq = icp_cases.csr(qs); xd, od = icp_cases.csr(ds)
    sig_q, sig_d = api.m2dp_generate(xq, iq, oq), api.m2dp_generate(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    ctx = _stream_context(0, exact_statistics=True)
    mt = Matcher("m2dp", 1, c, ctx=ctx)
    mt.reserve_database()
    maxc = max(len(d) for d in ds); ms = max(len(q) for q in qs)
    km = api.KeyframeMap(ctx, 8, len(xd), maxc)
    dsq, dsd, dfq = dev(sig_q), dev(sig_d), dev(fq)
    ranked = []
    for i in range(c):
        info = km.append_torch(dev(ds[i]), dev(idn[od[i]:od[i + 1]], np.float32), dev([0, len(ds[i])], np.int64), dev(fd[i:i + 1]),
                               ids=torch.tensor([i], dtype=torch.int32, device="cuda"))
        mt.append_database(dsd[4 * i:4 * i + 4])
        if mt.n < 3:
            continue
        idx, _ = mt.match(dsq[4 * i:4 * i + 4].contiguous(), 0, 2.0, 1)
        top = int(idx[0, 0])
        ranked.append(top == i)
        if top != i:
            assert mt.n < c, (i, top)
            idx = torch.tensor([[i]], dtype=torch.int32, device="cuda")
        T, stats, acc, hyp = mt.verify_dev(idx, (dev(qs[i]), dev([0, len(qs[i])], np.int64)), km, dfq[i:i + 1].contiguous(), None, ms, None,
                                           max_corr=1.0, min_fitness=0.6, max_rmse=0.3)
        torch.cuda.synchronize()
        assert list(info.cpu().numpy()) == [1, i, i + 1, 0]
        st = stats_host(stats)[0]
        er, et = icp_cases.pose_error(T[0, 0].cpu().numpy(), Rs[i], ts[i])
        print("  place", i, "db rows", mt.n, "top-1", top, "status", st["status"], "iters", st["iters"],
              "fitness %.3f rmse %.3f err %.3f deg %.3f m" % (st["fitness"], st["rmse"], er, et))
        assert bool(acc[0, 0]) and er < 0.2 and et < 0.05, i
    assert len(ranked) == c - 2 and ranked[-1]
    assert km.count() == (c, len(xd), 0) and list(km.ids[:c].cpu().numpy()) == list(range(c))
    km.close(); mt.close(); ctx.close()
