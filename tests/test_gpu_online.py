"""The online signature database on the device (pr_online, online.hip): a match against the rows held so far equals the
NumPy model over the oracle (online_model.py) at the kernels' edges and through the reference's corner rules, the append rule equals the
model with guard words behind both buffers, ONE captured step serves a growing database, the result agrees with the existing matcher,
and the whole online step - push, generate, match, append, map append, align, verify - replays as one graph with the bytes of the eager
calls.  Tolerances: idx equal, score 1e-9 (exact statistics), rows 1e-12 (oracle against device fp64)."""
import os

import numpy as np
import pytest
import torch

import helpers
import online_cases
import online_model
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import Matcher, _stream_context

pytestmark = pytest.mark.gpu

OVERFLOW = _lib.ONLINE_OVERFLOW
SCORE_TOL, ROWS_TOL = 1e-9, 1e-12


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def close(got, want, tol):
    """NaN and Inf equal as such, everything else within tol"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    inf = np.isinf(want)
    if not np.array_equal(np.isinf(got), inf) or not np.array_equal(got[inf], want[inf]):
        return False
    fin = np.isfinite(want)
    return bool((np.abs(got[fin] - want[fin]) <= tol).all())


def assert_match(got_idx, got_score, want_idx, want_score, what):
    gi, gs = got_idx.cpu().numpy(), got_score.cpu().numpy()
    print("  ", what, "idx", gi[0].tolist(), "max |score - model|",
          float(np.nanmax(np.abs(np.where(np.isfinite(want_score), gs - want_score, 0.0)), initial=0.0)))
    assert gi.shape == want_idx.shape and np.array_equal(gi, want_idx), (what, gi, want_idx)
    assert close(gs, want_score, SCORE_TOL), (what, gs, want_score)


def grow(odb, rows_dev, upto):
    """appends rows [count, upto) of rows_dev; the caller tracks the count"""
    rps = odb.rows_per_sig
    for j in range(upto[0], upto[1]):
        odb.append_torch(rows_dev[j * rps:(j + 1) * rps])


# ------------------------------------------------------------------------------------------------ 1. the kernels' edges
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_match_at_the_kernels_edges(type_):
    c = online_cases.edge_case(type_)
    ctx = _stream_context(0)
    cap = online_cases.NMAX + 60                           # a capacity that is no multiple of anything; NB = ONLINE_NB
    odb = api.OnlineDatabase(ctx, type_, cap, max_k=online_cases.MAX_K)
    db, q = dev(c["db"]), dev(c["q"])
    rows = torch.full((2, cap), -5.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in online_cases.COUNTS:
        grow(odb, db, (have, n))
        have = n
        for k, w in online_cases.KM:
            rows.fill_(-5.0)
            idx, score = odb.match_torch(q, w, 2.0, k, rows=rows)
            ctx.sync()
            wi, ws = online_model.match_rows(c["dp"][:n], c["di"][:n], w, 2.0, k)
            assert_match(idx, score, wi, ws, (type_, n, k, w))
            r = rows.cpu().numpy()
            assert close(r[0, :n], c["dp"][:n], ROWS_TOL) and close(r[1, :n], c["di"][:n], ROWS_TOL), (type_, n)
            assert (r[:, n:] == -5.0).all(), (type_, n)                        # nothing behind the count
        assert odb.count() == (n, 0)
    with pytest.raises(_lib.PRError, match="max_k"):
        odb.match_torch(q, 0, 2.0, online_cases.MAX_K + 1)
    odb.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the reference's corner rules
def test_reference_corner_rules():
    c = online_cases.corner_case()
    ctx = _stream_context(0)
    odb = api.OnlineDatabase(ctx, "sc", 64, max_k=8)
    db = dev(c["db"])
    rows = torch.zeros((2, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in online_cases.CORNER_COUNTS:
        grow(odb, db, (have, n))
        have = n
        for name in ("q", "zero"):
            hq = c[name]
            dp, di = online_model.distances("sc", hq, c["db"][:n])
            for k, w in online_cases.CORNER_KM:
                for pw in online_cases.CORNER_WEIGHTS:
                    idx, score = odb.match_torch(dev(hq), w, pw, k, rows=rows)
                    ctx.sync()
                    wi, ws = online_model.match_rows(dp, di, w, pw, k)
                    assert_match(idx, score, wi, ws, (name, n, k, w, pw))
                    gi = idx.cpu().numpy()[0]
                    if w == 0:
                        assert c["zero_row"] not in gi                         # a NaN distance is never selected
                    if name == "zero":                                         # a zero-norm query: every distance is NaN, so only
                        assert (gi[gi >= 0] > n - w).all()                     # the mask's +Inf rows are left (none without a mask)
            r = rows.cpu().numpy()
            assert close(r[0, :n], dp, ROWS_TOL) and close(r[1, :n], di, ROWS_TOL)
            assert np.isnan(r[:, c["zero_row"]]).all()
            for a, b in c["copies"]:
                if b < n:                                                      # exact copies: identical bits in both channels
                    assert same_bytes(r[:, a], r[:, b]), (a, b)
    idx, _ = odb.match_torch(dev(c["q"]), 0, 2.0, 2)
    ctx.sync()
    assert idx.cpu().numpy()[0].tolist() == [7, 20]                            # the tie of the copies goes to the lower index
    odb.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. append
GUARD = -7


def guarded(ctx, type_, cap):
    """a database over buffers one signature / four words longer than stated, the excess filled with a guard pattern"""
    rps, L = online_model.SHAPES[type_]
    big = dict(sig=torch.zeros(((cap + 1) * rps, L), dtype=torch.float64, device="cuda"), state=torch.zeros(8, dtype=torch.int32, device="cuda"))
    big["sig"][cap * rps:] = GUARD
    big["state"][4:] = GUARD
    odb = api.OnlineDatabase(ctx, type_, cap, buffers=dict(sig=big["sig"][:cap * rps], state=big["state"][:4]))

    def intact():
        assert bool((big["sig"][cap * rps:] == GUARD).all()) and bool((big["state"][4:] == GUARD).all())
    return odb, intact


@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_append_rule_overflow_and_guards(type_):
    rps, L = online_model.SHAPES[type_]
    ctx = _stream_context(0)
    cap = 3
    odb, intact = guarded(ctx, type_, cap)
    host_db = api.OnlineDatabase(ctx, type_, cap)
    model = online_model.OnlineModel(type_, cap)
    rng = np.random.default_rng(3)
    seq = [1, 0, None, 1, 0, 1, 1, 0, None]                # emitted per append: the fourth stored row does not exist
    want_flags = [0, 0, 0, 0, 0, OVERFLOW, OVERFLOW, OVERFLOW, OVERFLOW]
    for step, (e, wf) in enumerate(zip(seq, want_flags)):
        s = rng.random((rps, L))
        em = None if e is None else torch.tensor([e], dtype=torch.int32, device="cuda")
        info = odb.append_torch(dev(s), emitted=em)
        want = model.append(s, None if e is None else [e])
        ctx.sync()
        assert info.cpu().numpy().tolist() == want.tolist() and want[3] == wf, (step, info, want)
        assert same_bytes(odb.state.cpu().numpy(), model.state) and same_bytes(odb.sig.cpu().numpy(), model.sig), step
        intact()
        if e != 0:                                         # the host form on a second database: the same bytes
            assert host_db.append(s).tolist() == want.tolist(), step
            assert same_bytes(host_db.state.cpu().numpy(), model.state) and same_bytes(host_db.sig.cpu().numpy(), model.sig), step
    assert odb.count() == (cap, OVERFLOW)
    q = dev(rng.random((rps, L)))
    idx, score = odb.match_torch(q, 0, 2.0, 4, emitted=torch.tensor([0], dtype=torch.int32, device="cuda"))
    ctx.sync()
    assert idx.cpu().numpy().tolist() == [[-1] * 4] and np.isnan(score.cpu().numpy()).all()          # a match switched off
    odb.reset(); model.reset()
    ctx.sync()
    assert odb.count() == (0, 0) and not odb.state.cpu().numpy().any()
    s = rng.random((rps, L))
    assert odb.append_torch(dev(s)).cpu().numpy().tolist() == model.append(s).tolist() == [1, 0, 1, 0]
    ctx.sync()
    assert same_bytes(odb.sig.cpu().numpy(), model.sig)
    intact()
    odb.close(); host_db.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. growth under one capture
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_one_captured_step_serves_a_growing_database(type_):
    c = online_cases.edge_case(type_)
    rps, L = online_model.SHAPES[type_]
    K, W, STEPS = 3, 2, 40
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        a = api.OnlineDatabase(ctx, type_, 64, max_k=4)
        b = api.OnlineDatabase(ctx, type_, 64, max_k=4)
        model = online_model.OnlineModel(type_, 64)
        db = dev(c["db"][:STEPS * rps])
        sig = torch.zeros((rps, L), dtype=torch.float64, device="cuda")
        out = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"))
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        g = None
        for i in range(STEPS):
            sig.copy_(db[i * rps:(i + 1) * rps])           # the static tensor, refilled
            if i == 0:
                a.step_torch(sig, W, 2.0, K, out=out, info=info)               # one eager step, then the capture of the same call
                st.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    a.step_torch(sig, W, 2.0, K, out=out, info=info)
            else:
                g.replay()
            bi, bs, binfo = b.step_torch(sig, W, 2.0, K)
            st.synchronize()
            gi, gs = out[0].cpu().numpy(), out[1].cpu().numpy()
            assert same_bytes(gi, bi.cpu().numpy()) and same_bytes(gs, bs.cpu().numpy()), i   # the eager calls' bytes
            assert info.cpu().numpy().tolist() == binfo.cpu().numpy().tolist() == [1, i, i + 1, 0], i
            wi, ws, winfo = model.step(c["db"][i * rps:(i + 1) * rps], W, 2.0, K)
            assert_match(out[0], out[1], wi, ws, (type_, "replay", i))
            assert winfo.tolist() == [1, i, i + 1, 0]
        assert a.count() == b.count() == (STEPS, 0)
        assert same_bytes(a.sig.cpu().numpy(), b.sig.cpu().numpy()) and same_bytes(a.sig.cpu().numpy(), model.sig)
        del g
        a.close(); b.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. agreement with the existing matcher
def test_agrees_with_the_matcher_on_a_growing_database():
    N, K, W = 300, 2, 2
    db_h = online_cases.edge_case("sc")["db"][:N]
    q_h = online_cases.edge_case("sc")["q"]
    ctx = _stream_context(0, exact_statistics=True)
    mt = Matcher("sc", 1, N, ctx=ctx)
    mt.reserve_database()
    odb = api.OnlineDatabase(ctx, "sc", N, max_k=K)
    db, q = dev(db_h), dev(q_h)
    have = 0
    for n in (5, 10, 100, 257, 300):
        mt.append_database(db[have:n])
        grow(odb, db, (have, n))
        have = n
        mi, ms = mt.match(q, W, 2.0, K, q_row0=n)          # the query is row n for the mask, as in the online database
        oi, os_ = odb.match_torch(q, W, 2.0, K)
        torch.cuda.synchronize()
        mi, ms, oi, os_ = (t.cpu().numpy() for t in (mi, ms, oi, os_))
        print("   rows", n, "idx", oi[0].tolist(), "max |score - matcher|", float(np.abs(os_ - ms).max()))
        assert np.array_equal(mi, oi), (n, mi, oi)
        assert close(os_, ms, SCORE_TOL), (n, os_, ms)
    odb.close(); mt.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the whole step as one graph
@pytest.fixture(scope="module")
def seq07(golden_dir, tmp_path_factory):
    """the seq07 drive of test_gpu_map.py"""
    d = tmp_path_factory.mktemp("seq07o")
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    pts = str(d / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
    short = str(d / "poses140.txt")
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    pid, w, qid, xyz, it = api.read_poses_points(short, pts)
    return dict(pid=pid, w=w, xyz=xyz, it=it, cuts=api.split_points_by_pose(pid, qid))


def pose_inputs(drive, p):
    cuts = drive["cuts"]
    k = int(cuts[p + 1] - cuts[p])
    x = np.zeros((60, 3)); it = np.zeros(60, np.float32)
    x[:k] = drive["xyz"][cuts[p]:cuts[p + 1]]; it[:k] = drive["it"][cuts[p]:cuts[p + 1]]
    return drive["w"][p].reshape(12), x, it, k, int(drive["pid"][p])


KCAP, PCAP, MAXC = 112, 1 << 20, 9000
STEP_K, STEP_MASK = 2, 5


def run_drive(drive, captured):
    """push_torch -> pr_sc_generate_frames_dev -> step_torch (emitted = the push's info) -> KeyframeMap.append_push -> align -> verify from
    the map, per pose: eagerly, or as ONE graph captured behind the first eager step.  The match comes BEFORE the keyframe's own map
    append: every idx is a row both the database and the map held before this keyframe.  Returns per pose the host
    copies of idx, score, the database's state, the map's state, T, stats and accepted."""
    P = len(drive["pid"])
    res = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        lib = ctx.lib
        p = lambda t: t.data_ptr()
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
        it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda")
        sig = torch.zeros((1, 2400), dtype=torch.float64, device="cuda")
        mout = (torch.zeros((1, STEP_K), dtype=torch.int32, device="cuda"), torch.zeros((1, STEP_K), dtype=torch.float64, device="cuda"))
        oinfo = torch.zeros(4, dtype=torch.int32, device="cuda"); minfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        odb = api.OnlineDatabase(ctx, "sc", KCAP, max_k=STEP_K)
        out = win.empty_out()
        keep = dict(al=None, v=None)

        def load(i):
            w, hx, hit, k, pid = pose_inputs(drive, i)
            pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit))
            n.fill_(k); kid.fill_(pid)

        def step():
            win.push_torch(pose, x, it, n, out=out)
            ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig)))
            odb.step_torch(sig, STEP_MASK, 2.0, STEP_K, emitted=out["info"], out=mout, info=oinfo)
            km.append_push(out, pose=pose, id=kid, info=minfo)
            keep["al"] = odb.align(mout[0], sig, out=keep["al"])
            keep["v"] = km.verify_variants("sc", mout[0], keep["al"][0], (out["xyz"], out["offs"]), out["frame"][None], 9000, hypotheses=2,
                                           max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=10, out=keep["v"])

        g = None
        for i in range(P):
            load(i)
            if g is not None:
                g.replay()
            else:
                step()
                if captured:
                    st.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        step()
            st.synchronize()
            T, stats, acc, hyp = keep["v"]
            res.append(dict(idx=mout[0].cpu().numpy(), score=mout[1].cpu().numpy(), db_state=odb.state.cpu().numpy(), map_state=km.state.cpu().numpy(),
                            db_info=oinfo.cpu().numpy(), T=T.cpu().numpy(), stats=stats.cpu().numpy(), accepted=acc.cpu().numpy(),
                            variant=keep["al"][0].cpu().numpy()))
        counts = (odb.count(), km.count())
        del g
        odb.close(); km.close(); win.close(); ctx.close()
    return res, counts


def test_the_whole_online_step_as_one_graph(seq07):
    got, gcounts = run_drive(seq07, captured=True)
    want, wcounts = run_drive(seq07, captured=False)
    P = len(seq07["pid"])
    assert len(got) == len(want) == P == 140
    for i, (a, b) in enumerate(zip(got, want)):
        for name in ("idx", "score", "db_state", "map_state", "db_info", "T", "stats", "accepted", "variant"):
            assert same_bytes(a[name], b[name]), (i, name, a[name], b[name])
        kf = max(i - 29, 0)                                # keyframes after this pose: the 30 warm-up pushes leave both counts at 0
        assert a["db_state"].tolist() == [kf, 0, 0, 0] and a["map_state"].tolist() == [kf, 0, 0, 0], i
        if i < 30:
            assert (a["idx"] == -1).all() and np.isnan(a["score"]).all() and a["db_info"].tolist() == [0, -1, 0, 0] and not a["accepted"].any()
        else:
            assert a["db_info"].tolist() == [1, kf - 1, kf, 0]
            assert (a["idx"] < kf - 1).all()               # rows held before this keyframe only
            if kf - 1 >= STEP_MASK + STEP_K:               # enough unmasked rows: real candidates, outside the mask
                assert (a["idx"] >= 0).all() and (a["idx"] <= kf - 1 - STEP_MASK).all() and np.isfinite(a["score"]).all(), i
                assert (a["variant"][..., 0] >= 0).all()
    assert gcounts == wcounts and gcounts[0] == (110, 0) and gcounts[1][0] == 110 and gcounts[1][2] == 0
    print("   accepted pairs over the drive:", int(sum(a["accepted"].sum() for a in got)), "of", 110 * STEP_K)
