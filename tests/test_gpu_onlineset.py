"""The online signature sets on the device (pr_onlineset, online.hip): a FUSED (SC + M2DP) and a DELIGHT match against
the rows held so far equal the NumPy model over the oracle (onlineset_model.py) at the kernels' edges and through the reference's corner
rules; the fused rows are the bits two pr_online databases give; the fused result agrees with FusedMatcher; the append rule - ONE count,
every part on the same row or no part at all - equals the model with guard words behind every buffer; ONE captured step serves a growing
set; and the whole online step replays as one graph with the bytes of the eager calls.  Tolerances: idx equal; FUSED score 1e-9 (the
bound of this arithmetic), rows 1e-12 (oracle against device fp64); DELIGHT score bits equal."""
import os

import numpy as np
import pytest
import torch

import helpers
import onlineset_cases as cases
import onlineset_model as model
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import FusedMatcher, _stream_context

pytestmark = pytest.mark.gpu

OVERFLOW = _lib.ONLINE_OVERFLOW
SCORE_TOL, ROWS_TOL = 1e-9, 1e-12


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def devs(parts):
    return tuple(dev(a) for a in parts)


def arg(ts):
    """what OnlineSet takes as `sigs`: the pair for 'fused', the tensor for 'delight'"""
    return ts if len(ts) == 2 else ts[0]


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


def assert_match(got_idx, got_score, want_idx, want_score, what, bits=False):
    gi, gs = got_idx.cpu().numpy(), got_score.cpu().numpy()
    print("  ", what, "idx", gi[0].tolist(), "max |score - model|",
          float(np.nanmax(np.abs(np.where(np.isfinite(want_score), gs - want_score, 0.0)), initial=0.0)))
    assert gi.shape == want_idx.shape and np.array_equal(gi, want_idx), (what, gi, want_idx)
    if bits:
        assert close(gs, want_score, 0.0), (what, gs, want_score)                  # equal values (a NaN's payload aside)
    else:
        assert close(gs, want_score, SCORE_TOL), (what, gs, want_score)


def grow(oset, kind, db_dev, upto):
    """appends keyframes [upto[0], upto[1]) of db_dev (the tuple of the parts' device rows)"""
    for j in range(upto[0], upto[1]):
        oset.append_torch(arg(cases.rows_of(kind, db_dev, j)))


# ------------------------------------------------------------------------------------------------ 1. FUSED at the kernels' edges
def test_fused_match_at_the_kernels_edges():
    c = cases.fused_edge_case()
    ctx = _stream_context(0)
    cap = cases.NMAX + 60                                  # a capacity that is no multiple of anything; NB = ONLINESET_NB_FUSED
    oset = api.OnlineSet(ctx, "fused", cap, max_k=cases.MAX_K)
    db, q = devs(c["db"]), devs(c["q"])
    rows = torch.full((4, cap), -5.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in cases.FUSED_COUNTS:
        grow(oset, "fused", db, (have, n))
        have = n
        for pw in cases.WEIGHTS:
            f = model.fused_scores(c["d"][:, :n], pw) if n >= 2 else None
            for k, w in cases.KM:
                rows.fill_(-5.0)
                idx, score = oset.match_torch(q, w, pw, k, rows=rows)
                ctx.sync()
                wi, ws = model.select(f, w, k) if n >= 2 else model.match_rows("fused", c["d"][:, :n], w, pw, k)
                assert_match(idx, score, wi, ws, ("fused", n, k, w, pw))
                r = rows.cpu().numpy()
                assert close(r[:, :n], c["d"][:, :n], ROWS_TOL), n
                assert (r[:, n:] == -5.0).all(), n                                 # nothing behind the count
        assert oset.count() == (n, 0)
    with pytest.raises(_lib.PRError, match="max_k"):
        oset.match_torch(q, 0, 2.0, cases.MAX_K + 1)
    with pytest.raises(_lib.PRError, match="d_delight must be NULL"):               # a part of the other kind, at the C ABI
        ctx.check(ctx.lib.pr_onlineset_match_dev(oset.h, q[0].data_ptr(), q[1].data_ptr(), q[0].data_ptr(), None, 0, 2.0, 1, rows.data_ptr(),
                                                 rows.data_ptr(), None))
    oset.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the bits of pr_online
def test_fused_rows_are_the_bits_of_two_online_databases():
    c = cases.fused_edge_case()
    N = 260
    ctx = _stream_context(0)
    oset = api.OnlineSet(ctx, "fused", N, max_k=2)
    osc = api.OnlineDatabase(ctx, "sc", N, max_k=2)
    om2 = api.OnlineDatabase(ctx, "m2dp", N, max_k=2)
    db, q = devs(cases.rows_of("fused", c["db"], 0, N)), devs(c["q"])
    rows = torch.zeros((4, N), dtype=torch.float64, device="cuda")
    rsc = torch.zeros((2, N), dtype=torch.float64, device="cuda")
    rm2 = torch.zeros((2, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in (3, 257, N):
        grow(oset, "fused", db, (have, n))
        for j in range(have, n):
            osc.append_torch(db[0][j:j + 1]); om2.append_torch(db[1][4 * j:4 * j + 4])
        have = n
        oset.match_torch(q, 0, 2.0, 2, rows=rows)
        osc.match_torch(q[0], 0, 2.0, 2, rows=rsc)
        om2.match_torch(q[1], 0, 2.0, 2, rows=rm2)
        ctx.sync()
        r, a, b = rows.cpu().numpy(), rsc.cpu().numpy(), rm2.cpu().numpy()
        assert same_bytes(r[0:2, :n], a[:, :n]), n         # SC structure, SC intensity
        assert same_bytes(r[2:4, :n], b[:, :n]), n         # M2DP count, M2DP intensity
        assert not same_bytes(r[0, :n], r[1, :n]) and not same_bytes(r[2, :n], r[3, :n]) and not same_bytes(r[0:2, :n], r[2:4, :n])
    assert same_bytes(oset.sc.cpu().numpy(), osc.sig.cpu().numpy()) and same_bytes(oset.m2dp.cpu().numpy(), om2.sig.cpu().numpy())
    oset.close(); osc.close(); om2.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. agreement with FusedMatcher
def test_fused_agrees_with_the_fused_matcher():
    N, K, W = 300, 2, 2
    c = cases.fused_edge_case()
    ctx = _stream_context(0, exact_statistics=True)
    fm = FusedMatcher(1, N, ctx=ctx)
    oset = api.OnlineSet(ctx, "fused", N, max_k=K)
    db, q = devs(cases.rows_of("fused", c["db"], 0, N)), devs(c["q"])
    have = 0
    for n in (5, 10, 100, 257, 300):
        fm.pack_database(db[0][:n], db[1][:4 * n])
        grow(oset, "fused", db, (have, n))
        have = n
        mi, ms = fm.match(q[0], q[1], W, 2.0, K, q_row0=n)     # the query is row n for the mask, as in the online set
        oi, os_ = oset.match_torch(q, W, 2.0, K)
        torch.cuda.synchronize()
        mi, ms, oi, os_ = (t.cpu().numpy() for t in (mi, ms, oi, os_))
        print("   rows", n, "idx", oi[0].tolist(), "max |score - matcher|", float(np.abs(os_ - ms).max()))
        assert np.array_equal(mi, oi), (n, mi, oi)
        assert close(os_, ms, SCORE_TOL), (n, os_, ms)
    oset.close(); fm.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. FUSED corner rules
def test_fused_reference_corner_rules():
    c = cases.fused_corner_case()
    z = c["zero_row"]
    ctx = _stream_context(0)
    oset = api.OnlineSet(ctx, "fused", 64, max_k=40)
    db = devs(c["db"])
    rows = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in cases.CORNER_COUNTS:
        grow(oset, "fused", db, (have, n))
        have = n
        for name in ("q", "zero"):
            hq = c[name]
            d = model.distances("fused", hq, cases.rows_of("fused", c["db"], 0, n))
            for k, w in cases.CORNER_KM:
                for pw in cases.CORNER_WEIGHTS:
                    idx, score = oset.match_torch(devs(hq), w, pw, k, rows=rows)
                    ctx.sync()
                    wi, ws = model.match_rows("fused", d, w, pw, k)
                    assert_match(idx, score, wi, ws, (name, n, k, w, pw))
                    gi = idx.cpu().numpy()[0]
                    if w == 0:
                        assert z not in gi                                         # a NaN score is never selected
                    if name == "zero":                                             # a zero-norm SC query: every sum is NaN, so only
                        assert (gi[gi >= 0] > n - w).all()                         # the mask's +Inf rows are left (none without a mask)
                        assert np.isposinf(score.cpu().numpy()[0][gi >= 0]).all()
            r = rows.cpu().numpy()
            assert close(r[:, :n], d, ROWS_TOL)
            assert np.isnan(r[:2, z]).all() and np.isfinite(r[2:, z]).all()
            if n > 20:                                                             # copies in every part: identical bits in all four channels
                assert same_bytes(r[:, 7], r[:, 20])
            if n > 33:                                                             # SC copies only: the SC channels' bits, not M2DP's
                assert same_bytes(r[:2, 12], r[:2, 33]) and not same_bytes(r[2:, 12], r[2:, 33])
    idx, score = oset.match_torch(devs(c["q"]), 0, 2.0, 2)
    ctx.sync()
    assert idx.cpu().numpy()[0].tolist() == [7, 20]                                # the tie of the copies goes to the lower index
    s = score.cpu().numpy()[0]
    assert s[0] == s[1]
    idx, score = oset.match_torch(devs(c["q"]), 0, 2.0, 40)
    ctx.sync()
    gi, gs = idx.cpu().numpy()[0].tolist(), score.cpu().numpy()[0]
    assert z not in gi and gi[-1] == -1 and sorted(gi[:-1]) == [j for j in range(40) if j != z]
    assert abs(gs[gi.index(12)] - gs[gi.index(33)]) > 1e-6                         # copies in the SC part only: no tie
    oset.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. DELIGHT at its edges
def test_delight_match_at_the_kernels_edges():
    c = cases.delight_edge_case()
    ctx = _stream_context(0)
    cap = cases.NMAX + 6                                   # no multiple of 16: the last batch of the grid is partial
    oset = api.OnlineSet(ctx, "delight", cap, max_k=cases.MAX_K)
    assert cases.DELIGHT_EDGE + 1 <= cases.NMAX
    db, q = devs(c["db"]), devs(c["q"])
    rows = torch.full((1, cap), -5.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in cases.DELIGHT_COUNTS:
        grow(oset, "delight", db, (have, n))
        have = n
        for k, w in cases.KM:
            rows.fill_(-5.0)
            idx, score = oset.match_torch(q[0], w, 2.0, k, rows=rows)
            ctx.sync()
            wi, ws = model.match_rows("delight", c["d"][:, :n], w, 2.0, k)
            assert_match(idx, score, wi, ws, ("delight", n, k, w), bits=True)
            r = rows.cpu().numpy()
            assert same_bytes(r[:, :n], np.ascontiguousarray(c["d"][:, :n])), n     # the oracle's bits
            assert (r[:, n:] == -5.0).all(), n
        assert oset.count() == (n, 0)
    with pytest.raises(_lib.PRError, match="d_sc and d_m2dp must be NULL"):
        ctx.check(ctx.lib.pr_onlineset_match_dev(oset.h, q[0].data_ptr(), None, q[0].data_ptr(), None, 0, 2.0, 1, rows.data_ptr(),
                                                 rows.data_ptr(), None))
    oset.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. DELIGHT corner rules
def test_delight_reference_corner_rules():
    c = cases.delight_corner_case()
    z = c["zero_row"]
    ctx = _stream_context(0)
    oset = api.OnlineSet(ctx, "delight", 48, max_k=48)
    db = devs(c["db"])
    rows = torch.zeros((1, 48), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    have = 0
    for n in cases.CORNER_COUNTS:
        grow(oset, "delight", db, (have, n))
        have = n
        for name in ("q", "zero"):
            hq = c[name]
            d = model.distances("delight", hq, cases.rows_of("delight", c["db"], 0, n))
            for k, w in cases.CORNER_KM:
                idx, score = oset.match_torch(dev(hq[0]), w, 2.0, k, rows=rows)
                ctx.sync()
                wi, ws = model.match_rows("delight", d, w, 2.0, k)
                assert_match(idx, score, wi, ws, (name, n, k, w), bits=True)
            r = rows.cpu().numpy()
            assert same_bytes(r[:, :n], np.ascontiguousarray(d))
            if name == "zero":
                assert np.isposinf(r[0, z]) and np.isfinite(np.delete(r[0, :n], z)).all()      # zero against zero: +Inf, not NaN
            if n > 20:
                assert r[0, 7] == r[0, 20]
    idx, _ = oset.match_torch(dev(c["q"][0]), 0, 2.0, 2)
    ctx.sync()
    assert idx.cpu().numpy()[0].tolist() == [7, 20]
    idx, score = oset.match_torch(dev(c["zero"][0]), 0, 2.0, 40)
    ctx.sync()
    gi, gs = idx.cpu().numpy()[0], score.cpu().numpy()[0]
    assert gi[-1] == z and np.isposinf(gs[-1]) and sorted(gi.tolist()) == list(range(40))      # last, but selectable
    oset.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 7. append
GUARD = -7


def guarded(ctx, kind, cap):
    """a set over buffers one keyframe / four words longer than stated, the excess filled with a guard pattern"""
    big = {n: torch.zeros(((cap + 1) * r, L), dtype=torch.float64, device="cuda") for n, r, L in model.PARTS[kind]}
    big["state"] = torch.zeros(8, dtype=torch.int32, device="cuda")
    bufs = {}
    for n, r, L in model.PARTS[kind]:
        big[n][cap * r:] = GUARD
        bufs[n] = big[n][:cap * r]
    big["state"][4:] = GUARD
    bufs["state"] = big["state"][:4]
    oset = api.OnlineSet(ctx, kind, cap, buffers=bufs)

    def intact():
        for n, r, L in model.PARTS[kind]:
            assert bool((big[n][cap * r:] == GUARD).all()), n
        assert bool((big["state"][4:] == GUARD).all())
    return oset, intact


def bufs_equal(oset, m):
    return all(same_bytes(getattr(oset, n).cpu().numpy(), m.bufs[n]) for n, _, _ in m.parts) and same_bytes(oset.state.cpu().numpy(), m.state)


@pytest.mark.parametrize("kind", ["fused", "delight"])
def test_append_rule_one_count_overflow_and_guards(kind):
    ctx = _stream_context(0)
    cap = 3
    oset, intact = guarded(ctx, kind, cap)
    host = api.OnlineSet(ctx, kind, cap)
    m = model.OnlineSetModel(kind, cap)
    rng = np.random.default_rng(3)
    seq = [1, 0, None, 1, 0, 1, 1, 0, None]                # emitted per append: the fourth stored keyframe does not exist
    want_flags = [0, 0, 0, 0, 0, OVERFLOW, OVERFLOW, OVERFLOW, OVERFLOW]
    for step, (e, wf) in enumerate(zip(seq, want_flags)):
        s = tuple(rng.random((r, L)) for _, r, L in model.PARTS[kind])
        em = None if e is None else torch.tensor([e], dtype=torch.int32, device="cuda")
        info = oset.append_torch(arg(devs(s)), emitted=em)
        want = m.append(s, None if e is None else [e])
        ctx.sync()
        assert info.cpu().numpy().tolist() == want.tolist() and want[3] == wf, (step, info, want)
        assert bufs_equal(oset, m), step                   # every part on the same row - or, at capacity, NO part anywhere
        intact()
        if e != 0:                                         # the host form on a second set: the same bytes
            assert host.append(arg(s)).tolist() == want.tolist(), step
            assert bufs_equal(host, m), step
    assert oset.count() == (cap, OVERFLOW)
    q = arg(devs(tuple(rng.random((r, L)) for _, r, L in model.PARTS[kind])))
    idx, score = oset.match_torch(q, 0, 2.0, 4, emitted=torch.tensor([0], dtype=torch.int32, device="cuda"))
    ctx.sync()
    assert idx.cpu().numpy().tolist() == [[-1] * 4] and np.isnan(score.cpu().numpy()).all()          # a match switched off
    oset.reset(); m.reset()
    ctx.sync()
    assert oset.count() == (0, 0) and not oset.state.cpu().numpy().any()
    s = tuple(rng.random((r, L)) for _, r, L in model.PARTS[kind])
    assert oset.append_torch(arg(devs(s))).cpu().numpy().tolist() == m.append(s).tolist() == [1, 0, 1, 0]
    ctx.sync()
    assert bufs_equal(oset, m)
    intact()
    oset.close(); host.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 8. growth under one capture
@pytest.mark.parametrize("kind", ["fused", "delight"])
def test_one_captured_step_serves_a_growing_set(kind):
    c = cases.fused_edge_case() if kind == "fused" else cases.delight_edge_case()
    K, W, STEPS = 3, 2, 40
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        a = api.OnlineSet(ctx, kind, 64, max_k=4)
        b = api.OnlineSet(ctx, kind, 64, max_k=4)
        m = model.OnlineSetModel(kind, 64)
        db = devs(cases.rows_of(kind, c["db"], 0, STEPS))
        sig = tuple(torch.zeros((r, L), dtype=torch.float64, device="cuda") for _, r, L in model.PARTS[kind])
        out = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"))
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        g = None
        for i in range(STEPS):
            for t, src in zip(sig, cases.rows_of(kind, db, i)):
                t.copy_(src)                               # the static tensors, refilled
            if i == 0:
                a.step_torch(arg(sig), W, 2.0, K, out=out, info=info)              # one eager step, then the capture of the same call
                st.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    a.step_torch(arg(sig), W, 2.0, K, out=out, info=info)
            else:
                g.replay()
            bi, bs, binfo = b.step_torch(arg(sig), W, 2.0, K)
            st.synchronize()
            gi, gs = out[0].cpu().numpy(), out[1].cpu().numpy()
            assert same_bytes(gi, bi.cpu().numpy()) and same_bytes(gs, bs.cpu().numpy()), i   # the eager calls' bytes
            assert info.cpu().numpy().tolist() == binfo.cpu().numpy().tolist() == [1, i, i + 1, 0], i
            wi, ws, winfo = m.step(cases.rows_of(kind, c["db"], i), W, 2.0, K)
            assert_match(out[0], out[1], wi, ws, (kind, "replay", i), bits=kind == "delight")
            assert winfo.tolist() == [1, i, i + 1, 0]
        assert a.count() == b.count() == (STEPS, 0)
        assert bufs_equal(a, m) and bufs_equal(b, m)
        del g
        a.close(); b.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 9. the whole step on the seq07 drive
@pytest.fixture(scope="module")
def seq07(golden_dir, tmp_path_factory):
    """the seq07 drive of test_gpu_map.py / test_gpu_online.py"""
    d = tmp_path_factory.mktemp("seq07s")
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


def run_drive(drive, kind, captured):
    """Per pose, eagerly or as ONE graph captured behind the first eager step.
    'delight': push_torch -> pr_delight_generate_frames_dev -> step_torch (emitted = the push's info) -> KeyframeMap.append_push -> align ->
    verify_variants('delight') - the whole step is the graph.
    'fused':   push_torch and the two generators run EAGERLY into fixed buffers (pr_m2dp_generate_frames_dev allocates and forks, DESIGN.md
    4.18 Limits; they run for an emitting push only); the graph is step_torch -> append_push -> align -> verify_variants('sc', hypotheses=2).
    The match comes BEFORE the keyframe's own map append: every idx is a row both the set and the map held before this keyframe."""
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
        sig = tuple(torch.zeros((r, L), dtype=torch.float64, device="cuda") for _, r, L in model.PARTS[kind])
        mout = (torch.zeros((1, STEP_K), dtype=torch.int32, device="cuda"), torch.zeros((1, STEP_K), dtype=torch.float64, device="cuda"))
        oinfo = torch.zeros(4, dtype=torch.int32, device="cuda"); minfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        oset = api.OnlineSet(ctx, kind, KCAP, max_k=STEP_K)
        out = win.empty_out()
        keep = dict(al=None, v=None)
        verify = dict(max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=10)

        def load(i):
            w, hx, hit, k, pid = pose_inputs(drive, i)
            pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit))
            n.fill_(k); kid.fill_(pid)

        def front():
            """what stays outside the fused graph"""
            win.push_torch(pose, x, it, n, out=out)
            st.synchronize()
            if int(out["info"][0].item()):
                ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig[0])))
                ctx.check(lib.pr_m2dp_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig[1])))

        def step():
            if kind == "delight":
                win.push_torch(pose, x, it, n, out=out)
                ctx.check(lib.pr_delight_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, p(out["frame"]), p(sig[0])))
            oset.step_torch(arg(sig), STEP_MASK, 2.0, STEP_K, emitted=out["info"], out=mout, info=oinfo)
            km.append_push(out, pose=pose, id=kid, info=minfo)
            keep["al"] = oset.align(mout[0], arg(sig), out=keep["al"])
            var = keep["al"][0]
            if kind == "delight":
                keep["v"] = km.verify_variants("delight", mout[0], var[..., 0], (out["xyz"], out["offs"]), out["frame"][None], 9000, hypotheses=1,
                                               out=keep["v"], **verify)
            else:
                keep["v"] = km.verify_variants("sc", mout[0], var[..., :2], (out["xyz"], out["offs"]), out["frame"][None], 9000, hypotheses=2,
                                               out=keep["v"], **verify)

        g = None
        for i in range(P):
            load(i)
            if kind == "fused":
                front()
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
            res.append(dict(idx=mout[0].cpu().numpy(), score=mout[1].cpu().numpy(), set_state=oset.state.cpu().numpy(), map_state=km.state.cpu().numpy(),
                            set_info=oinfo.cpu().numpy(), T=T.cpu().numpy(), stats=stats.cpu().numpy(), accepted=acc.cpu().numpy(),
                            variant=keep["al"][0].cpu().numpy(), dist=keep["al"][1].cpu().numpy()))
        counts = (oset.count(), km.count())
        del g
        oset.close(); km.close(); win.close(); ctx.close()
    return res, counts


@pytest.mark.parametrize("kind", ["delight", "fused"])
def test_the_whole_online_step_as_one_graph(seq07, kind):
    got, gcounts = run_drive(seq07, kind, captured=True)
    want, wcounts = run_drive(seq07, kind, captured=False)
    P = len(seq07["pid"])
    assert len(got) == len(want) == P == 140
    for i, (a, b) in enumerate(zip(got, want)):
        for name in ("idx", "score", "set_state", "map_state", "set_info", "T", "stats", "accepted", "variant", "dist"):
            assert same_bytes(a[name], b[name]), (kind, i, name, a[name], b[name])
        kf = max(i - 29, 0)                                # keyframes after this pose: the 30 warm-up pushes leave both counts at 0
        assert a["set_state"].tolist() == [kf, 0, 0, 0] and a["map_state"].tolist() == [kf, 0, 0, 0], i
        if i < 30:
            assert (a["idx"] == -1).all() and np.isnan(a["score"]).all() and a["set_info"].tolist() == [0, -1, 0, 0] and not a["accepted"].any()
        else:
            assert a["set_info"].tolist() == [1, kf - 1, kf, 0]
            assert (a["idx"] < kf - 1).all()               # rows held before this keyframe only
            if kf - 1 >= STEP_MASK + STEP_K:               # enough unmasked rows: real candidates, outside the mask
                assert (a["idx"] >= 0).all() and (a["idx"] <= kf - 1 - STEP_MASK).all() and np.isfinite(a["score"]).all(), i
                assert (a["variant"][..., 0] >= 0).all()
    assert gcounts == wcounts and gcounts[0] == (110, 0) and gcounts[1][0] == 110 and gcounts[1][2] == 0
    print("   ", kind, "accepted pairs over the drive:", int(sum(a["accepted"].sum() for a in got)), "of", 110 * STEP_K)
