"""The pose-proximity candidate search and the batch add of the closure log without a device (pr_proximity, pr_posegraphb_add; DESIGN.md
4.27): the header's rule text, the exported and bound symbols, the scratch formula, every refusal that comes before a device is touched,
the NumPy restatement (proximity_np.py) against an independently written double loop, the committed pose histories, and the chain
search -> ICP -> log -> gate -> relax on the restatements."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

import gate_np
import posegraph_np as pg
import proximity_np as px
import trajeval_np as tn
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("pr_proximity_create", "pr_proximity_destroy", "pr_proximity_scratch_bytes", "pr_proximity_tile", "pr_proximity_search_dev",
         "pr_proximity_search", "pr_posegraphb_add_dev", "pr_posegraphb_add")
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ 1. header, symbols, formula, refusals
def test_header_carries_the_rule_and_the_symbols_are_bound():
    h = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for phrase in ("tests/proximity_np.py", "PR_PROXIMITY_QRANGE_CLAMPED iff", "i + min_gap <= q", "d2 < rad rad (strict)", "BLOCKED order",
                   "Bucket b = i / stride", "T0 = P_i P_q^-1", "|lo - i| <= known_window", "-1 / +Inf / identity / -1 / -1 / 0",
                   "cos_min == -1 forms no dot product", "c calls of pr_posegraphw_add_dev (k = 1)", "enum { PR_PROXIMITY_QRANGE_CLAMPED = 1 }"):
        assert phrase in h, phrase
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert C.sizeof(_lib.ProximityParams) == 48 and _lib.PROXIMITY_QRANGE_CLAMPED == px.QRANGE_CLAMPED == 1
    assert api.ProximitySearch.tile() == (16, 256)


def r16(x):
    return (x + 15) & ~15


def runs_of(cap, Q):
    rows, cols = api.ProximitySearch.tile()
    return 1 if -(-Q // rows) >= 128 else min(16, -(-cap // cols))


@pytest.mark.parametrize("cap,Q,K", [(256, 1, 1), (257, 17, 4), (4096, 4096, 4), (4096, 1, 32), (1 << 20, 2047, 32), (1 << 20, 65535, 1), (600, 2048, 31)])
def test_scratch_formula(cap, Q, K):
    QK = Q * K
    P = QK * runs_of(cap, Q)
    want = sum(r16(x) for x in (24 * cap, 24 * cap, 8 * cap, 4 * cap, 8 * P, 4 * P, 4 * QK, 8 * QK, 96 * QK, 4 * QK, 4 * QK, QK, 16))
    assert _lib.load().pr_proximity_scratch_bytes(cap, Q, K) == want


@pytest.mark.parametrize("cap,Q,K,word", [(0, 1, 1, "node_capacity"), ((1 << 20) + 1, 1, 1, "node_capacity"), (10, 1, 0, "k_max"), (10, 1, 33, "k_max"),
                                          (10, 0, 1, "query_capacity"), (10, 65536, 1, "query_capacity"), (10, 2048, 32, "query_capacity")])
def test_bad_sizes_are_refused_before_a_device_is_touched(cap, Q, K, word):
    lib = _lib.load()
    h = C.c_void_p(5)
    assert lib.pr_proximity_create(None, cap, Q, K, C.byref(h)) == _lib.PR_EINVAL and not h
    assert word in lib.pr_last_error(None).decode()
    assert lib.pr_proximity_scratch_bytes(cap, Q, K) == 0


def prm(**kw):
    d = dict(radius=5.0, growth=0.0, radius_max=5.0, cos_min=-1.0, min_gap=1, stride=1, k=1, known_window=0)
    d.update(kw)
    return _lib.ProximityParams(*(d[n] for n, _ in _lib.ProximityParams._fields_))


BAD_PARAMS = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=INF, radius_max=INF), "radius"), (dict(radius=NAN), "radius"),
              (dict(growth=-0.1), "growth"), (dict(growth=INF), "growth"), (dict(growth=NAN), "growth"), (dict(radius_max=4.0), "radius_max"),
              (dict(radius_max=INF), "radius_max"), (dict(radius_max=NAN), "radius_max"), (dict(cos_min=-1.5), "cos_min"), (dict(cos_min=1.5), "cos_min"),
              (dict(cos_min=NAN), "cos_min"), (dict(min_gap=0), "min_gap"), (dict(stride=0), "stride"), (dict(known_window=-1), "known_window")]


@pytest.mark.parametrize("kw,word", BAD_PARAMS)
def test_bad_search_parameters_are_refused_before_a_device_is_touched(kw, word):
    lib = _lib.load()
    p = prm(**kw)
    for fn, who in ((lib.pr_proximity_search_dev, "pr_proximity_search_dev: "), (lib.pr_proximity_search, "pr_proximity_search: ")):
        assert fn(None, None, None, None, C.byref(p), None, 0, None, None, None, None, None, None, None) == _lib.PR_EINVAL
        msg = lib.pr_last_error(None).decode()
        assert msg.startswith(who) and word in msg, msg


def test_null_pointers_log_and_batch_refusals():
    lib = _lib.load()
    p = prm()
    some = C.c_void_p(64)
    log = _lib.PoseGraphBuffers(some, some, some, some)
    for fn in (lib.pr_proximity_search_dev, lib.pr_proximity_search):
        def call(params=C.byref(p), lg=None, ec=0, known=None):
            assert fn(None, None, None, None, params, lg, ec, None, None, None, None, None, known, None) == _lib.PR_EINVAL
            return lib.pr_last_error(None).decode()
        assert "params is NULL" in call(params=None)
        assert "log_edge_capacity" in call(ec=-1) and "log_edge_capacity" in call(ec=(1 << 20) + 1)
        assert "known is NULL with a closure log" in call(lg=C.byref(log), ec=8)
        assert "buffer of the closure log is NULL" in call(lg=C.byref(_lib.PoseGraphBuffers(None, some, some, some)), ec=8, known=some)
        assert "handle is NULL" in call()                            # everything else is in order: only now the handle is looked at
    out = C.c_void_p()
    assert lib.pr_proximity_create(None, 10, 1, 1, None) == _lib.PR_EINVAL and "out is NULL" in lib.pr_last_error(None).decode()
    assert lib.pr_proximity_create(None, 10, 1, 1, C.byref(out)) == _lib.PR_EINVAL and "ctx is NULL" in lib.pr_last_error(None).decode()
    lib.pr_proximity_destroy(None)
    for fn, who in ((lib.pr_posegraphb_add_dev, "pr_posegraphb_add_dev: "), (lib.pr_posegraphb_add, "pr_posegraphb_add: ")):
        def add(c=4, w_rot=1.0, w_trans=1.0):
            assert fn(None, None, None, None, None, None, w_rot, w_trans, c, None) == _lib.PR_EINVAL
            msg = lib.pr_last_error(None).decode()
            assert msg.startswith(who), msg
            return msg
        assert "c=0" in add(c=0) and "c=65536" in add(c=65536) and "c=-1" in add(c=-1)
        for bad in (-1.0, INF, NAN):
            assert "w_rot" in add(w_rot=bad) and "w_trans" in add(w_trans=bad)
        assert "graph is NULL" in add()


def test_the_class_refuses_before_the_library():
    """another context, a map of another capacity, a k outside 1 .. k_max, a log of another context: raised before any library call"""
    ps = api.ProximitySearch.__new__(api.ProximitySearch)
    ctx = types.SimpleNamespace(device=0)
    ps.ctx, ps.h, ps.node_capacity, ps.query_capacity, ps.k_max, ps.lib = ctx, None, 100, 4, 2, None
    with pytest.raises(ValueError, match="share one context"):
        ps.search_map(types.SimpleNamespace(ctx=object(), keyframe_capacity=100), None, radius=1.0, min_gap=1)
    with pytest.raises(ValueError, match="keyframe_capacity"):
        ps.search_map(types.SimpleNamespace(ctx=ctx, keyframe_capacity=99), None, radius=1.0, min_gap=1)
    with pytest.raises(ValueError, match="share one context"):
        ps.verify_map_torch(types.SimpleNamespace(ctx=object(), keyframe_capacity=100), None, 10)
    with pytest.raises(ValueError, match="keyframe_capacity"):
        ps.verify_map_torch(types.SimpleNamespace(ctx=ctx, keyframe_capacity=7), None, 10)


# ------------------------------------------------------------------------------------------------ 2. the restatement against a double loop
class DoubleLoop:
    """the rule written row by row in Python floats: validity, centres and the blocked path length once, then every candidate (d2, i) of a
    query row"""

    def __init__(self, poses, n, cap):
        self.P = P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
        self.n = n
        self.ok = [a < n and all(math.isfinite(x) for x in P[a].ravel()) for a in range(cap)]
        self.cen = [self.centre(a) if self.ok[a] else None for a in range(cap)]
        C_ = -(-cap // 256)
        prev, acc, totals, w = None, 0.0, [], [0.0] * cap
        for i in range(cap):
            if i % C_ == 0:
                acc = 0.0
            if self.ok[i]:
                if prev is not None:
                    a, b = self.cen[i], self.cen[prev]
                    x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
                    acc = acc + math.sqrt((x * x + y * y) + z * z)
                prev = i
            w[i] = acc
            if i % C_ == C_ - 1 or i == cap - 1:
                totals.append(acc)
        self.s = [sum_in_order(totals[:i // C_]) + w[i] for i in range(cap)]

    def centre(self, a):
        R, t = self.P[a, :, :3].tolist(), self.P[a, :, 3].tolist()
        return [-((R[0][c] * t[0] + R[1][c] * t[1]) + R[2][c] * t[2]) for c in range(3)]

    def candidates(self, q, radius, growth, radius_max, cos_min, min_gap):
        if not (0 <= q < self.n and self.ok[q]):
            return None
        out, cq, s = [], self.cen[q], self.s
        for i in range(self.n):
            if not self.ok[i] or i + min_gap > q:
                continue
            ci = self.cen[i]
            x, y, z = ci[0] - cq[0], ci[1] - cq[1], ci[2] - cq[2]
            d2 = (x * x + y * y) + z * z
            rad = radius + growth * (s[q] - s[i])
            if not rad < radius_max:
                rad = radius_max
            if not d2 < rad * rad:
                continue
            if cos_min > -1.0:
                a, b = self.P[i, 2, :3].tolist(), self.P[q, 2, :3].tolist()
                if not (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2] >= cos_min:
                    continue
            out.append((d2, i))
        return out


def sum_in_order(xs):
    acc = 0.0
    for x in xs:
        acc = acc + x
    return acc


def bucketed(cands, stride, k):
    best = {}
    for d2, i in cands:
        b = i // stride
        if b not in best or (d2, i) < best[b]:
            best[b] = (d2, i)
    return sorted(best.values())[:k]


def drive(n, cap, seed=1, holes=()):
    P = np.zeros((cap, 12))
    P[:min(n, cap)] = px.two_lap_circle(max(n, 2), seed=seed, radius=6.0, rot=0.01, trans=0.05)[:min(n, cap)]
    for a in holes:
        P[a, 3] = NAN
    return P


@pytest.mark.parametrize("n,cap,stride,k,cos_min,growth", [(60, 64, 1, 64, -1.0, 0.0), (60, 64, 3, 4, -1.0, 0.05), (130, 300, 8, 2, 0.5, 0.02),
                                                          (130, 300, 200, 3, 0.0, 0.05), (257, 600, 5, 32, -1.0, 0.01)])
def test_restatement_equals_the_double_loop(n, cap, stride, k, cos_min, growth):
    P = drive(n, cap, holes=(7, n // 2))
    kw = dict(radius=2.5, growth=growth, radius_max=6.0, cos_min=cos_min, min_gap=5)
    kk = k
    res = px.search(P, n, (0, n), cap, n, stride=stride, k=kk, **kw)
    loop = DoubleLoop(P, n, cap)
    assert np.array_equal(np.array(loop.s), res["aux"]["s"])         # the blocked prefix, byte for byte
    total = 0
    for q in range(n):
        cands = loop.candidates(q, **kw)
        want = [] if cands is None else bucketed(cands, stride, kk)
        total += len(want)
        got = [(d, int(i)) for d, i in zip(res["d2"][q], res["idx"][q]) if i >= 0]
        assert got == want, (q, got, want)
        assert (res["idx"][q, len(want):] == -1).all() and np.isinf(res["d2"][q, len(want):]).all()
        if stride == 1 and cands is not None and len(cands) <= kk:
            assert got == sorted(cands)                              # k above the candidate count: every candidate in (d2, i) order
    assert total > n // 4 and res["info"][1] == total and res["info"][0] == n - 2


def test_prefix_equals_trajevals_blocked_dist():
    for n, cap in ((50, 64), (257, 600), (513, 2048)):
        P = drive(n, cap, holes=(3, 100) if n > 100 else (3,))
        valid, cen, _ = px.prepare(P, n, cap)
        assert np.array_equal(px.path_length(cen, valid), tn.blocked_prefix(tn.path_steps(cen, valid), cap))


def test_seed_equals_measure_entry_for_entry():
    P = drive(40, 40)
    res = px.search(P, 40, (0, 40), 40, 40, radius=3.0, min_gap=5, k=3)
    slots = np.flatnonzero(res["pair_src"] >= 0)
    assert len(slots) > 10
    for o in slots:
        i, q = int(res["pair_dst"][o]), int(res["pair_src"][o])
        A = P.reshape(-1, 3, 4)
        # the stated association, written out entry by entry
        Rq, tq, Ri, ti = A[q, :, :3], A[q, :, 3], A[i, :, :3], A[i, :, 3]
        tv = [-((Rq[0, c] * tq[0] + Rq[1, c] * tq[1]) + Rq[2, c] * tq[2]) for c in range(3)]
        want = np.zeros((3, 4))
        for r in range(3):
            for c in range(3):
                want[r, c] = (Ri[r, 0] * Rq[c, 0] + Ri[r, 1] * Rq[c, 1]) + Ri[r, 2] * Rq[c, 2]
            want[r, 3] = ((Ri[r, 0] * tv[0] + Ri[r, 1] * tv[1]) + Ri[r, 2] * tv[2]) + ti[r]
        assert np.array_equal(res["T0"][o], want)
        assert np.abs(res["T0"][o].reshape(12) - pg.measure(P, i, q)).max() < 1e-12      # posegraph_np's Z_ij (another association)


def test_known_rule_with_reversed_and_negative_edges():
    P = drive(60, 64)
    kw = dict(radius=3.0, min_gap=5, k=2, stride=4)
    free = px.search(P, 60, (0, 60), 64, 60, **kw)
    slots = np.flatnonzero(free["pair_src"] >= 0)
    a, b, c = slots[0], slots[len(slots) // 2], slots[-1]
    pair = lambda o: (int(free["pair_dst"][o]), int(free["pair_src"][o]))
    e = np.zeros((8, 2), np.int32)
    e[0] = pair(a)                                                   # (i, q)
    e[1] = pair(b)[::-1]                                             # reversed: (q, i)
    e[2] = (-1, pair(c)[1])                                          # a negative index never matches
    e[3] = (pair(c)[0] + 2, pair(c)[1] - 2)                          # two rows off at both ends
    e[4] = pair(slots[1])                                            # beyond the count
    state = np.array([4, 0, 0, 0], np.int32)
    w0 = px.search(P, 60, (0, 60), 64, 60, log=(e, state), log_edge_capacity=8, known_window=0, **kw)
    w2 = px.search(P, 60, (0, 60), 64, 60, log=(e, state), log_edge_capacity=8, known_window=2, **kw)
    assert w0["known"][a] == 1 and w0["known"][b] == 1 and w0["known"][c] == 0 and w2["known"][c] == 1
    assert w0["info"][2] == int(w0["known"].sum()) >= 2 and w2["info"][2] >= w0["info"][2] + 1
    for res in (w0, w2):
        kn = res["known"] == 1
        assert np.array_equal(res["idx"], free["idx"]) and np.array_equal(res["d2"], free["d2"])
        assert (res["pair_src"][kn] == -1).all() and (res["pair_dst"][kn] == -1).all()
        assert (res["T0"][kn].reshape(-1, 12) == px.IDENTITY).all()
        assert np.array_equal(res["T0"][~kn], free["T0"][~kn]) and np.array_equal(res["pair_src"][~kn], free["pair_src"][~kn])
    big = px.search(P, 60, (0, 60), 64, 60, log=(e, np.array([99, 0, 0, 0], np.int32)), log_edge_capacity=5, known_window=0, **kw)
    assert big["known"][slots[1]] == 1                               # a count beyond the capacity is clamped to it: edge 4 counts
    none = px.search(P, 60, (0, 60), 64, 60, log=(e, np.array([-3, 0, 0, 0], np.int32)), log_edge_capacity=8, known_window=0, **kw)
    assert none["info"][2] == 0


def test_qrange_flags_and_unsearched_rows():
    P = drive(30, 32, holes=(12,))
    kw = dict(radius=3.0, min_gap=3)
    for qr, want_flag, rows in (((0, 30), 0, 29), ((5, 8), 0, 7), ((25, 8), 1, 5), ((-2, 8), 1, 6), ((0, 0), 0, 0), ((0, 40), 1, 29), ((0, -1), 1, 0),
                                ((40, 2), 1, 0)):
        res = px.search(P, 30, qr, 32, 32, **kw)
        assert res["info"][3] == want_flag and res["info"][0] == rows, (qr, res["info"])
    for n_raw in (-5, 99):
        res = px.search(P, n_raw, (0, 32), 32, 32, **kw)
        assert res["info"][0] == (0 if n_raw < 0 else 31)             # clamped to the capacity: the two zero rows behind the drive count


def batch_inputs(c, seed=0):
    rng = np.random.default_rng(seed)
    i = rng.integers(-1, 50, c).astype(np.int32)
    j = rng.integers(-1, 50, c).astype(np.int32)
    T = rng.normal(size=(c, 12))
    T[rng.random(c) < 0.1, 5] = NAN
    acc = (rng.random(c) < 0.8).astype(np.uint8)
    w = rng.uniform(0.0, 5.0, (c, 2))
    for bad in (NAN, -1.0, INF):
        w[rng.random(c) < 0.05, rng.integers(0, 2)] = bad
    return i, j, T, acc, w


@pytest.mark.parametrize("c,cap,with_w", [(1, 8, True), (5, 8, False), (256, 100, True), (257, 400, True), (1025, 700, False)])
def test_batch_add_equals_single_adds(c, cap, with_w):
    i, j, T, acc, w = batch_inputs(c, seed=c)
    a, b = pg.PoseGraphModel(cap), pg.PoseGraphModel(cap)
    a.state[0] = b.state[0] = 3
    info = px.add_batch(a, i, j, T, acc, w if with_w else None, 2.0, 3.0)
    logged, first = 0, -1
    for p in range(c):
        ww = w[p] if with_w else np.array([2.0, 3.0])
        good = np.isfinite(ww).all() and (ww >= 0).all()
        r = b.add([i[p]], T[p], [acc[p] if good else 0], int(j[p]), *(ww if good else (1.0, 1.0)))
        if r[0] and first < 0:
            first = r[1]
        logged += r[0]
    for name in ("edge_ij", "edge_Z", "edge_w", "state"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert info[0] == logged and info[1] == first and info[2] == b.state[0] and info[3] == b.state[1]
    if (c, cap) == (256, 100):
        assert info[3] == 1 and info[2] == cap                       # across the capacity


def test_batch_add_leaves_the_model_alone_when_nothing_qualifies():
    m = pg.PoseGraphModel(4)
    m.state[:] = (77, 6, 0, 0)                                       # scribbled: nothing is committed by slots with a negative query row
    before = [m.edge_ij.copy(), m.edge_Z.copy(), m.edge_w.copy(), m.state.copy()]
    info = px.add_batch(m, [1, 2], [-1, -4], np.zeros((2, 12)), [1, 1])
    assert list(info) == [0, -1, 4, 0]
    for x, y in zip(before, (m.edge_ij, m.edge_Z, m.edge_w, m.state)):
        assert np.array_equal(x, y)
    info = px.add_batch(m, [1, 2], [5, 2], np.zeros((2, 12)), [0, 1])   # a valid query row: the clamped count is committed, nothing logged
    assert list(info) == [0, -1, 4, 0] and list(m.state) == [4, 0, 0, 0] and np.array_equal(m.edge_ij, before[0])


# ------------------------------------------------------------------------------------------------ 3. the committed pose histories
HISTORIES = {"seq06": ("kitti_seq06", "poses_history_file.txt"), "seq00": ("ref_sequences/kitti_seq00", "poses_history_file.txt.gz"),
             "seq05": ("ref_sequences/kitti_seq05", "poses_history_file.txt.gz"), "seq02": ("ref_sequences/kitti_seq02", "poses_history_file.txt.gz")}
# rows with a candidate at (radius 5, min_gap 50): growth 0 | growth 0.02, radius_max 30 | the same with cos_min 0.5.  What the restatement
# and the plain double loop below agree on; the same figures a plain cumsum path length gives.
PINNED = {"seq06": (193, 262, 224), "seq00": (130, 822, 728), "seq05": (193, 490, 432), "seq02": (0, 426, 311)}


def plain_rows(P, radius, growth, radius_max, cos_min, min_gap):
    """rows with a candidate by a plain double loop over blocks of numpy rows (a cumsum path length: the blocked one differs by rounding)"""
    A = P.reshape(-1, 3, 4)
    cen = -np.einsum("nji,nj->ni", A[:, :, :3], A[:, :, 3])
    s = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(cen, axis=0), axis=1))])
    ax = A[:, 2, :3]
    rows, margin = 0, np.inf
    for q in range(min_gap, len(P)):
        i = np.arange(0, q - min_gap + 1)
        d = np.linalg.norm(cen[i] - cen[q], axis=1)
        rad = np.minimum(radius + growth * (s[q] - s[i]), radius_max)
        ok = d < rad
        margin = min(margin, float(np.abs(d - rad).min() / radius))
        if cos_min > -1.0:
            dot = ax[i] @ ax[q]
            ok &= dot >= cos_min
            margin = min(margin, float(np.abs(dot - cos_min).min()))
        rows += bool(ok.any())
    return rows, margin


@pytest.mark.parametrize("name", sorted(HISTORIES))
def test_committed_pose_histories(name):
    d, f = HISTORIES[name]
    P = np.ascontiguousarray(np.loadtxt(os.path.join(GOLDEN, d, f))[:, 1:13])
    n = len(P)
    got = []
    for kw in (dict(), dict(growth=0.02, radius_max=30.0), dict(growth=0.02, radius_max=30.0, cos_min=0.5)):
        res = px.search(P, n, (0, n), n, n, radius=5.0, min_gap=50, **kw)
        rows = int((res["idx"][:, 0] >= 0).sum())
        plain, margin = plain_rows(P, 5.0, kw.get("growth", 0.0), kw.get("radius_max", 5.0), kw.get("cos_min", -1.0), 50)
        print(name, n, kw, "rows with a candidate:", rows, "plain loop:", plain, "smallest margin:", margin)
        assert margin > 1e-9                                         # no pair sits within rounding of a threshold: the two must agree
        assert rows == plain
        got.append(rows)
    assert tuple(got) == PINNED[name]
    if name == "seq02":
        assert got[0] == 0 and got[1] > 0                            # drift has opened the loop: only a growing radius finds it
    else:
        assert got[0] > 0


# ------------------------------------------------------------------------------------------------ 4. the chain scene
def centre_error(P, gt):
    c = lambda X: -np.einsum("nji,nj->ni", X.reshape(-1, 3, 4)[:, :, :3], X.reshape(-1, 3, 4)[:, :, 3])
    return float(np.linalg.norm(c(P) - c(gt), axis=1).max())


def thinned(Q, acc):
    """the accepted log thinned to one closure per tenth query row"""
    first, seen = np.zeros(len(Q), bool), set()
    for a in range(len(Q)):
        if acc[a] and Q[a] % 10 == 0 and Q[a] not in seen:
            seen.add(int(Q[a]))
            first[a] = True
    return first


def test_chain_scene_on_the_restatements():
    sc, run, c = px.chain_scene(), px.chain_run(), px.CHAIN
    sizes = [len(x) for x in sc["clouds"]]
    assert 700 <= min(sizes) and max(sizes) <= 860, (min(sizes), max(sizes))
    res, slots, acc = run["search"], run["slots"], run["accepted"]
    I, Q = res["pair_dst"][slots], res["pair_src"][slots]
    print("candidates", len(slots), "accepted", int(acc.sum()), "fitness min", run["fitness"].min(), "rmse max", run["rmse"].max())
    assert len(slots) >= 40 and acc.sum() >= 0.9 * len(slots)
    assert (np.abs(run["fitness"] - c["min_fitness"]) > 0.05 * c["min_fitness"]).all()       # no accept decision near a threshold
    assert (np.abs(run["rmse"] - c["max_rmse"]) > 0.05 * c["max_rmse"]).all()
    for a in np.flatnonzero(acc):
        assert np.abs(run["T"][a] - pg.measure(sc["gt"], I[a], Q[a])).max() < 0.05
    tabs = gate_np.default_tables(c["gate"]["max_gap"])
    dense = pg.PoseGraphModel(256)
    px.add_batch(dense, I, Q, run["T"], acc, None, *c["w"])
    out, _ = pg.relax(sc["est"], c["n"], dense.edge_ij, dense.edge_Z, dense.edge_w, dense.state[0], **c["relax"])
    before, after = centre_error(sc["est"], sc["gt"]), centre_error(out, sc["gt"])
    print("largest centre error", before, "->", after)
    assert after < 0.5 * before
    g = gate_np.gate(sc["est"], c["n"], dense, c["n"], rot_tab=tabs[0], trans2_tab=tabs[1], **c["gate"])
    thin = pg.PoseGraphModel(256)
    px.add_batch(thin, I, Q, run["T"], thinned(Q, acc), None, *c["w"])
    g2 = gate_np.gate(sc["est"], c["n"], thin, c["n"], rot_tab=tabs[0], trans2_tab=tabs[1], **c["gate"])
    print("gate keeps", g["info"][1], "of", dense.state[0], "dense and", g2["info"][1], "of", thin.state[0], "thinned")
    assert g["info"][1] >= 0.9 * dense.state[0] and thin.state[0] >= 3 and g2["info"][1] == 0
