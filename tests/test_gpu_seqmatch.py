"""The sequence matcher on the device (seqmatch.hip) against the NumPy restatement (seqmatch_np.py).

Equality is of BYTES throughout - idx, score, vel, the dense matrix, the ring, the row ids and the counter: the rule needs IEEE fp64
+, x, /, sqrt only, the kernels are built without contraction and selection by (score, index) does not depend on any order.  The one
exception is the payload of a NaN that arithmetic PRODUCED (the rule does not specify it): such NaNs only ever reach the ring, and
the ring is compared with every NaN mapped to one pattern.  Guard words stand behind every output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import seqmatch_np as sq
from so_dso_place_recognition_amd import _lib, api, synth
from so_dso_place_recognition_amd.matcher import Matcher, _stream_context
from test_gpu_online import pose_inputs, seq07  # noqa: F401  (seq07: the drive's fixture)
from test_seqmatch_cpu import SCENE_L, SCENE_VEL, alias_scene, causal_rows

pytestmark = pytest.mark.gpu

GUARD = -7
R, W = api.seq_tile()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ctx():
    c = _stream_context(0)
    yield c
    c.close()


def inputs(seed, m, n, with_i=True, grid=None):
    g = np.random.default_rng(seed)
    draw = (lambda: g.uniform(0.05, 1.0, (m, n))) if grid is None else (lambda: g.integers(0, grid, (m, n)).astype(np.float64))
    d_p = draw().astype(np.float32)
    d_i = draw().astype(np.float32) if with_i else None
    mom = np.stack([sq.row_moments(d_p), sq.row_moments(d_i)], 1).reshape(m, 2, 3) if with_i else None
    return d_p, d_i, mom


def run_dev(ctx, d_p, d_i, mom, steps, q0=0, d0=0, mw=0, pw=2.0, k=1, dense=True):
    """pr_seq_select_dev over guarded outputs -> host (idx, score, vel, S | None)"""
    m, n = d_p.shape
    flat = [torch.full((m * k + 8,), GUARD, dtype=dt, device="cuda") for dt in (torch.int32, torch.float64, torch.int32)]
    out = [t[:m * k].view(m, k) for t in flat]
    if dense:
        flat.append(torch.full((m * n + 8,), float(GUARD), dtype=torch.float64, device="cuda"))
        out.append(flat[3][:m * n].view(m, n))
    t_p, t_i = dev(d_p, np.float32), None if d_i is None else dev(d_i, np.float32)
    t_m = None if mom is None else dev(mom, np.float64)
    api.seq_select_torch(t_p, t_i, t_m, dev(steps, np.int32), q0, d0, mw, pw, k, dense=dense, ctx=ctx, out=tuple(out))
    ctx.sync()
    for t, size in zip(flat, (m * k, m * k, m * k, m * n)):
        assert (t[size:].cpu().numpy() == GUARD).all(), "a guard word was written"
    got = [t.cpu().numpy().copy() for t in out]
    return got + [None] * (4 - len(got))


def check(ctx, d_p, d_i, mom, steps, q0=0, d0=0, mw=0, pw=2.0, k=1, dense=True, what=""):
    steps = np.ascontiguousarray(steps, np.int32)
    got = run_dev(ctx, d_p, d_i, mom, steps, q0, d0, mw, pw, k, dense)
    want = sq.seq_select(d_p, d_i, mom, steps, q0, d0, mw, pw, k)
    for name, g, w in zip(("idx", "score", "vel", "S"), got, want):
        if g is None:
            continue
        bad = np.argwhere(g.view(np.int64 if g.dtype == np.float64 else np.int32) != w.view(np.int64 if w.dtype == np.float64 else np.int32))
        assert same_bytes(g, w), (what, name, d_p.shape, steps.shape, k, bad[:4].tolist(), [g[tuple(b)] for b in bad[:4]], [w[tuple(b)] for b in bad[:4]])
    return got, want


def table(L, V, seed=0):
    vel = [1, -1, 0.75, -0.75, 0, 1.25, -1.25, 0.5, -0.5, 2, -2, 1.5, -1.5, 0.25, -0.25, 1.75][:V]
    st = sq.seq_steps(L, vel)
    if len(st) < V:                                      # (L = 1: every row is the same) the rows the table asks for, duplicates and all
        st = np.concatenate([st, np.zeros((V - len(st), L), np.int32)])
    return st


LS = 8
SHAPES = [(m, n, LS, 6, 5, 1) for m in (1, 2, LS - 1, LS, LS + 1, R - 1, R, R + 1, 2 * R + 3) for n in (W + 1,)] + \
         [(2 * R + 3, n, LS, 6, 5, 0) for n in (2, 3, W - 1, W, W + 64, 2 * W + 5)] + \
         [(R + 1, W + 1, L, V, k, mw) for L, V, k, mw in ((1, 1, 1, 0), (2, 2, 32, 10), (32, 16, 5, 1), (32, 1, 1, 0), (1, 16, 32, 1), (2, 6, 1, 10))] + \
         [(40, 2 * W + 5, 32, 2, 5, 1), (3, 3, 2, 2, 5, 0), (5, W, 8, 6, 1, W), (5, W + 1, 8, 6, 3, W + 7)]


@pytest.mark.parametrize("m,n,L,V,k,mw", SHAPES)
def test_batch_shapes(ctx, m, n, L, V, k, mw):
    d_p, d_i, mom = inputs(m * 1000 + n + L, m, n)
    got, want = check(ctx, d_p, d_i, mom, table(L, V), mw=mw, k=k, what="shapes")
    cands = (want[3] < np.inf).sum(1)
    if mw >= n:
        assert (got[0] == -1).all() and np.isnan(got[1]).all() and (got[2] == -1).all()
    assert ((got[0] >= 0).sum(1) == np.minimum(cands, k)).all()                          # (uniform scores: no +Inf candidate)


def test_batch_no_rows(ctx):
    idx = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
    d = torch.zeros((0, 5), dtype=torch.float32, device="cuda")
    api.seq_select_torch(d, d, torch.zeros((0, 2, 3), dtype=torch.float64, device="cuda"), dev(table(2, 2), np.int32), k=1, ctx=ctx,
                         out=(idx[:0].view(0, 1), torch.zeros((0, 1), dtype=torch.float64, device="cuda"), idx[:0].view(0, 1)))
    ctx.sync()
    assert (idx.cpu().numpy() == GUARD).all()


def test_batch_many_row_tiles_one_part(ctx):
    """more than 512 row tiles: every workgroup walks all slabs of its rows and writes the outputs itself (no merge launch)"""
    m, n = 512 * R + 4, 2 * W + 5
    d_p, d_i, mom = inputs(77, m, n)
    check(ctx, d_p, d_i, mom, [[0, 1], [0, -1]], mw=1, k=3, dense=False, what="one part")


@pytest.mark.parametrize("name,steps", [("reach 0", [[0, 0, 0, 0]]), ("reach 1", [[0, 1, 1, 1], [0, 0, -1, -1]]),
                                        ("reach 64", [[0, 64, 64, 1], [0, -64, -1, -64], [0, 21, 42, 63]]),
                                        ("standstill row", [[0, 1, 2, 3], [0, 0, 0, 0], [0, -1, -2, -3]]),
                                        ("identical rows", [[0, 1, 2, 3], [0, 1, 2, 3], [0, -1, -2, -3], [0, -1, -2, -3]]),
                                        ("an unusable device row", [[0, 1, 2, 3], [1, 2, 3, 4], [0, 65, 1, 1], [0, -1, -2, -3]])])
def test_batch_step_tables(ctx, name, steps):
    for m, n in ((2 * R + 3, 2 * W + 5), (R, W + 64)):
        d_p, d_i, mom = inputs(len(name) + n, m, n)
        got, want = check(ctx, d_p, d_i, mom, steps, k=5, what=name)
        if name == "identical rows":
            assert set(np.unique(got[2])) <= {0, 2}                                       # the first of two identical rows wins
        if name == "an unusable device row":
            assert set(np.unique(got[2])) <= {0, 3}


def test_batch_row_offsets_and_a_reverse_trajectory_across_the_mask(ctx):
    m, n, mw = 2 * R + 3, W + 64, 10
    d_p, d_i, mom = inputs(5, m, n)
    steps = [[0, 1, 2, 3, 4, 5], [0, -3, -6, -9, -12, -15]]
    for q0, d0 in ((0, 0), (200, 150), (1000, 1000 + W // 2), (5, 0), (2 ** 31 - 100, 2 ** 31 - 1000)):
        got, want = check(ctx, d_p, d_i, mom, steps, q0=q0, d0=d0, mw=mw, k=5, what=("offsets", q0, d0))
    # query 20 against DB rows 0 .. n: the reverse trajectory from a cell below the band runs up through |row - col| < 10 and is dropped
    got, want = check(ctx, d_p, d_i, mom, steps, q0=100, d0=0, mw=mw, k=5)
    i = m - 1
    below = [j for j in range(n) if 100 + i - j >= mw and want[3][i, j] < np.inf]
    crossing = [j for j in below if any(abs((100 + i - l) - (j + 3 * l)) < mw for l in range(6))]
    assert crossing and all(sq.seq_dense(d_p, d_i, mom, np.array(steps, np.int32), 100, 0, mw)[1][i, j] == 0 for j in crossing)


def test_batch_special_values(ctx):
    m, n = 2 * R + 3, W + 64
    d_p, d_i, mom = inputs(9, m, n)
    d_p[3, 40] = np.nan; d_i[4, 300] = np.nan                                            # NaN distances
    d_p[6, 17] = np.inf; d_i[7, 18] = np.inf                                             # +Inf distances: candidates that sort last
    mom[9, 0, 2] = np.nan; mom[10, 1, 1] = np.nan                                        # NaN in mom: the whole row of f is NaN
    d_p[12, :] = np.float32(0.25); mom[12, 0] = sq.row_moments(d_p[12:13])[0]            # a constant row: sd = 0
    assert mom[12, 0, 2] == 0.0
    steps = table(4, 6)
    got, want = check(ctx, d_p, d_i, mom, steps, k=32)
    S = want[3]
    assert np.isinf(S[9]).all() and np.isinf(S[10]).all() and np.isinf(S[12]).all() and (S[6, 17] == np.inf)
    d_p2 = d_p[:, :20].copy(); d_i2 = d_i[:, :20].copy()
    d_p2[6, 17] = np.inf
    mom2 = np.stack([sq.row_moments(np.where(np.isinf(d_p2), np.nan, d_p2)), sq.row_moments(np.where(np.isinf(d_i2), np.nan, d_i2))], 1)
    got, want = check(ctx, d_p2, d_i2, mom2, [[0, 0], [0, 1]], k=20)
    assert np.isinf(got[1][6]).any() and (got[0][6] >= 0).all()                          # +Inf candidates are listed, behind the finite ones
    d_p3 = d_p2.copy(); d_p3[5, 3] = -np.inf
    check(ctx, d_p3, None, None, [[0, 0], [0, 1], [0, -1]], k=20, what="Inf - Inf: a NaN sum drops the velocity")


def test_batch_exact_ties(ctx):
    """an integer grid, one matrix, no normalisation: sums are exact, ties abound - across j (the smaller wins) and across v (the first)"""
    for m, n, L in ((2 * R + 3, 2 * W + 5, 4), (R, W, 8)):
        d_p, _, _ = inputs(21, m, n, with_i=False, grid=3)
        steps = [[0, 1, 2, 3, 4, 5, 6, 7][:L], [0, -1, -2, -3, -4, -5, -6, -7][:L], [0] * L, [0, 1, 1, 2, 2, 3, 3, 4][:L]]
        got, want = check(ctx, d_p, None, None, steps, k=32, what="ties")
        assert (np.diff(got[1], axis=1) == 0).mean() > 0.5 and len(np.unique(got[2])) > 1
        check(ctx, np.ones((m, n), np.float32), None, None, steps, k=5, mw=2, q0=3, what="all equal")


def test_batch_plain_and_dense_forms(ctx):
    m, n = 2 * R + 3, 2 * W + 5
    d_p, d_i, mom = inputs(31, m, n)
    steps = table(8, 6)
    a, _ = check(ctx, d_p, None, None, steps, k=5, mw=3, what="d_i = NULL")
    b, _ = check(ctx, d_p, None, None, steps, k=5, mw=3, dense=False)
    c, _ = check(ctx, d_p, d_i, mom, steps, k=5, mw=3)
    d, _ = check(ctx, d_p, d_i, mom, steps, k=5, mw=3, dense=False)
    for x, y in ((a, b), (c, d)):
        assert all(same_bytes(u, w) for u, w in zip(x[:3], y[:3])) and y[3] is None
    assert not same_bytes(a[1], c[1])


def test_batch_two_runs_and_a_replayed_capture(ctx):
    m, n, k = 2 * R + 3, 2 * W + 5, 5
    d_p, d_i, mom = inputs(41, m, n)
    steps = table(8, 6)
    first = run_dev(ctx, d_p, d_i, mom, steps, mw=2, k=k)
    again = run_dev(ctx, d_p, d_i, mom, steps, mw=2, k=k)
    assert all(same_bytes(x, y) for x, y in zip(first, again))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c2 = _stream_context(0)
        t_p, t_i, t_m, t_s = dev(d_p, np.float32), dev(d_i, np.float32), dev(mom, np.float64), dev(steps, np.int32)
        out = api.seq_select_torch(t_p, t_i, t_m, t_s, 0, 0, 2, 2.0, k, dense=True, ctx=c2)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            api.seq_select_torch(t_p, t_i, t_m, t_s, 0, 0, 2, 2.0, k, dense=True, ctx=c2, out=out)
        for t in out:
            t.zero_()
        g.replay()
        st.synchronize()
        assert all(same_bytes(t.cpu().numpy(), w) for t, w in zip(out, first))
        del g
        c2.close()


def test_host_form_and_matcher_agree_with_the_device_call(ctx):
    m, n, k, mw = 19, 150, 3, 4
    db = synth.sc_database(45, n)
    q, _ = synth.sc_queries(46, db, m)
    steps = api.seq_steps(4, [1, -1, 0])
    mt = Matcher("sc", m, n, ctx=ctx)
    mt.pack_database(torch.from_numpy(db).cuda())
    out = mt.match_sequence(torch.from_numpy(q).cuda(), steps, mw, 2.0, k, dense=True)
    ctx.sync()
    d_p, d_i = (t.cpu().numpy() for t in mt.distances())
    mom = mt._bufs["mom"].cpu().numpy()
    want = sq.seq_select(d_p, d_i, mom, steps, 0, 0, mw, 2.0, k)
    assert all(same_bytes(t.cpu().numpy(), w) for t, w in zip(out, want))
    hidx, hsc, hvel = api.match_topk_seq("sc", q, db, steps, mw, 2.0, k, ctx=ctx)
    assert same_bytes(hidx, want[0]) and same_bytes(hsc, want[1]) and same_bytes(hvel, want[2])
    mt.close()
    dl = Matcher("delight", 4, 12, ctx=ctx)                                              # one matrix: the d_i = NULL form
    g = np.random.default_rng(3)
    dbd, qd = g.random((12 * 16, 256)), g.random((4 * 16, 256))
    dl.pack_database(torch.from_numpy(dbd).cuda())
    o2 = dl.match_sequence(torch.from_numpy(qd).cuda(), steps, 0, 2.0, 2)
    ctx.sync()
    w2 = sq.seq_select(dl.distances()[0].cpu().numpy(), None, None, steps, 0, 0, 0, 2.0, 2)
    assert all(same_bytes(t.cpu().numpy(), w) for t, w in zip(o2, w2))
    h2 = api.match_topk_seq("delight", qd, dbd, steps, 0, 2.0, 2, ctx=ctx)
    assert all(same_bytes(x, w) for x, w in zip(h2, w2))
    dl.close()


@pytest.mark.parametrize("seed,reverse", [(7, False), (8, True)])
def test_alias_scene_on_the_device(ctx, seed, reverse):
    d_p, d_i, mom, truth, aliased = alias_scene(seed, reverse)
    got, _ = check(ctx, d_p, d_i, mom, api.seq_steps(SCENE_L, SCENE_VEL), k=2, dense=False, what="alias scene")
    late = np.arange(len(truth)) >= SCENE_L - 1
    assert (got[0][late, 0] == truth[late]).all()
    single = run_dev(ctx, d_p, d_i, mom, np.zeros((1, 1), np.int32), k=1, dense=False)[0][:, 0]
    assert (single[aliased] != truth[aliased]).all()


def test_the_executable_with_seq_len_and_its_refusals(ctx, tmp_path):
    BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin", "match_signatures")
    m, n, k, mw = 12, 40, 2, 3
    db = synth.sc_database(45, n)
    q, _ = synth.sc_queries(46, db, m)
    h1, h2, out = str(tmp_path / "q.bin"), str(tmp_path / "db.bin"), str(tmp_path / "out.txt")
    api.write_signatures(h1, q)
    api.write_signatures(h2, db)
    base = [BIN, "--type", "sc", "--hist1", h1, "--hist2", h2, "--out", out, "--topk", str(k), "--mask_width", str(mw)]
    r = subprocess.run(base + ["--seq_len", "4", "--seq_vel", "1,-1,0.75,1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "seq_len = 4" in r.stdout and "seq_velocities = 3" in r.stdout
    res = np.loadtxt(out).reshape(m, k, 2)
    widx, wsc, _ = api.match_topk_seq("sc", q, db, api.seq_steps(4, [1, -1, 0.75, 1]), mw, 2.0, k, ctx=ctx)
    assert np.array_equal(res[..., 0].astype(np.int32), widx) and same_bytes(res[..., 1], wsc)      # (%.17g round-trips a double)
    for extra, words in ((["--online", "1"], "cannot be combined"), (["--align_out", str(tmp_path / "a.txt")], "cannot be combined"),
                         (["--devices", "0"], "cannot be combined"),
                         (["--icp_out", str(tmp_path / "i.txt"), "--poses1", "x", "--pts1", "y"], "cannot be combined")):
        r = subprocess.run(base + ["--seq_len", "4"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and words in r.stderr, (extra, r.stderr)
    for args, words in ((["--seq_len", "33"], "--seq_len is 1 .. 32"), (["--seq_len", "32", "--seq_vel", "3"], "reaches beyond 64 rows"),
                        (["--seq_len", "4", "--seq_vel", "1,x"], "comma-separated list of numbers")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and words in r.stderr, (args, r.stderr)


# ---------------------------------------------------------------------------------------------------------------- the online form
def canon(a):
    """every NaN mapped to one pattern (the payload of a produced NaN is not specified)"""
    return np.where(np.isnan(a), np.nan, a)


class OnlineRig:
    def __init__(self, cap, ch, steps, max_k):
        self.ctx = _stream_context(0)
        self.cap, self.ch, self.max_k = cap, ch, max_k
        self.f = api.SequenceFilter(self.ctx, cap, ch, steps, max_k)
        self.model = sq.SeqFilter(cap, ch, steps, max_k)
        self.rows = torch.zeros((ch, cap), dtype=torch.float64, device="cuda")
        self.state = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
        self.emitted = torch.ones(1, dtype=torch.int32, device="cuda")
        self.flat = [torch.zeros(max_k + 8, dtype=dt, device="cuda") for dt in (torch.int32, torch.float64, torch.int32)] + \
                    [torch.zeros(12, dtype=torch.int32, device="cuda")]

    def push(self, rows, count, weights, normalize, mw, k, emitted=None, what=""):
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows, np.float64)))
        self.state[0] = int(count)
        for t in self.flat:
            t.fill_(GUARD)
        out = tuple(t[:k].view(1, k) for t in self.flat[:3]) + (self.flat[3][:4],)
        if emitted is not None:
            self.emitted.fill_(emitted)
        self.f.push_torch(self.rows, self.state, weights, normalize, mw, k, emitted=None if emitted is None else self.emitted, out=out)
        self.ctx.sync()
        for t, size in zip(self.flat, (k, k, k, 4)):
            assert (t[size:].cpu().numpy() == GUARD).all(), "a guard word was written"
        got = [t.cpu().numpy().reshape(-1).copy() for t in out]
        want = self.model.push(rows, count, weights, normalize, mw, k, emitted=emitted)
        for name, g, w in zip(("idx", "score", "vel", "info"), got, want):
            assert same_bytes(g, w), (what, name, count, g, w)
        self.same_state(what)
        return got

    def same_state(self, what=""):
        ring, ids, pushes = self.f.read()
        assert same_bytes(canon(ring), canon(self.model.ring)), (what, "ring")
        assert np.array_equal(ids, self.model.ids) and pushes == self.model.pushes, (what, ids, self.model.ids, pushes, self.model.pushes)

    def close(self):
        self.f.close(); self.ctx.close()


def rows_for(seed, count, cap, ch):
    g = np.random.default_rng(seed)
    return np.where(np.arange(cap) < count, g.uniform(0.1, 1.0, (ch, cap)), g.uniform(5, 6, (ch, cap)))


@pytest.mark.parametrize("ch,normalize,weights", [(1, False, (1.0,)), (1, True, (1.0,)), (2, True, (2.0, 1.0)), (4, True, (2.0, 1.0, 2.0, 1.0))])
def test_online_counts_masks_and_the_switch(ch, normalize, weights):
    L, cap = 4, 300
    rig = OnlineRig(cap, ch, api.seq_steps(L, [1, -1, 0, 0.5]), 8)
    counts = [0, 1, 2, 3, L - 1, L, L + 1, 40, 41, 42, 255, 256, 257, 258, cap - 1, cap]
    for t, n in enumerate(counts):
        got = rig.push(rows_for(100 + t, n, cap, ch), n, weights, normalize, 2 if t % 2 else 0, 1 + t % 8, what=(ch, t))
        assert got[3].tolist() == [1, min(L, t + 1), t + 1, 0]
    before = rig.f.read()
    got = rig.push(rows_for(7, 50, cap, ch), 50, weights, normalize, 0, 3, emitted=0, what="switched off")
    after = rig.f.read()
    assert same_bytes(before[0], after[0]) and same_bytes(before[1], after[1]) and before[2] == after[2] == len(counts)
    assert got[3].tolist() == [0, 0, len(counts), 0] and (got[0] == -1).all() and np.isnan(got[1]).all()
    rig.push(rows_for(8, 60, cap, ch), 60, weights, normalize, 5, 8, emitted=1, what="switched on")
    for scribble, n in ((-5, 0), (cap + 100, cap), (2 ** 31 - 1, cap)):                  # a scribbled count is clamped
        got = rig.push(rows_for(9, n, cap, ch), scribble, weights, normalize, 0, 2, what=("scribbled", scribble))
    r = rows_for(10, 70, cap, ch)
    r[0, 5] = np.nan; r[-1, 9] = np.inf
    rig.push(r, 70, weights, normalize, 0, 8, what="NaN and Inf entries")
    rig.push(rows_for(11, 71, cap, ch), 71, weights, normalize, 80, 4, what="mask >= n")
    rig.f.reset(); rig.model.reset()
    rig.same_state("reset")
    for t, n in enumerate((10, 11, 12)):
        got = rig.push(rows_for(200 + t, n, cap, ch), n, weights, normalize, 1, 8, what=("after reset", t))
        assert got[3].tolist() == [1, t + 1, t + 1, 0]
    rig.close()


def test_online_host_form_large_k_and_refusals():
    cap, L = 600, 3
    steps = api.seq_steps(L, [1, -1])
    rig = OnlineRig(cap, 2, steps, 128)
    for t, n in enumerate((300, 301, 302, 600)):
        rows = rows_for(300 + t, n, cap, 2)
        got = rig.f.push(rows, n, (2.0, 1.0), True, 3, 128 if t % 2 else 100)
        want = rig.model.push(rows, n, (2.0, 1.0), True, 3, 128 if t % 2 else 100)
        assert all(same_bytes(g, w) for g, w in zip(got, want)), t
        rig.same_state(("host form", t))
    for kw, words in ((dict(k=0), "k=0 outside"), (dict(k=129), "k=129 outside"), (dict(mask_width=-1), "mask_width=-1"),
                      (dict(weights=(np.inf, 1.0)), "weights[0] is not finite"), (dict(normalize=False), "normalize=0 needs channels == 1")):
        args = dict(rows=rows_for(1, 5, cap, 2), count=5, weights=(2.0, 1.0), normalize=True, mask_width=0, k=1)
        args.update(kw)
        with pytest.raises(_lib.PRError, match=words.replace("[", r"\[").replace("]", r"\]")):
            rig.f.push(**args)
    rig.same_state("refused calls change nothing")
    rig.close()


def test_online_read_with_null_outputs():
    """pr_seqmatch_read with each output alone and with none: what was passed equals, byte for byte, that of the read with all three"""
    L, cap = 4, 300
    rig = OnlineRig(cap, 1, api.seq_steps(L, [1, -1, 0, 0.5]), 8)
    for t, n in enumerate((40, 41)):
        rig.push(rows_for(100 + t, n, cap, 1), n, (1.0,), False, 0, 2, what=("read", t))
    ring, ids, pushes = rig.f.read()
    assert pushes == 2
    lib, h = rig.ctx.lib, rig.f.h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    r2, i2, n2 = np.full_like(ring, GUARD), np.full_like(ids, GUARD), C.c_int32(GUARD)
    rig.ctx.check(lib.pr_seqmatch_read(h, vp(r2), None, None))
    rig.ctx.check(lib.pr_seqmatch_read(h, None, vp(i2), None))
    rig.ctx.check(lib.pr_seqmatch_read(h, None, None, C.byref(n2)))
    rig.ctx.check(lib.pr_seqmatch_read(h, None, None, None))
    assert same_bytes(r2, ring) and same_bytes(i2, ids) and n2.value == pushes
    rig.close()


def test_the_drive_with_a_captured_sequence_push(seq07):
    """push -> SC generate -> match(rows=) -> SequenceFilter.push_torch(rows, db.state) -> append, per pose: eagerly, and as ONE graph
    captured behind the first eager step; the same bytes, and the restatement's over the rows the match wrote"""
    KCAP, K, MASK, L = 112, 2, 5, 4
    steps = api.seq_steps(L, [1, -1, 0])
    P = len(seq07["pid"])

    def run(captured):
        res = []
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ctx = _stream_context(0)
            lib = ctx.lib
            p = lambda t: t.data_ptr()
            pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
            it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
            sig = torch.zeros((1, 2400), dtype=torch.float64, device="cuda")
            rows = torch.zeros((2, KCAP), dtype=torch.float64, device="cuda")
            mout = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"))
            sout = (torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda"),
                    torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
            oinfo = torch.zeros(4, dtype=torch.int32, device="cuda")
            win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
            odb = api.OnlineDatabase(ctx, "sc", KCAP, max_k=K)
            seq = api.SequenceFilter(ctx, KCAP, 2, steps, K)
            out = win.empty_out()

            def step():
                win.push_torch(pose, x, it, n, out=out)
                ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig)))
                odb.match_torch(sig, MASK, 2.0, K, emitted=out["info"], out=mout, rows=rows)
                seq.push_torch(rows, odb.state, (2.0, 1.0), True, MASK, K, emitted=out["info"], out=sout)
                odb.append_torch(sig, emitted=out["info"], info=oinfo)

            g = None
            for i in range(P):
                w, hx, hit, kk, pid = pose_inputs(seq07, i)
                pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit)); n.fill_(kk)
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
                res.append(dict(rows=rows.cpu().numpy(), emitted=int(out["info"].cpu().numpy()[0]), count=int(oinfo.cpu().numpy()[1]),
                                **{nm: t.cpu().numpy().reshape(-1) for nm, t in zip(("idx", "score", "vel", "info"), sout)}))
            state = seq.read()
            del g
            seq.close(); odb.close(); win.close(); ctx.close()
        return res, state

    got, gstate = run(True)
    want, wstate = run(False)
    model = sq.SeqFilter(KCAP, 2, steps, K)
    pushed = 0
    for i, (a, b) in enumerate(zip(got, want)):
        for name in ("rows", "idx", "score", "vel", "info"):
            assert same_bytes(a[name], b[name]), (i, name)
        on = a["emitted"] != 0
        ref = model.push(a["rows"], max(a["count"], 0), (2.0, 1.0), True, MASK, K, emitted=None if on else 0)
        for name, w in zip(("idx", "score", "vel", "info"), ref):
            assert same_bytes(a[name], w), (i, name, a[name], w)
        pushed += on
    assert pushed == 110 and gstate[2] == wstate[2] == model.pushes == 110
    assert same_bytes(canon(gstate[0]), canon(wstate[0])) and same_bytes(canon(gstate[0]), canon(model.ring)) and np.array_equal(gstate[1], model.ids)
    late = [a for a in got if a["info"][0] and a["count"] >= MASK + K + L]
    assert late and all((a["idx"] >= 0).all() and (a["idx"] <= a["count"] - MASK).all() for a in late)
