"""The exact-row resolution (exact_row.hip) at the metric DB size, n = 100 000, and at a ragged n = 99 997 (not a multiple of the
8-entry tile; uneven slice bounds and shard sizes).  Below n ~ 8000 every exact-row kernel runs its tile loop once, combines partials of
one tile each and selects from ONE row slice: the paths checked here - the strided tile loops, the combine of 256 / 512 / 2048 multi-tile
partials, the P = 8 / 64 row slices and their merge, the mask across slice and shard boundaries - only run at this size.

Near-copy clusters (helpers.near_copy_clusters) whose members sit on both sides of every slice, shard and end boundary of both sizes
(helpers.slice_edges / cluster_spots), with exact duplicates (a tie only the index breaks) and members next to the query's own row (the
mask).  Reference: the CPU oracle's full fp64 rows of the queries 0 .. 129 and every clustered one, fused and ranked in numpy."""
import time

import numpy as np
import pytest
import torch

import helpers
from so_dso_place_recognition_amd import _lib, api, synth
from test_gpu_configs import oracle_rows, topk_rows, zscore_rows

pytestmark = pytest.mark.gpu

N, NR, M = 100_000, 99_997, 256          # the metric size, the ragged one, queries per call
COPIES, DUPS, R = 40, 12, 24             # cluster members (of them exact copies), clustered queries
SEEDS = {"sc": (45, 46), "m2dp": (43, 44)}
F16_TOL = (3e-2, 1e-3)                   # PR_SC_ARITH_F16 keeps its own score bound (test_gpu_configs: the cluster test)


class Case:
    """One DB of N entries with R clustered queries among M, the oracle's rows of the sampled queries and their reference top-k."""

    def __init__(self, type_):
        t0 = time.time()
        self.type = type_
        db_seed, q_seed = SEEDS[type_]
        gen = synth.sc_database_torch if type_ == "sc" else synth.m2dp_database_torch
        db = gen(db_seed, N).cpu().numpy()
        _, planted = (synth.sc_queries if type_ == "sc" else synth.m2dp_queries)(q_seed, db, M)
        once = [t for t in range(M) if (planted == planted[t]).sum() == 1 and planted[t] < NR - 3]
        rows = [t for t in range(3, M, 10) if t in once][:R]
        assert len(rows) == R
        pri = [N * s // 8 for s in range(1, 8)] + [NR * s // 8 for s in range(1, 8)]          # what each row's top entries straddle first
        pri += [n * g // 3 for n in (N, NR) for g in (1, 2)] + [N, NR]
        pri += [b for n in (N, NR) for b in helpers.slice_edges(n, slices=(8, 8))]           # shard-local slices
        pri += helpers.slice_edges(N) + helpers.slice_edges(NR)
        edges = list(dict.fromkeys(pri))
        top = {r: [N - M + t - 99, N - M + t - 100] for r, t in enumerate(rows)}            # masked / just not masked in a q_row0 = N - M call
        dup = {r: [t + 99, t + 100] for r, t in enumerate(rows)}                             # ... in a q_row0 = 0 call
        spots, self.placed = helpers.cluster_spots(N, rows, COPIES, DUPS, planted, edges, top, dup)
        self.db, self.q, self.planted, self.members = helpers.near_copy_clusters(type_, N, M, rows, COPIES, db_seed=db_seed, q_seed=q_seed,
                                                                                 spots=spots, dups=DUPS, db=db)
        self.spots = spots
        self.rows = np.array(rows)
        self.sample = np.union1d(rows, np.arange(130))                                        # (every query of the m = 130 calls)
        self.cl = np.isin(self.sample, rows)                                                  # the sample's clustered queries
        t1 = time.time()
        self.dp, self.di = oracle_rows(type_, self.query_rows(self.sample), [self.db[c:c + 25_000 * self.div] for c in range(0, len(self.db), 25_000 * self.div)])
        self.oracle_s = time.time() - t1
        print(f"\n{type_}: case built in {t1 - t0:.1f} s, oracle rows {self.dp.shape} in {self.oracle_s:.1f} s")
        oi, _ = self.ref(N, 0, 5)
        for i in np.flatnonzero(self.cl):                                                   # the five best of a clustered row are members
            assert set(oi[i].tolist()) <= set(self.members[int(self.sample[i])].tolist())

    @property
    def div(self):
        return 1 if self.type == "sc" else 4

    def query_rows(self, ts):
        return self.q.reshape(M, self.div, -1)[np.asarray(ts)].reshape(-1, self.q.shape[1])

    def fused(self, n, extra=None):
        dp, di = self.dp[:, :n], self.di[:, :n]
        if extra is not None:
            dp, di = np.concatenate([dp, extra[0]], 1), np.concatenate([di, extra[1]], 1)
        return 2.0 * zscore_rows(dp) + zscore_rows(di)

    def ref(self, n, mask, k, q_row0=0, f=None):
        f = self.fused(n) if f is None else f
        return topk_rows(f, self.sample + q_row0, mask, k)

    def check(self, idx, sc, ref, what, f16=False, resolved=None):
        """indices bit-exact on the sample; resolved rows (default: the clustered ones) within 1e-9, the others within the fp32 model."""
        oi, osc = ref
        idx, sc = np.asarray(idx)[self.sample], np.asarray(sc)[self.sample]
        bad = np.flatnonzero((idx != oi).any(1))
        assert len(bad) == 0, (what, self.sample[bad][:8], idx[bad][:2], oi[bad][:2])
        if f16:
            assert (np.abs(sc - osc) <= F16_TOL[0] + F16_TOL[1] * np.abs(osc)).all(), what
            return
        ex = self.cl if resolved is None else resolved
        assert np.abs(sc[ex] - osc[ex]).max() < 1e-9, (what, np.abs(sc[ex] - osc[ex]).max())
        fin = np.isfinite(osc[~ex])
        assert (np.abs(sc[~ex] - osc[~ex])[fin] <= helpers.score_tol(osc[~ex][fin])).all(), what

    def device_db(self, n):
        return torch.from_numpy(self.db[:n * self.div]).cuda()


_CASES = {}


@pytest.fixture(scope="module")
def case():
    def get(type_):
        if type_ not in _CASES:
            _CASES[type_] = Case(type_)
        return _CASES[type_]
    yield get
    _CASES.clear()


def _stream_ctx(**kw):
    return api.Context(0, stream=int(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream), **kw)


# ------------------------------------------------------------------------------------------------ 1. near-copy clusters, m = 256
@pytest.mark.parametrize("n", [N, NR])
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_clusters_host_calls(case, type_, n):
    """api.match_topk, m = 256 (P = 8 row slices), every arithmetic; k 1 / 5, mask 0 / 100 (members at |t - j| = 99 and 100)."""
    c = case(type_)
    for k in (1, 5):
        for mask in (0, 100):
            ref = c.ref(n, mask, k)
            for arith in ("f16x2", "f32", "f16"):
                ctx = api.Context(0, sc_arith=arith)
                idx, sc = api.match_topk(type_, c.q, c.db[:n * c.div], mask, 2.0, k, ctx=ctx)
                w = ctx.take_warnings()
                ctx.close()
                c.check(idx, sc, ref, (n, k, mask, arith), f16=arith == "f16")
                if arith != "f16":        # (its k + 56 candidates can hold a whole cluster: the margin check may pass without exact rows)
                    assert w & _lib.WARN_ORDER_RESOLVED, (n, k, mask, arith)


@pytest.mark.parametrize("n", [N, NR])
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_clusters_device_matcher(case, type_, n):
    """Matcher, m = 256: exact_order=True (the synchronous multi-pass form: it reads the flagged count back) and "async"; q_row0 = 0 and
    q_row0 = n - m (the mask window over the DB's last tile and slice); exact_order=False must be wrong for some clusters (teeth)."""
    from so_dso_place_recognition_amd.matcher import Matcher
    c = case(type_)
    mt = Matcher(type_, M, n, ctx=_stream_ctx())
    mt.pack_database(c.device_db(n))
    tq = torch.from_numpy(c.q).cuda()
    for k in (1, 5):
        for mask, q_row0 in ((0, 0), (100, 0), (100, n - M)):
            ref = c.ref(n, mask, k, q_row0)
            what = (n, k, mask, q_row0)
            i0, _ = mt.match(tq, mask, 2.0, k, q_row0=q_row0, exact_order=False)
            i0 = i0.cpu().numpy()
            assert ((i0[c.sample] != ref[0]).any(1) & c.cl).sum() >= 3, what          # the candidate list alone is wrong for clusters
            mt.take_warnings()
            idx, sc = mt.match(tq, mask, 2.0, k, q_row0=q_row0)
            assert (mt.take_warnings() & _lib.WARN_ORDER_RESOLVED) and mt.resolved >= len(c.rows), (what, mt.resolved)
            c.check(idx.cpu().numpy(), sc.cpu().numpy(), ref, what + ("sync",))
            idx, sc = mt.match(tq, mask, 2.0, k, q_row0=q_row0, exact_order="async")
            w = mt.take_warnings()
            assert (w & _lib.WARN_ORDER_RESOLVED) and not (w & _lib.WARN_ORDER_UNRESOLVED), what
            c.check(idx.cpu().numpy(), sc.cpu().numpy(), ref, what + ("async",))
    mt.close()


@pytest.mark.parametrize("n", [N, NR])
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_clusters_group_of_three_shards(case, type_, n):
    """pr_group with three virtual shards: members straddle the shard starts and the slices inside every shard."""
    c = case(type_)
    g = api.Group([0, 0, 0])
    g.set_database(type_, c.db[:n * c.div])
    for k in (1, 5):
        for mask in (0, 100):
            gi, gs = g.match_topk(c.q, mask, 2.0, k)
            assert g.last_flagged >= len(c.rows) and (g.take_warnings() & _lib.WARN_ORDER_RESOLVED), (n, k, mask, g.last_flagged)
            c.check(gi, gs, c.ref(n, mask, k), (n, k, mask, "group"))
    g.close()


# ------------------------------------------------------------------------------------------------ 2. online calls
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_online_calls_at_scale(case, type_):
    """m = 1 and m = 8 clustered queries against n = 100 000: P = 64 row slices, the direct form's NB = 256 cap."""
    from so_dso_place_recognition_amd.matcher import Matcher
    c = case(type_)
    mt = Matcher(type_, 8, N, ctx=_stream_ctx())
    mt.pack_database(c.device_db(N))
    for mq in (1, 8):
        ts = c.rows[:mq]
        pos = np.searchsorted(c.sample, ts)
        q = c.query_rows(ts)
        for k in (1, 5):
            oi, osc = topk_rows(c.fused(N)[pos], ts, 0, k)
            ctx = api.Context(0)
            idx, sc = api.match_topk(type_, q, c.db, 0, 2.0, k, ctx=ctx)
            assert ctx.take_warnings() & _lib.WARN_ORDER_RESOLVED, (mq, k)
            ctx.close()
            assert np.array_equal(idx, oi) and np.abs(sc - osc).max() < 1e-9, (mq, k, idx, oi)
            idx, sc = mt.match(torch.from_numpy(q).cuda(), 0, 2.0, k)
            assert mt.take_warnings() & _lib.WARN_ORDER_RESOLVED, (mq, k)
            idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
            assert np.array_equal(idx, oi) and np.abs(sc - osc).max() < 1e-9, (mq, k, idx, oi)
    mt.close()


# ------------------------------------------------------------------------------------------------ 3. every query through the exact row
@pytest.mark.parametrize("form", ["spectral", "direct"])
def test_every_query_through_the_exact_row(case, form, monkeypatch):
    """PR_FORCE_ORDER_FLAGS=1, m = 130 (three passes of 64): every score is the oracle's double to 1e-9 - the exact row statistics over
    100 000 entries (partials of 256 / 512 / 2048 workgroups, combined; across the three shards of a pr_group), SC, M2DP and fused."""
    from so_dso_place_recognition_amd.matcher import FusedMatcher, Matcher
    monkeypatch.setenv("PR_FORCE_ORDER_FLAGS", "1")                 # (both read when a context is made)
    if form == "direct":
        monkeypatch.setenv("PR_XROW", "direct")
    m, k, mask = 130, 3, 100
    s_sc, s_m2 = case("sc"), case("m2dp")
    sel = s_sc.sample < m
    assert sel.sum() == m and np.array_equal(s_sc.sample[sel], s_m2.sample[sel])
    for c in (s_sc, s_m2):
        f = c.fused(N)
        oi, osc = topk_rows(f[sel], c.sample[sel], mask, k)
        qm = c.q[:m * c.div]
        ctx = api.Context(0)
        idx, sc = api.match_topk(c.type, qm, c.db, mask, 2.0, k, ctx=ctx)
        assert ctx.take_warnings() & _lib.WARN_ORDER_RESOLVED
        ctx.close()
        _cmp(idx, sc, c.sample[sel], oi, osc, (form, c.type, "host"))
        mt = Matcher(c.type, m, N, ctx=_stream_ctx())
        mt.pack_database(c.device_db(N))
        idx, sc = mt.match(torch.from_numpy(qm).cuda(), mask, 2.0, k)
        assert mt.resolved == m
        _cmp(idx.cpu().numpy(), sc.cpu().numpy(), c.sample[sel], oi, osc, (form, c.type, "matcher"))
        mt.close()
        g = api.Group([0, 0, 0])
        g.set_database(c.type, c.db)
        gi, gs = g.match_topk(qm, mask, 2.0, k)
        assert g.last_flagged == m
        _cmp(gi, gs, c.sample[sel], oi, osc, (form, c.type, "group"))
        g.close()
    f = s_sc.fused(N) + s_m2.fused(N)                                 # the fused score: both types' z-scores (weights p, 1, p, 1)
    oi, osc = topk_rows(f[sel], s_sc.sample[sel], mask, k)
    fm = FusedMatcher(m, N, ctx=_stream_ctx())
    fm.pack_database(s_sc.device_db(N), s_m2.device_db(N))
    idx, sc = fm.match(torch.from_numpy(s_sc.q[:m]).cuda(), torch.from_numpy(s_m2.q[:4 * m]).cuda(), mask, 2.0, k)
    _cmp(idx.cpu().numpy(), sc.cpu().numpy(), s_sc.sample[sel], oi, osc, (form, "fused"))
    fm.close()


def _cmp(idx, sc, ts, oi, osc, what):
    """Every compared score fp64 throughout: the oracle's to 1e-9."""
    idx, sc = np.asarray(idx)[ts], np.asarray(sc)[ts]
    assert np.array_equal(idx, oi), (what, idx[(idx != oi).any(1)][:2], oi[(idx != oi).any(1)][:2])
    assert np.abs(sc - osc).max() < 1e-9, (what, np.abs(sc - osc).max())


# ------------------------------------------------------------------------------------------------ 4. a growing DB
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_growing_db_at_scale(case, type_):
    """Matcher with room for 110 000 entries: reserve_database with the first 99 000, append_database up to 100 000 and past it with
    500 more - among them four more members of every cluster, two beyond each end of its progression: the cluster's best is then an
    appended row, which the exact rows must read from the growing store."""
    from so_dso_place_recognition_amd.matcher import Matcher
    c = case(type_)
    d = c.div
    extra_n = 500
    extra = (synth.sc_database(SEEDS[type_][0], extra_n, first=N) if type_ == "sc" else synth.m2dp_database(SEEDS[type_][0], extra_n, first=N))
    rng = np.random.default_rng(9)
    where = rng.choice(extra_n - 1, size=4 * R - 1, replace=False).tolist() + [extra_n - 1]       # (the last row of the DB among them)
    L = COPIES - DUPS
    for r, t in enumerate(c.rows):
        e = c.db[d * c.planted[t]: d * c.planted[t] + d]
        v = c.db[d * c.spots[r, COPIES - 1]: d * c.spots[r, COPIES - 1] + d] - e               # the progression's step times L
        for j, a in enumerate((1 + 1 / L, 1 + 2 / L, -1 / L, -2 / L)):
            p = where[4 * r + j]
            extra[d * p: d * p + d] = e + a * v
    nf = N + extra_n
    ex = oracle_rows(type_, c.query_rows(c.sample), [extra])
    f = c.fused(N, ex)
    oi, _ = topk_rows(f, c.sample, 0, 1)
    assert (oi[c.cl, 0] >= N).sum() >= R * 3 // 4, oi[c.cl, 0]                              # teeth: the best is an appended row
    mt = Matcher(type_, M, 110_000, ctx=_stream_ctx())
    mt.reserve_database(torch.from_numpy(c.db[:99_000 * d]).cuda())
    for lo in range(99_000, N, 250):
        mt.append_database(torch.from_numpy(c.db[lo * d:(lo + 250) * d]).cuda())
    mt.append_database(torch.from_numpy(extra[:200 * d]).cuda())
    mt.append_database(torch.from_numpy(extra[200 * d:]).cuda())
    assert mt.n == nf
    tq = torch.from_numpy(c.q).cuda()
    for k in (1, 5):
        for mask, q_row0 in ((0, 0), (100, nf - M)):
            ref = c.ref(nf, mask, k, q_row0, f=f)
            idx, sc = mt.match(tq, mask, 2.0, k, q_row0=q_row0)
            assert (mt.take_warnings() & _lib.WARN_ORDER_RESOLVED) and mt.resolved >= len(c.rows), (k, mask, mt.resolved)
            c.check(idx.cpu().numpy(), sc.cpu().numpy(), ref, (nf, k, mask, q_row0, "grown"))
    mt.close()
