"""Every selection regime of bow_score_kernel against the CPU oracle, for both workgroup sizes (PR_BOW_THREADS = 64 | 256; the LDS
list holds 8 x threads survivors: 512 | 2048), at n = 3000 > both lists:
  listed        queries sharing words with many rows: every element <= tau fits the list;
  tie overflow  queries of 0 - 2 words (more than the list ties at d = 1) and masks that leave only +Inf, or fewer than k finite entries:
                the elements below tau, then the ties in index order tile by tile;
  k sweeps      64 threads and k = 128 > 64 thread minima: tau = +Inf, more finite elements than the 512-entry list;
and NaN distances (DB weights NaN on shared words) never selected.  Also: a captured match refuses to replay once the DB changed, the
host forms name themselves in their errors, and two ranks on one GPU (gloo) merge to the unsharded answer."""
import os
import sys

import numpy as np
import pytest

import oracle_lib
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import BowMatcher

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_rows(rng, n, cols, vocab, lo, hi, nan_w):
    out = -np.ones((2 * n, cols))
    for r in range(n):
        k = int(rng.integers(lo, hi + 1))
        ids = np.sort(rng.choice(vocab, size=k, replace=False)).astype(np.float64)
        w = rng.normal(0.1, 0.2, k)
        w[rng.random(k) < nan_w] = np.nan
        out[2 * r, :k] = ids
        out[2 * r + 1, :k] = w
    return out


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def oracle_topk(h1, h2, mask_width, k, q_row0=0, db_row0=0):
    d = oracle_lib.bow_distance(h1, h2)
    m, n = d.shape
    gi = q_row0 + np.arange(m)[:, None]
    gj = db_row0 + np.arange(n)[None, :]
    d = np.where(np.abs(gi - gj) < mask_width, np.inf, d)
    rc, idx, sc = oracle_lib.select_topk(d, 0, k)
    assert rc == 0
    return np.where(idx >= 0, idx + db_row0, -1).astype(np.int32), sc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


N, COLS, VOCAB = 3000, 40, 300


def data():
    rng = np.random.default_rng(77)
    db = random_rows(rng, N, COLS, VOCAB, 5, 30, nan_w=0.03)            # ~ 60 rows per word: shared words, some with NaN weights
    q = np.concatenate([random_rows(rng, 12, COLS, VOCAB, 10, 39, nan_w=0.02),   # many touched entries
                        random_rows(rng, 6, COLS, VOCAB, 0, 0, nan_w=0.0),       # no word: every entry ties at d = 1
                        random_rows(rng, 8, COLS, VOCAB, 1, 2, nan_w=0.0)])      # 1 - 2 words: > 2048 ties at d = 1
    return db, q


@pytest.mark.parametrize("threads", ["64", "256"])
@pytest.mark.parametrize("k", [1, 5, 128])
def test_selection_regimes_equal_the_oracle(monkeypatch, threads, k):
    monkeypatch.setenv("PR_BOW_THREADS", threads)
    db, q = data()
    d = oracle_lib.bow_distance(q, db)
    assert np.isnan(d).any() and (d == 1.0).sum(1).max() > 2048
    mt = BowMatcher(q.shape[0] // 2, N, COLS, VOCAB)
    mt.pack_database(dev(db))
    dq = dev(q)
    # (mask, q_row0): none; all +Inf (every entry masked); fewer than k finite entries (50 per query); a band in the middle
    for mw, q0 in ((0, 0), (N, 0), (N - 50, 0), (700, 1500)):
        idx, sc = mt.match(dq, mask_width=mw, k=k, q_row0=q0)
        oi, osc = oracle_topk(q, db, mw, k, q_row0=q0)
        assert np.array_equal(idx.cpu().numpy(), oi) and bits_equal(sc.cpu().numpy(), osc), (threads, k, mw, q0)
    # shards of one DB give the same merged lists (db_row0 in the mask and the indices)
    parts = []
    for r0, r1 in ((0, 1700), (1700, N)):
        sh = BowMatcher(q.shape[0] // 2, r1 - r0, COLS, VOCAB)
        sh.pack_database(dev(db[2 * r0:2 * r1]))
        parts.append(sh.match(dq, mask_width=700, k=k, db_row0=r0, q_row0=1500))
        sh.close()
    mi, ms = mt.merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
    oi, osc = oracle_topk(q, db, 700, k, q_row0=1500)
    assert np.array_equal(mi.cpu().numpy(), oi) and bits_equal(ms.cpu().numpy(), osc)
    mt.close()


@pytest.mark.parametrize("threads", ["64", "256"])
def test_host_forms_and_their_errors(monkeypatch, threads):
    monkeypatch.setenv("PR_BOW_THREADS", threads)
    db, q = data()
    ctx = api.Context(0)
    for k in (5, 128):
        idx, sc = api.bow_match_topk(q, db, 0, k, ctx=ctx)
        oi, osc = oracle_topk(q, db, 0, k)
        assert np.array_equal(idx, oi) and bits_equal(sc, osc), k
    assert bits_equal(api.bow_distance_f64(q, db, ctx=ctx), oracle_lib.bow_distance(q, db))
    bad = db[:10].copy()
    bad[6, :3] = [4, 2, 9]                                                 # row 3: descending ids
    for fn, call in (("pr_bow_match_topk_f64", lambda: api.bow_match_topk(q, bad, 0, 1, ctx=ctx)),
                     ("pr_bow_distance_f64", lambda: api.bow_distance_f64(q, bad, ctx=ctx))):
        with pytest.raises(_lib.PRError) as e:
            call()
        assert e.value.code == _lib.PR_EINVAL and f"{fn}: BoW row 3 " in str(e.value), str(e.value)
    ctx.close()


def test_capture_refuses_a_stale_graph():
    db, q = data()
    m = q.shape[0] // 2
    mt = BowMatcher.on_new_stream(m, N, COLS, VOCAB)
    with torch.cuda.stream(mt.stream):
        mt.reserve_database(dev(db[:2 * 2000]))
        static = dev(q)
    mt.stream.synchronize()
    cap = mt.capture(static, k=5)
    gi, gs = cap.run(dev(q))
    oi, osc = oracle_topk(q, db[:2 * 2000], 0, 5)
    assert np.array_equal(gi.cpu().numpy(), oi) and bits_equal(gs.cpu().numpy(), osc)
    with torch.cuda.stream(mt.stream):
        mt.append_database(dev(db[2 * 2000:]))
    with pytest.raises(RuntimeError, match="capture again"):
        cap.run(dev(q))
    cap2 = mt.capture(static, k=5)
    gi, gs = cap2.run(dev(q))
    oi, osc = oracle_topk(q, db, 0, 5)
    assert np.array_equal(gi.cpu().numpy(), oi) and bits_equal(gs.cpu().numpy(), osc)
    del cap, cap2
    mt.close()


def _rank(rank, world, port, k, mw, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch as T
    import torch.distributed as dist
    from so_dso_place_recognition_amd.matcher import BowMatcher as BM
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    T.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    db, q = data()
    lo, hi = N * rank // world, N * (rank + 1) // world
    mt = BM(q.shape[0] // 2, hi - lo, COLS, VOCAB)
    mt.pack_database(T.from_numpy(db[2 * lo:2 * hi]).cuda())
    idx, sc = mt.match(T.from_numpy(q).cuda(), mask_width=mw, k=k, db_row0=lo, q_row0=100)   # the plain path of sharded_topk over gloo
    T.cuda.synchronize()
    if rank == 0:
        out.put((idx.cpu().numpy(), sc.cpu().numpy()))
    mt.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_over_gloo():
    import multiprocessing as mp
    import queue as _q
    k, mw, world = 5, 40, 2
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = 29700 + os.getpid() % 1000
    procs = [ctx.Process(target=_rank, args=(r, world, port, k, mw, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = None
    for _ in range(240):
        try:
            res = out.get(timeout=1)
            break
        except _q.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(timeout=120)
    assert res is not None and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    db, q = data()
    oi, osc = oracle_topk(q, db, mw, k, q_row0=100)
    assert np.array_equal(res[0], oi) and bits_equal(res[1], osc)
