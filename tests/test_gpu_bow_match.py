"""The inverted-file BoW matcher (bow_match.hip: pr_bow_db_*, pr_bow_match_topk_*, pr_bow_distance_f64, matcher.BowMatcher) against
the CPU oracle (oracle_lib.bow_distance + select_topk on the global matrix): distances and top-k scores equal bit for bit, the fp64 order
below fp32 resolution, growth == bulk build across folds, shards, graph capture, rejection of non-conforming rows, 100k rows, and
the path from ORB descriptors through bow_generate_torch without a host copy."""
import numpy as np
import pytest

import oracle_lib
from resident_fuzz_cases import bits_equal, oracle_select
from so_dso_place_recognition_amd import _lib, api, synth
from so_dso_place_recognition_amd.matcher import BowMatcher, merge_topk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def random_rows(rng, n, cols, vocab, every=None, lo=0, hi=None, nan_w=0.02):
    """Conforming rows with every kind of end (-1, -7.5, NaN, a full row) and weights 0 / negative / NaN; `every`: a word in every row."""
    hi = cols if hi is None else hi
    out = -np.ones((2 * n, cols))
    base = 0 if every is None else 1
    for r in range(n):
        k = int(rng.integers(lo, hi + 1))
        ids = np.sort(rng.choice(np.arange(base, vocab), size=min(k, vocab - base), replace=False)).astype(np.float64)
        if every is not None:
            ids = np.concatenate([[float(every)], ids])[:cols]
        k = len(ids)
        w = rng.normal(0.1, 0.2, k)
        w[rng.random(k) < 0.1] = 0.0
        w[rng.random(k) < nan_w] = np.nan
        out[2 * r, :k] = ids
        out[2 * r + 1, :k] = w
        if k < cols:
            out[2 * r, k] = rng.choice([-1.0, -7.5, np.nan])
            out[2 * r, k + 1:] = rng.integers(-3, vocab, cols - k - 1)
    return out


def oracle_topk(h1, h2, mask_width, k, q_row0=0, db_row0=0):
    return oracle_select(oracle_lib.bow_distance(h1, h2), mask_width, k, q_row0, db_row0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("cols", [2, 8, 120, 4000])
def test_distances_bit_for_bit(ctx, cols):
    rng = np.random.default_rng(cols)
    vocab = 5000 if cols == 4000 else 300
    for m, n in ((1, 1), (7, 33)):
        h1 = random_rows(rng, m, cols, vocab)
        h2 = random_rows(rng, n, cols, vocab, every=0 if cols > 2 else None)
        got = api.bow_distance_f64(h1, h2, ctx=ctx)
        assert bits_equal(got, oracle_lib.bow_distance(h1, h2)), (m, n, cols)
    # rows of 0 words and rows filling every column (the last word is never read)
    h1 = np.array([[-1, -1, -1], [-1, -1, -1], [1, 2, 3], [0.2, 0.3, 0.5]], np.float64)
    h2 = np.array([[3, -1, -1], [0.5, -1, -1], [1, 2, 3], [0.1, 0.1, 0.8]], np.float64)
    got = api.bow_distance_f64(h1, h2, ctx=ctx)
    assert bits_equal(got, oracle_lib.bow_distance(h1, h2)) and got[1, 0] == 1.0 and got[0, 1] == 1.0


@pytest.mark.parametrize("k", [1, 5, 40, 128])
def test_topk_exact(ctx, k):
    rng = np.random.default_rng(100 + k)
    cols, vocab = 64, 150
    h2 = random_rows(rng, 300, cols, vocab, every=0, nan_w=0.0)
    h1 = np.concatenate([random_rows(rng, 30, cols, vocab, nan_w=0.0), random_rows(rng, 10, cols, vocab, lo=0, hi=2, nan_w=0.0)])
    for mw in (0, 4, 300):
        idx, sc = api.bow_match_topk(h1, h2, mw, k, ctx=ctx)
        oi, osc = oracle_topk(h1, h2, mw, k)
        assert np.array_equal(idx, oi) and bits_equal(sc, osc), (k, mw)
    # offsets, k > n, queries that touch fewer than k entries (the d = 1 fill-ins in index order)
    mt = BowMatcher(40, 300, cols, vocab, ctx=ctx)
    mt.pack_database(dev(h2[:60]))
    for q0, d0, mw in ((0, 0, 0), (17, 5, 4), (250, 230, 30)):
        idx, sc = mt.match(dev(h1), mask_width=mw, k=k, db_row0=d0, q_row0=q0)
        oi, osc = oracle_topk(h1, h2[:60], mw, k, q0, d0)
        assert np.array_equal(idx.cpu().numpy(), oi) and bits_equal(sc.cpu().numpy(), osc), (k, q0, d0, mw)
    mt.close()


def test_order_below_fp32_resolution(ctx):
    n = 20
    h2 = -np.ones((2 * n, 4))
    h2[0::2, 0] = 7
    h2[1::2, 0] = 0.5 - (n - np.arange(n)) * 1e-12          # d = 0.5 + delta_j: fp64 order is the reverse of the index order
    h1 = np.array([[7, -1, -1, -1], [0.5, -1, -1, -1]], np.float64)
    idx, sc = api.bow_match_topk(h1, h2, 0, 5, ctx=ctx)
    oi, osc = oracle_topk(h1, h2, 0, 5)
    assert np.array_equal(idx, oi) and bits_equal(sc, osc)
    assert idx[0].tolist() == [n - 1, n - 2, n - 3, n - 4, n - 5]
    fi, fs = api.match_topk("bow", h1, h2, 0, k=5, ctx=ctx)  # the fp32 all-pairs path: one value, index order
    assert fi[0].tolist() == [0, 1, 2, 3, 4] and len(set(fs[0].tolist())) == 1


def test_growth_equals_bulk(monkeypatch):
    monkeypatch.setenv("PR_BOW_TAIL_ROWS", "5")
    rng = np.random.default_rng(4)
    cols, vocab, n, k, mw = 40, 90, 48, 5, 3
    rows = random_rows(rng, n, cols, vocab, nan_w=0.0)
    c = api.Context(0, stream=int(torch.cuda.current_stream().cuda_stream))
    grow = BowMatcher(n, n, cols, vocab, ctx=c)
    grow.reserve_database()
    for t in range(n):                                   # match against everything before, then append (9 folds)
        q = dev(rows[2 * t:2 * t + 2])
        if t > 0:
            idx, sc = grow.match(q, mask_width=mw, k=k, q_row0=t)
            oi, osc = oracle_topk(rows[2 * t:2 * t + 2], rows[:2 * t], mw, k, q_row0=t)
            assert np.array_equal(idx.cpu().numpy(), oi) and bits_equal(sc.cpu().numpy(), osc), t
        grow.append_database(q)
    assert grow.n == n
    bulk = BowMatcher(n, n, cols, vocab, ctx=c)
    bulk.pack_database(dev(rows))
    big = BowMatcher(n, n, cols, vocab, ctx=c)
    big.reserve_database(dev(rows[:14]))
    big.append_database(dev(rows[14:]))                  # one append larger than the tail: several folds inside one call
    q = dev(rows)
    want_i, want_s = bulk.match(q, mask_width=mw, k=k)
    for mt in (grow, big):
        gi, gs = mt.match(q, mask_width=mw, k=k)
        assert torch.equal(gi, want_i) and bits_equal(gs.cpu().numpy(), want_s.cpu().numpy())
    for mt in (grow, bulk, big):
        mt.close()
    c.close()


def test_shards_merge_to_the_whole(ctx):
    rng = np.random.default_rng(5)
    cols, vocab, n, k = 48, 120, 200, 7
    rows = random_rows(rng, n, cols, vocab, every=0, nan_w=0.0)
    q = dev(random_rows(rng, 25, cols, vocab, nan_w=0.0))
    whole = BowMatcher(25, n, cols, vocab, ctx=ctx)
    whole.pack_database(dev(rows))
    wi, ws = whole.match(q, mask_width=6, k=k, q_row0=90)
    parts = []
    for r0, r1 in ((0, 120), (120, n)):
        mt = BowMatcher(25, r1 - r0, cols, vocab, ctx=ctx)
        mt.pack_database(dev(rows[2 * r0:2 * r1]))
        parts.append(mt.match(q, mask_width=6, k=k, db_row0=r0, q_row0=90))
    ia = torch.stack([p[0] for p in parts])
    sa = torch.stack([p[1] for p in parts])
    mi, ms = whole.merge(ia, sa, k)
    assert torch.equal(mi, wi) and bits_equal(ms.cpu().numpy(), ws.cpu().numpy())
    ti, ts = merge_topk(ia.cpu(), sa.cpu(), k)
    assert torch.equal(ti, wi.cpu()) and bits_equal(ts.numpy(), ws.cpu().numpy())
    whole.close()


def test_capture_and_chunks(monkeypatch):
    monkeypatch.setenv("PR_BOW_CHUNK", "7")
    rng = np.random.default_rng(6)
    cols, vocab, n, m, k = 32, 80, 150, 30, 5
    rows = random_rows(rng, n, cols, vocab, nan_w=0.0)
    qa = random_rows(rng, m, cols, vocab, nan_w=0.0)
    qb = random_rows(rng, m, cols, vocab, nan_w=0.0)
    mt = BowMatcher.on_new_stream(m, n, cols, vocab)
    with torch.cuda.stream(mt.stream):
        mt.pack_database(dev(rows))
        static = dev(qa)
    mt.stream.synchronize()
    cap = mt.capture(static, mask_width=2, k=k, q_row0=3)
    for qn in (qb, qa):                                  # m = 30 > chunk = 7: every chunk resolved
        gi, gs = cap.run(dev(qn))
        oi, osc = oracle_topk(qn, rows, 2, k, q_row0=3)
        assert np.array_equal(gi.cpu().numpy(), oi) and bits_equal(gs.cpu().numpy(), osc)
        with torch.cuda.stream(mt.stream):
            ui, us = mt.match(dev(qn), mask_width=2, k=k, q_row0=3)
        mt.stream.synchronize()
        assert torch.equal(ui, gi) and bits_equal(us.cpu().numpy(), gs.cpu().numpy())
    del cap
    mt.close()


def test_rejection(ctx):
    cols, vocab = 6, 20
    good = np.array([[1, 4, 9, -1, -1, -1], [0.2, 0.3, 0.5, -1, -1, -1]], np.float64)
    bad_ids = {"duplicate": [1, 4, 4, -1, -1, -1], "descending": [1, 9, 4, -1, -1, -1], "out_of_range": [1, 4, 20, -1, -1, -1],
               "fractional": [1, 4.5, 9, -1, -1, -1]}
    mt = BowMatcher(5, 10, cols, vocab, ctx=ctx)
    for kind, ids in bad_ids.items():
        rows = np.concatenate([good] * 3 + [np.array([ids, good[1]])] + [good])
        with pytest.raises(_lib.PRError) as e:
            mt.pack_database(dev(rows))
        assert e.value.code == _lib.PR_EINVAL and "row 3 " in str(e.value), kind
        mt.pack_database(dev(np.concatenate([good] * 2)))
        with pytest.raises(_lib.PRError) as e:
            mt.append_database(dev(np.concatenate([good, np.array([ids, good[1]])])))
        assert e.value.code == _lib.PR_EINVAL and "row 3 " in str(e.value), kind
        assert mt.n == 2
    # a non-conforming query row: -1 / NaN and PR_WARN_BOW_ROWS; its neighbours are answered
    db = np.concatenate([good, np.array([[4, 9, -1, -1, -1, -1], [0.5, 0.5, -1, -1, -1, -1]])])
    mt.pack_database(dev(db))
    ctx.take_warnings()
    q = np.concatenate([good, np.array([bad_ids["descending"], good[1]]), good])
    idx, sc = mt.match(dev(q), k=2)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert (idx[1] == -1).all() and np.isnan(sc[1]).all()
    oi, osc = oracle_topk(good, db, 0, 2)
    assert np.array_equal(idx[0], oi[0]) and np.array_equal(idx[2], oi[0]) and bits_equal(sc[[0, 2]], np.concatenate([osc, osc]))
    assert ctx.take_warnings() & _lib.WARN_BOW_ROWS
    assert not ctx.take_warnings() & _lib.WARN_BOW_ROWS
    mt.close()
    with pytest.raises(_lib.PRError) as e:
        api.bow_match_topk(q, db, 0, 1, ctx=ctx)
    assert e.value.code == _lib.PR_EINVAL and "row 1 " in str(e.value)
    with pytest.raises(_lib.PRError) as e:
        api.bow_distance_f64(db, q, ctx=ctx)
    assert e.value.code == _lib.PR_EINVAL


def test_scale_100k_zipf(ctx):
    n, m, cols, vocab, k = 100_000, 256, 160, 100_000, 5
    db = synth.bow_signatures_torch(11, n, cols=cols, vocab=vocab, fill=(40, 150), zipf=1.0)
    q = synth.bow_signatures_torch(12, m, cols=cols, vocab=vocab, fill=(40, 150), zipf=1.0)
    q[:128] = db[:128]                                   # the first 64 queries are DB rows
    mt = BowMatcher(m, n, cols, vocab, ctx=ctx, max_postings=n * 150)
    mt.pack_database(db)
    idx, sc = mt.match(q, mask_width=0, k=k)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    h2 = db.cpu().numpy()
    h1 = q.cpu().numpy()
    pick = np.random.default_rng(0).choice(m, 16, replace=False)
    pick[:2] = (0, 1)
    rows = np.concatenate([h1[2 * i:2 * i + 2] for i in pick])
    oi, osc = oracle_topk(rows, h2, 0, k)
    assert np.array_equal(idx[pick], oi) and bits_equal(sc[pick], osc)
    assert idx[0, 0] == 0 and idx[1, 0] == 1
    mt.close()


def test_end_to_end_from_orb_descriptors():
    import bow_np
    K = synth.bow_vocabulary(7, k=10, L=4, stop_frac=0.1)
    p, leaf, d, w = K
    voc = api.ORBVocabulary.from_arrays(10, 4, 0, 0, *K)
    n_first, revisits = 50, list(range(0, 50, 2))
    desc, offs, planted = synth.bow_drive(81, d[leaf > 0], n_first, revisits, per_image=300)
    cols, N = 400, len(offs) - 1
    rows = api.bow_generate_torch(torch.from_numpy(desc).cuda(), torch.from_numpy(offs).cuda(), voc, cols=cols)
    mt = BowMatcher(N, N, cols, voc.size())
    mt.pack_database(rows)                               # the generated device rows, no host copy
    idx, sc = mt.match(rows, mask_width=10, k=3)
    frames = [desc[offs[i]:offs[i + 1]] for i in range(N)]
    want = bow_np.rows(bow_np.Vocab(10, 4, 0, 0, *K), frames, cols)
    oi, osc = oracle_topk(want, want, 10, 3)
    assert np.array_equal(idx.cpu().numpy(), oi) and bits_equal(sc.cpu().numpy(), osc)
    top1 = idx[:, 0].cpu().numpy()
    hits = [f for f in range(N) if planted[f] >= 0]
    assert len(hits) >= 20 and all(top1[f] == planted[f] for f in hits)
    mt.close()
