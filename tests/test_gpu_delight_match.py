"""The device-resident DELIGHT matcher (delight_match.hip: pr_delight_db_*, pr_delight_match_topk_*, pr_delight_distance_f64,
matcher.DelightMatcher) against the CPU oracle (oracle_lib.delight_distance + select_topk on the global matrix): distances and top-k
scores equal bit for bit, ties and near-copies resolved in fp64, growth == bulk build, shards, graph capture, 100k entries."""
import numpy as np
import pytest

import oracle_lib
from resident_fuzz_cases import bits_equal, oracle_select
from so_dso_place_recognition_amd import api, synth
from so_dso_place_recognition_amd.matcher import DelightMatcher, merge_topk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def oracle_topk(h1, h2, mask_width, k, q_row0=0, db_row0=0):
    return oracle_select(oracle_lib.delight_distance(h1, h2), mask_width, k, q_row0, db_row0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def same(got, want):
    gi, gs = got
    wi, ws = want
    gi = host(gi) if hasattr(gi, "cpu") else gi
    gs = host(gs) if hasattr(gs, "cpu") else gs
    return np.array_equal(gi, wi) and bits_equal(gs, ws)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def run(ctx, q, db, mask_width=0, k=1, q_row0=0, db_row0=0, exact=False):
    mt = DelightMatcher(max(len(q) // 16, 1), max(len(db) // 16, 1), ctx=ctx, exact=exact)
    mt.pack_database(dev(db))
    idx, sc = mt.match(dev(q), mask_width, k, db_row0, q_row0)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.close()
    return (host(idx), host(sc)), fl


def sigs(seed, n):
    return synth.delight_database(seed, n)


@pytest.mark.parametrize("shape", [(1, 1), (5, 70), (65, 33), (3, 17)])
def test_distances_bit_for_bit(ctx, shape):
    m, n = shape
    rng = np.random.default_rng(m)
    h1, h2 = sigs(m, m), sigs(1000 + n, n)
    if n > 16:
        h2[16:32] = 0.0                                                 # an empty entry
        h2[32:48] += rng.normal(size=(16, 256))                         # negative and fractional entries
        h2[70, 9] = np.nan
        h1[:16] = 0.0
    assert bits_equal(api.delight_distance_f64(h1, h2, ctx=ctx), oracle_lib.delight_distance(h1, h2))


def test_topk_bit_for_bit(ctx):
    db = sigs(2, 300)
    q, _ = synth.delight_queries(1, db, 70)
    d = oracle_lib.delight_distance(q, db)
    for k in (1, 5, 128):
        for mask_width in (0, 4, 100):
            for q0, d0 in ((0, 0), (150, 20)):
                want = oracle_select(d, mask_width, k, q0, d0)
                for exact in (False, True):
                    got, _ = run(ctx, q, db, mask_width, k, q0, d0, exact)
                    assert same(got, want), (k, mask_width, q0, d0, exact)
            assert same(api.delight_match_topk(q, db, mask_width, k, ctx=ctx), oracle_select(d, mask_width, k))


def test_small_and_degenerate(ctx):
    rng = np.random.default_rng(3)
    q, db = sigs(4, 6), sigs(5, 3)                                      # n < k: -1 / NaN fill
    assert same(run(ctx, q, db, 0, 5)[0], oracle_topk(q, db, 0, 5))
    assert same(run(ctx, q[:16], db[:16], 0, 1)[0], oracle_topk(q[:16], db[:16], 0, 1))   # m = n = 1
    assert same(run(ctx, q, db, 2, 5)[0], oracle_topk(q, db, 2, 5))     # masked entries selected as +Inf
    db = sigs(6, 200)
    db[16 * 7:16 * 8] = 0.0                                             # all-zero histograms: +Inf against an empty query
    db[16 * 150:16 * 151] = 0.0
    q[:16] = 0.0
    for k in (1, 5):
        got, fl = run(ctx, q, db, 0, k)
        assert same(got, oracle_topk(q, db, 0, k))
    dbx = db.copy()
    dbx[16 * 17:16 * 18] = np.nan                                       # NaN rows on the DB side: every query takes its exact row
    dbx[16 * 50 + 3, 3] = np.nan
    got, fl = run(ctx, q, dbx, 0, 5)
    assert same(got, oracle_topk(q, dbx, 0, 5)) and fl == 6
    qx = q.copy()
    qx[16 * 2 + 5, 5] = np.nan                                          # ... and on the query side: that query alone
    qx[16 * 3:16 * 4] -= 0.25 * (rng.random((16, 256)) < 0.1)           # negative and fractional entries
    got, fl = run(ctx, qx, db, 0, 5)
    assert same(got, oracle_topk(qx, db, 0, 5)) and 2 <= fl < 6
    dbf = db + 0.5 * (rng.random(db.shape) < 0.01)
    assert same(run(ctx, q, dbf, 0, 5)[0], oracle_topk(q, dbf, 0, 5))
    big = np.where(rng.random((16 * 40, 256)) < 0.5, 0.0, 2.0 ** 24 - rng.integers(0, 1000, (16 * 40, 256)))   # counts near 2^24
    big[16 * 3:16 * 4] *= 4.0                                           # and beyond it
    for lo in (0, 4):
        got, fl = run(ctx, big[16 * 20:16 * 24], big[16 * lo:], 0, 3)
        assert same(got, oracle_topk(big[16 * 20:16 * 24], big[16 * lo:], 0, 3))
        assert (fl == 4) == (lo == 0)


def test_duplicates_and_permutation_images_take_the_lower_index(ctx):
    db = sigs(7, 500)
    e = db[16 * 250:16 * 251].copy()
    perm5 = e[np.arange(16) ^ 5]
    for j in (3, 4, 490, 499):
        db[16 * j:16 * (j + 1)] = e                                     # exact duplicates at low and high indices
    for j in (100, 300):
        db[16 * j:16 * (j + 1)] = perm5                                 # permutation images: the same distance to every query
    q = np.concatenate([e, perm5, db[:16], sigs(8, 2)])
    d = oracle_lib.delight_distance(q, db)
    assert len(set(d[4, [3, 4, 100, 250, 300, 490, 499]].tolist())) == 1
    for k in (1, 5, 9):
        want = oracle_select(d, 0, k)
        assert list(want[0][0, :min(k, 7)]) == [3, 4, 100, 250, 300, 490, 499][:k]
        assert same(run(ctx, q, db, 0, k)[0], want)
    same_db = np.tile(e, (150, 1))                                      # every distance ties: indices 0 .. k - 1
    got, fl = run(ctx, q[16 * 3:], same_db, 0, 7)
    assert np.array_equal(got[0], np.tile(np.arange(7, dtype=np.int32), (2, 1)))
    assert same(got, oracle_topk(q[16 * 3:], same_db, 0, 7))


@pytest.mark.parametrize("cs,k", [(12, 1), (40, 5)])
def test_near_copy_cluster_is_ranked_in_fp64(ctx, cs, k):
    """The members of a planted cluster differ from the query by one large common difference and by one count each in a bin of their
    own: the oracle's distances are distinct, round to one fp32 value, and are not in index order.  m = 256 and n = 3200 give slabs of
    100 entries, so the cluster at entry 1600 lies in one slab and fills its list of k + 8 keys."""
    n, m, r0 = 3200, 256, 1600
    db = synth.delight_signatures_torch(71, n, clusters=1, cluster_size=cs)
    q = synth.delight_signatures_torch(72, m)
    flat = db.view(n, 4096)
    base = flat[r0:r0 + cs].min(0).values
    dbh = host(db)
    for t, shift in enumerate((5000.0, 3000.0, 2000.0, 6000.0)):
        for step in range(8):                                           # a common difference that keeps the members' distances clear of
            row = base.clone()                                          # an fp32 rounding boundary (they span ~1e-8 of 2.4e-7)
            row[5 + t] += shift + 7.0 * step
            dm = oracle_lib.delight_distance(host(row.view(16, 256)), dbh)[0, r0:r0 + cs]
            if len(set(dm.astype(np.float32).tolist())) == 1:
                break
        q.view(m, 4096)[t] = row
    qh = host(q)
    d = oracle_lib.delight_distance(qh[:16 * 8], dbh)
    for t in range(4):
        dm = d[t, r0:r0 + cs]
        assert len(set(dm.tolist())) == cs                              # pairwise distinct in fp64 ...
        assert len(set(dm.astype(np.float32).tolist())) == 1            # ... one value in fp32 ...
        assert not np.array_equal(np.argsort(dm, kind="stable"), np.arange(cs))   # ... and not in index order
        assert np.delete(d[t], np.arange(r0, r0 + cs)).min() > dm.max()
    want = oracle_select(d, 0, k)
    mt = DelightMatcher(m, n, ctx=ctx)
    mt.pack_database(db)
    idx, sc = mt.match(q, 0, k)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.set_exact(True)
    xi, xs = mt.match(q, 0, k)
    torch.cuda.synchronize()
    assert mt.flagged_count() == m
    mt.close()
    print("flagged", fl, "oracle order of query 0:", want[0][0])
    assert same((host(idx)[:8], host(sc)[:8]), want)
    assert same((idx, sc), (host(xi), host(xs)))
    assert fl >= 1


def test_more_flagged_queries_than_one_pass_holds(ctx):
    """n = 4000 gives slabs of 48 (m = 100) and 142 (m = 300) entries: the 40 copies at entry 1000 fill a list with ties."""
    n = 4000
    db = synth.delight_signatures_torch(15, n)
    e = db[16 * 1000:16 * 1001].clone()
    db.view(n, 4096)[1000:1040] = e.view(1, 4096)
    dbh = host(db)
    for m in (100, 300):                                                # 300 > the 256 exact rows of one pass: chained passes
        q = e.repeat(m, 1)
        q[torch.arange(m, device="cuda") * 16, 0] += (torch.arange(m, device="cuda") % 5).to(torch.float64)
        mt = DelightMatcher(m, n, ctx=ctx)
        mt.pack_database(db)
        idx, sc = mt.match(q, 0, 5)
        torch.cuda.synchronize()
        fl = mt.flagged_count()
        mt.close()
        sample = np.r_[0:6, m - 3:m]
        qh = host(q).reshape(m, 16, 256)[sample].reshape(-1, 256)
        assert same((host(idx)[sample], host(sc)[sample]), oracle_topk(qh, dbh, 0, 5))
        assert np.array_equal(host(idx), np.tile(np.arange(1000, 1005, dtype=np.int32), (m, 1)))
        assert fl == m


def test_random_workload_flags_nothing(ctx):
    """128 x 50 000 without clusters, k = 5: the coarse pass must carry this workload alone (flagged == 0)."""
    n, m = 50000, 128
    db = synth.delight_signatures_torch(21, n)
    q = synth.delight_signatures_torch(22, m)
    mt = DelightMatcher(m, n, ctx=ctx)
    mt.pack_database(db)
    idx, sc = mt.match(q, 0, 5)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.set_exact(True)
    xi, xs = mt.match(q, 0, 5)
    torch.cuda.synchronize()
    assert mt.flagged_count() == m
    mt.close()
    print("flagged", fl)
    assert same((idx, sc), (host(xi), host(xs)))
    assert same((host(idx)[:2], host(sc)[:2]), oracle_topk(host(q)[:32], host(db), 0, 5))
    assert fl == 0


def test_growth_equals_bulk(ctx):
    rows = sigs(31, 1500)
    for j in range(1200, 1240):
        rows[16 * j:16 * (j + 1)] = rows[16 * 1200:16 * 1201]
    q = np.concatenate([sigs(32, 20), rows[16 * 1200:16 * 1203]])
    mtb = DelightMatcher(len(q) // 16, 1500, ctx=ctx)
    mtb.pack_database(dev(rows))
    bulk = mtb.match(dev(q), 3, 5)
    torch.cuda.synchronize()
    bulk, bulk_bytes = (host(bulk[0]), host(bulk[1])), mtb.device_bytes
    mtb.close()
    for n0 in (0, 492):
        mt = DelightMatcher(len(q) // 16, 1500, ctx=ctx)
        if n0 == 0:
            mt.reserve_database()
        else:
            mt.reserve_database(dev(rows[:16 * n0]))
        at = n0
        for step in (1, 7, 1000, 1500 - n0 - 1008):
            mt.append_database(dev(rows[16 * at:16 * (at + step)]))
            at += step
        assert mt.n == 1500 and mt.device_bytes == bulk_bytes
        got = mt.match(dev(q), 3, 5)
        torch.cuda.synchronize()
        assert same(got, bulk), n0
        with pytest.raises(api.PRError):
            mt.append_database(dev(rows[:16]))                          # beyond max_sigs
        mt.close()
    assert same(bulk, oracle_topk(q, rows, 3, 5))


@pytest.mark.parametrize("cuts", [(0, 500, 1001), (0, 300, 650, 1001)])
def test_shards_merge(ctx, cuts):
    db = sigs(41, 1001)
    for j in range(700, 740):
        db[16 * j:16 * (j + 1)] = db[16 * 700:16 * 701]
    q = np.concatenate([sigs(42, 30), db[16 * 700:16 * 702]])
    whole, _ = run(ctx, q, db, 5, 5, 900, 0)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        mt = DelightMatcher(len(q) // 16, hi - lo, ctx=ctx)
        mt.pack_database(dev(db[16 * lo:16 * hi]))
        parts.append(mt.match(dev(q), 5, 5, lo, 900))
        torch.cuda.synchronize()
        mt.close()
    idx, sc = merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), 5)
    torch.cuda.synchronize()
    assert same((idx, sc), whole)
    assert same(whole, oracle_topk(q, db, 5, 5, 900, 0))


def test_capture_replay_and_staleness():
    db = sigs(51, 800)
    for j in range(100, 140):
        db[16 * j:16 * (j + 1)] = db[16 * 100:16 * 101]
    q = np.concatenate([sigs(52, 10), db[16 * 100:16 * 102]])
    mt = DelightMatcher.on_new_stream(16, 1000)
    with torch.cuda.stream(mt.stream):
        mt.pack_database(dev(db))
        qs = dev(q)
        eager = mt.match(qs, 0, 5)
        mt.stream.synchronize()
        eager = (host(eager[0]), host(eager[1]))
    cap = mt.capture(qs, 0, 5)
    idx, sc = cap.run()
    torch.cuda.synchronize()
    assert same((idx, sc), eager) and same(eager, oracle_topk(q, db, 0, 5))
    q2 = np.concatenate([db[16 * 100:16 * 103], sigs(53, 9)])
    with torch.cuda.stream(mt.stream):
        qs.copy_(dev(q2))
        mt.stream.synchronize()
    idx, sc = cap.run()
    torch.cuda.synchronize()
    assert same((idx, sc), oracle_topk(q2, db, 0, 5))
    with torch.cuda.stream(mt.stream):
        mt.append_database(dev(db[:16]))
    with pytest.raises(RuntimeError):
        cap.run()
    mt.close()


def test_100k_entries_two_stage_equals_exact_rows(ctx):
    """The oracle is too slow at this size; the exact rows it is compared with are oracle-checked at small n above."""
    n, m = 100000, 128
    db = synth.delight_signatures_torch(61, n, clusters=6, cluster_size=40)
    q = synth.delight_signatures_torch(62, m)
    step = n // 7
    picks = [step, step + 3, 2 * step, 2 * step + 39, 3 * step, 4 * step, 5 * step, 6 * step, 10, 99999]
    q.view(m, 4096)[:len(picks)] = db.view(n, 4096)[picks]
    q.view(m, 4096)[:len(picks), 77] += 4000.0
    mt = DelightMatcher(m, n, ctx=ctx)
    assert mt.device_bytes < n * 49668 + 400e6
    mt.pack_database(db)
    idx, sc = mt.match(q, 50, 5)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.set_exact(True)
    xi, xs = mt.match(q, 50, 5)
    torch.cuda.synchronize()
    mt.close()
    print("flagged", fl)
    assert same((idx, sc), (host(xi), host(xs)))
    assert 1 <= fl < m // 4


def test_parent_path_on_the_cluster_is_recorded(ctx):
    """What api.match_topk('delight') - fp32 keys, no re-evaluation - returns on the cluster: printed for DESIGN.md 4.9, not asserted
    (equal fp32 keys leave its order to the rounding)."""
    n, r0, cs = 400, 200, 12
    db = synth.delight_signatures_torch(71, n, clusters=1, cluster_size=cs)
    base = db.view(n, 4096)[r0:r0 + cs].min(0).values.clone()
    base[5] += 5000.0
    qh, dbh = host(base.view(16, 256)), host(db)
    want = oracle_topk(qh, dbh, 0, 5)
    pidx, psc = api.match_topk("delight", qh, dbh, 0, 2.0, 5, ctx=ctx)
    print("oracle", want[0][0], "parent", pidx[0], "parent scores", psc[0])
    assert same(api.delight_match_topk(qh, dbh, 0, 5, ctx=ctx), want)
