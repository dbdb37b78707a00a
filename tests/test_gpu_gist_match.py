"""The device-resident GIST matcher (gist_match.hip: pr_gist_db_*, pr_gist_match_topk_*, pr_gist_distance_f64, matcher.GistMatcher)
against the CPU oracle (oracle_lib.gist_distance + select_topk on the global matrix): distances and top-k scores equal bit for bit,
ties and near-copies resolved by the exact-row path, growth == bulk build, shards, graph capture, 100k rows, and the path from
images through gist_generate_torch without a host copy."""
import numpy as np
import pytest

import oracle_lib
from resident_fuzz_cases import bits_equal, oracle_select
from so_dso_place_recognition_amd import api, synth
from so_dso_place_recognition_amd.matcher import GistMatcher, merge_topk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def oracle_topk(h1, h2, mask_width, k, q_row0=0, db_row0=0):
    return oracle_select(oracle_lib.gist_distance(h1, h2), mask_width, k, q_row0, db_row0)


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
    mt = GistMatcher(max(len(q), 1), max(len(db), 1), q.shape[1], ctx=ctx, exact=exact)
    mt.pack_database(dev(db))
    idx, sc = mt.match(dev(q), mask_width, k, db_row0, q_row0)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.close()
    return (host(idx), host(sc)), fl


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 70, 33), (65, 130, 96), (130, 64, 512), (3, 9, 960)])
def test_distances_bit_for_bit(ctx, shape):
    m, n, cols = shape
    h1 = synth.gist_signatures(m, m, cols)
    h2 = synth.gist_signatures(1000 + n, n, cols)
    assert bits_equal(api.gist_distance_f64(h1, h2, ctx=ctx), oracle_lib.gist_distance(h1, h2))


@pytest.mark.parametrize("k", [1, 5, 128])
@pytest.mark.parametrize("mask_width", [0, 4, 100])
def test_topk_bit_for_bit(ctx, k, mask_width):
    q = synth.gist_signatures(1, 70, 96)
    db = synth.gist_signatures(2, 300, 96)
    for q0, d0 in ((0, 0), (150, 20)):
        want = oracle_topk(q, db, mask_width, k, q0, d0)
        for exact in (False, True):
            got, _ = run(ctx, q, db, mask_width, k, q0, d0, exact)
            assert same(got, want), (k, mask_width, q0, d0, exact)
    assert same(api.gist_match_topk(q, db, mask_width, k, ctx=ctx), oracle_topk(q, db, mask_width, k))


def test_small_and_degenerate(ctx):
    rng = np.random.default_rng(3)
    q = synth.gist_signatures(4, 6, 33)
    db = synth.gist_signatures(5, 3, 33)                       # n < k: -1 / NaN fill
    assert same(run(ctx, q, db, 0, 5)[0], oracle_topk(q, db, 0, 5))
    assert same(run(ctx, q[:1], db, 0, 1)[0], oracle_topk(q[:1], db, 0, 1))           # m = 1
    assert same(run(ctx, q, db, 2, 5, 0, 0)[0], oracle_topk(q, db, 2, 5))             # masked entries selected as +Inf
    db = synth.gist_signatures(6, 200, 33)
    db[[0, 17, 199]] = np.nan                                   # NaN rows on the DB side ...
    db[50, 3] = np.nan
    q[2, 5] = np.nan                                            # ... and on the query side
    for k in (1, 5):
        assert same(run(ctx, q, db, 0, k)[0], oracle_topk(q, db, 0, k))
    same_db = np.tile(rng.random(40)[None, :], (150, 1))        # every distance ties: indices 0 .. k - 1
    qt = rng.random((4, 40))
    got, fl = run(ctx, qt, same_db, 0, 7)
    assert np.array_equal(got[0], np.tile(np.arange(7, dtype=np.int32), (4, 1))) and fl == 4
    assert same(got, oracle_topk(qt, same_db, 0, 7))
    db = synth.gist_signatures(7, 500, 64)
    db[[3, 4, 490, 499]] = db[250]                              # exact duplicates at low and high indices
    qq = db[[250, 3, 100]] + 0.0
    for k in (1, 5):
        assert same(run(ctx, qq, db, 0, k)[0], oracle_topk(qq, db, 0, k))
    big = synth.gist_signatures(8, 40, 20) + 1e3                # large common offset, differences of 1e-3
    big[:, :] = 1e3 + 1e-3 * big
    assert same(run(ctx, big[:5], big, 0, 3)[0], oracle_topk(big[:5], big, 0, 3))
    huge = synth.gist_signatures(9, 40, 20) * 1e6               # beyond the f16 range after centring
    assert same(run(ctx, huge[:5], huge, 0, 3)[0], oracle_topk(huge[:5], huge, 0, 3))


@pytest.mark.parametrize("n,k,v_db,v_q", [(12, 5, 1e5, 8e4), (40, 5, 8e4, 7e4), (300, 128, 7e4, 6.5e4)])
def test_db_rows_outside_the_f16_range_are_not_lost(ctx, n, k, v_db, v_q):
    """Finite DB rows that leave the f16 range after centring are never listed by the coarse pass, also where every slab's list has room
    left (n = 12: one slab of fewer than k + 8 rows; n = 300, k = 128: ten slabs of ~32 rows).  Here they are the nearest rows of queries
    that do not overflow themselves, so the answer is only right if every query goes to its exact row."""
    db = synth.gist_signatures(70 + n, n, 20)
    far = [1, n // 2, n - 2]
    db[far, 0] = v_db                                           # centred: v_db - 3 v_db / n > 65520, beyond f16
    q = synth.gist_signatures(71 + n, 6, 20)
    q[:4, 0] = v_q                                              # centred: v_q - 3 v_db / n < 65000, the queries pack normally
    assert v_db - 3 * v_db / n > 65520 and v_q - 3 * v_db / n < 65000
    want = oracle_topk(q, db, 0, k)
    assert set(want[0][0, :3]) == set(far)                      # the overflow rows are the three nearest of query 0
    got, fl = run(ctx, q, db, 0, k)
    assert same(got, want)
    assert fl == len(q)


@pytest.mark.parametrize("eps", [0.0, 1e-9, 1e-6])
def test_near_copy_clusters_take_the_exact_row(ctx, eps):
    rng = np.random.default_rng(11)
    db = synth.gist_signatures(12, 3000, 128)
    db[1000:1040] = db[1000] + eps * rng.normal(size=(40, 128))
    q = np.concatenate([db[1005:1008] + eps * rng.normal(size=(3, 128)), synth.gist_signatures(13, 5, 128)])
    for k in (1, 5):
        got, fl = run(ctx, q, db, 0, k)
        assert same(got, oracle_topk(q, db, 0, k))
        assert fl > 0


def test_more_flagged_queries_than_one_pass_holds(ctx):
    rng = np.random.default_rng(14)
    db = synth.gist_signatures(15, 2000, 64)
    db[500:540] = db[500] + 1e-9 * rng.normal(size=(40, 64))
    for m in (100, 300):                                        # 300 > the 256 exact rows of one pass: chained passes
        q = db[500] + 1e-9 * rng.normal(size=(m, 64))
        got, fl = run(ctx, q, db, 0, 5)
        assert same(got, oracle_topk(q, db, 0, 5))
        assert fl == m


def test_random_workload_flags_nothing(ctx):
    """n = 50 000, cols = 512, m = 128, k = 5: the coarse pass must carry this workload alone (flagged == 0)."""
    db = synth.gist_signatures(21, 50000, 512)
    q = synth.gist_signatures(22, 128, 512)
    mt = GistMatcher(128, 50000, 512, ctx=ctx)
    mt.pack_database(dev(db))
    idx, sc = mt.match(dev(q), 0, 5)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    mt.set_exact(True)
    xi, xs = mt.match(dev(q), 0, 5)
    torch.cuda.synchronize()
    assert mt.flagged_count() == 128
    mt.close()
    print("flagged", fl)
    assert same((idx, sc), (host(xi), host(xs)))
    assert same((host(idx)[:16], host(sc)[:16]), oracle_topk(q[:16], db, 0, 5))
    assert fl == 0


def test_growth_equals_bulk(ctx):
    rows = synth.gist_signatures(31, 1500, 96)
    rows[1200:1240] = rows[1200]
    q = np.concatenate([synth.gist_signatures(32, 20, 96), rows[1200:1203]])
    bulk, _ = run(ctx, q, rows, 3, 5)
    for n0 in (0, 492):
        mt = GistMatcher(len(q), 1500, 96, ctx=ctx)
        if n0 == 0:
            mt.reserve_database()
        else:
            mt.reserve_database(dev(rows[:n0]))
        at = n0
        for step in (1, 7, 1000, 1500 - n0 - 1008):
            mt.append_database(dev(rows[at:at + step]))
            at += step
        assert mt.n == 1500
        got = mt.match(dev(q), 3, 5)
        torch.cuda.synchronize()
        assert same(got, bulk), n0
        with pytest.raises(api.PRError):
            mt.append_database(dev(rows[:1]))                   # beyond max_sigs
        mt.close()
    assert same(bulk, oracle_topk(q, rows, 3, 5))


def test_shards_merge(ctx):
    db = synth.gist_signatures(41, 1001, 96)
    db[700:740] = db[700]
    q = np.concatenate([synth.gist_signatures(42, 30, 96), db[700:702]])
    whole, _ = run(ctx, q, db, 5, 5, 900, 0)
    parts = []
    for lo, hi in ((0, 500), (500, 1001)):
        mt = GistMatcher(len(q), hi - lo, 96, ctx=ctx)
        mt.pack_database(dev(db[lo:hi]))
        parts.append(mt.match(dev(q), 5, 5, lo, 900))
        torch.cuda.synchronize()
        mt.close()
    idx, sc = merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), 5)
    torch.cuda.synchronize()
    assert same((idx, sc), whole)
    assert same(whole, oracle_topk(q, db, 5, 5, 900, 0))


def test_capture_replay_and_staleness():
    db = synth.gist_signatures(51, 800, 96)
    db[100:140] = db[100]
    q = np.concatenate([synth.gist_signatures(52, 10, 96), db[100:102]])
    mt = GistMatcher.on_new_stream(16, 1000, 96)
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
    q2 = np.concatenate([db[100:103], synth.gist_signatures(53, 9, 96)])
    with torch.cuda.stream(mt.stream):
        qs.copy_(dev(q2))
        mt.stream.synchronize()
    idx, sc = cap.run()
    torch.cuda.synchronize()
    assert same((idx, sc), oracle_topk(q2, db, 0, 5))
    with torch.cuda.stream(mt.stream):
        mt.append_database(dev(db[:1]))
    with pytest.raises(RuntimeError):
        cap.run()
    mt.close()


def test_100k_rows_two_stage_equals_exact_rows(ctx):
    n, m, cols = 100000, 4096, 512
    db = synth.gist_signatures_torch(61, n, cols, clusters=6, cluster_size=40, eps=1e-9)
    q = synth.gist_signatures_torch(62, m, cols)
    step = n // 7
    q[:12] = db[[step, step + 3, 2 * step, 2 * step + 39, 3 * step, 4 * step, 5 * step, 6 * step, 6 * step + 1, 6 * step + 2, 10, 99999]]
    free0 = torch.cuda.mem_get_info()[0]
    mt = GistMatcher(m, n, cols, ctx=ctx)
    held = free0 - torch.cuda.mem_get_info()[0]
    assert mt.device_bytes < 1.6e9 and held < 1.6e9            # below the m x n fp32 matrix of the all-pairs path alone
    mt.pack_database(db)
    idx, sc = mt.match(q, 50, 5)
    torch.cuda.synchronize()
    fl = mt.flagged_count()
    assert 10 <= fl < m // 8
    assert torch.cuda.mem_get_info()[0] >= free0 - 1.6e9
    mt.set_exact(True)
    xi, xs = mt.match(q, 50, 5)
    torch.cuda.synchronize()
    mt.close()
    assert same((idx, sc), (host(xi), host(xs)))
    sample = np.r_[0:12, np.linspace(12, m - 1, 52).astype(int)]
    dbh, qh = host(db), host(q)
    d = oracle_lib.gist_distance(qh[sample], dbh)
    d = np.where(np.abs(sample[:, None] - np.arange(n)[None, :]) < 50, np.inf, d)
    rc, oi, osc = oracle_lib.select_topk(d, 0, 5)
    assert rc == 0 and np.array_equal(host(idx)[sample], oi) and bits_equal(host(sc)[sample], osc)


def test_images_to_match_without_a_host_copy(ctx):
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    imgs = torch.randint(0, 256, (6, 256, 256), generator=g, device="cuda", dtype=torch.uint8)
    rows = api.gist_generate_torch(imgs).to(torch.float64).contiguous()
    torch.cuda.synchronize()
    mt = GistMatcher(1, 16, rows.shape[1], ctx=ctx)
    mt.pack_database(rows)
    idx, sc = mt.match(rows[4:5].contiguous(), 0, 1)
    torch.cuda.synchronize()
    mt.close()
    assert int(idx[0, 0]) == 4 and float(sc[0, 0]) == 0.0 and not np.signbit(float(sc[0, 0]))
