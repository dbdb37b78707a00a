"""CPU restatements behind the two-stage DELIGHT matcher (delight_match.hip): the normative fp64 arithmetic, the error
bound of the coarse fp32 pass, and the containment rule that decides whether a candidate list provably holds the exact top-k."""
import numpy as np
import pytest

import delight_np as dn
import oracle_lib
from so_dso_place_recognition_amd import synth


def test_normative_order_is_the_oracles_and_no_other():
    db = synth.delight_database(1, 5)
    q, _ = synth.delight_queries(2, db, 3)
    want = oracle_lib.delight_distance(q, db)
    assert np.array_equal(dn.bits(dn.distance(q, db)), dn.bits(want))
    assert np.any(dn.bits(dn.distance(q, db, order="row")) != dn.bits(want))
    a = np.zeros((16, 256)); b = np.zeros((16, 256))           # few occupied bins: a term's last bit survives the sum
    a[0, 0], b[0, 0] = 7.0, 4.0
    want = oracle_lib.delight_distance(a, b)
    assert np.array_equal(dn.bits(dn.distance(a, b)), dn.bits(want))
    assert np.any(dn.bits(dn.distance(a, b, form="divide_first")) != dn.bits(want))


def test_negative_fractional_and_empty_inputs_follow_the_oracle():
    rng = np.random.default_rng(3)
    db = synth.delight_database(4, 4)
    db[:16] = 0.0                                               # no occupied bin against an empty query: +Inf
    db[16:32] += rng.normal(size=(16, 256))                     # negative and fractional entries
    db[40, 7] = np.nan
    q = np.concatenate([np.zeros((16, 256)), db[16:32] * 0.5, synth.delight_database(5, 1)])
    want = oracle_lib.delight_distance(q, db)
    got = dn.distance(q, db)
    assert np.isinf(want[0, 0]) and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(dn.bits(got[ok]), dn.bits(want[ok]))


def test_moving_the_factor_two_is_exact_except_in_the_subnormal_range():
    """2 ((a - b)(a - b)) / sum only scales by a power of two, so on counts it cannot differ from the normative form; it does once the
    square is subnormal, which is why the kernels keep the normative form for every input."""
    db = synth.delight_database(6, 3)
    assert np.array_equal(dn.bits(dn.distance(db[:16], db, form="square_first")), dn.bits(oracle_lib.delight_distance(db[:16], db)))
    a = np.zeros((16, 256)); b = np.zeros((16, 256))
    a[0, 0] = 1.01e-160
    want = oracle_lib.delight_distance(a, b)
    assert np.array_equal(dn.bits(dn.distance(a, b)), dn.bits(want))
    assert np.any(dn.bits(dn.distance(a, b, form="square_first")) != dn.bits(want))


def _pairs():
    rng = np.random.default_rng(7)
    db = synth.delight_database(8, 6).reshape(6, 16, 256)
    q, _ = synth.delight_queries(9, db.reshape(96, 256), 3)
    q = q.reshape(3, 16, 256)
    out = [(q[i], db[j]) for i in range(3) for j in range(6)]                       # random histograms, near matches among them
    near = np.where(rng.random((4, 16, 256)) < 0.5, 0.0, 2.0 ** 24 - rng.integers(0, 1000, (4, 16, 256)))
    out += [(near[0], near[1]), (near[2], near[3]), (near[0], db[0]), (np.full((16, 256), 2.0 ** 24), np.zeros((16, 256)))]
    for r, c, r2, c2, v, v2 in [(0, 0, 0, 0, 7.0, 9.0), (3, 17, 3, 17, 1.0, 2.0 ** 24), (2, 5, 9, 200, 3.0, 3.0), (5, 1, 0, 1, 1.0, 1.0)]:
        a = np.zeros((16, 256)); b = np.zeros((16, 256))                              # all but one bin empty
        a[r, c] = v; b[r2, c2] = v2
        out.append((a, b))
    return out


@pytest.mark.parametrize("sign", [1.0, -1.0, "random"])
def test_bound_holds_against_the_float32_emulation(sign):
    rng = np.random.default_rng(10)
    worst = 0.0
    for a, b in _pairs():
        assert dn.coarse_exact(a) and dn.coarse_exact(b)
        d = oracle_lib.delight_distance(a, b)[0, 0]
        s = rng.choice([-1.0, 1.0], size=(16, 256)) if sign == "random" else sign
        key = float(dn.coarse_key(a, b, s))
        assert np.isfinite(d) and np.isfinite(key)
        assert abs(key - d) <= dn.REL * d + dn.ABS, (key, d)
        worst = max(worst, abs(key - d) / (dn.REL * d + dn.ABS))
    print("largest |key - d| / bound:", worst)
    empty = np.zeros((16, 256))
    assert np.isinf(oracle_lib.delight_distance(empty, empty)[0, 0]) and np.isinf(dn.coarse_key(empty, empty, 1.0))


def test_rows_outside_the_image_are_not_coarse_exact():
    base = synth.delight_database(11, 1)
    assert dn.coarse_exact(base)
    for v in (-1.0, 0.5, np.nan, np.inf, 2.0 ** 24 + 2.0):
        x = base.copy(); x[3, 3] = v
        assert not dn.coarse_exact(x)


def test_containment_flags_exact_ties_and_near_copies():
    """A list of C rows out of C + 3 copies of one entry: the three unlisted copies tie with the k-th score exactly, so the rule must
    not call the list complete, whichever way the reciprocal errs on each copy."""
    db = synth.delight_database(12, 1).reshape(16, 256)
    q, _ = synth.delight_queries(13, db, 1)
    k, C = 5, 13
    for flip in (0, 1):
        rows = np.repeat(db[None], C + 3, 0)
        d = oracle_lib.delight_distance(q, rows.reshape(-1, 256))[0]
        keys = np.array([dn.coarse_key(q, r, 1.0 if (t + flip) % 2 else -1.0) for t, r in enumerate(rows)], np.float32)
        listed = np.argsort(keys, kind="stable")[:C]
        w = keys[listed].max()
        kth = np.sort(d[listed])[k - 1]
        assert np.sort(d)[k - 1] <= kth
        assert not dn.contained(kth, w)
    far = synth.delight_database(14, 40).reshape(40, 16, 256)                         # unrelated rows: the same list is complete
    keys = np.array([dn.coarse_key(q, r, 1.0) for r in far], np.float32)
    d = oracle_lib.delight_distance(q, db)[0, 0]
    assert dn.contained(d, keys.min())
    assert dn.contained(1.0, np.inf) and not dn.contained(np.inf, np.inf)


def test_cluster_construction_is_below_fp32_and_above_fp64():
    torch = pytest.importorskip("torch")
    for cs in (12, 40):
        db = synth.delight_signatures_torch(7, 100, device="cpu", clusters=1, cluster_size=cs).numpy()
        r0 = 50
        mem = db.reshape(100, 4096)[r0:r0 + cs]
        assert all(dn.coarse_exact(x) for x in mem)
        q = mem.min(0)
        q[5] += 5000.0
        d = oracle_lib.delight_distance(q.reshape(16, 256), db)[0]
        dm = d[r0:r0 + cs]
        assert len(set(dm.tolist())) == cs and len(set(dm.astype(np.float32).tolist())) == 1
        assert not np.array_equal(np.argsort(dm, kind="stable"), np.arange(cs))
        assert np.delete(d, np.arange(r0, r0 + cs)).min() > 2.0 * dm.max()
