"""The inputs of tests/m2dp_match_cases.py do what its docstring claims - conditions on the inputs, checked on the host: the f16 split of
every entry is (h, b 2^-12); every partial sum of a row pair is exact in fp32 in any order; the model changes in most outputs when one of
the split-f16 cross products is lost, and every one of the 16 variant pairs decides a share of the outputs (otherwise the GPU test could
pass over a kernel that drops a product or a variant); the model equals the fp64 oracle within the bound derived below."""
import numpy as np
import pytest

import m2dp_match_cases as M
import oracle_lib


@pytest.fixture(scope="module")
def full():
    q, db = M.grid()
    return {"q": q, "db": db, "exp": {a: M.expected(*M.cases(a), a) for a in M.ARITHS}}


def test_the_draw_is_the_stated_size_and_seeded():
    q, db = M.grid()
    assert q.shape == (4 * 97, 384) and db.shape == (4 * 1031, 384)
    q2, db2 = M._build()
    assert np.array_equal(q, q2) and np.array_equal(db, db2)


def test_f16_split_reproduces_h_and_b():
    for x in M.grid():
        hi, lo = M.split(x)
        assert np.isin(hi, (-3.0, -2.0, 2.0, 3.0)).all()
        b = lo * 4096.0
        assert np.array_equal(b, np.round(b)) and np.abs(b).max() == 3 and (b == 0).any()
        assert np.array_equal((hi + lo) / 256.0, x)                                   # nothing is left over: x = (h + b 2^-12) / 256
        two = np.abs(hi) == 2
        assert (b[two] * np.sign(hi[two]) >= 0).all() and (b[~two] * np.sign(hi[~two]) < 0).any()
        # the variants carry signs: every row has both, in both blocks of both channels
        blocks = x.reshape(-1, 2, 192)
        for part in (blocks[..., :64], blocks[..., 64:]):
            assert ((part > 0).any(-1) & (part < 0).any(-1)).all()
    for x, g in zip(M.grid32(), M.grid()):
        assert np.array_equal(x * 256.0, M.split(g)[0]) and np.array_equal(M.split(x)[1], np.zeros_like(x))
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)             # the fp32 pack's cast is exact


def test_every_partial_sum_is_exact_in_fp32(full):
    """Sum of |term| over the 576 terms of every row pair of the full 97 x 1031 set, at scale 2^12, is below 2^24, and every term is a
    multiple of 2^-12: whatever the order and grouping, no partial sum needs more than 24 bits."""
    worst = 0.0
    for ch in (0, 1):
        c = slice(192 * ch, 192 * ch + 192)
        qh, ql = (np.abs(a) for a in M.split(full["q"][:, c]))
        dh, dl = (np.abs(a) for a in M.split(full["db"][:, c]))
        for a in (qh, dh):
            assert np.array_equal(a, np.round(a))                                     # hi: integers
        for a in (ql, dl):
            assert np.array_equal(a * 4096.0, np.round(a * 4096.0))                   # lo: multiples of 2^-12, so is every product with a hi
        tot = (qh @ dh.T + qh @ dl.T + ql @ dh.T) * 4096.0
        worst = max(worst, tot.max())
    print(f"max sum of |terms| x 2^12 = {worst:.3g} (limit 2^24 = {2.0 ** 24:.3g})")
    assert worst < 2.0 ** 24


def test_fp32_accumulation_in_random_order_equals_the_model(full):
    rng = np.random.default_rng(7)
    s = M.model_s(full["q"], full["db"], "f16x2")
    s32 = M.model_s(*M.grid32(), "f32")
    g32 = M.grid32()
    for _ in range(200):
        ch, i, j = int(rng.integers(2)), int(rng.integers(4 * M.N_Q)), int(rng.integers(4 * M.N_DB))
        c = slice(192 * ch, 192 * ch + 192)
        qh, ql = M.split(full["q"][i, c])
        dh, dl = M.split(full["db"][j, c])
        terms = np.concatenate([qh * dh, qh * dl, ql * dh]).astype(np.float32)
        assert np.array_equal(terms.astype(np.float64), np.concatenate([qh * dh, qh * dl, ql * dh]))
        acc = np.float32(0.0)
        for t in terms[rng.permutation(576)]:
            acc = np.float32(acc + t)
        assert float(acc) == s[ch, i, j]
        # the fp32 kernel multiplies the unscaled values: products of h / 256 and their sums
        a, b = g32[0][i, c].astype(np.float32), g32[1][j, c].astype(np.float32)
        acc = np.float32(0.0)
        for k in rng.permutation(192):
            acc = np.float32(acc + np.float32(a[k] * b[k]))
        assert float(acc) * 65536.0 == s32[ch, i, j]


@pytest.mark.parametrize("drop", ["hl", "lh"])
def test_a_lost_cross_product_changes_most_outputs(full, drop):
    want = M.bits(full["exp"]["f16x2"])
    lost = M.bits(M.expected(full["q"], full["db"], "f16x2", drop))
    share = (want != lost).mean()
    print(f"model without {drop}: {100 * share:.1f} % of the outputs differ")
    assert share > 0.5
    for n in (1, 7, 8, 9, 63):                 # ... and at the small DB prefixes too, where a test has few outputs to see it in
        assert (want[:, :, :n] != lost[:, :, :n]).any()


def test_single_product_and_split_models_differ(full):
    assert (M.bits(full["exp"]["f16x2"]) != M.bits(full["exp"]["f16"])).mean() > 0.5


@pytest.mark.parametrize("arith", M.ARITHS)
def test_every_variant_pair_decides_a_share_of_the_outputs(full, arith):
    s = M.model_s(*M.cases(arith), arith)
    c, m4, n4 = s.shape
    blk = s.reshape(c, m4 // 4, 4, n4 // 4, 4).transpose(0, 1, 3, 2, 4).reshape(c, m4 // 4, n4 // 4, 16)
    mx = blk.max(-1, keepdims=True)
    unique = (blk == mx).sum(-1) == 1
    share = np.array([((blk.argmax(-1) == v) & unique).mean() for v in range(16)])
    print(f"{arith}: unique maximiser shares {np.round(100 * share, 1)} %")
    assert share.min() >= 0.01
    # a dropped variant pair changes the stored value wherever it was the unique maximiser
    second = np.sort(blk, -1)[..., -2]
    assert (M.bits((0.5 - second[unique] * 2.0 ** -17).astype(np.float32)) != M.bits((0.5 - mx[..., 0][unique] * 2.0 ** -17).astype(np.float32))).mean() > 0.9


def _oracle(q, db):
    rc, dp, di = oracle_lib.m2dp_distance(q, db)
    assert rc == 0
    return np.stack([dp, di])


def test_split_model_against_the_oracle_within_the_derived_bound(full):
    """The oracle takes the doubles as they are, so it differs from the split-f16 model by the lo.lo' products the kernel never forms
    - at most 192 (3 2^-12)^2 2^-17 < 1e-9 -, the model's one rounding to fp32 (half an ulp of the value) and its own fp64 summation
    (192 products of magnitude <= 1.4e-4 each, under 1e-15 in all)."""
    want = _oracle(full["q"], full["db"])
    got = full["exp"]["f16x2"].astype(np.float64)
    bound = 1e-9 + 0.5 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64) + 1e-15
    err = np.abs(got - want)
    print(f"split-f16 model against the oracle: max {err.max():.2e}, max bound {bound.max():.2e}")
    assert (err <= bound).all()
    # the single-product model lacks hi.lo' + lo.hi' as well: 2 x 192 x 3 x 3 2^-12 x 2^-17 on top
    err1 = np.abs(full["exp"]["f16"].astype(np.float64) - want)
    assert (err1 <= bound + 2 * 192 * 9 * 2.0 ** -12 * 2.0 ** -17).all()


def test_fp32_set_equals_the_oracle_exactly(full):
    want = _oracle(*M.grid32())
    assert M.first_difference(full["exp"]["f32"], want.astype(np.float32)) is None
    assert np.array_equal(full["exp"]["f32"].astype(np.float64), want)               # every distance of this set is an fp32 number already


def test_unit_family_values():
    q, db = M.unit_family()
    want = _oracle(q, db)
    for arith in M.ARITHS:
        d = M.expected(q, db, arith)
        assert np.array_equal(d.astype(np.float64), want)
        assert np.isin(d, M.UNIT_VALUES).all()
        for ch in (0, 1):
            assert set(np.unique(d[ch])) == set(M.UNIT_VALUES)
            assert (d[ch, M.UNIT_ZERO_Q] == 0.5).all() and (d[ch, :, M.UNIT_ZERO_DB] == 0.5).all()
    for a in (q, db):                                                                # 256 x = +-256: an f16, nothing left for lo
        hi, lo = M.split(a)
        assert np.isin(hi, (-256.0, 0.0, 256.0)).all() and not lo.any()


def test_unit_rows_against_grid_rows_are_exact():
    """A one-hot signature against grid rows: S = 256 (+-(h + b 2^-12) +- (h' + b' 2^-12)), two terms per arithmetic product."""
    uq, udb = M.unit_family()
    gq, gdb = M.grid()
    for q, db in ((uq, gdb[:4 * 65]), (gq[:4 * 33], udb)):
        want = _oracle(q, db)
        d = M.expected(q, db, "f16x2")
        assert np.abs(d.astype(np.float64) - want).max() <= 0.5 * np.spacing(np.float32(0.5))    # no lo.lo': a unit row has no lo
        assert (M.bits(d) != M.bits(M.expected(q, db, "f16"))).any()
