"""CPU restatements behind the two-stage GIST matcher (gist_match.hip): the normative fp64 arithmetic, the error bound of
the coarse f16 pass, and the containment rule that decides whether a candidate list provably holds the exact top-k."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from so_dso_place_recognition_amd import synth

U23 = 2.0 ** -23


def seq_distance(a, b):
    """d = ((0 + t_0) + t_1) + ..., t_c = RN(RN(a_c - b_c)^2): one rounding per operation, ascending columns"""
    d = np.zeros((len(a), len(b)))
    for c in range(a.shape[1]):
        t = a[:, c][:, None] - b[:, c][None, :]
        d = d + t * t
    return d


def fma_distance(a, b):
    """acc = fma(t, t, acc): the square is not rounded on its own"""
    out = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            acc = 0.0
            for c in range(a.shape[1]):
                t = float(a[i, c] - b[j, c])
                acc = float(Fraction(t) * Fraction(t) + Fraction(acc))
            out[i, j] = acc
    return out


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def test_normative_arithmetic_is_the_oracles_and_no_other():
    a = synth.gist_signatures(1, 4, 33)
    b = synth.gist_signatures(2, 6, 33)
    want = oracle_lib.gist_distance(a, b)
    assert np.array_equal(bits(seq_distance(a, b)), bits(want))
    assert np.any(bits(fma_distance(a, b)) != bits(want))
    expanded = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    assert np.any(bits(expanded) != bits(want))


# ---------------------------------------------------------------------------------------------- the pack and the coarse key, as the kernels do
def pack(rows, mu):
    """-> (a' as float64, nd float32, rs float32): f16 rounding through fp32, subnormals flushed, |a'|^2 and the residual norm rounded up"""
    v = rows - mu[None, :]
    with np.errstate(over="ignore"):
        h = v.astype(np.float32).astype(np.float16)
    h = np.where(np.abs(h.astype(np.float32)) < 2.0 ** -14, np.float16(0), h)
    hd = h.astype(np.float64)
    assert np.all(np.isfinite(hd))
    nrm = (hd * hd).sum(1)
    res = ((v - hd) ** 2).sum(1)
    r = np.sqrt(res) * (1 + 2.0 ** -20) + 2.0 ** -48 * (np.sqrt(nrm) + np.sqrt(res))
    rs = np.nextafter(r.astype(np.float32), np.float32(np.inf))
    rs = np.where((r > 0) & (rs < 2.0 ** -120), np.float32(2.0 ** -120), rs).astype(np.float32)
    return hd, nrm.astype(np.float32), rs


def coarse_keys(qa, qn, da, dn):
    """key = fma(-2, acc, nq + nd) in fp32, acc accumulated in fp32 (here column by column; the bound holds for any order)"""
    acc = np.zeros((len(qa), len(da)), np.float32)
    for c in range(qa.shape[1]):
        acc = acc + (qa[:, c].astype(np.float32)[:, None] * da[:, c].astype(np.float32)[None, :])
    s = qn[:, None] + dn[None, :]
    return (s.astype(np.float64) - 2.0 * acc.astype(np.float64)).astype(np.float32)


def lower_bound(key, nq, ndmax, rq, rbmax, cols):
    """L with d >= L for every row whose key is >= `key` (gist_rerank_kernel)"""
    KP = (cols + 63) // 64 * 64
    eacc = (KP + 8) * U23 * (float(nq) + float(ndmax)) * 1.01
    x = float(key) - eacc
    if not x > 0.0:
        return 0.0
    y = np.sqrt(x) * (1 - 2.0 ** -40) - float(rq) - float(rbmax)
    return y * y * (1 - (cols + 8) * 2.0 ** -50) if y > 0 else 0.0


def cases(rng):
    yield "random", synth.gist_signatures(5, 12, 96), synth.gist_signatures(6, 300, 96)
    off = 1e3 + 1e-3 * rng.normal(size=(312, 40))
    yield "offset", off[:12], off[12:]
    tiny = 1e-6 * rng.random((312, 40))
    yield "tiny", tiny[:12], tiny[12:]
    z = synth.gist_signatures(7, 312, 70)
    z[rng.random(z.shape) < 0.5] = 0.0
    z[5] = 0.0
    z[40] = 0.0
    yield "zeros", z[:12], z[12:]


def test_coarse_key_stays_within_the_bound():
    rng = np.random.default_rng(3)
    for name, q, db in cases(rng):
        for mu in (db[:1024].mean(0), np.zeros(db.shape[1])):
            qa, qn, qr = pack(q, mu)
            da, dn, dr = pack(db, mu)
            key = coarse_keys(qa, qn, da, dn)
            d = oracle_lib.gist_distance(q, db)
            for i in range(len(q)):
                for j in range(len(db)):
                    L = lower_bound(key[i, j], qn[i], dn[j], qr[i], dr[j], q.shape[1])      # this pair's own E(i, j)
                    assert d[i, j] >= L, (name, i, j, d[i, j], L)
            # and the bound is not vacuous where the data allow it
            if name == "random":
                Ls = np.array([[lower_bound(key[i, j], qn[i], dn.max(), qr[i], dr.max(), 96) for j in range(len(db))] for i in range(len(q))])
                assert np.all(Ls > 0.97 * d - 1e-2)


def contained(cand_exact_sorted, k, w, nq, ndmax, rq, rbmax, cols):
    if len(cand_exact_sorted) < k or not (np.isfinite(ndmax) and np.isfinite(rbmax)):      # a row outside the f16 range is never listed
        return False
    L = np.inf if w == np.inf else lower_bound(w, nq, ndmax, rq, rbmax, cols)
    return bool(cand_exact_sorted[k - 1] < L)


@pytest.mark.parametrize("seed", range(6))
def test_containment_never_accepts_an_incomplete_list(seed):
    rng = np.random.default_rng(100 + seed)
    cols, n, k = 64, 400, int(rng.choice([1, 5]))
    C = k + 8
    db = synth.gist_signatures(200 + seed, n, cols)
    size = int(rng.integers(2, 65))
    eps = float(rng.choice([0.0, 1e-9, 1e-6, 1e-3]))
    r0 = int(rng.integers(0, n - size))
    db[r0:r0 + size] = db[r0] + eps * rng.normal(size=(size, cols))
    q = np.concatenate([db[r0:r0 + 4] + eps * rng.normal(size=(4, cols)), synth.gist_signatures(300 + seed, 12, cols)])
    mu = db.mean(0)
    qa, qn, qr = pack(q, mu)
    da, dn, dr = pack(db, mu)
    key = coarse_keys(qa, qn, da, dn)
    d = oracle_lib.gist_distance(q, db)
    accepted = plain = 0
    for i in range(len(q)):
        order = np.argsort(key[i], kind="stable")
        lst = order[:C]
        w = key[i, order[C - 1]]                               # the largest listed key: every row outside has key >= w
        ex = sorted((d[i, j], j) for j in lst)
        truth = sorted((d[i, j], j) for j in range(n))[:k]
        if contained([e[0] for e in ex], k, w, qn[i], dn.max(), qr[i], dr.max(), cols):
            accepted += 1
            plain += i >= 4
            assert ex[:k] == truth, (seed, i)
    assert plain > 0, "the rule accepted none of the 12 queries outside the cluster: the test would be vacuous"


def test_containment_rejects_when_a_row_left_the_f16_range():
    assert contained([0.1, 0.2], 1, np.inf, 1.0, 1.0, 1e-4, 1e-4, 64)
    assert not contained([0.1, 0.2], 1, np.inf, 1.0, np.inf, 1e-4, np.inf, 64)


def test_matcher_arguments_need_no_device():
    from so_dso_place_recognition_amd import matcher
    for bad in ((0, 10, 8), (4, 0, 8), (4, 10, 0)):
        with pytest.raises(ValueError):
            matcher.GistMatcher(*bad)
