"""The property the inverted-file BoW matcher rests on, checked on the CPU: accumulating, per (query, entry) pair, the common words'
terms ((s + |va - vb|) - |va|) - |vb| word-major in ascending word order from +0.0 gives processBoW.m's merge result bit for bit on
CONFORMING rows (ids integers in [0, n_words), strictly ascending before the row's end), and not on the other kinds - which is why the
library rejects them.  The row's end is the reference's: the first column p < cols - 1 with !(id > -1); the last column is never read."""
import numpy as np
import pytest

import oracle_lib


def row_length(ids):
    cols = len(ids)
    p = 0
    while p < cols - 1 and ids[p] > -1:
        p += 1
    return p


def conforming(ids, n_words):
    L = row_length(ids)
    x = ids[:L]
    return bool(np.all(x == np.rint(x)) and np.all(x < n_words) and np.all(np.diff(x) > 0))


def inverted_distance(h1, h2, n_words):
    """numpy restatement of the library's index: word-major postings of the DB rows, each query's words applied in ascending order.
    Ids the index cannot hold (fractional, >= n_words) have no postings."""
    m, n = h1.shape[0] // 2, h2.shape[0] // 2
    post = {}
    for j in range(n):
        ids, w = h2[2 * j], h2[2 * j + 1]
        for p in range(row_length(ids)):
            x = ids[p]
            if x == np.rint(x) and 0 <= x < n_words:
                post.setdefault(int(x), []).append((j, w[p]))
    acc = np.zeros((m, n))
    for i in range(m):
        ids, w = h1[2 * i], h1[2 * i + 1]
        for p in range(row_length(ids)):
            x = ids[p]
            if not (x == np.rint(x) and 0 <= x < n_words):
                continue
            va = w[p]
            for j, vb in post.get(int(x), []):
                acc[i, j] = ((acc[i, j] + abs(va - vb)) - abs(va)) - abs(vb)
    return 1.0 - (-acc / 2.0)


def random_rows(rng, n, cols, vocab, every=None):
    out = -np.ones((2 * n, cols))
    for r in range(n):
        k = int(rng.integers(0, cols + 1))
        ids = np.sort(rng.choice(np.arange(1 if every is not None else 0, vocab), size=min(k, vocab - 1), replace=False)).astype(np.float64)
        if every is not None:
            ids = np.concatenate([[every], ids])[:cols]
        k = len(ids)
        w = rng.normal(0.1, 0.2, k)
        w[rng.random(k) < 0.1] = 0.0
        out[2 * r, :k] = ids
        out[2 * r + 1, :k] = w
        if k < cols:
            out[2 * r, k] = rng.choice([-1.0, -7.5, np.nan])
            out[2 * r, k + 1:] = rng.integers(-3, vocab, cols - k - 1)        # whatever lies behind the end is never read
    return out


def bits_equal(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize("cols", [2, 8, 40])
def test_inverted_file_equals_merge_on_conforming_rows(cols):
    rng = np.random.default_rng(cols)
    vocab = 60
    h1 = random_rows(rng, 12, cols, vocab)
    h2 = random_rows(rng, 30, cols, vocab, every=0.0)                      # word 0 in every DB row: a list as long as the DB
    assert all(conforming(r, vocab) for r in list(h1[0::2]) + list(h2[0::2]))
    assert bits_equal(inverted_distance(h1, h2, vocab), oracle_lib.bow_distance(h1, h2))


def test_nan_weights_propagate_like_the_merge():
    h1 = np.array([[1, 4, 9, -1], [0.5, np.nan, 0.25, -1]], np.float64)
    h2 = np.array([[4, 9, -1, -1], [0.3, -0.2, -1, -1], [1, 2, -1, -1], [0.1, 0.1, -1, -1]], np.float64)
    d = oracle_lib.bow_distance(h1, h2)
    assert np.isnan(d[0, 0]) and not np.isnan(d[0, 1])
    assert bits_equal(inverted_distance(h1, h2, 10), d)


@pytest.mark.parametrize("kind", ["duplicate", "descending", "out_of_range", "fractional"])
def test_non_conforming_rows_break_the_equality(kind):
    n_words = 10
    q = {"duplicate": [3, 3, -1, -1], "descending": [5, 3, -1, -1], "out_of_range": [2, 12, -1, -1], "fractional": [2.5, 4, -1, -1]}[kind]
    db = {"duplicate": [3, -1, -1, -1], "descending": [3, 5, -1, -1], "out_of_range": [2, 12, -1, -1], "fractional": [2.5, 4, -1, -1]}[kind]
    h1 = np.array([q, [0.5, 0.25, -1, -1]], np.float64)
    h2 = np.array([db, [0.25, 0.5, -1, -1]], np.float64)
    assert not conforming(h1[0], n_words)
    assert not bits_equal(inverted_distance(h1, h2, n_words), oracle_lib.bow_distance(h1, h2))


def test_row_end_is_the_references():
    # terminators -1, -7.5, NaN: nothing behind them is read; the last column is never read (a full row drops its last word)
    for term in (-1.0, -7.5, np.nan):
        h1 = np.array([[1, 2, term, 3, 3], [0.5, 0.5, 0.5, 0.5, 0.5]], np.float64)
        h2 = np.array([[3, -1, -1, -1, -1], [0.5, -1, -1, -1, -1]], np.float64)
        assert row_length(h1[0]) == 2 and conforming(h1[0], 10)
        assert oracle_lib.bow_distance(h1, h2)[0, 0] == 1.0 == inverted_distance(h1, h2, 10)[0, 0]
    h1 = np.array([[1, 2, 3], [0.5, 0.25, 0.25]], np.float64)
    h2 = np.array([[3, -1, -1], [0.5, -1, -1]], np.float64)
    assert row_length(h1[0]) == 2
    assert oracle_lib.bow_distance(h1, h2)[0, 0] == 1.0 == inverted_distance(h1, h2, 10)[0, 0]
    # an id just above -1 before the end is read (and is not conforming); -1 itself ends the row
    assert row_length(np.array([-0.5, 2, 3, 0])) == 3 and not conforming(np.array([-0.5, 2, 3, 0]), 10)
