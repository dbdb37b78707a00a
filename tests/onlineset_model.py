"""The online signature sets (pr_onlineset) restated in NumPy over the CPU oracle: the normative statement of a match of a
FUSED (SC + M2DP, BASELINE config 5) or a DELIGHT set against the rows held so far, and of the append / emitted / overflow rule with ONE
count for all parts.  The device tests compare the kernels with this; the CPU tests check its own properties."""
import numpy as np

import online_model
import oracle_lib

OVERFLOW = online_model.OVERFLOW
PARTS = {"fused": (("sc", 1, 2400), ("m2dp", 4, 384)), "delight": (("delight", 16, 256),)}
CHANNELS = {"fused": 4, "delight": 1}


def as_parts(kind, sigs):
    """the keyframe's parts as a tuple of float64 arrays [rows, len] in PARTS order"""
    ts = tuple(sigs) if isinstance(sigs, (tuple, list)) else (sigs,)
    assert len(ts) == len(PARTS[kind])
    return tuple(np.ascontiguousarray(t, np.float64).reshape(r, L) for t, (_, r, L) in zip(ts, PARTS[kind]))


def distances(kind, sigs, rows):
    """d [C, n]: the distances of one query to the n entries of `rows` (a tuple of the parts' row arrays), by the oracle.  FUSED: C = 4 in
    the order SC structure, SC intensity, M2DP count, M2DP intensity, each part through online_model.distances; DELIGHT: C = 1."""
    q = as_parts(kind, sigs)
    if kind == "fused":
        d0, d1 = online_model.distances("sc", q[0], rows[0])
        d2, d3 = online_model.distances("m2dp", q[1], rows[1])
        assert len(d0) == len(d2)
        return np.stack([d0, d1, d2, d3])
    db = np.ascontiguousarray(rows[0], np.float64).reshape(-1, 256)
    if db.shape[0] == 0:
        return np.empty((1, 0))
    return oracle_lib.delight_distance(q[0], db)[0:1].copy()


def fused_scores(d, p_weight):
    """f [n] of d [4, n] in pr_ref_match_topk_fused's order: per channel the mean over the entries that are not NaN, the variance about
    it (N - 1), then f = 0; f += p z0; f += 1 z1; f += p z2; f += 1 z3.  Sequential sums, as the oracle's loops."""
    n = d.shape[1]
    f = np.zeros(n)
    with np.errstate(all="ignore"):
        for c in range(4):
            a = d[c]
            ok = ~np.isnan(a)
            cnt = int(ok.sum())
            mu = 0.0
            for x in a[ok]:
                mu += x
            mu = mu / cnt if cnt else np.nan
            va = 0.0
            for x in a[ok]:
                va += (x - mu) * (x - mu)
            sd = np.sqrt(np.float64(va) / np.float64(cnt - 1)) if cnt != 1 else np.nan
            wt = float(p_weight) if c % 2 == 0 else 1.0
            f = f + wt * ((a - mu) / sd)
    return f


def select(f, mask_width, k):
    """run_test.m:47-57 for the query that will become row n = len(f): oracle_lib.select_topk on an (n + 1) x n matrix whose LAST row is
    the query, so the oracle's mask |i - j| < mask_width sees i = n.  The mask comes after the scores: a masked NaN is a selectable +Inf."""
    n = len(f)
    idx = np.full((1, k), -1, np.int32)
    score = np.full((1, k), np.nan)
    if n == 0:
        return idx, score
    M = np.zeros((n + 1, n))
    M[n] = f
    rc, oi, os_ = oracle_lib.select_topk(M, int(mask_width), int(k))
    assert rc == 0
    idx[0] = oi[n]; score[0] = os_[n]
    return idx, score


def match_rows(kind, d, mask_width, p_weight, k):
    """(idx int32 [1, k], score f64 [1, k]) of the distances d [C, n].  FUSED under two entries: no statistics, every slot -1 / NaN.
    DELIGHT: the score is the distance (run_test.m:26-41), one entry is enough."""
    n = d.shape[1]
    if kind == "fused":
        if n < 2:
            return np.full((1, k), -1, np.int32), np.full((1, k), np.nan)
        return select(fused_scores(d, p_weight), mask_width, k)
    return select(d[0], mask_width, k)


class OnlineSetModel:
    def __init__(self, kind, capacity):
        self.kind = kind
        self.parts = PARTS[kind]
        self.capacity = int(capacity)
        self.bufs = {n: np.zeros((self.capacity * r, L)) for n, r, L in self.parts}
        self.state = np.zeros(4, np.int32)

    @property
    def count(self):
        return int(self.state[0])

    def reset(self):
        self.state[:] = 0

    def rows(self, n=None):
        n = self.count if n is None else n
        return tuple(self.bufs[name][:n * r] for name, r, _ in self.parts)

    def append(self, sigs, emitted=None):
        """info int32 [4] = appended, row | -1, count after, flags.  Every part goes to the same row or none does."""
        n, flags = int(self.state[0]), int(self.state[1])
        if emitted is not None and int(np.asarray(emitted).reshape(-1)[0]) == 0:
            return np.array([0, -1, n, flags], np.int32)
        if n >= self.capacity:
            flags |= OVERFLOW
            self.state[1] = flags
            return np.array([0, -1, n, flags], np.int32)
        for a, (name, r, _) in zip(as_parts(self.kind, sigs), self.parts):
            self.bufs[name][n * r:(n + 1) * r] = a
        self.state[0] = n + 1
        return np.array([1, n, n + 1, flags], np.int32)

    def match(self, sigs, mask_width=0, p_weight=2.0, k=1, emitted=None):
        """(idx int32 [1, k], score f64 [1, k], d [C, count]); emitted[0] == 0: all -1 / NaN and no distances"""
        C = CHANNELS[self.kind]
        if emitted is not None and int(np.asarray(emitted).reshape(-1)[0]) == 0:
            return np.full((1, k), -1, np.int32), np.full((1, k), np.nan), np.empty((C, 0))
        d = distances(self.kind, sigs, self.rows()) if self.count else np.empty((C, 0))
        return match_rows(self.kind, d, mask_width, p_weight, k) + (d,)

    def step(self, sigs, mask_width=0, p_weight=2.0, k=1, emitted=None):
        idx, score, _ = self.match(sigs, mask_width, p_weight, k, emitted)
        return idx, score, self.append(sigs, emitted)
