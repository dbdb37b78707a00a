"""The rule of the sequence matcher (pr_seq_select_dev and pr_seqmatch; the text of include/place_recognition.h) restated
in NumPy, fp64 throughout.  Written from the header, not from the kernels: no tiles, no halo, no lists held in registers - whole rows,
one velocity and one lag at a time.  NumPy's element-wise fp64 operations are the IEEE ones and nothing is contracted, so the device
(built with -ffp-contract=off) equals this bit for bit."""
import numpy as np

MAX_L, MAX_V, MAX_STEP, MAX_K = 32, 16, 64, 32
ONLINE_MAX_K = 128
LANES = 256            # partial sums of the online row statistics


def seq_steps(L, velocities):
    """api.seq_steps restated: the entry for lag l is sign(v) * floor(|v| l + 0.5); identical rows are dropped, keeping the first."""
    rows = []
    for v in velocities:
        sg = (v > 0) - (v < 0)
        row = [int(sg * np.floor(abs(float(v)) * l + 0.5)) for l in range(L)]
        if row not in rows:
            rows.append(row)
    return np.array(rows, np.int32).reshape(len(rows), L)


def row_usable(row):
    """a row of a DEVICE table that breaks the rule is a dropped velocity"""
    return row[0] == 0 and int(np.abs(row).max()) <= MAX_STEP


def cell_scores(d_p, d_i, mom, p_weight):
    """rule 1"""
    if d_i is None:
        return d_p.astype(np.float64)
    with np.errstate(all="ignore"):
        mean_p, sd_p = mom[:, 0, 1], np.sqrt(mom[:, 0, 2] / (mom[:, 0, 0] - 1.0))
        mean_i, sd_i = mom[:, 1, 1], np.sqrt(mom[:, 1, 2] / (mom[:, 1, 0] - 1.0))
        zp = (d_p.astype(np.float64) - mean_p[:, None]) / sd_p[:, None]
        zi = (d_i.astype(np.float64) - mean_i[:, None]) / sd_i[:, None]
        return np.float64(p_weight) * zp + zi


def seq_dense(d_p, d_i, mom, steps, q_row0=0, db_row0=0, mask_width=0, p_weight=2.0):
    """rules 1 - 6 -> (S f64 [m, n] with +Inf where the cell is no candidate, vel i32 [m, n] with -1 there)"""
    m, n = d_p.shape
    V, L = steps.shape
    f = cell_scores(d_p, d_i, mom, p_weight)
    a, c = np.arange(m, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    f = np.where(np.abs((q_row0 + a) - (db_row0 + c)) < mask_width, np.nan, f)            # a masked cell cannot be a term
    S = np.full((m, n), np.inf)
    vel = np.full((m, n), -1, np.int32)
    cols0 = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(m):
            Li = min(L, i + 1)
            best, bv = np.full(n, np.nan), np.full(n, -1, np.int32)
            for v in range(V):
                if not row_usable(steps[v]):
                    continue
                s = np.zeros(n)
                for l in range(Li):
                    cols = cols0 - int(steps[v, l])
                    ok = (cols >= 0) & (cols < n)
                    s = s + np.where(ok, f[i - l, np.clip(cols, 0, n - 1)], np.nan)
                q = s / np.float64(Li)
                better = ~np.isnan(q) & ((bv < 0) | (q < best))
                best, bv = np.where(better, q, best), np.where(better, v, bv).astype(np.int32)
            S[i], vel[i] = np.where(bv >= 0, best, np.inf), bv
    return S, vel


def topk_rows(S, vel, k, db_row0=0):
    """rule 7"""
    m, n = S.shape
    idx, score, v = np.full((m, k), -1, np.int32), np.full((m, k), np.nan), np.full((m, k), -1, np.int32)
    for i in range(m):
        cand = np.flatnonzero(vel[i] >= 0)
        order = cand[np.lexsort((cand, S[i, cand]))][:k]
        t = len(order)
        idx[i, :t], score[i, :t], v[i, :t] = db_row0 + order, S[i, order], vel[i, order]
    return idx, score, v


def seq_select(d_p, d_i, mom, steps, q_row0=0, db_row0=0, mask_width=0, p_weight=2.0, k=1):
    """pr_seq_select_dev -> (idx, score, vel, S)"""
    S, vel = seq_dense(d_p, d_i, mom, steps, q_row0, db_row0, mask_width, p_weight)
    return (*topk_rows(S, vel, k, db_row0), S)


def row_moments(d):
    """(count, mean, M2) per row over the non-NaN entries, fp64 two-pass: the shape of mom [m][3] of one channel.  (A stand-in for
    pr_row_moments_dev in tests that make their own moments: the sequence rule takes mom as an input.)"""
    x = d.astype(np.float64)
    ok = ~np.isnan(x)
    cnt = ok.sum(1).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.where(cnt > 0, np.where(ok, x, 0.0).sum(1) / np.maximum(cnt, 1.0), 0.0)
        m2 = np.where(ok, (x - mean[:, None]) ** 2, 0.0).sum(1)
    return np.stack([cnt, mean, m2], 1)


# ---------------------------------------------------------------------------------------------------------------- the online form
def lane_tree_sum(x):
    """The online row statistics' one order of summation, fixed by len(x) alone: partial sum t of 256 adds the non-NaN x[j], j = t,
    t + 256, ... in ascending j from 0.0; then p[t] += p[t + s] for s = 128, 64, .. 1; the sum is p[0]."""
    p = np.zeros(LANES)
    for r in range(0, len(x), LANES):
        ch = x[r:r + LANES]
        ok = ~np.isnan(ch)
        p[:len(ch)] = np.where(ok, p[:len(ch)] + np.where(ok, ch, 0.0), p[:len(ch)])
    s = LANES // 2
    while s > 0:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


class SeqFilter:
    """pr_seqmatch restated: the ring of the last L fused rows, the slots' row ids and the push counter."""

    def __init__(self, capacity, channels, steps, max_k):
        self.cap, self.ch, self.steps, self.max_k = capacity, channels, np.asarray(steps, np.int32), max_k
        self.V, self.L = self.steps.shape
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.L, self.cap))
        self.ids = np.zeros(self.L, np.int32)
        self.pushes = 0

    def fused_row(self, rows, n, weights, normalize):
        """rule 2: F_n[j], j < n"""
        if not normalize:
            return rows[0, :n].astype(np.float64).copy()
        F = np.zeros(n)
        with np.errstate(all="ignore"):
            for c in range(self.ch):
                x = rows[c, :n]
                cnt = np.float64((~np.isnan(x)).sum())
                mean = lane_tree_sum(x) / cnt
                d = x - mean
                sd = np.sqrt(lane_tree_sum(d * d) / (cnt - 1.0))
                F = F + np.float64(weights[c]) * ((x - mean) / sd)
        return F

    def push(self, rows, count, weights, normalize=True, mask_width=0, k=1, emitted=None):
        """-> (idx i32 [k], score f64 [k], vel i32 [k], info i32 [4])"""
        idx, score, vel = np.full(k, -1, np.int32), np.full(k, np.nan), np.full(k, -1, np.int32)
        if emitted is not None and emitted == 0:
            return idx, score, vel, np.array([0, 0, self.pushes, 0], np.int32)
        n = min(max(int(count), 0), self.cap)
        L, slot = self.L, self.pushes % self.L
        F = self.fused_row(np.asarray(rows, np.float64).reshape(self.ch, self.cap), n, weights, normalize)
        self.ring[slot, :n] = F
        Ln = min(L, self.pushes + 1)
        j = np.arange(n)
        best, bv = np.full(n, np.nan), np.full(n, -1, np.int32)
        with np.errstate(all="ignore"):
            for v in range(self.V):
                s = np.zeros(n) + F
                for l in range(1, Ln):
                    sl = (self.pushes - l) % L
                    nl = int(self.ids[sl])
                    c = j - int(self.steps[v, l])
                    ok = (c >= 0) & (c < nl) & (np.abs(nl - c) >= mask_width)
                    s = s + np.where(ok, self.ring[sl, np.clip(c, 0, self.cap - 1)], np.nan)
                q = s / np.float64(Ln)
                better = ~np.isnan(q) & ((bv < 0) | (q < best))
                best, bv = np.where(better, q, best), np.where(better, v, bv).astype(np.int32)
        cand = np.flatnonzero((bv >= 0) & (n - j >= mask_width))
        order = cand[np.lexsort((cand, best[cand]))][:k]
        t = len(order)
        idx[:t], score[:t], vel[:t] = order, best[order], bv[order]
        self.ids[slot] = n
        self.pushes += 1
        return idx, score, vel, np.array([1, Ln, self.pushes, 0], np.int32)
