"""The online signature database (pr_online) restated in NumPy over the CPU oracle: the normative statement of the append /
emitted / overflow rule and of a match against the rows held so far.  The device tests compare the kernels with this; the CPU tests check
its own properties."""
import numpy as np

import oracle_lib

OVERFLOW = 1
SHAPES = {"sc": (1, 2400), "m2dp": (4, 384)}


def distances(type_, sig, rows):
    """(d_p [n], d_i [n]) of one query signature against n database entries, by the oracle (processSC.m / processM2DP.m)."""
    rps, L = SHAPES[type_]
    q = np.ascontiguousarray(sig, np.float64).reshape(rps, L)
    db = np.ascontiguousarray(rows, np.float64).reshape(-1, L)
    n = db.shape[0] // rps
    if n == 0:
        return np.empty(0), np.empty(0)
    _, dp, di = (oracle_lib.sc_distance if type_ == "sc" else oracle_lib.m2dp_distance)(q, db)     # (PR_REF_ENAN: the NaN are in dp / di)
    return dp[0].copy(), di[0].copy()


def match_rows(dp, di, mask_width, p_weight, k):
    """run_test.m:38-57 for the query that will become row n = len(dp): it sits in the LAST row of an (n + 1) x n distance matrix, so the
    oracle's mask |i - j| < mask_width sees i = n.  Under two entries there are no row statistics: every slot is -1 / NaN.
    Returns (idx int32 [1, k], score f64 [1, k])."""
    n = len(dp)
    idx = np.full((1, k), -1, np.int32)
    score = np.full((1, k), np.nan)
    if n < 2:
        return idx, score
    Dp = np.zeros((n + 1, n)); Di = np.zeros((n + 1, n))
    Dp[n] = dp; Di[n] = di
    with np.errstate(all="ignore"):
        oi, os_ = oracle_lib.fuse_topk(Dp, Di, int(mask_width), float(p_weight), int(k))
    idx[0] = oi[n]; score[0] = os_[n]
    return idx, score


class OnlineModel:
    def __init__(self, type_, capacity):
        self.type = type_
        self.rps, self.L = SHAPES[type_]
        self.capacity = int(capacity)
        self.sig = np.zeros((self.capacity * self.rps, self.L))
        self.state = np.zeros(4, np.int32)

    @property
    def count(self):
        return int(self.state[0])

    def reset(self):
        self.state[:] = 0

    def append(self, sig, emitted=None):
        """info int32 [4] = appended, row | -1, count after, flags"""
        n, flags = int(self.state[0]), int(self.state[1])
        if emitted is not None and int(np.asarray(emitted).reshape(-1)[0]) == 0:
            return np.array([0, -1, n, flags], np.int32)
        if n >= self.capacity:
            flags |= OVERFLOW
            self.state[1] = flags
            return np.array([0, -1, n, flags], np.int32)
        self.sig[n * self.rps:(n + 1) * self.rps] = np.asarray(sig, np.float64).reshape(self.rps, self.L)
        self.state[0] = n + 1
        return np.array([1, n, n + 1, flags], np.int32)

    def match(self, sig, mask_width=0, p_weight=2.0, k=1, emitted=None):
        """(idx int32 [1, k], score f64 [1, k], d_p [count], d_i [count]); emitted[0] == 0: all -1 / NaN and no distances"""
        if emitted is not None and int(np.asarray(emitted).reshape(-1)[0]) == 0:
            return np.full((1, k), -1, np.int32), np.full((1, k), np.nan), np.empty(0), np.empty(0)
        dp, di = distances(self.type, sig, self.sig[:self.count * self.rps])
        return match_rows(dp, di, mask_width, p_weight, k) + (dp, di)

    def step(self, sig, mask_width=0, p_weight=2.0, k=1, emitted=None):
        idx, score, _, _ = self.match(sig, mask_width, p_weight, k, emitted)
        return idx, score, self.append(sig, emitted)
