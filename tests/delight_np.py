"""numpy restatements behind the two-stage DELIGHT matcher (delight_match.hip): the normative fp64 arithmetic, a float32
emulation of the coarse key with an injectable reciprocal error, and the bound and the containment rule as the kernels apply them."""
import numpy as np

XORS = (0, 5, 6, 3)                      # entry row r ^ X against query row r (processDELIGHT.m:2-5)
REL = 4200.0 * 2.0 ** -24                # |key - d| <= REL d + ABS (delight_match.hip: DM_REL, DM_ABS)
ABS = float.fromhex("0x1.01p-17")
RCP_ERR = 2.0 ** -23                     # v_rcp_f32: 1 ulp


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def distance(h1, h2, order="column", form="normative"):
    """[m, n] fp64 distances of h1 [16 m, 256] against h2 [16 n, 256], one rounding per operation.
    order: 'column' (c outer, r inner: the normative one) or 'row'; form: 'normative' ((2 (a - b)) (a - b)) / sum,
    'divide_first' (2 (a - b)) ((a - b) / sum), or 'square_first' (2 ((a - b) (a - b))) / sum."""
    A = np.asarray(h1, np.float64).reshape(-1, 16, 256)
    B = np.asarray(h2, np.float64).reshape(-1, 16, 256)
    m, n = len(A), len(B)
    best = np.full((m, n), np.inf)
    steps = [(r, c) for c in range(256) for r in range(16)] if order == "column" else [(r, c) for r in range(16) for c in range(256)]
    with np.errstate(all="ignore"):
        for x in XORS:
            ts = np.zeros((m, n)); tc = np.zeros((m, n))
            for r, c in steps:
                a = A[:, r, c][:, None]; b = B[:, r ^ x, c][None, :]
                s = a + b; d = a - b
                if form == "normative":
                    t = ((2.0 * d) * d) / s
                elif form == "divide_first":
                    t = (2.0 * d) * (d / s)
                else:
                    t = (2.0 * (d * d)) / s
                on = s > 0
                ts = np.where(on, ts + t, ts); tc = np.where(on, tc + 1.0, tc)
            ts = ts / tc
            best = np.where(best > ts, ts, best)
    return best


def coarse_exact(sig):
    """the per-row flag of the pack: every element an integer in [0, 2^24]"""
    s = np.asarray(sig, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((s >= 0) & (s <= 2.0 ** 24) & (s == np.floor(s))))


def coarse_key(a, b, rcp_sign):
    """The coarse kernel's key of one pair (a, b: [16, 256] coarse-exact) in float32, operation by operation (delight.hip chi2_perm4 and
    the reduction of delight_match_kernel), with the reciprocal's relative error set to rcp_sign * RCP_ERR (scalar or [16, 256])."""
    f = np.float32
    A = a.astype(f) + f(2.0 ** -30)
    B = b.astype(f)
    rows = np.arange(16)
    with np.errstate(all="ignore"):
        s = [A + B[rows ^ x] for x in XORS]
        d = [A - B[rows ^ x] for x in XORS]
        p01 = s[0] * s[1]; p23 = s[2] * s[3]; P = p01 * p23
        R = ((1.0 / P.astype(np.float64)) * (1.0 + np.asarray(rcp_sign, np.float64) * RCP_ERR)).astype(f)
        q23 = R * p23; q01 = R * p01
        rec = [q23 * s[1], q23 * s[0], q01 * s[3], q01 * s[2]]
        za = a == 0
        key = f(np.inf)
        for k, x in enumerate(XORS):
            t = ((d[k] * d[k]).astype(np.float64) * rec[k].astype(np.float64)).reshape(16, 64, 2, 2)   # [r][lane][h][component]
            acc = np.zeros((64, 2), f)
            for r in range(16):
                for h in range(2):
                    acc = (acc.astype(np.float64) + t[r, :, h, :]).astype(f)                          # fma: one rounding
            ts = acc[:, 0] + acc[:, 1]
            for o in (32, 16, 8, 4, 2, 1):
                ts = ts + ts[np.arange(64) ^ o]
            tc = f(4096 - int(np.sum(za & (b[rows ^ x] == 0))))
            v = f(2.0) * ts[0] / tc
            if key > v:
                key = v
    return key


def lower_bound(w):
    """L of the containment test: every row outside the lists has d >= L"""
    if not w < np.inf:
        return np.inf
    return max(0.0, (float(w) - ABS) / (1.0 + REL) * (1.0 - 2.0 ** -40))


def contained(kth_score, w):
    return bool(kth_score < lower_bound(w))
