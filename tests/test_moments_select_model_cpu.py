"""A numpy model of moments_select_kernel's candidate scheme (csrc/fuse_select.hip): corner (t_p, t_i) from low sample quantiles, the
L-shaped region {d_p <= t_p or d_i <= t_i} as the candidate list, acceptance when the list did not overflow and its k-th best score is
STRICTLY below F(t_p, t_i).  What the kernel's correctness rests on is checked here for every row: whenever the model accepts, the k
best (score, index) pairs of the list are those of the whole row.  The score is the kernel's expression in numpy's fp64 (correctly
rounded division, as div_rn gives)."""
import math

import numpy as np

CAP = 4096            # FS_CAP
SEG = CAP // 4        # a wave's quarter of the list


def corner_plan(n):
    """(samp, rank) as launch_moments_select picks them."""
    T = CAP * 5.0 / 8.0
    samp = 16
    while samp > 1 and 128.0 * samp * T / n > 80.0:
        samp >>= 1
    D = 128.0 * samp * T / n
    rank = int(math.floor((64.0 * (1.0 - math.exp(-D / 256.0)) if samp > 1 else D / 4.0) + 0.5))
    return samp, min(max(rank, 1), 32)


def corner(dp, di, masked):
    """Per channel the mean over the four waves of the rank-th smallest of a wave's 64 thread minima over columns tid + 256 u, u < samp
    (NaN and masked entries left out)."""
    n = dp.shape[0]
    samp, rank = corner_plan(n)
    t = []
    for d in (dp, di):
        s = np.where(masked[:256 * samp] | np.isnan(d[:256 * samp]), np.float32(np.inf), d[:256 * samp]).reshape(samp, 256).min(axis=0)
        s = np.sort(s.reshape(4, 64), axis=1)[:, rank - 1]            # (ties between threads: equal values, the same threshold)
        t.append(np.float32(((s[0] + s[1]) + (s[2] + s[3])) * np.float32(0.25)))
    return t[0], t[1]


def score_fn(dp, di, p):
    """(F, usable): the row's score expression under its own statistics (N - 1 std over the non-NaN entries, per channel)."""
    st = []
    for d in (dp, di):
        v = d[~np.isnan(d)].astype(np.float64)
        st.append((v.mean(), v.std(ddof=1)) if v.size > 1 else (0.0, np.nan))
    (mp, sp), (mi, si) = st
    usable = all(1e-290 < s < 1e290 for s in (sp, si)) and p > 0
    with np.errstate(all="ignore"):
        return (lambda a, b: p * ((np.float64(a) - mp) / sp) + (np.float64(b) - mi) / si), usable


def topk(score, index, k):
    order = np.lexsort((index, score))[:k]
    return list(zip(score[order].tolist(), index[order].tolist()))


def model(dp, di, k, p=2.0, mask_width=0, ig=0, db_row0=0, t=None):
    """-> (accepted, list's top-k, whole row's top-k).  t: a corner given by hand instead of the sampled one."""
    n = dp.shape[0]
    j = np.arange(n)
    masked = np.abs(ig - (db_row0 + j)) < mask_width
    tp, ti = corner(dp, di, masked) if t is None else t
    F, usable = score_fn(dp, di, p)
    with np.errstate(all="ignore"):
        f = F(dp, di)
    alive = ~np.isnan(f) & ~masked
    full = topk(f[alive], j[alive], k)
    if not usable:
        return False, None, full
    region = (dp <= tp) | (di <= ti)
    wave = ((j // 4) % 256) // 64                                       # (rows that start on a 16-byte boundary)
    if np.bincount(wave[region], minlength=4).max() > SEG:
        return False, None, full
    lst = region & alive
    got = topk(f[lst], j[lst], k)
    with np.errstate(all="ignore"):
        corner_score = F(tp, ti)
    ok = len(got) == k and got[-1][0] < corner_score                   # strictly: a tie does not count
    return bool(ok), got, full


def check(dp, di, k, **kw):
    ok, got, full = model(dp.astype(np.float32), di.astype(np.float32), k, **kw)
    if ok:
        assert got == full[:k], (got, full)
    return ok


def test_accepted_lists_hold_the_rows_top_k():
    rng = np.random.default_rng(7)
    accepted = 0
    for n in (4097, 5000, 20_011, 40_000):
        for k in (1, 9, 16):
            for trial in range(6):
                kind = trial % 6
                dp = rng.random(n); di = rng.random(n)
                if kind == 1:                                          # bell-shaped, independent
                    dp = np.clip(0.5 + 0.1 * rng.standard_normal(n), 0, 1); di = np.clip(0.5 + 0.1 * rng.standard_normal(n), 0, 1)
                elif kind == 2:                                        # negative correlation
                    di = np.clip(1.0 - dp + 0.05 * rng.standard_normal(n), 0, 1)
                elif kind == 3:                                        # duplicated elements: few distinct pairs, masses of equal scores
                    dp = np.round(dp * 50) / 50; di = np.round(di * 50) / 50
                elif kind == 4:                                        # 40 copies of one pair around the k-th place, NaN columns
                    c = rng.choice(n, 45, replace=False)
                    dp[c[:5]] = di[c[:5]] = 1e-3; dp[c[5:]] = di[c[5:]] = 2e-3
                    dp[rng.choice(n, 30)] = np.nan; di[0] = np.nan
                elif kind == 5:                                        # positive correlation
                    di = np.clip(dp + 0.05 * rng.standard_normal(n), 0, 1)
                mw = 100 if trial % 2 else 0
                accepted += check(dp, di, k, mask_width=mw, ig=37 + trial * 500, db_row0=11)
    assert accepted >= 48          # (of 72, twelve of them negatively correlated: the check above is not vacuous)


def test_ties_across_the_corner_are_not_accepted():
    """Scores that tie EXACTLY across the corner: with one huge outlier per channel every other element's z-score is the same double, so
    an element outside the region (both distances a float above the corner) ties with the list's best - and, with a lower index,
    precedes it.  The k-th score then equals F(t_p, t_i): only the strict comparison keeps the row from being accepted."""
    n, k = 6000, 3
    lo, hi = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    dp = np.full(n, hi, np.float32); di = np.full(n, hi, np.float32)
    dp[-1] = di[-1] = np.float32(3e37)                                 # the outliers: sigma ~ 4e35, differences of 1e-7 vanish
    dp[100:110] = lo; di[200:210] = lo                                 # the region: these twenty
    ok, got, full = model(dp, di, k, t=(lo, lo))
    F, _ = score_fn(dp, di, 2.0)
    assert F(lo, lo) == F(hi, hi) == F(lo, hi)                         # the ties are exact
    assert [j for _, j in full] == [0, 1, 2]                           # the row's best lie outside the region ...
    assert not ok                                                      # ... and the model does not accept
    # the same row with the corner above every ordinary element: the list holds them all and is accepted only if it did not overflow
    assert not model(dp, di, k, t=(hi, hi))[0]
    # an element exactly AT the corner that is the k-th best: equal to F, not below it
    rng = np.random.default_rng(3)
    a = (0.3 + 0.7 * rng.random(n)).astype(np.float32); b = (0.3 + 0.7 * rng.random(n)).astype(np.float32)
    a[17] = b[17] = np.float32(0.1)
    ok, got, full = model(a, b, 1, t=(np.float32(0.1), np.float32(0.1)))
    assert got == full[:1] and got[0][1] == 17 and not ok


def test_fall_through_is_rare_on_independent_channels_at_100k():
    """The cap that keeps the check above from hiding a scheme that never accepts: at n = 100 000, k = 9 (the k + 8 of a top-1 call), at
    most 1 % of random independent-channel rows may take the second sweep."""
    rng = np.random.default_rng(11)
    n, rows, fell = 100_000, 300, 0
    for r in range(rows):
        if r % 2:
            dp = rng.random(n, dtype=np.float32); di = rng.random(n, dtype=np.float32)
        else:
            dp = np.clip(0.5 + 0.1 * rng.standard_normal(n), 0, 1); di = np.clip(0.5 + 0.12 * rng.standard_normal(n), 0, 1)
        fell += not check(dp, di, 9)
    print(f"fall-through: {fell} of {rows} rows")
    assert fell <= rows // 100
