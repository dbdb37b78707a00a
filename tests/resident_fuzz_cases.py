"""Seeded adversarial cases for the device-resident BoW, GIST and DELIGHT matchers (bow_match.hip, gist_match.hip, delight_match.hip),
and the oracle's answer to them.  Pure numpy; imported by tests/test_resident_fuzz_cases.py (CPU: the generator delivers what its labels
claim), tests/test_gpu_fuzz_resident.py (GPU: every form of the call against the oracle, bit for bit) and tools/fuzz_all.py (open seeds).

draw(kind, seed, i) is deterministic.  It mixes, with the probabilities below: edge shapes (m, n, k, mask, row offsets, cols), near-copy
clusters of one place sized around the candidate list C = k + 8 and put inside a slab, across a slab border, at row 0, at row n - 1 or
half under the mask, magnitude edges of each coarse arithmetic, and exact ties.  What a case holds is listed in its label; the flags of
a cluster (`wins`, `shuffled`, `fp32flat`, `straddles`) are derived from the generator's own fp64 arithmetic and checked against the
oracle by the CPU test.  The slab geometry is restated from gist_match.cpp / delight_match.cpp (slab_count, slab_bounds); the CPU test
pins the restatement against the constants in the source text."""
import numpy as np

KINDS = ("bow", "gist", "delight")
DIV = {"bow": 2, "gist": 1, "delight": 16}            # matrix rows per signature

# ------------------------------------------------------------------------------------------------ the mix (fixed probabilities)
P_M = ((1, .06), (2, .06), (31, .04), (32, .05), (33, .04), (63, .04), (64, .04), (65, .04), (255, .04), (256, .05), (257, .06), ("random", .48))
P_N = (("one", .04), ("k-1", .07), ("k", .09), ("k+1", .09), ("random", .71))
P_K = ((1, .2), (2, .1), (5, .3), (40, .15), ("119..128", .25))
P_MASK = ((0, .35), (1, .15), (4, .2), (100, .2), (">n", .1))
P_OFFSETS = 0.4                                       # non-zero q_row0 / db_row0
P_COLS = ((1, .03), (2, .05), (7, .07), (8, .07), (15, .06), (16, .07), (17, .06), (96, .17), (512, .12), (960, .08), ("random", .22))
P_CLUSTERS = ((0, .15), (1, .4), (2, .27), (3, .18))  # clusters per case (n >= 12)
P_SIZE = (("C-2", .12), ("C-1", .12), ("C", .16), ("C+1", .14), ("C+2", .14), (40, .17), (130, .15))
P_PLACE = (("inside", .25), ("border", .25), ("row0", .15), ("last", .15), ("masked", .2))
P_COMPETE = 0.5                                       # a further cluster shares the query (and the place) of the first
P_EXACT_COPIES = 0.15                                 # a cluster of exact copies (every member ties)
P_COMMON = 0.55                                       # the query differs from the place by one common difference (members nearly tie)
P_CROWD = 0.12                                        # every query looks at the first cluster's place (m >= 257: more than one exact-row pass)
P_TIES = 0.35                                         # duplicated rows / permutation images at a low and a high index
P_EDGE = 0.18                                         # each magnitude edge of the kind, independently
N_MAX, M_MAX = 6000, 400
WORK = {"bow": 3e8, "gist": 4e8, "delight": 2.5e5}    # m n cols (bow, gist), m n (delight: 4 x 4096 terms per pair) the oracle is asked for
CELLS = 6e6                                           # n cols of one case

# the committed seed set: (seed, i) per kind, chosen on the CPU so that every label of flat_features() is held by at least three cases
# and holds in the oracle's distances (tests/test_resident_fuzz_cases.py).  DELIGHT's slabs are mostly narrower than a cluster, so three
# draws of other seeds that plant one inside a slab are added by name.
SEED_SET = {"bow": tuple((4, i) for i in range(48)),
            "gist": tuple((4, i) for i in range(48)),
            "delight": tuple((3, i) for i in range(48)) + ((6, 6), (6, 12), (1, 15))}

# ------------------------------------------------------------------------------------------------ the matchers' geometry, restated
MAX_CAND, MAX_SLABS, QCAP, XCAP = 2048, 256, 4096, 256  # resident_match.hpp: S C <= MAX_CAND, exact rows per pass
GIST_SLAB_WORK, GIST_MIN_SLABS, GIST_TILE = 1536, 4, 32
DELIGHT_SLAB_WORK, DELIGHT_QUERIES_PER_WG, DELIGHT_MIN_ENTRIES = 2048, 4, 8
BOW_TAIL_ROWS = 1024                                  # bow_match.cpp: rows of the tail segment a growing DB folds into its main lists


def slab_count(kind, m, n, k):
    """S of one match chunk (launch_coarse of gist_match.cpp / delight_match.cpp); m <= QCAP queries are one chunk"""
    C, mc = k + 8, min(m, QCAP)
    if kind == "gist":
        qtiles, DT = (mc + GIST_TILE - 1) // GIST_TILE, (n + GIST_TILE - 1) // GIST_TILE
        S = max(GIST_MIN_SLABS, (GIST_SLAB_WORK + qtiles - 1) // qtiles)
        S = min(S, min(MAX_CAND // C, MAX_SLABS))
        return max(1, min(S, DT))
    if kind == "delight":
        qb = (mc + DELIGHT_QUERIES_PER_WG - 1) // DELIGHT_QUERIES_PER_WG
        S = (DELIGHT_SLAB_WORK + qb - 1) // qb
        S = min(S, min(MAX_CAND // C, MAX_SLABS))
        return max(1, min(S, (n + DELIGHT_MIN_ENTRIES - 1) // DELIGHT_MIN_ENTRIES))
    raise ValueError(kind)


def slab_bounds(kind, m, n, k, tail_rows=BOW_TAIL_ROWS):
    """first rows of the slabs and n: slab s holds rows [b[s], b[s + 1]).  GIST cuts tiles of 32 rows (DT s / S), DELIGHT entries (n s / S).
    BoW has no slabs: its borders are those of the tail segment of a growing DB (rows tail_rows t)."""
    if kind == "bow":
        return np.unique(np.r_[np.arange(0, n, tail_rows), n])
    S = slab_count(kind, m, n, k)
    s = np.arange(S + 1, dtype=np.int64)
    if kind == "gist":
        DT = (n + GIST_TILE - 1) // GIST_TILE
        return np.minimum(DT * s // S * GIST_TILE, n)
    return n * s // S


# ------------------------------------------------------------------------------------------------ the oracle's answer
def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def mask_distances(d, mask_width, q_row0=0, db_row0=0):
    m, n = d.shape
    gi = q_row0 + np.arange(m)[:, None]
    gj = db_row0 + np.arange(n)[None, :]
    return np.where(np.abs(gi - gj) < mask_width, np.inf, d)


def oracle_select(d, mask_width, k, q_row0=0, db_row0=0):
    """run_test.m:47-57 on the global distance matrix d of rows [db_row0, db_row0 + n): mask, then the k smallest by (score, index)"""
    import oracle_lib
    rc, idx, sc = oracle_lib.select_topk(mask_distances(d, mask_width, q_row0, db_row0), 0, k)
    assert rc == 0
    return np.where(idx >= 0, idx + db_row0, -1).astype(np.int32), sc


def oracle_distance(kind, h1, h2):
    import oracle_lib
    return getattr(oracle_lib, kind + "_distance")(h1, h2)


def oracle_topk(kind, h1, h2, mask_width, k, q_row0=0, db_row0=0):
    return oracle_select(oracle_distance(kind, h1, h2), mask_width, k, q_row0, db_row0)


# ------------------------------------------------------------------------------------------------ drawing
class Case:
    """kind, q, db (matrices of DIV[kind] rows per signature), cols, vocab (bow), m, n, k, mask_width, q_row0, db_row0,
    chunks (growth schedule: the reserved start, possibly 0, then the appends; sum n), cuts (shard borders 0 .. n), tail_rows (bow: the
    tail segment of the grown form), label (tuple of str), clusters / ties (lists of dict, see _plant)."""

    def rows(self, a, lo, hi):
        d = DIV[self.kind]
        return a[d * lo:d * hi]

    def __repr__(self):
        return f"{self.kind} m={self.m} n={self.n} k={self.k} mask={self.mask_width} q0={self.q_row0} d0={self.db_row0} [{' '.join(self.label)}]"


def _pick(rng, table):
    p = np.array([t[1] for t in table], np.float64)
    return table[int(rng.choice(len(table), p=p / p.sum()))][0]


def _estimate(kind, q1, db, cols):
    """the generator's own fp64 distances of one query against every DB signature (plain numpy; not the normative summation order)"""
    with np.errstate(all="ignore"):
        if kind == "gist":
            return ((db - q1[None, :]) ** 2).sum(1)
        if kind == "delight":
            B = db.reshape(-1, 16, 256)
            A = q1.reshape(16, 256)
            out = np.empty(len(B))
            r = np.arange(16)
            for j0 in range(0, len(B), 256):
                Bc = B[j0:j0 + 256]
                best = np.full(len(Bc), np.inf)
                for x in (0, 5, 6, 3):
                    b = Bc[:, r ^ x, :]
                    s = A[None] + b
                    t = np.where(s > 0, 2.0 * (A[None] - b) ** 2 / s, 0.0)
                    v = t.sum((1, 2)) / (s > 0).sum((1, 2))
                    best = np.where(best > v, v, best)
                out[j0:j0 + 256] = best
            return out
        n = len(db) // 2
        ids, w = q1[0], q1[1]
        L = _bow_len(ids, cols)
        qw = dict(zip(ids[:L].tolist(), w[:L].tolist()))
        out = np.ones(n)
        for j in range(n):
            Lj = _bow_len(db[2 * j], cols)
            s = 0.0
            for x, v in zip(db[2 * j, :Lj].tolist(), db[2 * j + 1, :Lj].tolist()):
                u = qw.get(x)
                if u is not None:
                    s += abs(u - v) - abs(u) - abs(v)
            out[j] = 1.0 + s / 2.0
        return out


def _bow_len(ids, cols):
    p = 0
    while p < cols - 1 and ids[p] > -1.0:
        p += 1
    return p


def _shapes(kind, rng, big):
    k = _pick(rng, P_K)
    k = int(rng.integers(119, 129)) if k == "119..128" else int(k)
    m = _pick(rng, P_M)
    m = int(rng.integers(1, M_MAX + 1)) if m == "random" else int(m)
    crowd = rng.random() < P_CROWD
    if crowd:
        m = int(rng.choice([257, 300, M_MAX]))
    cols = 256
    if kind != "delight":
        cols = _pick(rng, P_COLS)
        cols = int(rng.integers(1, 4001)) if cols == "random" else int(cols)
    nk = _pick(rng, P_N)
    n = {"one": 1, "k-1": k - 1, "k": k, "k+1": k + 1}.get(nk)
    if n is None:
        n = int(10.0 ** rng.uniform(1.2, np.log10(N_MAX)))
    if big:
        m, n = int(rng.integers(1, 5)), int(10.0 ** rng.uniform(4.2, 5.0))
    n = max(1, n)
    per = 1 if kind == "delight" else (min(cols, 120) if kind == "bow" else cols)
    if not big:
        n = int(min(n, max(k + 1, CELLS // cols)))
        if m * n * per > WORK[kind]:                  # too much for the oracle: shrink the random one of the two, else n
            if nk == "random" or crowd:
                n = int(max(1, WORK[kind] // (m * per)))
            else:
                m = int(max(1, WORK[kind] // (n * per)))
    mw = _pick(rng, P_MASK)
    mw = n + 5 if mw == ">n" else int(mw)
    q0 = d0 = 0
    if rng.random() < P_OFFSETS:
        d0 = int(rng.integers(1, 5000))
        q0 = max(0, d0 + int(rng.integers(-m, n + 1)))
    return m, n, k, cols, mw, q0, d0, crowd


def _schedule(rng, n):
    """(chunks, cuts): a growth schedule of at most 12 steps and 1 - 4 shards"""
    chunks = [int(rng.choice([0, 0, 1, n // 3, n // 2]))]
    at = chunks[0]
    while at < n:
        c = int(min(n - at, rng.choice([1, 1, 2, 7, 16, 33, 200, 1000, 1500])))
        if len(chunks) >= 11:
            c = n - at
        chunks.append(c)
        at += c
    G = int(min(n, rng.integers(1, 5)))
    inner = np.sort(rng.choice(np.arange(1, n), size=G - 1, replace=False)) if G > 1 else []
    return tuple(chunks), tuple(int(x) for x in np.r_[0, inner, n])


# --------------------------------------------------------------------------------------------------------------- content per kind
def _gist_rows(rng, n, cols):
    return np.abs(rng.normal(0.1, 0.05, size=(n, cols)))


def _delight_rows(rng, n):
    out = np.empty((n, 16, 256))
    for s0 in range(0, n, 2048):
        r = min(n, s0 + 2048) - s0
        u = rng.random((r, 16, 256))
        out[s0:s0 + r] = np.floor(u * (4.0 + 28.0 * rng.random((r, 16, 1))) * (u < 0.5))
    return out.reshape(16 * n, 256)


def _bow_doc(rng, cols, vocab, zipf, lo=1, hi=None):
    """(ids, weights) of one document: distinct ascending ids, L1-normalised positive weights"""
    hi = min(cols, 120, vocab) if hi is None else hi
    L = int(rng.integers(min(lo, hi), hi + 1))
    if zipf:
        ids = np.unique(np.minimum((rng.pareto(1.0, 2 * L + 2)).astype(np.int64), vocab - 1))[:L]
    else:
        ids = np.sort(rng.choice(vocab, size=L, replace=False))
    w = rng.random(len(ids)) + 0.05
    return ids.astype(np.float64), w / max(w.sum(), 1e-300)


def _bow_put(out, r, ids, w, rng=None):
    cols = out.shape[1]
    L = min(len(ids), cols)
    out[2 * r] = -1.0
    out[2 * r + 1] = -1.0
    out[2 * r, :L] = ids[:L]
    out[2 * r + 1, :L] = w[:L]
    if rng is not None and L < cols and rng.random() < 0.3:     # another terminator, and what follows it is never read
        out[2 * r, L] = rng.choice([-7.5, np.nan, -1.0])
        out[2 * r, L + 1:] = rng.integers(-3, 50, cols - L - 1)


def _bow_rows(rng, n, cols, vocab, zipf):
    out = -np.ones((2 * n, cols))
    for r in range(n):
        _bow_put(out, r, *_bow_doc(rng, cols, vocab, zipf), rng=rng)
    return out


def _sig(c, a, j):
    d = DIV[c.kind]
    return a[d * j:d * (j + 1)]


def _set(c, a, j, v):
    d = DIV[c.kind]
    a[d * j:d * (j + 1)] = v


def _member(c, rng, place, t, cs, eps, aux):
    """near-copy t of `place` (a signature): the member-to-place difference is eps (relative) for GIST and BoW; for DELIGHT one count
    (+1 or -1) in the member's private bin, whose level aux['levels'][t] sets how much that count weighs"""
    if c.kind == "gist":
        return place + eps * aux["unit"] * rng.normal(size=place.shape)
    if c.kind == "bow":
        v = -np.ones_like(place)
        L = aux["Lm"]
        v[0, :L] = place[0, :L]
        v[1, :L] = place[1, :L] * (1.0 + eps * rng.normal(size=L))
        return v
    v = place.copy().reshape(4096)
    if eps > 0:
        v[aux["bins"][t]] += aux["signs"][t]
    return v.reshape(16, 256)


def _plant(c, rng, crowd):
    """clusters: dict(query, rows [cs] ascending, place, size, exact, wins, shuffled, fp32flat, straddles); the flags are the generator's
    own findings (None where it claims nothing).  Clusters that compete share query and place."""
    kind, m, n, k = c.kind, c.m, c.n, c.k
    C = k + 8
    nc = int(_pick(rng, P_CLUSTERS)) if n >= 12 else 0
    if crowd and n >= 12:
        nc = max(nc, 1)
    nc = min(nc, m)
    bounds = slab_bounds(kind, m, n, k, c.tail_rows)
    taken = np.zeros(n, bool)
    c.clusters, c.ties = [], []
    first = None
    for ci in range(nc):
        size = _pick(rng, P_SIZE)
        cs = {"C-2": C - 2, "C-1": C - 1, "C": C, "C+1": C + 1, "C+2": C + 2}.get(size, size)
        if cs > n - 2:
            cs, size = n - 2, "clipped"
        place = _pick(rng, P_PLACE)
        compete = first is not None and rng.random() < P_COMPETE
        qi = first["query"] if compete else int(rng.choice(np.setdiff1d(np.arange(m), [x["query"] for x in c.clusters])))
        r0 = None
        if place == "masked":                                               # the upper end of the query's mask window cuts the cluster
            if not c.clusters and not 1 <= c.mask_width <= n:
                c.mask_width = int(rng.choice([4, 100]))
            r0 = c.q_row0 - c.db_row0 + qi + c.mask_width - cs // 2         # rows below q_row0 - db_row0 + qi + mask_width are masked
            if not 1 <= c.mask_width <= n or r0 < 0 or r0 + cs > n:
                r0, place = None, "inside"                                  # the window does not reach into the DB
        if place == "border":
            ok = [b for b in bounds[1:-1] if b - cs // 2 >= 0 and b - cs // 2 + cs <= n]
            if ok:
                r0 = int(rng.choice(ok)) - cs // 2
            else:
                place = "inside"
        if place == "row0":
            r0 = 0
        if place == "last":
            r0 = n - cs
        if place == "inside":
            w = np.diff(bounds)
            ok = np.nonzero(w >= cs)[0]
            if len(ok):
                s = int(rng.choice(ok))
                r0 = int(bounds[s]) + int(rng.integers(0, w[s] - cs + 1))
            else:
                r0, place = int(rng.integers(0, n - cs + 1)), "anywhere"
        if taken[r0:r0 + cs].any():
            continue
        taken[r0:r0 + cs] = True
        rows = np.arange(r0, r0 + cs)
        exact = rng.random() < P_EXACT_COPIES
        if compete:
            base, aux, eps, common = first["_base"], first["_aux"], first["_eps"], first["_common"]
            exact = first["exact"]
        else:
            base = _sig(c, c.db, int(rng.integers(0, n))).copy()
            aux = {}
            common = rng.random() < P_COMMON
            if kind == "gist":
                aux["unit"] = 0.05 * c.scale
                eps = 0.0 if exact else 10.0 ** rng.uniform(-12, -2)
            elif kind == "bow":
                ids, w = _bow_doc(rng, c.cols, c.vocab, False, lo=min(6, c.cols), hi=max(min(c.cols, 60, c.vocab), 1))
                base = -np.ones((2, c.cols))
                base[0, :len(ids)] = ids
                base[1, :len(ids)] = w
                aux["L"] = _bow_len(base[0], c.cols)
                aux["Lm"] = max(1, aux["L"] // 2) if common else aux["L"]   # the members lack half of the query's words: one common part
                eps = 0.0 if exact else 10.0 ** rng.uniform(-13, -2)
            else:
                level = int(rng.integers(2000, 9000)) if rng.random() < 0.4 else int(10.0 ** rng.uniform(0.5, 4))
                aux["bins"] = rng.choice(4096, size=3 * 140 + 1, replace=False)     # private bins of up to three clusters, and the common one
                aux["levels"] = level + 3 * rng.permutation(3 * 140)
                aux["signs"] = rng.choice([-1.0, 1.0], size=3 * 140)
                flat = base.reshape(4096)
                flat[aux["bins"][:-1]] = aux["levels"]
                base = flat.reshape(16, 256)
                aux["next"] = 0
                eps = 0.0 if exact else 1.0
        t0 = 0
        if kind == "delight":
            t0 = aux["next"]
            aux["next"] += cs
        for t, j in enumerate(rows):
            _set(c, c.db, j, _member(c, rng, base, t0 + t, cs, eps, aux))
        if not compete:
            # the query: the place itself with a member-sized difference, or with one common difference far above the members' spread
            if kind == "gist":
                qv = base + eps * aux["unit"] * rng.normal(size=base.shape)
                if common:
                    qv = base + 10.0 ** rng.uniform(-3, -0.5) * aux["unit"] * rng.normal(size=base.shape)
            elif kind == "bow":
                qv = base.copy()
            else:
                qv = base.copy().reshape(4096)
                if common:
                    qv[aux["bins"][-1]] += float(rng.integers(2000, 6000)) if rng.random() < 0.4 else float(int(10.0 ** rng.uniform(0, 3.7)))
                qv = qv.reshape(16, 256)
            _set(c, c.q, qi, qv)
            if crowd and not c.clusters:                                    # every query looks at this place
                for i in range(m):
                    if i != qi:
                        if kind == "gist":
                            _set(c, c.q, i, qv + max(eps, 1e-9) * aux["unit"] * rng.normal(size=base.shape))
                        elif kind == "bow":
                            v = qv.copy()
                            Lq = _bow_len(v[0], c.cols)
                            v[1, :Lq] *= 1.0 + 1e-9 * rng.normal(size=Lq)
                            _set(c, c.q, i, v)
                        else:
                            v = qv.copy().reshape(4096)
                            v[aux["bins"][-1]] += float(i % 5)
                            _set(c, c.q, i, v.reshape(16, 256))
        cl = dict(query=qi, rows=rows, place=place, size=str(size), exact=bool(exact), compete=bool(compete), _base=base, _aux=aux, _eps=eps,
                  _common=common)
        c.clusters.append(cl)
        if first is None:
            first = cl
    # exact ties outside the clusters: a source row copied (DELIGHT: as a permutation image too) to a low and a high index
    if rng.random() < P_TIES and n >= 8:
        free = np.nonzero(~taken)[0]
        if len(free) >= 4:
            lo, hi = free[:max(2, len(free) // 8)], free[-max(2, len(free) // 8):]
            spots = np.unique(np.r_[rng.choice(lo, 2, replace=False), rng.choice(hi, 2, replace=False)])
            src = _sig(c, c.db, int(spots[0])).copy()
            for t, j in enumerate(spots):
                v = src
                if kind == "delight" and t % 2:
                    v = src[np.arange(16) ^ (5, 6, 3)[t % 3]]               # a permutation image: the same distance to every query
                _set(c, c.db, int(j), v)
            others = np.setdiff1d(np.arange(m), [x["query"] for x in c.clusters])
            if len(others):
                qi = int(rng.choice(others))
                _set(c, c.q, qi, src)
                c.ties.append(dict(query=qi, rows=spots))


def _edges(c, rng):
    """magnitude edges of the kind's coarse arithmetic, on rows outside the clusters; -> labels"""
    kind, m, n = c.kind, c.m, c.n
    out = []
    taken = np.zeros(n, bool)
    for cl in c.clusters:
        taken[cl["rows"]] = True
    for t in c.ties:
        taken[t["rows"]] = True
    free = np.nonzero(~taken)[0]
    qfree = np.setdiff1d(np.arange(m), [x["query"] for x in c.clusters] + [t["query"] for t in c.ties])

    def some(pool, most=3):
        return rng.choice(pool, size=min(len(pool), int(rng.integers(1, most + 1))), replace=False) if len(pool) else []

    def hit(name):
        return rng.random() < P_EDGE and (out.append(name) or True)

    if kind == "gist":
        if hit("f16edge"):                           # near the f16 overflow after centring
            for j in some(free):
                c.db[j, int(rng.integers(0, c.cols))] = rng.uniform(6e4, 7e4) * rng.choice([-1.0, 1.0])
            for i in some(qfree, 2):
                c.q[i, int(rng.integers(0, c.cols))] = rng.uniform(6e4, 7e4)
        if hit("subnormal"):                         # rows whose entries lie in the f16 subnormal range
            for j in some(free):
                c.db[j] *= 10.0 ** rng.uniform(-5, -3.5)
            for i in some(qfree, 2):
                c.q[i] *= 10.0 ** rng.uniform(-5, -3.5)
        if hit("infnan"):
            v = rng.choice([np.inf, -np.inf, np.nan])
            if rng.random() < 0.5 and len(free):
                c.db[int(rng.choice(free)), int(rng.integers(0, c.cols))] = v
            elif len(qfree):
                c.q[int(rng.choice(qfree)), int(rng.integers(0, c.cols))] = v
            else:
                out.pop()
    elif kind == "delight":
        D, Q = c.db.reshape(n, 4096), c.q.reshape(m, 4096)
        if hit("near2^24"):
            for j in some(free):
                D[j] = np.where(rng.random(4096) < 0.5, 0.0, 2.0 ** 24 - rng.integers(0, 1000, 4096))
            for i in some(qfree, 2):
                Q[i] = np.where(rng.random(4096) < 0.5, 0.0, 2.0 ** 24 - rng.integers(0, 1000, 4096))
        if hit("eq2^24"):
            for j in some(free, 2):
                D[j, rng.choice(4096, 40, replace=False)] = 2.0 ** 24
            for i in some(qfree, 1):
                Q[i, rng.choice(4096, 40, replace=False)] = 2.0 ** 24
        side = "db" if rng.random() < 0.4 else "q"  # a row the fp32 image cannot hold: on the DB side every query takes its exact row
        pool, A = (free, D) if side == "db" else (qfree, Q)
        if len(pool):
            if hit("above2^24") and (out.append("image-miss:" + side) or True):
                A[int(rng.choice(pool)), int(rng.integers(0, 4096))] = 2.0 ** 24 + 2.0 * int(rng.integers(1, 1000))
            if hit("fractional") and (out.append("image-miss:" + side) or True):
                A[int(rng.choice(pool)), rng.choice(4096, 5, replace=False)] += 0.5
            if hit("negative") and (out.append("image-miss:" + side) or True):
                A[int(rng.choice(pool)), rng.choice(4096, 5, replace=False)] = -3.0
            if hit("nan") and (out.append("image-miss:" + side) or True):
                A[int(rng.choice(pool)), int(rng.integers(0, 4096))] = np.nan
        if hit("zero_db"):
            for j in some(free):
                D[j] = 0.0
        if hit("zero_q"):
            for i in some(qfree, 2):
                Q[i] = 0.0
    else:
        src = int(rng.integers(0, m))
        L = _bow_len(c.q[2 * src], c.cols)
        if hit("oneword"):
            for j in some(free):
                _bow_put(c.db, j, np.array([float(rng.integers(0, c.vocab))]), np.array([1.0]))
            for i in some(qfree, 1):
                _bow_put(c.q, i, np.array([float(rng.integers(0, c.vocab))]), np.array([1.0]))
        if hit("identical"):                         # the same document at several rows: ties
            for j in some(free, 4):
                c.db[2 * j:2 * j + 2] = c.q[2 * src:2 * src + 2]
        if hit("disjoint"):                          # a query that shares no word with any document: every distance is exactly 1
            if len(qfree) and c.vocab >= 2:
                i = int(rng.choice(qfree))
                w = float(c.vocab - 1)
                for j in range(n):
                    Lj = _bow_len(c.db[2 * j], c.cols)
                    if Lj and c.db[2 * j, Lj - 1] == w:
                        _bow_put(c.db, j, c.db[2 * j, :Lj - 1], c.db[2 * j + 1, :Lj - 1])
                _bow_put(c.q, i, np.array([w]), np.array([1.0]))
            else:
                out.pop()
        if hit("empty"):
            for j in some(free):
                _bow_put(c.db, j, np.array([]), np.array([]))
            for i in some(qfree, 1):
                _bow_put(c.q, i, np.array([]), np.array([]))
        if hit("subfp32") and L >= 1:                # weights that differ below fp32 resolution, in descending order of the index
            js = some(free, 6)
            for t, j in enumerate(np.sort(js)):
                c.db[2 * j:2 * j + 2] = c.q[2 * src:2 * src + 2]
                c.db[2 * j + 1, 0] = c.q[2 * src + 1, 0] * (1.0 - (len(js) - t) * 1e-12)
    return out


def _flags(c):
    """what the generator finds in its own arithmetic, after everything is planted"""
    kind, n = c.kind, c.n
    bounds = slab_bounds(kind, c.m, n, c.k, c.tail_rows)
    for cl in c.clusters:
        qi = cl["query"]
        mine = np.concatenate([x["rows"] for x in c.clusters if x["query"] == qi])
        est = _estimate(kind, _sig(c, c.q, qi) if kind != "gist" else c.q[qi], c.db, c.cols)
        gj = c.db_row0 + np.arange(n)
        est = np.where(np.abs(c.q_row0 + qi - gj) < c.mask_width, np.inf, est)
        dm = est[cl["rows"]]
        vis = np.isfinite(dm)
        rest = np.delete(est, mine)
        rest = rest[~np.isnan(rest)]
        cl["masked"] = int((~vis).sum())
        top = np.max(est[mine][np.isfinite(est[mine])]) if np.isfinite(est[mine]).any() else np.inf
        cl["wins"] = bool(np.isfinite(top) and (len(rest) == 0 or rest.min() > top + 0.01 * abs(top) + 1e-300))
        v = dm[vis]
        cl["shuffled"] = bool(len(v) >= 3 and len(np.unique(v)) == len(v) and not np.array_equal(np.argsort(v, kind="stable"), np.arange(len(v))))
        cl["fp32flat"] = bool(len(v) >= 3 and len(np.unique(v)) == len(v) and v.min() > 1e-30 and (v.max() - v.min()) / v.min() < 2.0 ** -25)
        cl["straddles"] = bool(np.any((bounds[1:-1] > cl["rows"][0]) & (bounds[1:-1] <= cl["rows"][-1])))


def draw(kind, seed, i, big=False):
    """Case i of `seed` for `kind`; big: 1 - 4 queries against 16 000 - 100 000 rows (runs outside the suite)."""
    rng = np.random.default_rng([KINDS.index(kind), int(seed), int(i), int(big)])
    c = Case()
    c.kind, c.seed, c.i = kind, seed, i
    c.m, c.n, c.k, c.cols, c.mask_width, c.q_row0, c.db_row0, crowd = _shapes(kind, rng, big)
    m, n = c.m, c.n
    c.vocab, c.scale, c.tail_rows = 0, 1.0, BOW_TAIL_ROWS
    label = []
    if kind == "gist":
        c.db, c.q = _gist_rows(rng, n, c.cols), _gist_rows(rng, m, c.cols)
        if rng.random() < P_EDGE:                    # a constant offset on every row: the pack has to centre
            c.db += 1e3
            c.q += 1e3
            label.append("offset1e3")
    elif kind == "delight":
        c.db, c.q = _delight_rows(rng, n), _delight_rows(rng, m)
    else:
        c.vocab = int(rng.choice([50, 400, 5000, 100000]))
        zipf = rng.random() < 0.5
        c.tail_rows = int(rng.choice([5, 64, BOW_TAIL_ROWS]))
        c.db, c.q = _bow_rows(rng, n, c.cols, c.vocab, zipf), _bow_rows(rng, m, c.cols, c.vocab, zipf)
        if zipf:
            label.append("zipf")
    _plant(c, rng, crowd)
    label += _edges(c, rng)
    _flags(c)
    c.chunks, c.cuts = _schedule(rng, n)
    # the label: shapes, then what was planted
    C = c.k + 8
    label += [t for t, on in (("m-edge", m in (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)), ("n<k", n < c.k), ("n=k", n == c.k),
                              ("n=k+1", n == c.k + 1), ("k>=119", c.k >= 119),
                              ("mask>n", c.mask_width > n), ("offsets", c.q_row0 > 0 or c.db_row0 > 0), ("crowd", crowd and bool(c.clusters)),
                              ("ties", bool(c.ties))) if on]
    if kind != "delight":
        label.append("cols%8" if c.cols % 8 else "cols=8x")
    for cl in c.clusters:
        label.append("cluster:" + cl["place"])
        label.append("size:" + cl["size"])
        label += [t for t in ("exact", "compete", "wins", "shuffled", "fp32flat", "straddles") if cl[t]]
        if cl["masked"] and cl["masked"] < len(cl["rows"]):
            label.append("part-masked")
    c.label = tuple(label)
    c.C = C
    return c


def flat_features(kind):
    """the labels every kind's seed set must hold at least three times (tests/test_resident_fuzz_cases.py)"""
    common = ["m-edge", "n<k", "n=k", "n=k+1", "k>=119", "mask>n", "offsets", "crowd", "ties", "cluster:inside", "cluster:border", "cluster:row0", "cluster:last",
              "cluster:masked", "part-masked", "size:C-2", "size:C-1", "size:C", "size:C+1", "size:C+2", "size:40", "size:130", "exact", "compete",
              "wins", "shuffled", "fp32flat", "straddles"]
    own = {"gist": ["offset1e3", "f16edge", "subnormal", "infnan", "cols%8"],
           "delight": ["near2^24", "eq2^24", "above2^24", "fractional", "negative", "nan", "zero_db", "zero_q"],
           "bow": ["zipf", "oneword", "identical", "disjoint", "empty", "subfp32", "cols%8"]}
    return common + own[kind]
