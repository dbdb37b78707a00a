"""Shared test helpers: the config-1 synthetic points file: the reference's real pose files come
without their points (missing blobs), so points are synthesised around every pose and written in PosesPts format."""
import numpy as np

from so_dso_place_recognition_amd import api, synth


def read_poses(path):
    ids, W = [], []
    for line in open(path):
        t = line.split()
        if len(t) >= 13:
            ids.append(int(t[0]))
            W.append(np.array(t[1:13], np.float64).reshape(3, 4))
    return np.array(ids, np.int32), np.stack(W)


def write_synthetic_points(poses_path, pts_path, per_pose=120, seed=41, max_poses=None):
    ids, W = read_poses(poses_path)
    if max_poses:
        ids, W = ids[:max_poses], W[:max_poses]
    pid, pts, its = [], [], []
    for i, w in zip(ids, W):
        p, it = synth.scene_cloud(seed, int(i), per_pose)           # camera frame, ||p|| < 45
        R, t = w[:, :3], w[:, 3]
        world = (p - t) @ np.linalg.inv(R).T                         # camToWorld
        pid.append(np.full(per_pose, i, np.int32)); pts.append(world); its.append(it)
    api.write_points(pts_path, np.concatenate(pid), np.concatenate(pts), np.concatenate(its))
    return ids


def score_tol(score, sigmas=None, p_weight=2.0, eps=3e-8):
    """How far a returned fused z-score may be from the oracle's.  The returned score is p (d_p - mu_p)/s_p + (d_i - mu_i)/s_i
    (run_test.m:40) with the pair's distances re-evaluated in fp64, but the row statistics mu, s still come from the fp32
    all-pairs pass, whose distances carry ~2.5e-8 of noise each (max error 1.3e-7; BASELINE.json allows 1e-5).  Measured
    (tools/probe_bias.py, n = 20 000): |mu error| <= 5e-9, relative s error <= 2.5e-7 (the maximum over 120 noisy variants
    compresses the bulk of a row by that much); and when a match is an extreme outlier of a SHORT row it makes up most of the
    row's variance itself, so its own fp32 error e enters s: ds/s ~ z e / ((n - 1) s).  Together
        |score - oracle| <= 1e-5 + 3e-7 |score| + eps (p/s_p + 1/s_i) (1 + score^2/(n - 1)),   eps = 3e-8
    = 1e-5 outright for |z| < 30 at the usual s ~ 5e-3 and n >= 10^4; synthetic planted matches sit at z ~ -160, toy inputs have
    s ~ 2e-3 and n ~ 10^2.  sigmas: (s_p, s_i, n) from row_sigmas (arrays broadcastable to score) or None to leave the last
    term out (large n, usual s).  eps: the fp32 pass's error in a row MEAN; 3e-8 covers SC and M2DP rows of unrelated entries,
    1e-7 rows whose M2DP entries are all near-copies (every dot ~ 2, scaled by 2^16: the MFMA's fp32 accumulation truncates, and the
    common ~6e-8 shift of such a row's distances is not shared by the re-evaluated pair)."""
    tol = 1e-5 + 3e-7 * np.abs(score)
    if sigmas is not None:
        sp, si, n = sigmas
        tol = tol + eps * (p_weight / np.asarray(sp) + 1.0 / np.asarray(si)) * (1.0 + np.square(score) / (n - 1.0))
    return tol


def row_sigmas(dp, di):
    """(N-1 standard deviations of the rows of two distance matrices, NaN left out, shaped [m, 1]; row length)."""
    return np.nanstd(dp, axis=1, ddof=1)[:, None], np.nanstd(di, axis=1, ddof=1)[:, None], dp.shape[1]


def near_copy_clusters(type_, n, m, rows, copies=40, seed=21, db_seed=45, q_seed=46, spots=None, dups=0, db=None):
    """A synthetic DB / query set in which, for every query t of `rows`, `copies` DB entries at random positions are NEAR-COPIES of the
    query's planted entry: the same signature with a handful of values scaled by 1 + c delta (c = 1 .. copies), delta drawn per query
    from 1e-8.5 .. 1e-5.5 - their distances to the query form an arithmetic progression with a step of ~1e-10 ... 1e-7, at or below
    what the fp32-grade all-pairs pass resolves (1e-7), so more than k + 8 entries tie in its eyes: the place a vehicle stood at,
    revisited (the text files carry 6 digits).  Returns (db, queries, planted, members): members[t] = the cluster's DB indices
    (planted entry first).
    spots [len(rows), copies]: the members' DB positions (default: random ones); member c of row r goes to spots[r, c].
    dups: members c < dups are EXACT copies of the planted entry (a tie that only the index breaks); member c >= dups is scaled by
    1 + (c + 1 - dups) delta.  db: the DB to plant into, modified in place (default: synth's sampler with db_seed).
    With spots, dups and db left at their defaults the result is what it always was."""
    rng = np.random.default_rng(seed)
    if type_ == "sc":
        db = synth.sc_database(db_seed, n) if db is None else db
        q, planted = synth.sc_queries(q_seed, db, m)
    else:
        db = synth.m2dp_database(db_seed, n) if db is None else db
        q, planted = synth.m2dp_queries(q_seed, db, m)
    if spots is None:
        pool = np.setdiff1d(np.arange(n), planted)
        spots = rng.choice(pool, size=len(rows) * copies, replace=False).reshape(len(rows), copies)
    else:
        spots = np.asarray(spots, np.int64).reshape(len(rows), copies)
        assert len(np.unique(spots)) == spots.size and spots.min() >= 0 and spots.max() < n and not np.isin(spots, planted).any()
    members = {}
    for r, t in enumerate(rows):
        delta = 10.0 ** rng.uniform(-8.5, -5.5)
        sign = rng.choice([-1.0, 1.0])
        if type_ == "sc":
            e = db[planted[t]]
            pick = rng.choice(np.nonzero(e[:1200] > 0)[0], size=30, replace=False)
            for c in range(copies):
                x = e.copy()
                x[pick] *= 1.0 + sign * (c + 1 - dups if c >= dups else 0) * delta
                db[spots[r, c]] = x
        else:
            e = db[4 * planted[t]: 4 * planted[t] + 4]
            pick = rng.choice(64, size=20, replace=False)
            for c in range(copies):
                x = e.copy()
                x[:, pick] *= 1.0 + sign * (c + 1 - dups if c >= dups else 0) * delta * 0.03     # (M2DP rows are unit vectors: a dot moves by ~delta itself)
                db[4 * spots[r, c]: 4 * spots[r, c] + 4] = x
        members[int(t)] = np.concatenate([[planted[t]], spots[r]])
    return db, q, planted, members


CLUSTER_CASE = (1400, 48, tuple(range(0, 48, 3)), 40)      # (n, m, queries with a cluster, copies): tests/dist_order_case.py builds the same


def slice_edges(n, slices=(8, 64), shards=3):
    """Every boundary at which the exact-row resolution may cut a row of an n-entry DB: the row slices [n s / P, n (s + 1) / P) of its
    selection for both slice counts it picks from (integer division, as the kernel computes j_lo / j_hi), the shard starts g n / G of a
    `shards`-way pr_group split and the slices inside every shard (the smaller slice count), and n itself (the DB's last entries).
    Sorted, without 0."""
    e = {n}
    for g in range(shards):
        lo, hi = n * g // shards, n * (g + 1) // shards
        e.add(lo)
        e.update(lo + (hi - lo) * s // slices[0] for s in range(1, slices[0]))
    for P in slices:
        e.update(n * s // P for s in range(1, P))
    e.discard(0)
    return sorted(e)


def straddle(b, n):
    """The DB positions b - 2 .. b + 1 around boundary b (inside the DB), the last entry below the boundary first: b - 1, b, b - 2, b + 1."""
    return [j for j in (b - 1, b, b - 2, b + 1) if 0 <= j < n]


def cluster_spots(n, rows, copies, dups, planted, edges, top_extra=None, dup_extra=None, seed=5):
    """Member positions [len(rows), copies] for near_copy_clusters(..., spots=, dups=) that put the entries a top-k returns ON the given
    boundaries.  The positions around edges[i] (straddle) go to row i mod R (edges in priority order): its first two boundaries to the
    near-copies with the largest multipliers (members copies - 1, copies - 2, ...: the cluster's best when the near-copies come closer to the
    query than the planted entry), the later ones to its exact duplicates (a tie the lowest index wins: the planted entry's competitors when
    the near-copies move away), what is left to the other near-copies.  top_extra[r] / dup_extra[r]: positions that go to row r's top
    near-copies / duplicates before the boundaries (e.g. next to the query's own row, for the mask).  Free members take random positions.
    Positions already taken (planted entries, an earlier boundary's) are skipped; returns (spots, every position that was placed)."""
    R = len(rows)
    rng = np.random.default_rng(seed)
    used = set(int(p) for p in planted)

    def take(ps):
        out = []
        for p in ps:
            if 0 <= p < n and int(p) not in used:
                used.add(int(p)); out.append(int(p))
        return out

    top = [take((top_extra or {}).get(r, [])) for r in range(R)]
    dup = [take((dup_extra or {}).get(r, [])) for r in range(R)]
    quads = [[] for _ in range(R)]
    for i, b in enumerate(edges):
        quads[i % R].append(take(straddle(b, n)))
    spots = np.full((R, copies), -1, np.int64)
    for r in range(R):
        near_top = top[r] + [p for qd in quads[r][:2] for p in qd]
        dlist = dup[r] + [p for qd in quads[r][2:] for p in qd]
        rest = dlist[dups:]
        spots[r, :min(dups, len(dlist))] = dlist[:dups]
        for i, p in enumerate(near_top[:copies - dups]):
            spots[r, copies - 1 - i] = p
        rest += near_top[copies - dups:]
        free = [c for c in range(copies) if spots[r, c] < 0]
        assert len(rest) <= len(free), (r, len(rest), len(free))            # every boundary position is placed
        for c, p in zip(free, rest):
            spots[r, c] = p
    placed = set(int(p) for p in spots.ravel() if p >= 0)
    free = np.setdiff1d(np.arange(n), np.array(sorted(used)))
    holes = np.argwhere(spots < 0)
    spots[holes[:, 0], holes[:, 1]] = rng.choice(free, size=len(holes), replace=False)
    return spots, placed
