"""The near-copy cluster construction of tests/test_gpu_exact_rows_at_scale.py checked against the CPU oracle alone (no GPU): members
where they were asked to be, the oracle's best entries of a clustered query inside its cluster, exact duplicates in ascending index
order, near-copies strictly ordered - and the helper's default output unchanged (the existing cluster tests keep their inputs)."""
import numpy as np
import pytest

import helpers
import oracle_lib
from so_dso_place_recognition_amd import synth


def _near_copy_clusters_before_placement_control(type_, n, m, rows, copies=40, seed=21, db_seed=45, q_seed=46):
    """helpers.near_copy_clusters as it was before its spots / dups / db arguments (random positions, no exact copies)."""
    rng = np.random.default_rng(seed)
    if type_ == "sc":
        db = synth.sc_database(db_seed, n)
        q, planted = synth.sc_queries(q_seed, db, m)
    else:
        db = synth.m2dp_database(db_seed, n)
        q, planted = synth.m2dp_queries(q_seed, db, m)
    pool = np.setdiff1d(np.arange(n), planted)
    spots = rng.choice(pool, size=len(rows) * copies, replace=False).reshape(len(rows), copies)
    members = {}
    for r, t in enumerate(rows):
        delta = 10.0 ** rng.uniform(-8.5, -5.5)
        sign = rng.choice([-1.0, 1.0])
        if type_ == "sc":
            e = db[planted[t]]
            pick = rng.choice(np.nonzero(e[:1200] > 0)[0], size=30, replace=False)
            for c in range(copies):
                x = e.copy()
                x[pick] *= 1.0 + sign * (c + 1) * delta
                db[spots[r, c]] = x
        else:
            e = db[4 * planted[t]: 4 * planted[t] + 4]
            pick = rng.choice(64, size=20, replace=False)
            for c in range(copies):
                x = e.copy()
                x[:, pick] *= 1.0 + sign * (c + 1) * delta * 0.03
                db[4 * spots[r, c]: 4 * spots[r, c] + 4] = x
        members[int(t)] = np.concatenate([[planted[t]], spots[r]])
    return db, q, planted, members


@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_default_clusters_are_unchanged(type_):
    a = helpers.near_copy_clusters(type_, *helpers.CLUSTER_CASE)
    b = _near_copy_clusters_before_placement_control(type_, *helpers.CLUSTER_CASE)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3].keys() == b[3].keys() and all(np.array_equal(a[3][t], b[3][t]) for t in b[3])


def test_slice_edges():
    e = helpers.slice_edges(100_000)
    assert {12_500 * s for s in range(1, 8)} <= set(e) and {100_000 * s // 64 for s in range(1, 64)} <= set(e)
    assert {33_333, 66_666, 100_000} <= set(e) and 33_333 + 33_333 * 3 // 8 in e and 0 not in e
    e = helpers.slice_edges(99_997)
    assert 99_997 * 5 // 64 in e and 99_997 * 3 // 8 in e and 2 * 99_997 // 3 in e and 99_997 in e
    assert helpers.straddle(12_500, 100_000) == [12_499, 12_500, 12_498, 12_501] and helpers.straddle(100_000, 100_000) == [99_999, 99_998]


@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_boundary_clusters_against_the_oracle(type_):
    n, m, copies, dups = 3000, 64, 40, 12
    rows = list(range(1, m, 4))
    db_seed, q_seed = 45, 46
    db = synth.sc_database(db_seed, n) if type_ == "sc" else synth.m2dp_database(db_seed, n)
    _, planted = (synth.sc_queries if type_ == "sc" else synth.m2dp_queries)(q_seed, db, m)
    edges = helpers.slice_edges(n)
    top = {r: [n - m + t - 99, n - m + t - 100] for r, t in enumerate(rows)}
    dup = {r: [t + 99, t + 100] for r, t in enumerate(rows)}
    spots, placed = helpers.cluster_spots(n, rows, copies, dups, planted, edges, top, dup)
    db, q, planted2, members = helpers.near_copy_clusters(type_, n, m, rows, copies, db_seed=db_seed, q_seed=q_seed, spots=spots,
                                                          dups=dups, db=db)
    assert np.array_equal(planted, planted2)
    for r, t in enumerate(rows):                                        # members where they were asked to be
        assert np.array_equal(members[t][1:], spots[r])
    want = {j for b in edges for j in helpers.straddle(b, n)} - set(planted.tolist())
    assert want <= placed and placed <= set(spots.ravel().tolist())     # every position around every boundary holds a member
    div = 1 if type_ == "sc" else 4
    for r, t in enumerate(rows):                                        # the copies are copies, bit for bit
        e = db[div * planted[t]: div * planted[t] + div]
        for c in range(copies):
            x = db[div * spots[r, c]: div * spots[r, c] + div]
            assert np.array_equal(x, e) == (c < dups), (t, c)
    rc, oidx, osc = oracle_lib.match_topk(0 if type_ == "sc" else 1, q, db, 0, 2.0, copies + 1)
    assert rc == 0
    far = 0
    for r, t in enumerate(rows):
        cl = members[t].tolist()
        assert set(oidx[t, :5]) <= set(cl) and set(oidx[t]) == set(cl), t      # the whole cluster first
        tie = set([int(planted[t])] + spots[r, :dups].tolist())
        pos = [i for i, j in enumerate(oidx[t]) if j in tie]
        assert pos == list(range(pos[0], pos[0] + dups + 1)), t                  # the exact copies: one run of equal scores ...
        assert np.all(osc[t, pos] == osc[t, pos[0]]) and np.all(np.diff(oidx[t, pos]) > 0), t          # ... in ascending index order
        near = [i for i in range(copies + 1) if i not in pos]
        assert np.all(np.diff(osc[t, near]) > 0), t                              # near-copies: strictly increasing scores
        assert np.all(np.diff(osc[t]) < 1e-3), t                                # ... a hair's breadth apart
        far += pos[0] == 0
    assert 0 < far < len(rows)                    # both kinds: clusters led by the exact copies, and by near-copies approaching the query
