"""The case generator of the resident-matcher fuzz (tests/resident_fuzz_cases.py) delivers what its labels claim: conditions on the CPU
oracle's fp64 distances alone, over the committed seed set, and the generator's restatement of the matchers' slab geometry against the
constants in the source text."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import resident_fuzz_cases as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "so_dso_place_recognition_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def const(text, name):
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


def test_geometry_restates_the_source_text():
    g, d, b = source("gist_match.cpp"), source("delight_match.cpp"), source("bow_match.cpp")
    core = source("resident_match.hpp")        # what the two kinds share is defined once, there
    assert const(core, "MAX_CAND") == F.MAX_CAND and const(core, "MAX_SLABS") == F.MAX_SLABS and const(core, "QCAP") == F.QCAP
    assert f"db->xcap = std::min({F.XCAP}, db->qcap);" in core
    assert "const int n = db->count, C = k + 8;" in core
    for text in (g, d):
        # ... and the kinds use those very names: no definition of their own
        assert "namespace rm = pr::resident;\nusing pr::fail;\nusing rm::MAX_CAND;\nusing rm::MAX_SLABS;\nusing rm::QCAP;\n" in text
        assert not re.search(r"constexpr int (MAX_CAND|MAX_SLABS|QCAP)\b", text) and "xcap =" not in text and "C = k" not in text
        assert "S = std::min(S, std::min(MAX_CAND / C, MAX_SLABS));" in text
    assert "return create_db(ctx, max_sigs, cols, QCAP, out);" in g and "return create_db(ctx, max_sigs, QCAP, out);" in d
    assert f"const int qtiles = (mc + {F.GIST_TILE - 1}) / {F.GIST_TILE}, DT = (n + {F.GIST_TILE - 1}) / {F.GIST_TILE};" in g
    assert f"int S = std::max({F.GIST_MIN_SLABS}, ({F.GIST_SLAB_WORK} + qtiles - 1) / qtiles);" in g
    assert "S = std::max(1, std::min(S, DT));" in g
    assert "const int t0 = (int)((long long)DT * s / S), t1 = (int)((long long)DT * (s + 1) / S);" in source("gist_match.hip")
    assert f"const int qb = (mc + {F.DELIGHT_QUERIES_PER_WG - 1}) / {F.DELIGHT_QUERIES_PER_WG};" in d
    assert f"int S = ({F.DELIGHT_SLAB_WORK} + qb - 1) / qb;" in d
    assert f"S = std::max(1, std::min(S, (n + {F.DELIGHT_MIN_ENTRIES - 1}) / {F.DELIGHT_MIN_ENTRIES}));" in d
    assert "const int j0 = (int)((long long)n * s / S), j1 = (int)((long long)n * (s + 1) / S);" in source("delight_match.hip")
    assert f'env_int("PR_BOW_TAIL_ROWS", {F.BOW_TAIL_ROWS})' in b
    # the figures the existing GPU tests quote for their own shapes
    assert np.all(np.diff(F.slab_bounds("delight", 256, 3200, 1)) == 100)          # test_near_copy_cluster_is_ranked_in_fp64
    assert int(np.diff(F.slab_bounds("delight", 100, 4000, 5)).min()) == 48         # test_more_flagged_queries_than_one_pass_holds
    assert int(np.diff(F.slab_bounds("delight", 300, 4000, 5)).min()) == 142
    assert F.slab_count("gist", 6, 300, 128) == 10 and F.slab_count("gist", 6, 12, 5) == 1   # test_db_rows_outside_the_f16_range_are_not_lost
    for kind in ("gist", "delight"):
        for m, n, k in ((1, 1, 1), (400, 6000, 128), (33, 77, 5), (257, 100000, 1)):
            bnd = F.slab_bounds(kind, m, n, k)
            assert bnd[0] == 0 and bnd[-1] == n and np.all(np.diff(bnd) >= 0) and (len(bnd) - 1) * (k + 8) <= F.MAX_CAND


@pytest.mark.parametrize("kind", F.KINDS)
def test_draws_are_reproducible(kind):
    for seed, i in F.SEED_SET[kind][:12]:
        a, b = F.draw(kind, seed, i), F.draw(kind, seed, i)
        assert F.bits_equal(a.q, b.q) and F.bits_equal(a.db, b.db) and a.label == b.label
        assert (a.m, a.n, a.k, a.mask_width, a.q_row0, a.db_row0, a.chunks, a.cuts) == (b.m, b.n, b.k, b.mask_width, b.q_row0, b.db_row0, b.chunks, b.cuts)
    other = F.draw(kind, F.SEED_SET[kind][0][0] + 1000, 0)
    first = F.draw(kind, *F.SEED_SET[kind][0])
    assert other.q.shape != first.q.shape or not np.array_equal(other.q, first.q)


@pytest.mark.parametrize("kind", F.KINDS)
def test_cases_are_well_formed_and_within_the_matchers_arguments(kind):
    """what the GPU forms need of a case: a case they could not take is the generator's to reject, not the device test's to skip"""
    div = F.DIV[kind]
    for seed, i in F.SEED_SET[kind]:
        c = F.draw(kind, seed, i)
        assert 1 <= c.k <= 128 and c.m >= 1 and c.n >= 1 and c.mask_width >= 0 and c.q_row0 >= 0 and c.db_row0 >= 0
        assert c.q.shape == (div * c.m, c.cols) and c.db.shape == (div * c.n, c.cols) and c.q.dtype == c.db.dtype == np.float64
        assert sum(c.chunks) == c.n and all(x >= 0 for x in c.chunks) and len(c.chunks) <= 12
        assert c.cuts[0] == 0 and c.cuts[-1] == c.n and all(b > a for a, b in zip(c.cuts[:-1], c.cuts[1:]))
        if kind == "delight":
            assert c.m * c.n <= F.WORK[kind]
        if kind == "bow":                                                   # conforming rows: integer ids in [0, vocab), strictly ascending
            for a, cnt in ((c.q, c.m), (c.db, c.n)):
                for r in range(cnt):
                    ids = a[2 * r, :F._bow_len(a[2 * r], c.cols)]
                    assert np.all(ids == np.rint(ids)) and np.all(ids >= 0) and np.all(ids < c.vocab) and np.all(np.diff(ids) > 0)


@pytest.mark.parametrize("kind", F.KINDS)
def test_every_label_holds_in_the_oracles_distances(kind):
    seen = Counter()
    for seed, i in F.SEED_SET[kind]:
        c = F.draw(kind, seed, i)
        seen.update(set(c.label))
        bounds = F.slab_bounds(kind, c.m, c.n, c.k, c.tail_rows)
        qs = sorted({cl["query"] for cl in c.clusters} | {t["query"] for t in c.ties})
        if not qs:
            continue
        d = F.mask_distances(F.oracle_distance(kind, np.concatenate([c.rows(c.q, x, x + 1) for x in qs]), c.db), 0)
        gj = c.db_row0 + np.arange(c.n)
        for cl in c.clusters:
            qi = cl["query"]
            row = np.where(np.abs(c.q_row0 + qi - gj) < c.mask_width, np.inf, d[qs.index(qi)])
            dm = row[cl["rows"]]
            vis = dm[np.isfinite(dm)]
            tag = (kind, seed, i, cl["place"], cl["size"])
            assert cl["masked"] == int(np.isinf(dm).sum()), tag
            if cl["exact"] and not cl["compete"]:                           # planted exact ties: one value
                assert len(set(vis.tolist())) <= 1, tag
            if cl["shuffled"]:                                              # pairwise distinct in fp64 and not in index order
                assert len(set(vis.tolist())) == len(vis) >= 3, tag
                assert not np.array_equal(np.argsort(vis, kind="stable"), np.arange(len(vis))), tag
            if cl["fp32flat"]:
                assert len(set(vis.tolist())) == len(vis) and len(set(vis.astype(np.float32).tolist())) <= 2, tag
            if cl["wins"]:
                mine = np.concatenate([x["rows"] for x in c.clusters if x["query"] == qi])
                rest = np.delete(row, mine)
                rest = rest[~np.isnan(rest)]
                top = row[mine][np.isfinite(row[mine])].max()
                assert len(rest) == 0 or rest.min() > top, tag
            inner = bounds[1:-1]
            assert cl["straddles"] == bool(np.any((inner > cl["rows"][0]) & (inner <= cl["rows"][-1]))), tag
            if cl["place"] == "border":
                assert cl["straddles"], tag
            if cl["place"] == "inside":
                assert not cl["straddles"], tag
            if cl["place"] == "row0":
                assert cl["rows"][0] == 0, tag
            if cl["place"] == "last":
                assert cl["rows"][-1] == c.n - 1, tag
            if cl["place"] == "masked":
                assert 0 < cl["masked"] < len(cl["rows"]), tag
            size = {"C-2": c.C - 2, "C-1": c.C - 1, "C": c.C, "C+1": c.C + 1, "C+2": c.C + 2, "40": 40, "130": 130}.get(cl["size"])
            assert size is None or size == len(cl["rows"]), tag
        for t in c.ties:                                                    # duplicated rows (permutation images): one distance, low and high index
            row = d[qs.index(t["query"])][t["rows"]]
            assert len(set(row.tolist())) == 1 and len(t["rows"]) >= 2 and t["rows"][0] < t["rows"][-1], (kind, seed, i)
    missing = {f: seen[f] for f in F.flat_features(kind) if seen[f] < 3}
    assert not missing, f"{kind}: labels held by fewer than 3 cases of the seed set: {missing}"
