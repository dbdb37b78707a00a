"""Seeded adversarial fuzz of the device-resident BoW, GIST and DELIGHT matchers (matcher.BowMatcher / GistMatcher / DelightMatcher and
api.{bow,gist,delight}_match_topk) against the CPU oracle: oracle_lib.*_distance on the global matrix, then the mask, then select_topk.
Cases come from tests/resident_fuzz_cases.py (committed seed set; what they hold is checked on the CPU by test_resident_fuzz_cases.py).

Every case is answered in six forms, each compared with the oracle over all of its queries - indices equal, scores bit for bit:
  (a) the matcher with a bulk-packed DB;
  (b) the same with exact=True (BoW has no coarse pass to switch off: its second form runs the queries in chunks of 7, PR_BOW_CHUNK);
  (c) the DB grown in place by the case's schedule (reserve + appends; BoW with the case's tail segment, PR_BOW_TAIL_ROWS);
  (d) the DB cut at the case's shard borders, every shard matched with its db_row0, the lists merged by matcher.merge_topk;
  (e) the host-buffer entry point (it takes no row offsets: compared with the oracle's answer at q_row0 = db_row0 = 0);
  (f) one case in four: the call captured in a graph and replayed twice, both replays equal to the oracle.
No case and no query is excluded.  One line per case is printed (-s): label, m, n, k, mask, flagged, seconds (oracle share apart).

Budgets: the module should add no more than about a quarter to the wall time of `pytest tests -m gpu`, and the CPU oracle should stay
the smaller part of each case (DELIGHT: m n <= 2.5e5 pairs per case).  Measured on an MI355X (first run, also in DESIGN.md 7): the
module takes 26.0 s of the 412.6 s of `pytest tests -m gpu`, so it adds 6.7 % to the rest - inside the first budget.  The second is
missed: over the 147 cases the oracle takes 11.3 s and the six GPU forms 2.8 s (the per-case lines carry both times; drawing the cases
is the rest of the module's time).  If the wall time ever goes over, cut the seed set (resident_fuzz_cases.SEED_SET, with
tests/test_resident_fuzz_cases.py keeping every label at three cases)."""
import time

import numpy as np
import pytest

import resident_fuzz_cases as F
from so_dso_place_recognition_amd import api
from so_dso_place_recognition_amd.matcher import BowMatcher, DelightMatcher, GistMatcher, merge_topk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(kind, seed, i) for kind in F.KINDS for seed, i in F.SEED_SET[kind]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def differs(got, want):
    """None, or where the answer leaves the oracle's"""
    gi, gs = host(got[0]), host(got[1])
    wi, ws = want
    if np.array_equal(gi, wi) and F.bits_equal(gs, ws):
        return None
    bad = np.nonzero((gi != wi).any(1) | ~((gs == ws) | (np.isnan(gs) & np.isnan(ws))).all(1))[0]
    i = int(bad[0]) if len(bad) else 0
    return f"{len(bad)} queries differ; query {i}: idx {gi[i][:8]} / oracle {wi[i][:8]}, score {gs[i][:4]} / oracle {ws[i][:4]}"


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def make(c, max_q, max_db, ctx=None, exact=False, stream=False):
    if c.kind == "bow":
        return BowMatcher.on_new_stream(max_q, max_db, c.cols, c.vocab) if stream else BowMatcher(max_q, max_db, c.cols, c.vocab, ctx=ctx)
    if c.kind == "gist":
        return GistMatcher.on_new_stream(max_q, max_db, c.cols) if stream else GistMatcher(max_q, max_db, c.cols, ctx=ctx, exact=exact)
    return DelightMatcher.on_new_stream(max_q, max_db) if stream else DelightMatcher(max_q, max_db, ctx=ctx, exact=exact)


def flagged(c, mt):
    """queries the last match answered from their exact rows; the BoW matcher scores every pair exactly and has no such count"""
    return mt.flagged_count() if c.kind != "bow" else 0


def match(c, mt, q, db_row0=None):
    out = mt.match(q, c.mask_width, c.k, c.db_row0 if db_row0 is None else db_row0, c.q_row0)
    torch.cuda.synchronize()
    return out


def bulk(c, ctx):
    mt = make(c, c.m, c.n, ctx)
    mt.pack_database(dev(c.db))
    got = match(c, mt, dev(c.q))
    fl = flagged(c, mt)
    mt.close()
    return got, fl


@pytest.mark.parametrize("kind,seed,i", CASES)
def test_every_form_equals_the_oracle(ctx, monkeypatch, kind, seed, i):
    c = F.draw(kind, seed, i)
    t0 = time.time()
    d = F.oracle_distance(kind, c.q, c.db)
    want = F.oracle_select(d, c.mask_width, c.k, c.q_row0, c.db_row0)
    want0 = F.oracle_select(d, c.mask_width, c.k)
    t_oracle = time.time() - t0
    t0 = time.time()
    q = dev(c.q)
    bad = {}
    # (a) bulk
    got, fl = bulk(c, ctx)
    bad["bulk"] = differs(got, want)
    # (b) every query through its exact row (BoW: the queries in chunks of 7)
    if kind == "bow":
        monkeypatch.setenv("PR_BOW_CHUNK", "7")
        got, _ = bulk(c, ctx)
        monkeypatch.delenv("PR_BOW_CHUNK")
    else:
        mt = make(c, c.m, c.n, ctx, exact=True)
        mt.pack_database(dev(c.db))
        got = match(c, mt, q)
        assert mt.flagged_count() == c.m
        mt.close()
    bad["exact"] = differs(got, want)
    # (c) grown in place
    if kind == "bow":
        monkeypatch.setenv("PR_BOW_TAIL_ROWS", str(c.tail_rows))
    mt = make(c, c.m, c.n, ctx)
    if kind == "bow":
        monkeypatch.delenv("PR_BOW_TAIL_ROWS")
    at = c.chunks[0]
    mt.reserve_database(dev(c.rows(c.db, 0, at)) if at else None)
    for step in c.chunks[1:]:
        mt.append_database(dev(c.rows(c.db, at, at + step)))
        at += step
    assert mt.n == c.n
    bad["grown"] = differs(match(c, mt, q), want)
    mt.close()
    # (d) shards, merged
    parts = []
    for lo, hi in zip(c.cuts[:-1], c.cuts[1:]):
        mt = make(c, c.m, hi - lo, ctx)
        mt.pack_database(dev(c.rows(c.db, lo, hi)))
        parts.append(match(c, mt, q, c.db_row0 + lo))
        mt.close()
    got = merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), c.k)
    torch.cuda.synchronize()
    bad["shards"] = differs(got, want)
    # (e) the host-buffer entry point
    got = getattr(api, kind + "_match_topk")(c.q, c.db, c.mask_width, c.k, ctx=ctx)
    bad["host"] = differs(got, want0)
    # (f) captured and replayed twice
    if i % 4 == 0:
        mt = make(c, c.m, c.n, stream=True)
        with torch.cuda.stream(mt.stream):
            mt.pack_database(dev(c.db))
            qs = dev(c.q)
            mt.stream.synchronize()
        cap = mt.capture(qs, c.mask_width, c.k, c.db_row0, c.q_row0)
        for rep in (1, 2):
            got = cap.run()
            torch.cuda.synchronize()
            bad[f"replay {rep}"] = differs(got, want)
        del cap
        mt.close()
    print(f"\n{c!r} flagged={fl} {time.time() - t0:.2f}s (oracle {t_oracle:.2f}s)", end="")
    bad = {form: why for form, why in bad.items() if why}
    assert not bad, f"{c!r}: {bad}"


@pytest.mark.parametrize("kind", F.KINDS)
def test_seed_set_reaches_both_paths(ctx, kind):
    """The seed set keeps both answers of the two-stage matchers in play: cases the coarse pass carries alone, cases with some queries on
    their exact rows, and cases with more flagged queries than one exact-row pass holds (XCAP: chained passes).
    The BoW matcher has no coarse pass and no flagged count - every score comes from the inverted file.  Its two paths are the main lists
    and the tail segment of a grown DB: the seed set must hold grown forms that never fold, that fold, and that fold more than once
    inside one append."""
    if kind == "bow":
        never = folds = many = 0
        for seed, i in F.SEED_SET["bow"]:
            c = F.draw("bow", seed, i)
            tail = min(c.tail_rows, c.n)
            never += c.n - c.chunks[0] <= tail
            folds += c.n - c.chunks[0] > tail
            many += any(step > 2 * tail for step in c.chunks[1:])
        print(f"\nbow: grown forms that never fold {never}, that fold {folds}, with several folds in one append {many}")
        assert never >= 1 and folds >= 1 and many >= 1
        return
    none = some = chained = total = 0
    for seed, i in F.SEED_SET[kind]:
        c = F.draw(kind, seed, i)
        _, fl = bulk(c, ctx)
        total += fl
        none += fl == 0
        some += 0 < fl < c.m
        chained += fl > F.XCAP
        print(f"\n{c!r} flagged={fl}", end="")
    print(f"\n{kind}: {total} flagged queries; cases with none {none}, with some but not all {some}, with more than {F.XCAP}: {chained}")
    assert none >= 1 and some >= 1 and chained >= 1
