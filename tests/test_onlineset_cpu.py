"""The online signature sets (pr_onlineset) without a device: the ABI surface, the argument errors that are returned before
any device is touched, the NumPy model the GPU tests compare the kernels with (onlineset_model.py) against the oracle's fused matcher and
its own append / emitted properties, and the separation of the committed cases (onlineset_cases.py) on the oracle - the condition under
which the device must return the model's indices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import online_cases
import onlineset_cases as cases
import onlineset_model as model
import oracle_lib
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_onlineset_create", "pr_onlineset_destroy", "pr_onlineset_reset", "pr_onlineset_count", "pr_onlineset_match_dev",
         "pr_onlineset_append_dev", "pr_onlineset_append")
OVERFLOW = model.OVERFLOW
FUSED, DELIGHT = 0, 1
PR_MAX_SIGS = 4000000


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "place_recognition.h")).read(), flags=re.S)


def test_onlineset_symbols_are_declared_and_bound():
    code = header()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n                     # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_onlineset_")) == sorted(NAMES)
    assert not any(n.startswith("pr_online_") for n in NAMES)                        # a family of its own: pr_online_* stays as it is
    assert re.search(r"enum\s*\{\s*PR_ONLINESET_FUSED\s*=\s*0\s*,\s*PR_ONLINESET_DELIGHT\s*=\s*1\s*\}", code)
    assert (_lib.ONLINESET_FUSED, _lib.ONLINESET_DELIGHT) == (FUSED, DELIGHT) and _lib.ONLINE_OVERFLOW == OVERFLOW
    assert "typedef struct pr_onlineset pr_onlineset;" in code
    fields = re.search(r"typedef struct pr_onlineset_buffers \{(.*?)\} pr_onlineset_buffers;", code, flags=re.S).group(1)
    names = tuple(re.findall(r"\*\s*(\w+)\s*;", fields))
    assert names == tuple(n for n, _ in _lib.OnlineSetBuffers._fields_) == ("sc", "m2dp", "delight", "state")
    assert C.sizeof(_lib.OnlineSetBuffers) == 4 * C.sizeof(C.c_void_p)
    for i, n in enumerate(names):                      # the record layout: four pointers in the header's order
        assert getattr(_lib.OnlineSetBuffers, n).offset == i * C.sizeof(C.c_void_p)
    for kind in ("fused", "delight"):
        assert set(api.OnlineSet.NAMES[kind]) <= set(names)
        assert tuple(n for n, _, _ in api.OnlineSet.PARTS[kind]) + ("state",) == api.OnlineSet.NAMES[kind]
        assert api.OnlineSet.PARTS[kind] == model.PARTS[kind] and api.OnlineSet.CHANNELS[kind] == model.CHANNELS[kind]
    assert all(hasattr(api.OnlineSet, m) for m in ("match_torch", "append_torch", "step_torch", "align", "append", "reset", "count", "close"))
    assert (_lib.ONLINESET_NB_FUSED, _lib.ONLINESET_NB_DELIGHT) == (cases.NB_FUSED, cases.NB_DELIGHT)
    assert cases.NB_FUSED == online_cases.NB           # FUSED_COUNTS are online_cases.COUNTS: the same edges
    assert {cases.DELIGHT_EDGE - 1, cases.DELIGHT_EDGE, cases.DELIGHT_EDGE + 1} <= set(cases.DELIGHT_COUNTS) and cases.DELIGHT_EDGE + 1 <= cases.NMAX


def _bufs(kind, null=None, extra=None):
    """a pr_onlineset_buffers of non-NULL addresses (for the kind's parts) that are never dereferenced: every case fails before the device"""
    store = (C.c_double * 8)()
    a = C.addressof(store)
    b = _lib.OnlineSetBuffers(*((a, a, None, a) if kind == FUSED else (None, None, a, a)))
    if null:
        setattr(b, null, None)
    if extra:
        setattr(b, extra, a)
    return b, store


@pytest.mark.parametrize("args,word", [
    ((2, 16, 4), "kind=2"), ((-1, 16, 4), "kind=-1"),
    ((FUSED, 0, 4), "capacity=0"), ((DELIGHT, -3, 4), "capacity=-3"), ((FUSED, PR_MAX_SIGS + 1, 4), "PR_MAX_SIGS"),
    ((FUSED, 16, 0), "max_k=0"), ((DELIGHT, 16, 129), "max_k=129"), ((FUSED, 16, -1), "max_k=-1"),
    ((FUSED, 16, 4), "ctx is NULL"), ((DELIGHT, PR_MAX_SIGS, 128), "ctx is NULL")])
def test_onlineset_create_argument_errors(args, word):
    """Value checks come before anything touches a device: PR_EINVAL and a message that names the argument.  (The NULL context is the last
    check: a valid argument set reaches it.)"""
    lib = _lib.load()
    kind, cap, max_k = args
    b, keep = _bufs(kind if kind in (FUSED, DELIGHT) else FUSED)
    h = C.c_void_p(1)
    assert lib.pr_onlineset_create(None, kind, C.byref(b), cap, max_k, C.byref(h)) == _lib.PR_EINVAL and not h.value
    msg = lib.pr_last_error(None).decode()
    assert "pr_onlineset_create" in msg and word in msg, msg


@pytest.mark.parametrize("kind,null,extra,word", [
    (FUSED, "sc", None, "a buffer is NULL"), (FUSED, "m2dp", None, "a buffer is NULL"), (FUSED, "state", None, "a buffer is NULL"),
    (DELIGHT, "delight", None, "a buffer is NULL"), (DELIGHT, "state", None, "a buffer is NULL"),
    (FUSED, None, "delight", "delight must be NULL"), (DELIGHT, None, "sc", "sc and m2dp must be NULL"),
    (DELIGHT, None, "m2dp", "sc and m2dp must be NULL")])
def test_onlineset_create_buffers_of_the_wrong_kind(kind, null, extra, word):
    lib = _lib.load()
    b, keep = _bufs(kind, null=null, extra=extra)
    h = C.c_void_p(1)
    assert lib.pr_onlineset_create(None, kind, C.byref(b), 16, 4, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert word.encode() in lib.pr_last_error(None), lib.pr_last_error(None)


def test_onlineset_null_handles_and_values():
    lib = _lib.load()
    b, keep = _bufs(FUSED)
    n, f = C.c_int32(7), C.c_int32(7)
    buf = (C.c_double * 64)()
    assert lib.pr_onlineset_create(None, FUSED, C.byref(b), 16, 4, None) == _lib.PR_EINVAL and b"out is NULL" in lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_onlineset_create(None, FUSED, None, 16, 4, C.byref(h)) == _lib.PR_EINVAL and b"buffers is NULL" in lib.pr_last_error(None)
    assert lib.pr_onlineset_reset(None) == _lib.PR_EINVAL and b"pr_onlineset_reset" in lib.pr_last_error(None)
    assert lib.pr_onlineset_count(None, C.byref(n), C.byref(f)) == _lib.PR_EINVAL and b"pr_onlineset_count" in lib.pr_last_error(None)
    match = lambda mask, p, k: lib.pr_onlineset_match_dev(None, buf, buf, None, buf, mask, p, k, buf, buf, buf)
    assert match(0, 2.0, 1) == _lib.PR_EINVAL and b"pr_onlineset_match_dev: set is NULL" in lib.pr_last_error(None)
    assert match(-1, 2.0, 1) == _lib.PR_EINVAL and b"mask_width=-1" in lib.pr_last_error(None)
    for p in (float("nan"), float("inf"), -float("inf")):
        assert match(0, p, 1) == _lib.PR_EINVAL and b"p_weight is not finite" in lib.pr_last_error(None)
    for k in (0, -2, 129):
        assert match(0, 2.0, k) == _lib.PR_EINVAL and b"k=%d outside" % k in lib.pr_last_error(None)
    assert lib.pr_onlineset_append_dev(None, buf, buf, None, buf, buf) == _lib.PR_EINVAL
    assert b"pr_onlineset_append_dev: set is NULL" in lib.pr_last_error(None)
    assert lib.pr_onlineset_append(None, buf, buf, None, buf) == _lib.PR_EINVAL and b"pr_onlineset_append: set is NULL" in lib.pr_last_error(None)
    lib.pr_onlineset_destroy(None)                     # a no-op


def test_onlineset_rejects_an_unknown_kind_before_the_library_and_pr_online_is_unchanged():
    with pytest.raises(ValueError, match="'fused' or 'delight'"):
        api.OnlineSet(None, "sc", 16)
    with pytest.raises(ValueError, match="'sc' or 'm2dp'"):
        api.OnlineDatabase(None, "delight", 16)
    lib = _lib.load()
    store = (C.c_double * 8)()
    b = _lib.OnlineBuffers(C.addressof(store), C.addressof(store))
    h = C.c_void_p(1)
    assert lib.pr_online_create(None, _lib.TYPE_DELIGHT, C.byref(b), 16, 4, C.byref(h)) == _lib.PR_EINVAL and b"type=2" in lib.pr_last_error(None)


# ------------------------------------------------------------------------------------------------ the model against the oracle
def test_model_fusion_equals_the_oracles_fused_matcher():
    """m = 1, n = 12, mask 0, k = 5: the model's four z-scores and their sum against pr_ref_match_topk_fused - indices equal, scores
    within 1e-12 (measured: 0.0 at both weights)."""
    c = cases.fused_edge_case()
    n, k = 12, 5
    sc, m2 = cases.rows_of("fused", c["db"], 0, n)
    for p in cases.WEIGHTS:
        rc, oi, os_ = oracle_lib.match_topk_fused(c["q"][0], c["q"][1], sc, m2, 0, p, k)
        assert rc == 0
        mi, ms = model.match_rows("fused", c["d"][:, :n], 0, p, k)
        print("   p", p, "idx", mi[0].tolist(), "max |model - oracle|", float(np.abs(ms - os_).max()))
        assert np.array_equal(mi, oi) and mi[0, 0] == 1
        assert np.abs(ms - os_).max() <= 1e-12
    # the channel order: d[0:2] are SC's rows and d[2:4] M2DP's, as the one-part model gives them
    import online_model
    dp, di = online_model.distances("sc", c["q"][0], sc)
    ep, ei = online_model.distances("m2dp", c["q"][1], m2)
    assert np.array_equal(c["d"][:, :n], np.stack([dp, di, ep, ei]))


def test_model_mask_comes_after_the_sum_and_delight_needs_one_row_only():
    d = np.array([[0.1, 0.2, np.nan, 0.4, 0.3]] * 4)
    d = d + np.arange(4)[:, None] * 0.01 * np.arange(5)[None, :]
    idx, score = model.match_rows("fused", d, 0, 2.0, 5)
    assert 2 not in idx[0] and idx[0, -1] == -1 and np.isnan(score[0, -1])            # NaN is never selected ...
    idx, score = model.match_rows("fused", d, 4, 2.0, 5)                              # ... but under the mask (rows 2, 3, 4 of n = 5) it is +Inf
    assert idx[0].tolist()[2:] == [2, 3, 4] and np.isposinf(score[0, 2:]).all() and np.isfinite(score[0, :2]).all()
    for n in (0, 1):
        idx, score = model.match_rows("fused", d[:, :n], 0, 2.0, 3)
        assert (idx == -1).all() and np.isnan(score).all()
    idx, score = model.match_rows("delight", d[:1, :1], 0, 2.0, 3)
    assert idx[0].tolist() == [0, -1, -1] and score[0, 0] == d[0, 0] and np.isnan(score[0, 1:]).all()
    idx, score = model.match_rows("delight", d[:1, :0], 0, 2.0, 3)
    assert (idx == -1).all() and np.isnan(score).all()
    idx, score = model.match_rows("delight", d[:1], 2, 2.0, 5)                        # n = 5: row 4 masked; the NaN row is left out
    assert idx[0].tolist() == [0, 1, 4 - 1, 4, -1] and np.isposinf(score[0, 3])


# ------------------------------------------------------------------------------------------------ the model's own properties
def parts(kind, tag):
    rng = np.random.default_rng(tag)
    return tuple(rng.random((r, L)) + tag for _, r, L in model.PARTS[kind])


@pytest.mark.parametrize("kind", ["fused", "delight"])
def test_model_one_count_for_all_parts_and_overflow_is_sticky(kind):
    m = model.OnlineSetModel(kind, 3)
    infos = [m.append(parts(kind, t)) for t in range(5)]
    assert [list(i) for i in infos] == [[1, 0, 1, 0], [1, 1, 2, 0], [1, 2, 3, 0], [0, -1, 3, OVERFLOW], [0, -1, 3, OVERFLOW]]
    assert list(m.state) == [3, OVERFLOW, 0, 0] and m.count == 3
    for t in range(3):                                 # every part of keyframe t sits on row t; the overflowing keyframes left no part
        for got, want in zip(cases.rows_of(kind, m.rows(3), t), parts(kind, t)):
            assert np.array_equal(got, want)
    assert list(m.append(parts(kind, 9), emitted=[0])) == [0, -1, 3, OVERFLOW]         # the flag stays in every later info
    m.reset()
    assert list(m.state) == [0, 0, 0, 0] and list(m.append(parts(kind, 7))) == [1, 0, 1, 0]


@pytest.mark.parametrize("kind", ["fused", "delight"])
def test_model_emitted_zero_changes_nothing(kind):
    m = model.OnlineSetModel(kind, 4)
    m.append(parts(kind, 1)); m.append(parts(kind, 2))
    bufs, state = {n: a.copy() for n, a in m.bufs.items()}, m.state.copy()
    idx, score, info = m.step(parts(kind, 3), k=3, emitted=[0])
    assert list(idx[0]) == [-1, -1, -1] and np.isnan(score).all() and list(info) == [0, -1, 2, 0]
    assert all(np.array_equal(m.bufs[n], bufs[n]) for n in bufs) and np.array_equal(m.state, state)
    idx, score, info = m.step(parts(kind, 3), k=3, emitted=[1])
    assert list(info) == [1, 2, 3, 0] and idx[0, 0] >= 0 and idx[0, 2] == -1 and np.isnan(score[0, 2])


# ------------------------------------------------------------------------------------------------ the committed cases are separated
def test_fused_edge_cases_are_separated_on_the_oracle():
    """For every count, (k, mask) and weight: consecutive scores among the model's k + 1 best differ by more than 1e-6 (or are both the
    mask's +Inf), and the planted row 1 wins wherever it is held and not masked."""
    c = cases.fused_edge_case()
    gap = np.inf
    for n in cases.FUSED_COUNTS:
        for p in cases.WEIGHTS:
            f = model.fused_scores(c["d"][:, :n], p) if n >= 2 else None
            for k, w in cases.KM:
                idx, score = (model.select(f, w, k + 1) if n >= 2 else model.match_rows("fused", c["d"][:, :n], w, p, k + 1))
                assert cases.separated("fused", c["db"], idx[0], score[0], tol=1e-6), (n, k, w, p, idx, score)
                if n >= 2 and n - 1 >= w:
                    assert idx[0, 0] == 1, (n, k, w, p, idx)
                s = score[0][np.isfinite(score[0])]
                if len(s) > 1:
                    gap = min(gap, float(np.diff(s).min()))
    print("   smallest gap between consecutive returned scores:", gap)
    assert gap > 1e-6


def test_fused_corner_cases_are_separated_on_the_oracle():
    c = cases.fused_corner_case()
    for q in (c["q"], c["zero"]):
        d = model.distances("fused", q, c["db"])
        for n in cases.CORNER_COUNTS:
            for k, w in cases.CORNER_KM:
                for p in cases.CORNER_WEIGHTS:
                    idx, score = model.match_rows("fused", d[:, :n], w, p, k + 1)
                    assert cases.separated("fused", c["db"], idx[0], score[0], tol=1e-6), (n, k, w, p, idx, score)
    d = model.distances("fused", c["q"], c["db"])
    z = c["zero_row"]
    assert np.isnan(d[:2, z]).all() and np.isfinite(d[2:, z]).all() and np.isfinite(np.delete(d, z, axis=1)).all()
    assert cases.same_rows("fused", c["db"], 7, 20) and not cases.same_rows("fused", c["db"], 12, 33)
    assert np.array_equal(d[:, 7], d[:, 20]) and np.array_equal(d[:2, 12], d[:2, 33]) and not np.array_equal(d[2:, 12], d[2:, 33])
    idx, score = model.match_rows("fused", d, 0, 2.0, 2)
    assert list(idx[0]) == [7, 20] and score[0, 0] == score[0, 1]                     # the tie goes to the lower index
    idx, _ = model.match_rows("fused", d, 0, 2.0, 40)
    assert z not in idx[0] and idx[0, -1] == -1                                       # the zero SC row is never returned
    dz = model.distances("fused", c["zero"], c["db"])
    idx, score = model.match_rows("fused", dz, 3, 2.0, 5)                             # a zero SC query: only the masked rows, as +Inf
    assert idx[0].tolist() == [38, 39, -1, -1, -1] and np.isposinf(score[0, :2]).all()


def test_delight_cases_are_separated_on_the_oracle():
    c = cases.delight_edge_case()
    gap = np.inf
    for n in cases.DELIGHT_COUNTS:
        for k, w in cases.KM:
            idx, score = model.match_rows("delight", c["d"][:, :n], w, 2.0, k + 1)
            assert cases.separated("delight", c["db"], idx[0], score[0]), (n, k, w, idx, score)
            if n >= 2 and n - 1 >= w:
                assert idx[0, 0] == 1
            s = score[0][np.isfinite(score[0])]
            if len(s) > 1:
                gap = min(gap, float(np.diff(s).min()))
    print("   smallest gap:", gap)
    c = cases.delight_corner_case()
    z = c["zero_row"]
    for q in (c["q"], c["zero"]):
        d = model.distances("delight", q, c["db"])
        for n in cases.CORNER_COUNTS:
            for k, w in cases.CORNER_KM:
                idx, score = model.match_rows("delight", d[:, :n], w, 2.0, k + 1)
                assert cases.separated("delight", c["db"], idx[0], score[0]), (n, k, w, idx, score)
    d = model.distances("delight", c["q"], c["db"])
    assert d[0, 7] == d[0, 20] and np.isfinite(d).all()
    idx, _ = model.match_rows("delight", d, 0, 2.0, 2)
    assert list(idx[0]) == [7, 20]
    dz = model.distances("delight", c["zero"], c["db"])
    assert np.isposinf(dz[0, z]) and np.isfinite(np.delete(dz[0], z)).all()           # zero against zero: +Inf, not NaN
    idx, score = model.match_rows("delight", dz, 0, 2.0, 40)
    assert idx[0, -1] == z and np.isposinf(score[0, -1]) and sorted(idx[0]) == list(range(40))       # last, but selectable
