"""The online signature database (pr_online) without a device: the ABI surface, the argument errors that are returned before
any device is touched, the properties of the NumPy model the GPU tests compare the kernels with (online_model.py), and the separation of
the committed match cases (online_cases.py) on the oracle - the condition under which the device must return the oracle's indices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import online_cases
import online_model
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_online_create", "pr_online_destroy", "pr_online_reset", "pr_online_count", "pr_online_match_dev", "pr_online_append_dev",
         "pr_online_append")
OVERFLOW = online_model.OVERFLOW


def test_online_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_online_")) == sorted(NAMES)
    assert re.search(r"#define\s+PR_ONLINE_OVERFLOW\s+1\b", code) and _lib.ONLINE_OVERFLOW == 1 == OVERFLOW
    assert "typedef struct pr_online pr_online;" in code
    fields = re.search(r"typedef struct pr_online_buffers \{(.*?)\} pr_online_buffers;", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*;", fields)) == tuple(n for n, _ in _lib.OnlineBuffers._fields_) == api.OnlineDatabase.NAMES
    assert C.sizeof(_lib.OnlineBuffers) == 2 * C.sizeof(C.c_void_p)
    assert all(hasattr(api.OnlineDatabase, m) for m in ("match_torch", "append_torch", "step_torch", "align", "append", "reset", "count", "close"))
    assert hasattr(api.KeyframeMap, "verify_variants")
    for n in NAMES:                                    # the argument counts of the bindings are the header's
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n
    assert _lib.ONLINE_NB == online_cases.NB and {online_cases.NB - 1, online_cases.NB, online_cases.NB + 1} <= set(online_cases.COUNTS)


def _bufs(null=None):
    """a pr_online_buffers of non-NULL addresses that are never dereferenced (every case below fails before the device is touched)"""
    store = (C.c_double * 8)()
    b = _lib.OnlineBuffers(*([C.addressof(store)] * 2))
    if null:
        setattr(b, null, None)
    return b, store


PR_MAX_SIGS = 4000000


@pytest.mark.parametrize("args,word", [
    ((2, 16, 4), "type=2"), ((-1, 16, 4), "type=-1"), ((4, 16, 4), "type=4"),
    ((0, 0, 4), "capacity=0"), ((1, -3, 4), "capacity=-3"), ((0, PR_MAX_SIGS + 1, 4), "PR_MAX_SIGS"),
    ((0, 16, 0), "max_k=0"), ((1, 16, 129), "max_k=129"), ((0, 16, -1), "max_k=-1"),
    ((0, 16, 4), "ctx is NULL"), ((1, PR_MAX_SIGS, 128), "ctx is NULL")])
def test_online_create_argument_errors(args, word):
    """Value checks come before anything touches a device: PR_EINVAL and a message that names the argument.  (The NULL context is the last
    check: a valid argument set reaches it.)"""
    lib = _lib.load()
    assert f"#define PR_MAX_SIGS {PR_MAX_SIGS} " in open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    b, keep = _bufs()
    h = C.c_void_p(1)
    type_, cap, max_k = args
    assert lib.pr_online_create(None, type_, C.byref(b), cap, max_k, C.byref(h)) == _lib.PR_EINVAL and not h.value
    msg = lib.pr_last_error(None).decode()
    assert "pr_online_create" in msg and word in msg, msg


@pytest.mark.parametrize("name", api.OnlineDatabase.NAMES)
def test_online_create_null_buffer(name):
    lib = _lib.load()
    b, keep = _bufs(null=name)
    h = C.c_void_p(1)
    assert lib.pr_online_create(None, 0, C.byref(b), 16, 4, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert b"a buffer is NULL" in lib.pr_last_error(None)


def test_online_null_handles_and_values():
    lib = _lib.load()
    b, keep = _bufs()
    n, f = C.c_int32(7), C.c_int32(7)
    buf = (C.c_double * 64)()
    assert lib.pr_online_create(None, 0, C.byref(b), 16, 4, None) == _lib.PR_EINVAL and b"out is NULL" in lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_online_create(None, 0, None, 16, 4, C.byref(h)) == _lib.PR_EINVAL and b"buffers is NULL" in lib.pr_last_error(None)
    assert lib.pr_online_reset(None) == _lib.PR_EINVAL and b"pr_online_reset" in lib.pr_last_error(None)
    assert lib.pr_online_count(None, C.byref(n), C.byref(f)) == _lib.PR_EINVAL and b"pr_online_count" in lib.pr_last_error(None)
    match = lambda mask, p, k: lib.pr_online_match_dev(None, buf, buf, mask, p, k, buf, buf, buf)
    assert match(0, 2.0, 1) == _lib.PR_EINVAL and b"pr_online_match_dev: database is NULL" in lib.pr_last_error(None)
    assert match(-1, 2.0, 1) == _lib.PR_EINVAL and b"mask_width=-1" in lib.pr_last_error(None)
    for p in (float("nan"), float("inf"), -float("inf")):
        assert match(0, p, 1) == _lib.PR_EINVAL and b"p_weight is not finite" in lib.pr_last_error(None)
    for k in (0, -2, 129):
        assert match(0, 2.0, k) == _lib.PR_EINVAL and b"k=%d outside" % k in lib.pr_last_error(None)
    assert lib.pr_online_append_dev(None, buf, buf, buf) == _lib.PR_EINVAL and b"pr_online_append_dev: database is NULL" in lib.pr_last_error(None)
    assert lib.pr_online_append(None, buf, buf) == _lib.PR_EINVAL and b"pr_online_append: database is NULL" in lib.pr_last_error(None)
    lib.pr_online_destroy(None)                        # a no-op


def test_online_database_rejects_an_unknown_type_before_the_library():
    with pytest.raises(ValueError, match="'sc' or 'm2dp'"):
        api.OnlineDatabase(None, "delight", 16)


# ------------------------------------------------------------------------------------------------ the model's own properties
def row(type_, tag):
    rps, L = online_model.SHAPES[type_]
    return np.random.default_rng(tag).random((rps, L)) + tag


@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_model_count_never_exceeds_the_capacity_and_overflow_is_sticky(type_):
    m = online_model.OnlineModel(type_, 3)
    rps = m.rps
    infos = [m.append(row(type_, t)) for t in range(5)]
    assert [list(i) for i in infos] == [[1, 0, 1, 0], [1, 1, 2, 0], [1, 2, 3, 0], [0, -1, 3, OVERFLOW], [0, -1, 3, OVERFLOW]]
    assert list(m.state) == [3, OVERFLOW, 0, 0] and m.count == 3
    for t in range(3):
        assert np.array_equal(m.sig[t * rps:(t + 1) * rps], row(type_, t))
    assert list(m.append(row(type_, 9), emitted=[0])) == [0, -1, 3, OVERFLOW]          # the flag stays in every later info
    m.reset()
    assert list(m.state) == [0, 0, 0, 0] and list(m.append(row(type_, 7))) == [1, 0, 1, 0]


@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_model_emitted_zero_changes_nothing(type_):
    m = online_model.OnlineModel(type_, 4)
    m.append(row(type_, 1)); m.append(row(type_, 2))
    sig, state = m.sig.copy(), m.state.copy()
    idx, score, info = m.step(row(type_, 3), k=3, emitted=[0])
    assert list(idx[0]) == [-1, -1, -1] and np.isnan(score).all() and list(info) == [0, -1, 2, 0]
    assert np.array_equal(m.sig, sig) and np.array_equal(m.state, state)
    idx, score, info = m.step(row(type_, 3), k=3, emitted=[1])
    assert list(info) == [1, 2, 3, 0] and idx[0, 0] >= 0 and idx[0, 2] == -1 and np.isnan(score[0, 2])


def test_model_under_two_rows_nothing_is_reported_and_the_query_is_row_n():
    c = online_cases.edge_case("sc")
    for n in (0, 1):
        idx, score = online_model.match_rows(c["dp"][:n], c["di"][:n], 5, 2.0, 3)
        assert (idx == -1).all() and np.isnan(score).all()
    # the mask counts from row n: with mask_width = 2 exactly the last row (|n - j| = 1) is +Inf and comes last
    n = 6
    idx, score = online_model.match_rows(c["dp"][:n], c["di"][:n], 2, 2.0, n)
    assert idx[0, -1] == n - 1 and np.isposinf(score[0, -1]) and np.isfinite(score[0, :-1]).all()
    assert sorted(idx[0]) == list(range(n))


# ------------------------------------------------------------------------------------------------ the committed cases are separated
@pytest.mark.parametrize("type_", ["sc", "m2dp"])
def test_edge_cases_are_separated_on_the_oracle(type_):
    """For every case and every count it is matched at, consecutive scores among the oracle's k + 1 best differ by more than 1e-6 or
    belong to exact copies (or are both the mask's +Inf: online_cases.separated)."""
    c = online_cases.edge_case(type_)
    rps = online_model.SHAPES[type_][0]
    checked = 0
    for n in online_cases.COUNTS:
        for k, w in online_cases.KM:
            idx, score = online_model.match_rows(c["dp"][:n], c["di"][:n], w, 2.0, k + 1)
            assert online_cases.separated(c["db"], rps, idx[0], score[0]), (type_, n, k, w, idx, score)
            checked += 1
    assert checked == len(online_cases.COUNTS) * len(online_cases.KM)


def test_corner_cases_are_separated_on_the_oracle():
    c = online_cases.corner_case()
    for q in (c["q"], c["zero"]):
        dp, di = online_model.distances("sc", q, c["db"])
        for n in online_cases.CORNER_COUNTS:
            for k, w in online_cases.CORNER_KM:
                for p in online_cases.CORNER_WEIGHTS:
                    idx, score = online_model.match_rows(dp[:n], di[:n], w, p, k + 1)
                    assert online_cases.separated(c["db"], 1, idx[0], score[0]), (n, k, w, p, idx, score)
    dp, di = online_model.distances("sc", c["q"], c["db"])
    assert np.isnan(dp[c["zero_row"]]) and np.isnan(di[c["zero_row"]]) and np.isfinite(np.delete(dp, c["zero_row"])).all()
    for a, b in c["copies"]:
        assert dp[a] == dp[b] and di[a] == di[b]
    idx, _ = online_model.match_rows(dp, di, 0, 2.0, 2)
    assert list(idx[0]) == [7, 20]                     # the planted row and its copy: the tie goes to the lower index
