"""The resident keyframe map (pr_map) without a device: the ABI surface, the argument errors that are returned before any
device is touched, and the properties of the append rule on the NumPy model the GPU tests compare the kernels with (map_model.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_model
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_map_create", "pr_map_destroy", "pr_map_reset", "pr_map_count", "pr_map_append_dev", "pr_map_append", "pr_map_verify_dev")
OVERFLOW, DROPPED = map_model.OVERFLOW, map_model.DROPPED


def test_map_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_map_")) == sorted(NAMES)
    assert "PR_MAP_OVERFLOW = 1, PR_MAP_DROPPED = 2" in code and (_lib.MAP_OVERFLOW, _lib.MAP_DROPPED) == (1, 2) == (OVERFLOW, DROPPED)
    # the record of the seven buffers: the header's fields in the header's order, seven pointers
    fields = re.search(r"typedef struct pr_map_buffers \{(.*?)\} pr_map_buffers;", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*;", fields)) == tuple(n for n, _ in _lib.MapBuffers._fields_) == api.KeyframeMap.NAMES
    assert C.sizeof(_lib.MapBuffers) == 7 * C.sizeof(C.c_void_p)
    assert all(hasattr(api.KeyframeMap, m) for m in ("append_torch", "append_push", "append", "reset", "count", "close", "verify_dev", "clouds"))
    # the argument counts of the bindings are the header's
    for n in NAMES:
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n


def _bufs(null=None):
    """a pr_map_buffers of non-NULL addresses that are never dereferenced (every case below fails before the device is touched)"""
    store = (C.c_double * 8)()
    b = _lib.MapBuffers(*([C.addressof(store)] * 7))
    if null:
        setattr(b, null, None)
    return b, store


@pytest.mark.parametrize("args,word", [
    ((0, 100, 10, 1), "capacities"), ((-1, 100, 10, 1), "capacities"), ((4, 0, 10, 1), "capacities"), ((4, -5, 10, 1), "capacities"),
    ((4, 100, 0, 1), "capacities"), ((4, 100, 10, 0), "capacities"), ((4, 100, 10, -2), "capacities"),
    ((4, 100, 101, 1), "max_cloud_points"), ((4, 1 << 40, 1 << 30, 1 << 8), "2^38"), ((4, 100, 10, 1), "ctx is NULL")])
def test_map_create_argument_errors(args, word):
    """Value checks come before anything touches a device: PR_EINVAL and a message that names the argument.  (The NULL context is the last
    check: a valid argument set reaches it.)"""
    lib = _lib.load()
    b, keep = _bufs()
    h = C.c_void_p(1)
    rc = lib.pr_map_create(None, C.byref(b), *args, C.byref(h))
    assert rc == _lib.PR_EINVAL and not h.value
    msg = lib.pr_last_error(None).decode()
    assert "pr_map_create" in msg and word in msg, msg


@pytest.mark.parametrize("name", api.KeyframeMap.NAMES)
def test_map_create_null_buffer(name):
    lib = _lib.load()
    b, keep = _bufs(null=name)
    h = C.c_void_p(1)
    assert lib.pr_map_create(None, C.byref(b), 4, 100, 10, 1, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert b"a buffer is NULL" in lib.pr_last_error(None)


def test_map_null_handles_and_values():
    lib = _lib.load()
    b, keep = _bufs()
    k, f, n = C.c_int32(7), C.c_int32(7), C.c_int64(7)
    buf = (C.c_double * 64)()
    assert lib.pr_map_create(None, C.byref(b), 4, 100, 10, 1, None) == _lib.PR_EINVAL and b"out is NULL" in lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_map_create(None, None, 4, 100, 10, 1, C.byref(h)) == _lib.PR_EINVAL and b"buffers is NULL" in lib.pr_last_error(None)
    assert lib.pr_map_reset(None) == _lib.PR_EINVAL and b"pr_map_reset" in lib.pr_last_error(None)
    assert lib.pr_map_count(None, C.byref(k), C.byref(n), C.byref(f)) == _lib.PR_EINVAL and b"pr_map_count" in lib.pr_last_error(None)
    assert lib.pr_map_append_dev(None, buf, buf, buf, buf, buf, buf, buf, 1, 10, buf) == _lib.PR_EINVAL
    assert b"pr_map_append_dev: map is NULL" in lib.pr_last_error(None)
    assert lib.pr_map_append_dev(None, buf, buf, buf, buf, buf, buf, buf, -1, 10, buf) == _lib.PR_EINVAL
    assert b"pr_map_append_dev: N=-1" in lib.pr_last_error(None)
    assert lib.pr_map_append_dev(None, buf, buf, buf, buf, buf, buf, buf, 1, -1, buf) == _lib.PR_EINVAL
    assert b"max_points=-1" in lib.pr_last_error(None)
    assert lib.pr_map_append(None, buf, buf, buf, buf, buf, buf, buf, 1, buf) == _lib.PR_EINVAL
    assert b"pr_map_append: map is NULL" in lib.pr_last_error(None)
    assert lib.pr_map_append(None, buf, buf, buf, buf, buf, buf, buf, -3, buf) == _lib.PR_EINVAL and b"N=-3" in lib.pr_last_error(None)
    assert lib.pr_map_verify_dev(None, 0, buf, buf, 1, buf, 1, 1, buf, buf, 1, 1, 10, 30, 1.0, 1e-6, 1e-6, 3, 0.5, 0.5, buf, buf, buf, buf) == _lib.PR_EINVAL
    assert b"pr_map_verify_dev: map is NULL" in lib.pr_last_error(None)
    lib.pr_map_destroy(None)                        # a no-op


# ------------------------------------------------------------------------------------------------ the model's own properties
def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 5, (n, 3)), rng.random(n).astype(np.float32)


def frame(n, tag):
    f = np.arange(16, dtype=np.float64) + 100.0 * tag
    f[13] = n
    return f


def one(model, n, tag, **kw):
    x, it = cloud(n, tag)
    return model.append(x, it, [0, n], frame(n, tag), poses=np.full(12, float(tag)), ids=[tag], **kw)


def test_model_a_row_is_always_consumed_while_rows_remain():
    m = map_model.MapModel(5, 100, 40)
    sizes = [10, 41, 40, 30, 30]                       # stored, too large, stored, stored, does not fit
    infos = [one(m, n, t + 1) for t, n in enumerate(sizes)]
    assert [int(i[0]) for i in infos] == [1] * 5 and [int(i[1]) for i in infos] == [0, 1, 2, 3, 4] and [int(i[2]) for i in infos] == [1, 2, 3, 4, 5]
    assert list(m.offs) == [0, 10, 10, 50, 80, 80]     # the fifth cloud of 30 does not fit into the 20 points left
    assert [int(i[3]) for i in infos] == [0, OVERFLOW | DROPPED, OVERFLOW, OVERFLOW, OVERFLOW | DROPPED]
    assert list(m.ids) == [1, 2, 3, 4, 5] and np.array_equal(m.poses[:, 0], [1, 2, 3, 4, 5])      # pose and id of a dropped row are stored
    assert not m.frames[1].any() and not m.frames[4].any() and m.frames[0, 13] == 10 and m.frames[3, 13] == 30
    x, _ = cloud(40, 3)
    assert np.array_equal(m.xyz[10:50], x)
    i = one(m, 1, 6)                                   # no row left: not appended, nothing moves
    assert list(i) == [0, -1, 5, OVERFLOW] and list(m.offs) == [0, 10, 10, 50, 80, 80]


def test_model_overflow_is_sticky_and_dropped_is_the_calls():
    m = map_model.MapModel(4, 100, 40)
    assert list(one(m, 5, 1)) == [1, 0, 1, 0]
    assert list(one(m, 50, 2)) == [1, 1, 2, OVERFLOW | DROPPED]
    assert list(one(m, 5, 3)) == [1, 2, 3, OVERFLOW] and list(m.state) == [3, OVERFLOW, 0, 0]
    assert list(one(m, 5, 4, emitted=[0])) == [0, -1, 3, OVERFLOW]
    m.reset()
    assert list(m.state) == [0, 0, 0, 0] and not m.offs.any() and not m.frames.any()
    assert list(one(m, 5, 5)) == [1, 0, 1, 0]


def test_model_a_dropped_cloud_never_advances_offs_and_max_points_counts_from_the_calls_first_point():
    m = map_model.MapModel(8, 1000, 300, max_append=5)
    sizes = [0, 257, 1, 0, 256]
    offs = 7 + np.concatenate([[0], np.cumsum(sizes)])
    x, it = cloud(int(offs[-1]), 9)
    fr = np.stack([frame(n, t) for t, n in enumerate(sizes)])
    i = m.append(x, it, offs, fr, max_points=258)      # the last cloud lies beyond the 258 points the call covers
    assert list(i) == [5, 0, 5, OVERFLOW | DROPPED] and list(m.offs[:6]) == [0, 0, 257, 258, 258, 258]
    assert np.array_equal(m.xyz[:258], x[7:265]) and not m.frames[4].any() and m.frames[1, 13] == 257
    assert np.all(np.diff(m.offs[:m.keyframes + 1]) >= 0) and m.offs[0] == 0
    i = m.append(x, it, [20, 10], frame(0, 7))         # a negative size counts as 0: an empty cloud under its own frame
    assert list(i) == [1, 5, 6, OVERFLOW] and m.offs[6] == 258 and m.frames[5, 0] == 700.0
    i = m.append(x, it, [0, 0, 301, 301], np.stack([frame(0, 1), frame(301, 2), frame(0, 3)]))
    assert list(i) == [2, 6, 8, OVERFLOW | DROPPED] and not m.frames[7].any() and m.frames[6, 0] == 100.0
