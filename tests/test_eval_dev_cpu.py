"""CPU-side checks of the device evaluation (csrc/eval.hip, eval_dev.cpp): the header declares its entry points and _lib.py binds them with
matching signatures, argument errors are PR_EINVAL before any device is touched, and the rule every combine of partial minima follows
(smaller d, then smaller j) reproduces the sequential first minimum of run_test.m:4-16 under any partition of the scan."""
import ctypes as C
import os
import re

import numpy as np

from so_dso_place_recognition_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pr_ground_truth_pairs_dev", "pr_precision_recall_dev", "pr_ground_truth_pairs", "pr_precision_recall_gpu")


def _declarations():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(2): (m.group(1).strip(), m.group(3)) for m in re.finditer(r"^([a-z0-9_ ]+?[ *])(pr_[a-z0-9_]+)\s*\(([^;]*?)\);", txt, flags=re.M | re.S)}


def _ctype(decl):
    decl = " ".join(decl.replace("const ", "").split())
    if "*" in decl:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int": C.c_int, "double": C.c_double}[decl.split()[0]]


def test_header_declares_the_functions_and_lib_binds_them():
    decls = _declarations()
    for name in NEW + ("pr_trapz_dev", "pr_eval_tile_rows", "pr_set_eval_path"):
        assert name in decls, name
        res, args = _lib.SYMBOLS[name]
        want = [] if decls[name][1].strip() == "void" else [_ctype(a) for a in decls[name][1].split(",")]
        got = [C.c_void_p if (a is C.c_void_p or hasattr(a, "contents")) else a for a in args]
        assert got == want, (name, got, want)
        assert res is _ctype(decls[name][0] + " x")
    assert [a for a in re.findall(r"(\w+)\s*[,)]", decls["pr_precision_recall_dev"][1] + ")")][:5] == ["ctx", "d_diff_v", "d_diff_idx", "ld", "m"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_argument_errors_are_einval_without_a_device():
    lib = _lib.load()
    assert lib.pr_eval_tile_rows() >= 64
    g = np.zeros((4, 3)); v = np.zeros(4); i = np.zeros(4, np.int32)
    a, t = C.c_double(), C.c_double()
    gt_forms = (lib.pr_ground_truth_pairs_dev, lib.pr_ground_truth_pairs)
    for fn in gt_forms:
        for m, n, cols, word in ((-1, 4, 3, "negative"), (4, -2, 3, "negative"), (4, 4, 0, "cols"), (4, 4, -3, "cols")):
            assert fn(None, _p(g), m, _p(g), n, cols, 1.0, 0, None, None, None, None) == _lib.PR_EINVAL
            assert word in lib.pr_last_error(None).decode()
        assert fn(None, None, 4, _p(g), 4, 3, 1.0, 0, None, None, None, None) == _lib.PR_EINVAL
        assert "NULL" in lib.pr_last_error(None).decode()
        assert fn(None, _p(g), 4, _p(g), 4, 3, 1.0, 0, None, None, None, None) == _lib.PR_EINVAL       # no context
        assert "ctx" in lib.pr_last_error(None).decode()
    sc = np.zeros(3)
    for m, n, cols, word in ((-1, 4, 3, "negative"), (4, -1, 3, "negative"), (4, 4, 0, "cols")):
        assert lib.pr_precision_recall_dev(None, _p(v), _p(i), 1, m, _p(g), _p(g), n, cols, 1.0, 0, _p(sc), None, None, None, None) == _lib.PR_EINVAL
        assert word in lib.pr_last_error(None).decode()
        assert lib.pr_precision_recall_gpu(None, _p(v), _p(i), m, _p(g), _p(g), n, cols, 1.0, 0, C.byref(a), C.byref(t), None, None, None, None,
                                           None, None) == _lib.PR_EINVAL
        assert word in lib.pr_last_error(None).decode()
    assert lib.pr_precision_recall_dev(None, _p(v), _p(i), 0, 4, _p(g), _p(g), 4, 3, 1.0, 0, _p(sc), None, None, None, None) == _lib.PR_EINVAL
    assert "ld" in lib.pr_last_error(None).decode()
    assert lib.pr_precision_recall_dev(None, _p(v), _p(i), 1, 4, _p(g), _p(g), 4, 3, 1.0, 0, None, None, None, None, None) == _lib.PR_EINVAL
    assert "NULL" in lib.pr_last_error(None).decode()
    assert lib.pr_precision_recall_gpu(None, None, _p(i), 4, _p(g), _p(g), 4, 3, 1.0, 0, C.byref(a), C.byref(t), None, None, None, None, None,
                                       None) == _lib.PR_EINVAL
    assert lib.pr_trapz_dev(None, _p(v), _p(v), -1, _p(sc)) == _lib.PR_EINVAL
    assert lib.pr_set_eval_path(None, 0, 0) == _lib.PR_EINVAL


def _sequential(d):
    """run_test.m:5-16: strict `min_diff > diff` from (+Inf, -1)."""
    md, mj = np.inf, -1
    for j, x in enumerate(d):
        if md > x:
            md, mj = x, j
    return md, mj


def _combine(a, b):
    """What every combine of two partial results does: the smaller d, on equal d the smaller j; (+Inf, -1) is "no candidate"."""
    if b[1] >= 0 and (b[0] < a[0] or (b[0] == a[0] and b[1] < a[1])):
        return b
    return a


def test_partition_combine_rule_is_the_sequential_first_minimum():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(0, 40))
        d = rng.integers(0, 4, n).astype(np.float64)                # tie-heavy
        d[rng.random(n) < 0.15] = np.nan
        d[rng.random(n) < 0.15] = np.inf
        if trial % 7 == 0:
            d[:] = rng.choice([np.nan, np.inf], n)                  # no candidate at all
        want = _sequential(d)
        for parts in (1, 2, 3, 7):
            cuts = np.sort(rng.integers(0, n + 1, parts - 1))
            bounds = [0, *cuts, n]
            partials = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                md, mj = _sequential(d[lo:hi])
                partials.append((md, mj + lo if mj >= 0 else -1))
            for order in (range(len(partials)), reversed(range(len(partials))), rng.permutation(len(partials))):
                acc = (np.inf, -1)
                for k in order:
                    acc = _combine(acc, partials[k])
                assert acc == want, (d, bounds, acc, want)
