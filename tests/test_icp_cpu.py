"""CPU-side checks of the ICP refinement (csrc/icp.hip, icp.cpp): the header declares its entry points and _lib.py binds them with matching
signatures, argument errors are PR_EINVAL before any device is touched; the restatement (icp_np.py) is self-consistent on the committed
cases - the order of its sums moves R and t by less than 1e-12, and every pass keeps the correspondences and the inlier sets decided by
a relative margin of at least 1e-9, which makes device and restatement provably choose the same ones; and the rule every combine of
partial minima follows (smaller d2, then smaller j) reproduces the sequential first minimum under any partition of the scan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_cases
import icp_np
from so_dso_place_recognition_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pr_icp_nn_dev", "pr_icp_pairs_dev", "pr_icp_nn", "pr_icp_pairs", "pr_icp_tile_rows", "pr_set_icp_path")


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
    for name in NEW:
        assert name in decls, name
        res, args = _lib.SYMBOLS[name]
        want = [] if decls[name][1].strip() == "void" else [_ctype(a) for a in decls[name][1].split(",")]
        got = [C.c_void_p if (a is C.c_void_p or hasattr(a, "contents")) else a for a in args]
        assert got == want, (name, got, want)
        assert res is _ctype(decls[name][0] + " x")
    names = re.findall(r"(\w+)\s*[,)]", decls["pr_icp_pairs_dev"][1] + ")")
    assert names[13:18] == ["max_iter", "max_corr", "tol_rmse", "tol_fitness", "min_inliers"] and names[-2:] == ["d_T_out", "d_stats"]
    hdr = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for word, value in (("CONVERGED", icp_np.CONVERGED), ("MAX_ITER", icp_np.MAX_ITER), ("TOO_FEW", icp_np.TOO_FEW),
                        ("DEGENERATE", icp_np.DEGENERATE), ("NO_PAIR", icp_np.NO_PAIR)):
        assert re.search(rf"#define PR_ICP_{word} {value}\b", hdr) and getattr(_lib, "ICP_" + word) == value
    assert icp_np.STATS_DTYPE.itemsize == 32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_argument_errors_are_einval_without_a_device():
    lib = _lib.load()
    assert lib.pr_icp_tile_rows() >= 64
    x = np.zeros((8, 3)); o = np.array([0, 4, 8], np.int64); ps = np.zeros(2, np.int32); T = np.zeros((2, 3, 4))
    oo = np.zeros(3, np.int64); ji = np.zeros(8, np.int32); dd = np.zeros(8); st = np.zeros(2, icp_np.STATS_DTYPE)

    def err(rc, word):
        assert rc == _lib.PR_EINVAL
        assert word in lib.pr_last_error(None).decode(), (word, lib.pr_last_error(None))

    def nn_dev(xq=x, oq=o, Nq=2, c=2, T_=T, ms=4, md=4, out=oo):
        return lib.pr_icp_nn_dev(None, _p(xq) if xq is not None else None, _p(oq) if oq is not None else None, Nq, _p(x), _p(o), 2, _p(ps), _p(ps), c,
                                 _p(T_) if T_ is not None else None, ms, md, _p(out) if out is not None else None, _p(ji), _p(dd))

    def nn_host(Nq=2, c=2, T_=T, oq=o):
        return lib.pr_icp_nn(None, _p(x), _p(oq) if oq is not None else None, Nq, _p(x), _p(o), 2, _p(ps), _p(ps), c,
                             _p(T_) if T_ is not None else None, _p(oo), _p(ji), _p(dd))

    def pairs(fn, dev, Nq=2, c=2, T0=T, max_iter=5, max_corr=1.0, min_inliers=3, ms=4, stats=st):
        bounds = (ms, 4) if dev else ()
        return fn(None, _p(x), _p(o), Nq, _p(x), _p(o), 2, _p(ps), _p(ps), c, _p(T0) if T0 is not None else None, *bounds, max_iter, max_corr,
                  1e-6, 1e-6, min_inliers, _p(T), _p(stats) if stats is not None else None)

    for kw in (dict(Nq=-1), dict(c=-1), dict(ms=-1), dict(md=-3)):
        err(nn_dev(**kw), "negative")
    for kw in (dict(xq=None), dict(oq=None), dict(T_=None), dict(out=None)):
        err(nn_dev(**kw), "NULL")
    err(nn_dev(), "ctx")
    err(nn_host(Nq=-1), "negative"); err(nn_host(c=-2), "negative"); err(nn_host(T_=None), "NULL"); err(nn_host(oq=None), "NULL")
    err(nn_host(), "ctx")
    for fn, dev in ((lib.pr_icp_pairs_dev, True), (lib.pr_icp_pairs, False)):
        err(pairs(fn, dev, Nq=-1), "negative"); err(pairs(fn, dev, c=-1), "negative")
        err(pairs(fn, dev, T0=None), "NULL"); err(pairs(fn, dev, stats=None), "NULL")
        err(pairs(fn, dev, max_iter=-1), "max_iter")
        for bad in (0.0, -1.0, np.inf, np.nan):
            err(pairs(fn, dev, max_corr=bad), "max_corr")
        err(pairs(fn, dev, min_inliers=2), "min_inliers")
        err(pairs(fn, dev), "ctx")
    err(pairs(lib.pr_icp_pairs_dev, True, ms=-1), "negative")
    assert lib.pr_set_icp_path(None, 0) == _lib.PR_EINVAL


@pytest.mark.parametrize("name", list(icp_cases.CASES))
def test_restatement_is_self_consistent_and_its_choices_have_margins(name):
    c, ref = icp_cases.case(name), icp_cases.reference(name)
    assert ref["status"] == icp_np.CONVERGED and 2 <= ref["iters"] < icp_cases.PARAMS["max_iter"]
    assert len(ref["nn_margin"]) == ref["iters"] + 1                      # every pass, the final one included
    print(name, len(c["P"]), len(c["Q"]), "iters", ref["iters"], "nn margin %.2e corr margin %.2e stop margin %.2e"
          % (min(ref["nn_margin"]), min(ref["corr_margin"]), ref["stop_margin"]))
    assert min(ref["nn_margin"]) >= 1e-9 and min(ref["corr_margin"]) >= 1e-9
    assert ref["stop_margin"] >= 1e-6                                     # the convergence tests are not on their thresholds either
    for order in ("forward", "reversed"):
        other = icp_np.icp(c["P"], c["Q"], c["T0"], order=order, **icp_cases.PARAMS)
        dT = np.abs(other["T"] - ref["T"])
        print("  ", order, "max |dR| %.1e max |dt| %.1e" % (dT[:, :3].max(), dT[:, 3].max()))
        assert dT.max() < 1e-12
        assert (other["status"], other["iters"], other["n_inl"], other["fitness"]) == (ref["status"], ref["iters"], ref["n_inl"], ref["fitness"])
        assert abs(other["rmse"] - ref["rmse"]) < 1e-12
    e0, e1 = icp_cases.pose_error(c["T0"], c["R"], c["t"]), icp_cases.pose_error(ref["T"], c["R"], c["t"])
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)                      # the refinement is closer to the planted motion than its seed


def test_restatement_status_paths():
    c = icp_cases.case("box300_hand")
    P, Q, T0 = c["P"], c["Q"], c["T0"]
    r = icp_np.icp(P, Q, T0, max_iter=0, max_corr=1.0)
    assert r["status"] == icp_np.MAX_ITER and r["iters"] == 0 and np.array_equal(r["T"], T0) and r["n_inl"] > 0
    r = icp_np.icp(P, Q, T0, max_iter=5, max_corr=1e-4)
    assert r["status"] == icp_np.TOO_FEW and r["iters"] == 0 and np.array_equal(r["T"], T0)
    r = icp_np.icp(P, Q, T0, max_iter=4, tol_rmse=0.0, tol_fitness=0.0)
    assert r["status"] == icp_np.MAX_ITER and r["iters"] == 4
    line = np.outer(np.arange(20.0), [1.0, 2.0, -1.0])
    r = icp_np.icp(line + [0.01, 0, 0], line, T0, max_iter=5)
    assert r["status"] == icp_np.DEGENERATE and r["iters"] == 0
    r = icp_np.icp(np.zeros((0, 3)), Q, T0, max_iter=5)
    assert r["status"] == icp_np.TOO_FEW and r["fitness"] == 0.0 and r["rmse"] == 0.0


def test_partition_combine_rule_is_the_sequential_first_minimum():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(0, 40))
        g = rng.integers(0, 3, (n, 3)).astype(np.float64)          # a tie-heavy integer grid: d2 of a point to its cells
        d = ((g[:, 0] * g[:, 0]) + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        d[rng.random(n) < 0.15] = np.nan
        d[rng.random(n) < 0.15] = np.inf
        if trial % 7 == 0:
            d[:] = rng.choice([np.nan, np.inf], n)                  # no candidate at all
        want = icp_np.sequential_first_min(d)
        for parts in (1, 2, 3, 7):
            cuts = np.sort(rng.integers(0, n + 1, parts - 1))
            bounds = [0, *cuts, n]
            partials = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                md, mj = icp_np.sequential_first_min(d[lo:hi])
                partials.append((md, mj + lo if mj >= 0 else -1))
            for order in (range(len(partials)), reversed(range(len(partials))), rng.permutation(len(partials))):
                acc = (np.inf, -1)
                for k in order:
                    acc = icp_np.combine(acc, partials[k])
                assert acc == want, (d, bounds, acc, want)
        if n:                                                       # and the vectorised form the GPU tests compare against
            j, v = icp_np.nn(np.zeros((1, 3)), g)
            dd = np.where(np.isnan(((g * g).sum(1))), np.inf, ((g[:, 0] * g[:, 0]) + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            assert (v[0], j[0]) == icp_np.sequential_first_min(dd)
