"""The registration information (pr_reginfo, pr_posegraphw_add) without a device: the ABI surface and the header's
rule text, the scratch formula, the argument errors returned before any device is touched, what the Python classes refuse before they
call the library, and the restatement the GPU tests compare the kernels with (reginfo_np.py): its closed-form point H against the explicit
sum of J^T J, its marginal covariances against the Schur complements of H in mpmath, the margins of the committed cases and the weighted
add rule slot by slot."""
import ctypes as C
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

import posegraph_np as pg
import reginfo_np as rn
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_reginfo_create", "pr_reginfo_destroy", "pr_reginfo_scratch_bytes", "pr_reginfo_point_dev", "pr_reginfo_plane_dev", "pr_reginfo_point",
         "pr_reginfo_plane")
ADD = ("pr_posegraphw_add_dev", "pr_posegraphw_add")
MARGIN = 1e3                                     # no decision within this factor of min_ratio or of the pivot test, on either side


@pytest.fixture(scope="module")
def cases():
    pc, pl = rn.point_case(), rn.plane_case()
    return dict(point=(pc, rn.run_point_case(pc, detail=True)), plane=(pl, rn.run_plane_case(pl, detail=True)))


def test_symbols_rule_text_and_classes():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES + ADD:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_reginfo_")) == sorted(NAMES)
    assert "typedef struct pr_reginfo pr_reginfo;" in code
    for m in ("point_torch", "plane_torch", "pairs_torch", "maploc_torch", "point", "plane", "close"):
        assert hasattr(api.RegistrationInfo, m), m
    assert hasattr(api.PoseGraph, "add_weighted_torch") and hasattr(api.PoseGraph, "add_weighted")
    assert api.RegInfo._fields == ("H", "cov", "spec", "w", "stat", "ok")
    for words in ("pr_reginfo", "DESIGN.md 4.25", "nn_d2 < fl(max_corr^2)", "u = p' - t", "J = [-[u]x | I]", "H_ww = (tr S) I - S", "H_wv = [sum u]x",
                  "H_vv = n I", "dof = 3 n - 6", "dof = n_pl - 6", "J = [u x n, n]", "r = (n_0 e_0 + n_1 e_1) + n_2 e_2", "64-lane shuffle tree",
                  "chunk index order", "PR_REGINFO_OFF when", "PR_REGINFO_NONFINITE when", "PR_REGINFO_TOO_FEW when", "L D L^T of H without pivoting",
                  "not d_k > 1e-12 H_kk", "by six solves", "no Schur complement is formed", "8 sweeps, pivots (0,1), (0,2), (1,2)",
                  "the component of largest magnitude is positive", "NOT cr0 >= min_ratio cr2", "s2 = max(SSE / dof, sigma_min^2)",
                  "exactly 0.0 when any flag is set", "-R^T w and -R^T v", "200 pc nchunks", "checked before an address is formed",
                  "both of its weights are finite and >= 0", "{n_inl, n_used,"):
        assert words in txt, words
    for name, bit in (("OFF", 1), ("NONFINITE", 2), ("TOO_FEW", 4), ("SINGULAR", 8), ("WEAK_ROT", 16), ("WEAK_TRANS", 32)):
        assert re.search(r"PR_REGINFO_%s = %d\b" % (name, bit), code) and getattr(_lib, "REGINFO_" + name) == bit == getattr(rn, name)
    hip = open(os.path.join(CSRC, "reginfo.hip")).read()
    body = re.sub(r"//[^\n]*", "", hip)
    assert "atomic" not in body and "while" not in body and "bj < in.ocap" in hip and '#include "mapplane_normal.hpp"' in hip
    assert "jacobi_rotate(A, V, 0, 1, 2)" in hip and "MP_SWEEPS" in hip and "1e-12 * H[k][k]" in hip
    hpp = open(os.path.join(CSRC, "reginfo.hpp")).read()
    assert "REGINFO_POINT_SUMS = %d" % rn.POINT_SUMS in hpp and "REGINFO_PLANE_SUMS = %d" % rn.PLANE_SUMS in hpp and "REGINFO_NS = %d" % rn.NS in hpp
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"reginfo\.o: reginfo\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "reginfo_host.o" in mk
    pgh = open(os.path.join(CSRC, "posegraph.hip")).read()
    assert pgh.count("__global__") == 7 and "posegraph_add_weighted_kernel" in pgh           # a second add kernel beside the first


def test_scratch_size_formula():
    lib = _lib.load()
    for pc, ms in ((8, 513), (5, 257), (1, 0), (64, 4096), (3, 1), (65535, 256), (2, 255), (6, 512)):
        want = rn.scratch_bytes(pc, ms)
        assert want > 0 and want % 16 == 0 and lib.pr_reginfo_scratch_bytes(pc, ms) == want, (pc, ms)
    for bad in ((0, 1), (65536, 1), (1, -1), (1, (1 << 26) + 1)):
        assert lib.pr_reginfo_scratch_bytes(*bad) == 0 and rn.scratch_bytes(*bad) == 0, bad


def test_argument_errors_before_any_device():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    err = lambda: lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_reginfo_create(None, 4, 16, None) == _lib.PR_EINVAL and b"out is NULL" in err()
    assert lib.pr_reginfo_create(None, 0, 16, C.byref(h)) == _lib.PR_EINVAL and b"pair_capacity=0" in err() and not h.value
    assert lib.pr_reginfo_create(None, 65536, 16, C.byref(h)) == _lib.PR_EINVAL and b"pair_capacity=65536" in err()
    assert lib.pr_reginfo_create(None, 4, -1, C.byref(h)) == _lib.PR_EINVAL and b"max_src_pts=-1" in err()
    assert lib.pr_reginfo_create(None, 4, (1 << 26) + 1, C.byref(h)) == _lib.PR_EINVAL and b"max_src_pts=" in err()
    assert lib.pr_reginfo_create(None, 4, 16, C.byref(h)) == _lib.PR_EINVAL and b"ctx is NULL" in err()
    lib.pr_reginfo_destroy(None)                      # a no-op
    inf, nan = float("inf"), float("nan")
    for name in ("pr_reginfo_point_dev", "pr_reginfo_point", "pr_reginfo_plane_dev", "pr_reginfo_plane"):
        f, who, plane = getattr(lib, name), name.encode(), "plane" in name
        floor = 6 if plane else 3

        def call(mc=0.5, mi=10, mr=1e-3, sm=0.01, wm=1e6, Nq=1):
            extra = (buf, 16, buf, buf) if plane else ()
            return f(None, buf, buf, Nq, buf, 1, buf, None, buf, buf, buf, *extra, mc, mi, mr, sm, wm, buf, buf, buf, buf, buf, buf)
        assert call() == _lib.PR_EINVAL and who + b": handle is NULL" in err()
        for mc in (0.0, -1.0, nan, inf):
            assert call(mc=mc) == _lib.PR_EINVAL and who + b": max_corr=" in err(), mc
        for sm in (0.0, -1.0, nan, inf):
            assert call(sm=sm) == _lib.PR_EINVAL and who + b": sigma_min=" in err(), sm
        for mr in (-1e-9, 1.0000001, nan, inf):
            assert call(mr=mr) == _lib.PR_EINVAL and who + b": min_ratio=" in err(), mr
        for wm in (0.0, -1.0, nan):
            assert call(wm=wm) == _lib.PR_EINVAL and who + b": w_max=" in err(), wm
        for mi in (floor - 1, 0, -1):
            assert call(mi=mi) == _lib.PR_EINVAL and who + (b": min_inliers=%d < %d" % (mi, floor)) in err()
        assert call(Nq=-1) == _lib.PR_EINVAL and b"Nq=-1" in err()
        assert call(mr=0.0, wm=inf, mi=floor) == _lib.PR_EINVAL and b"handle is NULL" in err()        # 0, 1, +Inf and the floor are inside
        assert call(mr=1.0) == _lib.PR_EINVAL and b"handle is NULL" in err()
    ibuf = (C.c_int32 * 64)()
    for name in ADD:
        f, who = getattr(lib, name), name.encode()
        row = ibuf if name.endswith("_dev") else 3
        for k in (0, -1, 129):
            assert f(None, ibuf, buf, ibuf, row, k, buf, ibuf) == _lib.PR_EINVAL and who + b": k=%d outside 1 .. 128" % k in err()
        assert f(None, ibuf, buf, ibuf, row, 5, buf, ibuf) == _lib.PR_EINVAL and who + b": graph is NULL" in err()


def test_the_classes_refuse_before_the_library():
    import torch

    class Fake:
        pass
    ri = api.RegistrationInfo.__new__(api.RegistrationInfo)
    ri.ctx = Fake(); ri.ctx.device = 0
    ri.h, ri.pair_capacity, ri.max_src_pts, ri._work = None, 2, 16, {}
    x, o, ps, T = torch.zeros((8, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 3, 4), dtype=torch.float64)
    nn = (torch.zeros(2, dtype=torch.int64), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="xyz_q must be a contiguous CUDA tensor"):
        ri.point_torch(x, o, ps, T, nn)                # not on the device
    with pytest.raises(ValueError, match="xyz_q must be a contiguous CUDA tensor"):
        ri.plane_torch(x, o, ps, T, nn, x, x, ps)
    km = Fake(); km.ctx, km.clouds = object(), (x, o)
    with pytest.raises(ValueError, match="must live on this handle's context"):
        ri.pairs_torch((x, o), km, torch.zeros((1, 1), dtype=torch.int32), T, torch.ones((1, 1), dtype=torch.bool), 16, 16)
    with pytest.raises(ValueError, match="exceeds pair_capacity"):
        ri.pairs_torch((x, o), (x, o), torch.zeros((1, 3), dtype=torch.int32), T, torch.ones((1, 3), dtype=torch.bool), 16, 16)
    with pytest.raises(ValueError, match="exceeds the handle's"):
        ri.pairs_torch((x, o), (x, o), torch.zeros((1, 1), dtype=torch.int32), T, torch.ones((1, 1), dtype=torch.bool), 17, 16)
    pl = Fake(); pl.ctx, pl.ml = object(), Fake()
    with pytest.raises(ValueError, match="must live on this handle's context"):
        ri.maploc_torch(pl, x, o, ps, T, x, ps)
    with pytest.raises(ValueError, match="CSR set"):
        ri.point(np.zeros((8, 3)), [0, 4], [0], np.zeros((1, 3, 4)), ([0, 4], np.zeros(4, np.int32), np.zeros(4)))
    with pytest.raises(ValueError, match=r"T must be \[c, 3, 4\]"):
        ri.point(np.zeros((8, 3)), [0, 8], [0, 0], np.zeros((1, 3, 4)), ([0, 4, 8], np.zeros(8, np.int32), np.zeros(8)))
    with pytest.raises(ValueError, match="nn must be"):
        ri.point(np.zeros((8, 3)), [0, 8], [0], np.zeros((1, 3, 4)), ([0, 9], np.zeros(8, np.int32), np.zeros(8)))
    with pytest.raises(ValueError, match=r"normals must be \[out_capacity, 3\]"):
        ri.plane(np.zeros((8, 3)), [0, 8], [0], np.zeros((1, 3, 4)), ([0, 8], np.zeros(8, np.int32), np.zeros(8)), np.zeros((5, 3)), np.zeros((4, 3)),
                 np.zeros(5, np.int32))
    g = api.PoseGraph.__new__(api.PoseGraph)
    g.h = None
    with pytest.raises(ValueError, match="idx must be a contiguous CUDA tensor"):
        g.add_weighted_torch(torch.zeros(2, dtype=torch.int32), T, ps, ps, T)
    with pytest.raises(ValueError, match=r"w \[k, 2\]"):
        g.add_weighted([1, 2], np.zeros((2, 3, 4)), [1, 1], 5, np.zeros((3, 2)))


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_closed_form_point_H_is_the_explicit_sum_of_JtJ(cases):
    pc, res = cases["point"]
    seen = 0
    for p, name in enumerate(pc["names"]):
        if res["stat"][p, 3] & (rn.OFF | rn.NONFINITE):
            continue
        sp = rn.slot_points(pc["xq"], pc["oq"], pc["src"], pc["acc"], pc["nn"][0], p, pc["max_src_pts"])
        q0, o0, ns = sp
        H = np.zeros((6, 6)); A = np.zeros((6, 6))
        for i in range(ns):
            if not (pc["nn"][1][o0 + i] >= 0 and pc["nn"][2][o0 + i] < rn.POINT["max_corr"] ** 2):
                continue
            _, u = rn._u_of(pc["T"][p], pc["xq"][q0 + i])
            K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
            J = np.hstack([-K, np.eye(3)])
            H += J.T @ J
            A += np.abs(J).T @ np.abs(J)
        assert (np.abs(res["H"][p] - H) <= 4 * max(ns, 1) * 2.0 ** -53 * A + 1e-300).all(), name
        assert np.array_equal(res["H"][p], res["H"][p].T)
        seen += 1
    assert seen >= 15


def test_the_marginal_covariances_are_the_inverse_schur_complements(cases):
    mp.mp.dps = 50
    seen = 0
    for kind in ("point", "plane"):
        case, res = cases[kind]
        for p, name in enumerate(case["names"]):
            if res["stat"][p, 3] & ~(rn.WEAK_ROT | rn.WEAK_TRANS):
                continue
            H = mp.matrix(res["H"][p].tolist())
            S = mp.inverse(H)
            Hww, Hwv, Hvv = H[0:3, 0:3], H[0:3, 3:6], H[3:6, 3:6]
            for blk, schur in ((S[0:3, 0:3], Hww - Hwv * mp.inverse(Hvv) * Hwv.T), (S[3:6, 3:6], Hvv - Hwv.T * mp.inverse(Hww) * Hwv)):
                d = mp.inverse(blk) - schur
                assert max(abs(d[r, c]) for r in range(3) for c in range(3)) <= mp.mpf(10) ** -30 * max(abs(schur[r, r]) for r in range(3)), name
            # and the restatement's fp64 Sigma is that inverse to eps cond(H)
            cond = float(np.linalg.cond(res["H"][p]))
            err = max(abs(mp.mpf(float(res["cov"][p, r, c])) - S[r, c]) for r in range(6) for c in range(6)) / max(abs(S[r, r]) for r in range(6))
            assert float(err) <= 8 * 2.0 ** -52 * cond, (name, float(err), cond)
            seen += 1
    assert seen >= 20


def test_the_committed_cases_show_what_they_are_named_for(cases):
    pc, rp = cases["point"]
    pl, rl = cases["plane"]
    P = {n: i for i, n in enumerate(pc["names"])}
    L = {n: i for i, n in enumerate(pl["names"])}
    flag = lambda r, p: int(r["stat"][p, 3])
    for s in rn.SIZES:
        want = rn.OFF if s == 0 else (rn.TOO_FEW if s < 3 else 0)
        assert flag(rp, P["size %d" % s]) == want and rp["stat"][P["size %d" % s], 0] == s, s
    assert rp["stat"][P["size 2"]].tolist() == [2, 2, 0, rn.TOO_FEW] and rp["stat"][P["n = 2"]].tolist() == [2, 2, 0, rn.TOO_FEW]      # dof = 0
    assert rp["stat"][P["all outliers"]].tolist() == [0, 0, -6, rn.TOO_FEW]
    assert rp["stat"][P["a point at max_corr and one ulp inside"]].tolist() == [7, 7, 15, 0]
    assert flag(rp, P["a NaN in T"]) == flag(rp, P["a NaN / Inf source point"]) == rn.NONFINITE
    assert flag(rp, P["collinear on an integer grid"]) == rn.SINGULAR and rp["stat"][P["a span longer than max_src_pts"], 0] == pc["max_src_pts"]
    assert [flag(rp, P[n]) for n in ("pair_src -1", "pair_src Nq", "accepted 0")] == [rn.OFF] * 3
    box, idx, sse = P["the 60-point box"], P["nn_idx >= out_capacity"], P["SSE = 0"]
    assert flag(rp, box) == 0 and rp["stat"][box].tolist() == [60, 60, 174, 0] and rp["H"][idx].tobytes() == rp["H"][box].tobytes()
    assert rp["spec"][sse, 12] == 0.0 and rp["spec"][sse, 13] == rn.POINT["sigma_min"] ** 2 and (rp["w"][sse] < rn.POINT["w_max"]).all()
    capped = rn.run_point_case(pc, w_max=50.0)
    assert (capped["w"][capped["ok"]] == 50.0).all() and capped["ok"].sum() >= 10                  # w_max reached on every clean slot
    for p in range(len(pc["names"])):
        if flag(rp, p):
            assert not rp["w"][p].any() and not rp["cov"][p].any() and not rp["spec"][p, :12].any()
        if flag(rp, p) & (rn.OFF | rn.NONFINITE):
            assert not rp["H"][p].any()
    assert rl["stat"][L["n_pl = 6"]].tolist() == [6, 6, 0, rn.TOO_FEW]
    q = L["ninfo <= 0 on every correspondent"]
    assert rl["stat"][q].tolist() == [40, 0, -6, rn.TOO_FEW]
    assert flag(rl, L["one floor"]) == flag(rl, L["the exact corridor"]) == rn.SINGULAR
    j = L["the jittered corridor"]
    assert flag(rl, j) == rn.WEAK_TRANS and not rl["w"][j].any() and rl["cov"][j].any()              # weak: everything but the weights
    assert rl["spec"][j, 9] > 1.0 - 1e-8 and abs(rl["spec"][j, 10]) < 1e-3 and abs(rl["spec"][j, 11]) < 1e-3        # dir_t is the corridor axis
    assert flag(rl, L["the corner scene"]) == 0 and rl["stat"][L["the corner scene"], 0] == 810 and (rl["w"][L["the corner scene"]] > 0).all()
    for s in rn.SIZES:
        want = rn.OFF if s == 0 else (rn.TOO_FEW if s <= 3 else 0)
        assert flag(rl, L["scene, size %d" % s]) == want, s


def test_conditions_and_margins_of_the_committed_cases(cases):
    """every case whose cov / spec / w the GPU test compares has cond(H) <= 1e8, and no decision lies within a factor 1e3 of min_ratio or
    of the pivot test"""
    worst_cond, lo, hi = 0.0, math.inf, 0.0
    for kind, prm in (("point", rn.POINT), ("plane", rn.PLANE)):
        case, res = cases[kind]
        for p, name in enumerate(case["names"]):
            f = int(res["stat"][p, 3])
            if f & (rn.OFF | rn.NONFINITE | rn.TOO_FEW):
                continue
            H = res["H"][p].tolist()
            _, d, ok, _ = rn.ldl(H, detail=True)
            assert ok == (not f & rn.SINGULAR), name
            for k in range(6):                                     # d_k against 1e-12 H_kk: up to the first failed pivot
                if not math.isfinite(d[k]):
                    break
                if d[k] > rn.PIVOT * H[k][k]:
                    assert d[k] >= MARGIN * rn.PIVOT * H[k][k], (name, k, d[k], H[k][k])
                else:
                    assert d[k] <= rn.PIVOT * H[k][k] / MARGIN, (name, k, d[k], H[k][k])
                    break
            if f & rn.SINGULAR:
                continue
            cond = float(np.linalg.cond(res["H"][p]))
            worst_cond = max(worst_cond, cond)
            assert cond <= rn.COND_MAX, (name, cond)
            sp = res["spec"][p]
            for l0, l2, bit in ((sp[0], sp[2], rn.WEAK_ROT), (sp[3], sp[5], rn.WEAK_TRANS)):
                ratio = l0 / l2
                if f & bit:
                    assert 0 < ratio <= prm["min_ratio"] / MARGIN, (name, ratio)
                    hi = max(hi, ratio)
                else:
                    assert ratio >= MARGIN * prm["min_ratio"], (name, ratio)
                    lo = min(lo, ratio)
    print("   largest cond(H) %.3g; smallest passing ratio %.3g, largest failing ratio %.3g" % (worst_cond, lo, hi))
    assert worst_cond > 1e7 and hi > 0.0                            # the jittered corridor is among them


def test_the_measured_bound_is_far_below_the_quantities_it_guards(cases):
    """the two restatements (kernel order; reversed sums with the inverse and the eigen-decomposition in mpmath) agree to a small multiple
    of eps cond(H): what 100 x their difference bounds is rounding, not the rule"""
    for kind in ("point", "plane"):
        case, res = cases[kind]
        prm = rn.POINT if kind == "point" else rn.PLANE
        for p, name in enumerate(case["names"]):
            f = int(res["stat"][p, 3])
            if f & ~(rn.WEAK_ROT | rn.WEAK_TRANS) or res["sums"][p] is None:
                continue
            m = rn.finish_mp(kind == "plane", rn.reversed_sum(res["terms"][p]), prm["min_ratio"], prm["sigma_min"], prm["w_max"])
            assert m["flags"] == f, name
            cond = float(np.linalg.cond(res["H"][p]))
            for k in ("cov", "spec", "w"):
                a, b = res[k][p], m[k]
                if k == "spec":
                    a, b = np.delete(a, range(6, 12)), np.delete(b, range(6, 12))
                    for o in (0, 3):                                 # a direction moves by the rounding over its eigenvalue's relative gap
                        gap = (res["spec"][p, o + 2] - res["spec"][p, o + 1]) / res["spec"][p, o + 2]
                        assert np.abs(res["spec"][p, 6 + o:9 + o] - m["spec"][6 + o:9 + o]).max() <= 64 * 2.0 ** -52 * cond / gap, (name, "dir", o)
                assert np.abs(a - b).max() <= 64 * 2.0 ** -52 * cond * np.abs(a).max(), (name, k)


# ------------------------------------------------------------------------------------------------ the weighted add
def _slots(k, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(-1, 30, k).astype(np.int32)
    T = rng.normal(0.0, 1.0, (k, 12))
    acc = (rng.random(k) < 0.8).astype(np.uint8)
    w = np.abs(rng.normal(50.0, 20.0, (k, 2)))
    return idx, T, acc, w


def test_the_weighted_add_rule_slot_by_slot():
    idx, T, acc, w = _slots(12, 1)
    idx[:] = np.arange(12); acc[:] = 1
    idx[1] = -1; acc[2] = 0; idx[3] = 40; T[4, 5] = np.nan                 # the four conditions of add
    w[5, 0] = np.nan; w[6, 1] = -1e-300; w[7, 0] = np.inf; w[8] = (0.0, 0.0); w[9, 1] = -0.0        # and the fifth
    m = pg.PoseGraphModel(64)
    info = rn.add_weighted(m, idx, T, acc, 40, w)
    kept = [0, 8, 9, 10, 11]
    assert info.tolist() == [5, 0, 5, 0] and m.edge_ij[:5].tolist() == [[i, 40] for i in kept]
    assert m.edge_w[:5].tobytes() == w[kept].tobytes() and m.edge_Z[:5].tobytes() == T[kept].tobytes()
    assert rn.add_weighted(m, idx, T, acc, -1, w).tolist() == [0, -1, 5, 0] and m.state[0] == 5    # switched off
    # constant weights: posegraph_np's add, byte for byte; and the overflow rule
    for cap in (64, 7):
        a, b = pg.PoseGraphModel(cap), pg.PoseGraphModel(cap)
        for q in range(3):
            idx, T, acc, _ = _slots(5, 10 + q)
            ia = a.add(idx, T, acc, 31 + q, 100.0, 10.0)
            ib = rn.add_weighted(b, idx, T, acc, 31 + q, np.tile((100.0, 10.0), (5, 1)))
            assert ia.tolist() == ib.tolist()
        assert all(getattr(a, n).tobytes() == getattr(b, n).tobytes() for n in ("edge_ij", "edge_Z", "edge_w", "state"))
        assert (a.state[1] == pg.OVERFLOW) == (cap == 7)
    m = pg.PoseGraphModel(4); m.state[0] = 1 << 30                          # a scribbled count is clamped
    assert rn.add_weighted(m, [1], np.zeros((1, 12)), [1], 9, [[1.0, 1.0]]).tolist() == [0, -1, 4, pg.OVERFLOW]
