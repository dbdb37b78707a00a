"""The plane-metric map localiser (pr_mapplane) without a device: the ABI surface and the header's rule text, the scratch
formula, the argument errors returned before any device is touched, what the Python class refuses before it calls the library, and the
restatement the GPU tests compare the kernels with (mapplane_np.py): its normals against an mpmath eigenvector, its solve against an
mpmath solve, its Jacobian against central differences, the margins of the committed cases, and the committed scene - point-to-plane
ends at no more than half the point form's translation error."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import icp_np
import maploc_np as mnp
import mapplane_np as pnp
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_mapplane_create", "pr_mapplane_destroy", "pr_mapplane_scratch_bytes", "pr_mapplane_normals_dev", "pr_mapplane_refine_dev",
         "pr_mapplane_normals", "pr_mapplane_refine")
EPS = float(np.finfo(np.float64).eps)
# 4 x the largest ratio angle / (eps l2 / (l1 - l0)) the restatement shows against mpmath over the committed cases (0.976, the jittered
# plane) and 4 x the largest ratio error / (eps cond(A)) of its solve (0.0337): measured here, recorded in DESIGN.md 4.22; the GPU test
# holds the device to the same bounds
C_ANGLE = 4.0
C_SOLVE = 0.14


def angle_bound(l0, l1, l2):
    return C_ANGLE * EPS * l2 / (l1 - l0) + 1e-13


def test_mapplane_symbols_rule_text_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_mapplane_")) == sorted(NAMES)
    assert "typedef struct pr_mapplane pr_mapplane;" in code
    assert re.search(r"pr_mapplane_create\(pr_ctx\* ctx, pr_maploc\* ml, pr_mapplane\*\* out\)", code)
    for m in ("normals_torch", "refine_torch", "localize_torch", "normals", "refine", "close"):
        assert hasattr(api.PlaneLocalizer, m), m
    for words in ("pr_mapplane", "DESIGN.md 4.22", "d2 = ((dx dx) + dy dy) + dz dz < fl(radius^2)", "d = q - x_j", "C_ab = S_ab - (s_a s_b) / k",
                  "8 sweeps, pivots (0,1), (0,2), (1,2)", "skipped when C_pq is exactly 0", "the lower index first on ties",
                  "l1 > 0 and l0 <= max_ratio l1", "ninfo = -k", "u = p' - t", "r = (n_0 e_0 + n_1 e_1) + n_2 e_2", "J = [u x n, n]",
                  "L D L^T without pivoting", "d_k <= 1e-12 A_kk", "below th2 = 1e-4", "radius (1 + 2^-10) > cell", "min_inliers < 6",
                  "240 pc nchunks"):
        assert words in txt, words
    hip = open(os.path.join(CSRC, "mapplane.hip")).read()
    assert "step < Tn" in hip and "0x9E3779B97F4A7C15ull" in hip and '#include "icp_common.hpp"' in hip
    assert "row >= (u64)v.ocap" in hip and "bj < A.max_dst" in hip                  # rows are bounded before an address is formed
    assert "atomic" not in re.sub(r"//[^\n]*", "", hip) and "while" not in re.sub(r"//[^\n]*", "", hip)
    assert "MP_SWEEPS = %d" % pnp.SWEEPS in hip and "th2 < 1e-4" in hip and pnp.SERIES_BELOW == 1e-4
    assert "MAPPLANE_SUMS = %d" % pnp.SUMS in open(os.path.join(CSRC, "kernels.hpp")).read()
    cpp = open(os.path.join(CSRC, "mapplane.cpp")).read()
    assert "radius * pr::MAPLOC_SLACK > mp->v->cell" in cpp and "max_corr * pr::MAPLOC_SLACK > mp->v->cell" in cpp
    assert cpp.count("launch_maploc_probe(") == 1                                  # the pass's search is the localiser's own launch
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"mapplane\.o: mapplane\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "-ffp-contract=off" in mk


def test_mapplane_scratch_size_formula():
    lib = _lib.load()
    for pc, ms in ((8, 513), (5, 257), (1, 0), (64, 4096), (3, 1), (65535, 256), (2, 255), (6, 512)):
        want = pnp.scratch_bytes(pc, ms)
        assert want > 0 and want % 16 == 0 and lib.pr_mapplane_scratch_bytes(pc, ms) == want, (pc, ms)
    for bad in ((0, 1), (65536, 1), (1, -1), (1, (1 << 26) + 1)):
        assert lib.pr_mapplane_scratch_bytes(*bad) == 0 and pnp.scratch_bytes(*bad) == 0, bad


def test_mapplane_argument_errors_before_any_device():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    err = lambda: lib.pr_last_error(None)
    h = C.c_void_p(1)
    assert lib.pr_mapplane_create(None, buf, None) == _lib.PR_EINVAL and b"out is NULL" in err()
    assert lib.pr_mapplane_create(None, None, C.byref(h)) == _lib.PR_EINVAL and b"localiser is NULL" in err() and not h.value
    assert lib.pr_mapplane_create(None, buf, C.byref(h)) == _lib.PR_EINVAL and b"ctx is NULL" in err()
    lib.pr_mapplane_destroy(None)                      # a no-op
    for name in ("pr_mapplane_normals_dev", "pr_mapplane_normals"):
        f, who = getattr(lib, name), name.encode()
        assert f(None, 0.4, 5, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": plane localiser is NULL" in err()
        for r in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert f(None, r, 5, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": radius=" in err(), r
        for mn in (2, 0, -1, 28):
            assert f(None, 0.4, mn, 0.1, buf, buf) == _lib.PR_EINVAL and who + b": min_nbrs=%d outside 3 .. 27" % mn in err()
        for mr in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
            assert f(None, 0.4, 5, mr, buf, buf) == _lib.PR_EINVAL and who + b": max_ratio=" in err(), mr
        assert f(None, 0.4, 3, 1.0, buf, buf) == _lib.PR_EINVAL and b"plane localiser is NULL" in err()      # 3, 27 and 1.0 are inside
        assert f(None, 0.4, 27, 1.0, None, buf) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
        assert f(None, 0.4, 27, 1.0, buf, None) == _lib.PR_EINVAL and b"a required pointer is NULL" in err()
    for name in ("pr_mapplane_refine_dev", "pr_mapplane_refine"):
        f, who = getattr(lib, name), name.encode()
        call = lambda mc=0.5, it=5, tr=1e-6, tf=1e-6, mi=6: f(None, buf, buf, 1, buf, 1, buf, None, it, mc, tr, tf, mi, buf, buf, buf, buf)
        assert call() == _lib.PR_EINVAL and who + b": plane localiser is NULL" in err()
        for mc in (0.0, -1.0, float("nan"), float("inf")):
            assert call(mc=mc) == _lib.PR_EINVAL and who + b": max_corr=" in err(), mc
        assert call(it=-1) == _lib.PR_EINVAL and who + b": max_iter=-1 < 0" in err()
        for mi in (5, 3, 0):
            assert call(mi=mi) == _lib.PR_EINVAL and who + b": min_inliers=%d < 6" % mi in err()
        assert call(tr=float("nan")) == _lib.PR_EINVAL and b"is NaN" in err()
        assert call(tf=float("nan")) == _lib.PR_EINVAL and b"is NaN" in err()


def test_plane_localizer_refuses_before_the_library():
    import torch

    class Fake:
        pass
    ml = Fake(); ml.ctx = object()
    with pytest.raises(ValueError, match="share one context"):
        api.PlaneLocalizer(object(), ml)               # a localiser of another context: refused before any handle exists
    wm = Fake(); wm.state, wm.out_capacity = torch.zeros(4, dtype=torch.int32), 16
    pl = api.PlaneLocalizer.__new__(api.PlaneLocalizer)
    pl.ctx, pl.ml, pl.wm, pl.h, pl.pair_capacity, pl.max_src_pts = ml.ctx, ml, wm, None, 4, 16
    x, o, ps, T = torch.zeros((8, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 3, 4), dtype=torch.float64)
    n, i = torch.zeros((16, 3), dtype=torch.float64), torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError, match="normals must be a contiguous CUDA tensor"):
        pl.normals_torch(0.4, out=(n, i))              # not on the device
    with pytest.raises(ValueError, match="xyz_q must be a contiguous CUDA tensor"):
        pl.refine_torch(x, o, ps, T, n, i)
    with pytest.raises(ValueError, match="CSR set"):
        pl.refine(np.zeros((8, 3)), [0, 4], [0], np.zeros((1, 3, 4)), n.numpy(), i.numpy())
    with pytest.raises(ValueError, match=r"T must be \[c, 3, 4\]"):
        pl.refine(np.zeros((8, 3)), [0, 8], [0, 0], np.zeros((1, 3, 4)), n.numpy(), i.numpy())
    with pytest.raises(ValueError, match=r"normals must be \[out_capacity, 3\]"):
        pl.refine(np.zeros((8, 3)), [0, 8], [0], np.zeros((1, 3, 4)), np.zeros((15, 3)), i.numpy())


# ------------------------------------------------------------------------------------------------ the restatement
def _mp_eigen(kept):
    """(eigenvalues ascending, eigenvector of the smallest) of the exact covariance of the kept offsets, 60 digits"""
    k = len(kept)
    d = [[mp.mpf(v) for v in dd] for _, dd, _ in kept]
    s = [sum(x[a] for x in d) for a in range(3)]
    Cm = mp.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            Cm[a, b] = sum(x[a] * x[b] for x in d) - s[a] * s[b] / k
    E, Q = mp.eigsy(Cm)
    order = sorted(range(3), key=lambda i: E[i])
    return [E[i] for i in order], [Q[a, order[0]] for a in range(3)]


def mp_angle(n, kept):
    """(angle between n and the mpmath eigenvector of l0, its bound)"""
    L, v = _mp_eigen(kept)
    nn = [mp.mpf(float(x)) for x in n]
    cr = [nn[1] * v[2] - nn[2] * v[1], nn[2] * v[0] - nn[0] * v[2], nn[0] * v[1] - nn[1] * v[0]]
    ang = float(mp.asin(min(mp.sqrt(sum(c * c for c in cr)) / (mp.sqrt(sum(x * x for x in v)) * mp.sqrt(sum(x * x for x in nn))), 1)))
    return ang, angle_bound(float(L[0]), float(L[1]), float(L[2]))


def all_cases():
    cases = dict(pnp.normal_cases())
    sc = pnp.corner_scene()
    cases["the scene"] = (sc["xyz"], sc["cell"], pnp.SCENE_NORMALS["radius"], pnp.SCENE_NORMALS["min_nbrs"], pnp.SCENE_NORMALS["max_ratio"])
    return cases


def test_normals_against_an_mpmath_eigenvector_and_the_margins_of_the_committed_cases():
    mp.mp.dps = 60
    worst, seen_valid = 0.0, 0
    for name, (xyz, cell, radius, mn, mr) in all_cases().items():
        assert radius * mnp.SLACK <= cell, name
        ix = mnp.index(xyz, len(xyz), cell)
        for j in ix["rows"]:
            info, n, det = pnp.row_normal(ix, xyz, int(j), radius, mn, mr, detail=True)
            l0, l1, l2 = det["l"]
            assert abs(info) == det["k"] >= 1 and (info > 0) == det["valid"]
            if l1 > 0:                                                            # no decision within 1e-6 relative of its threshold
                assert abs(l0 - mr * l1) > 1e-6 * mr * l1, (name, j)
            if "exactly radius" not in name:
                assert all(abs(d2 - radius * radius) > 1e-6 * radius * radius for _, d2 in det["seen"]), (name, j)
            if info > 0:
                seen_valid += 1
                assert abs(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) - 1.0) <= 4 * EPS and max(n, key=abs) > 0
                ang, bound = mp_angle(n, pnp.row_neighbours(ix, xyz, int(j), radius)[0])
                assert ang <= bound, (name, j, ang, bound)
                worst = max(worst, ang / (bound - 1e-13) * C_ANGLE)
            else:
                assert n == (0.0, 0.0, 0.0)
    print("   largest angle / (eps l2 / (l1 - l0)) over %d valid rows: %.3g (C_ANGLE = %g)" % (seen_valid, worst, C_ANGLE))
    assert seen_valid > 200 and 4.0 * worst <= C_ANGLE * 1.05 and worst > 0.1      # the constant is 4 x what is measured here


def test_the_committed_normal_cases_show_what_they_are_named_for():
    cases = pnp.normal_cases()
    got = {}
    for name, (xyz, cell, radius, mn, mr) in cases.items():
        ix = mnp.index(xyz, len(xyz), cell)
        got[name] = (ix,) + pnp.normals(ix, xyz, radius, mn, mr)
    ix, nrm, info = got["jittered plane"]
    tilt = np.array([0.5, 0.6, 0.62]) / np.linalg.norm([0.5, 0.6, 0.62])
    assert (info > 0).sum() > 40 and (info < 0).sum() > 10 and (np.abs(nrm[info > 0] @ tilt) > 0.9).all()
    a, b = got["plane unshifted"], got["plane shifted by 5e6"]
    assert a[2].tolist() == b[2].tolist() and (a[2] > 0).sum() > 30 and a[1].tobytes() == b[1].tobytes()      # the offsets are the same bits
    ix, nrm, info = got["two planes meeting in an edge"]
    v = nrm[info > 0]
    assert ((np.abs(v[:, 2]) == 1.0).any() and (np.abs(v[:, 0]) == 1.0).any()) and (info < 0).any()
    ix, nrm, info = got["a line"]
    assert (info <= 0).all() and (info < -1).any() and not nrm.any()               # l1 = 0: invalid whatever k
    ix, nrm, info = got["an isolated row"]
    assert info[40] == -1 and not nrm[40].any()
    ix, nrm, info = got["k = min_nbrs - 1 and k = min_nbrs"]
    assert info[0] == -3 and info[7] == 4 and info[4] == 5
    ix, nrm, info = got["a neighbour at exactly radius and one ulp inside"]
    assert info[0] == 4 and cases["a neighbour at exactly radius and one ulp inside"][0][1][0] - 0.5 == 0.75      # rows 2, 3, 4 in; row 1 at the radius out
    ix, nrm, info = got["NaN and Inf rows"]
    assert info[3] == 0 and info[7] == 0 and (info[[0, 1, 2]] != 0).all()
    ix, nrm, info = got["three rows in one voxel"]
    assert info[60] == 0 and info[61] == 0 and info[4] != 0 and ix["flags"] & mnp.DUPLICATE
    ix, nrm, info = got["the first and last voxel of the range"]
    assert info[0] == 4 and info[5] == 4
    ix, nrm, info = got["-0.0 coordinates"]
    assert info[0] == -3 and info[1] == 0 and info[2] == 0                          # (0.9, 0.1, 0) and (0.1, 0.9, -0) share row 0's voxel
    ix, nrm, info = got["the colliding keys"]
    assert len(ix["rows"]) == 32 and (info != 0).all() and (np.abs(info[10:]) > 1).any()


def _refine_world():
    rc = pnp.refine_case()
    return rc, pnp.table(rc["normals"], rc["ninfo"])


def test_plane_update_against_an_mpmath_solve_and_the_tree():
    mp.mp.dps = 60
    rc, normal_of = _refine_world()
    worst = 0.0
    for s in (2, 3, 4, 5):
        P = rc["xq"][rc["oq"][s]:rc["oq"][s + 1]]
        sums, idx, d2 = pnp.plane_pass_sums(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][s], normal_of, 0.499)
        j2, e2 = mnp.nn(rc["ix"], rc["xyz"], rc["row"], icp_np.transform(rc["seeds"][s], P), 0.499)
        assert np.array_equal(idx, j2) and d2.tobytes() == e2.tobytes()            # the boxed scan is the voxel walk
        assert sums[0] == (idx >= 0).sum() and sums[2] == sum(rc["ninfo"][j] > 0 for j in idx[idx >= 0]) >= 6
        assert abs(sums[1] - d2[idx >= 0].sum()) <= 1e-12 * sums[1]
        A, b = pnp.system_of(sums)
        assert all(A[r][c] == A[c][r] for r in range(6) for c in range(6))
        x = pnp.ldl_solve(A, b)
        xm = mp.lu_solve(mp.matrix(A), -mp.matrix(b))
        err = float(max(abs(mp.mpf(x[i]) - xm[i]) for i in range(6)) / max(abs(xm[i]) for i in range(6)))
        cond = float(np.linalg.cond(np.array(A)))
        assert err <= C_SOLVE * EPS * cond, (s, err, cond)
        worst = max(worst, err / (EPS * cond))
    print("   largest solve error / (eps cond(A)): %.3g (C_SOLVE = %g)" % (worst, C_SOLVE))
    assert 4.0 * worst <= C_SOLVE * 1.05
    # a singular system (one plane alone), a NaN and too few plane correspondents
    P = rc["xq"][rc["oq"][6]:rc["oq"][7]]
    sums, _, _ = pnp.plane_pass_sums(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][6], normal_of, 0.499)
    assert sums[2] >= 6 and pnp.plane_update(sums, rc["seeds"][6], 6)[0] == icp_np.DEGENERATE
    bad = sums.copy(); bad[5] = np.nan
    assert pnp.plane_update(bad, rc["seeds"][6], 6)[0] == icp_np.DEGENERATE
    assert pnp.plane_update(sums, rc["seeds"][6], int(sums[2]) + 1)[0] == icp_np.TOO_FEW
    # Exp(w): the series meets the closed form at the threshold and both are rotations
    for th in (1e-9, 9.99e-3, 1.0001e-2, 0.3, 3.0):
        w = [th * 2.0 / 3.0, -th / 3.0, th * 2.0 / 3.0]
        E = np.array(pnp.exp_so3(w))
        assert np.abs(E @ E.T - np.eye(3)).max() <= 8 * EPS and abs(np.trace(E) - (1 + 2 * np.cos(th))) <= 8 * EPS


def test_the_jacobian_against_central_differences():
    rng = np.random.default_rng(5)
    for _ in range(20):
        w0 = rng.normal(0, 0.5, 3)
        T = np.hstack([np.array(pnp.exp_so3(list(w0))), rng.normal(0, 30.0, (3, 1))])
        s, n = rng.normal(0, 10.0, 3), rng.normal(0, 1.0, 3)
        n /= np.linalg.norm(n)
        q = icp_np.transform(T, s)[0] + rng.normal(0, 0.2, 3)
        J, r = pnp.point_terms(T, s, q, n)

        def res(xi):
            E = np.array(pnp.exp_so3(list(xi[:3])))
            Tn = np.hstack([E @ T[:, :3], (T[:, 3] + xi[3:])[:, None]])
            return float(n @ (icp_np.transform(Tn, s)[0] - q))

        assert abs(res(np.zeros(6)) - r) <= 1e-12
        h = 1e-6
        for a in range(6):
            e = np.zeros(6); e[a] = h
            assert abs((res(e) - res(-e)) / (2 * h) - J[a]) <= 1e-7 * max(1.0, abs(J[a])), (a, J[a])


def test_the_scene_point_to_plane_halves_the_point_forms_translation_error():
    """The committed scene: a floor and two walls at cell 0.5, a source of 810 points at other in-plane positions, a seed turned by 1
    degree and shifted by 0.15 m.  Measured: point-to-point ends 8.3e-2 m from the truth, point-to-plane 4e-16 m."""
    sc = pnp.corner_scene()
    xyz, row = sc["xyz"], sc["row"]
    assert 780 <= len(sc["src"]) <= 820 and abs(np.linalg.norm(sc["seed"][:, 3] - sc["truth"][:, 3]) - 0.15) < 1e-12
    ang = np.arccos((np.trace(sc["seed"][:, :3] @ sc["truth"][:, :3].T) - 1) / 2)
    assert abs(np.rad2deg(ang) - 1.0) < 1e-9
    ix = mnp.index(xyz, len(xyz), sc["cell"])
    assert ix["flags"] == 0 and len(ix["rows"]) == len(xyz)                        # one row per voxel
    nrm, info = pnp.normals(ix, xyz, **pnp.SCENE_NORMALS)
    kw = dict(max_iter=30, max_corr=0.499, tol_rmse=1e-9, tol_fitness=1e-9)
    plane = pnp.icp_plane(ix, xyz, row, sc["src"], sc["seed"], pnp.table(nrm, info), min_inliers=6, **kw)
    point = mnp.icp(ix, xyz, row, sc["src"], sc["seed"], min_inliers=3, **kw)
    ep, eq = (float(np.linalg.norm(r["T"][:, 3] - sc["truth"][:, 3])) for r in (plane, point))
    print("   translation error: point-to-plane %.3g m, point-to-point %.3g m" % (ep, eq))
    assert plane["status"] == point["status"] == icp_np.CONVERGED and ep <= 0.5 * eq and eq > 0.01


def test_the_refine_case_shows_what_the_device_test_asserts():
    rc, normal_of = _refine_world()
    kw = dict(max_iter=30, max_corr=0.499, tol_rmse=1e-9, tol_fitness=1e-9, min_inliers=6)
    want = [icp_np.TOO_FEW, icp_np.TOO_FEW, icp_np.CONVERGED, icp_np.CONVERGED, icp_np.CONVERGED, icp_np.CONVERGED, icp_np.DEGENERATE,
            icp_np.TOO_FEW, icp_np.TOO_FEW]
    for s, st in enumerate(want):
        P = rc["xq"][rc["oq"][s]:rc["oq"][s + 1]]
        assert len(P) == (pnp.REFINE_SIZES + (120, 40, 5))[s]
        r = pnp.icp_plane(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][s], normal_of, **kw)
        assert r["status"] == st, (s, r["status"])
        if st == icp_np.CONVERGED:
            assert np.linalg.norm(r["T"][:, 3] - rc["truth"][:, 3]) < 1e-9 and r["iters"] >= 3
        if s == 7:
            assert r["n_inl"] == 40 and r["n_plane"] == [0]                         # every correspondent's row has ninfo <= 0
        if s == 8:
            assert r["n_inl"] == 5 and r["n_plane"] == [5]                          # 5 plane correspondents against min_inliers 6
    P = rc["xq"][rc["oq"][5]:rc["oq"][6]]
    r = pnp.icp_plane(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][5], normal_of, **dict(kw, max_iter=2, tol_rmse=0.0, tol_fitness=0.0))
    assert r["status"] == icp_np.MAX_ITER and r["iters"] == 2
    a = pnp.icp_plane(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][5], normal_of, excl=(1, 1), **kw)
    b = pnp.icp_plane(rc["ix"], rc["xyz"], rc["row"], P, rc["seeds"][5], normal_of, **kw)
    assert a["status"] == icp_np.CONVERGED and a["n_plane"] != b["n_plane"]         # the window changes the correspondences
