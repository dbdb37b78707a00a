"""The ICP update on the device (csrc/icp.hip: icp_finish_kernel and the 17 sums that feed it) against the 60-digit Kabsch of icp_mp.py on
the cases of icp_update_cases.py: thin inlier sets down to s2 / s1 = 1e-10, the degeneracy rule's two sides, large and tiny motions,
equal singular values, reflections, clouds up to 1e4 m from the origin, and the reduction's chunk edges and masked lanes.  One step
(max_iter = 1, both tolerances 0) under every launch geometry (pr_set_icp_path) and, on the conditioning and reduction cases, under the
grid search: status, iters, n_inl and fitness equal to the restatement's, R orthonormal to 1e-14, and T within

    tol_R = 32 eps s1 / s2 + 1e-13,    tol_t = tol_R (1 + |mu_p'|) + 1e-12 (1 + |mu_q|) metres

of the reference's T1 (s1, s2 and the means are the reference's; test_icp_update_cpu.py shows the restatement within a tenth of this bound
and a port of the earlier H^T H arithmetic 5 to 1e5 times over it).  The sums are pivoted, so the 1e3 and 1e4 m cases hold the same bound.
Every comparison prints its error as a fraction of the bound before it asserts."""
import numpy as np
import pytest

import icp_cases
import icp_mp
import icp_np
import icp_update_cases as uc
from resident_fuzz_cases import bits_equal
from so_dso_place_recognition_amd import _lib, api

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)          # pr_set_icp_path: by shape | every workgroup scans the whole target | split target + combine
UPDATES = tuple(n for n in uc.CASES if uc.case(n)["expect"] == uc.UPDATE)
STOPS = tuple(n for n in uc.CASES if uc.case(n)["expect"] != uc.UPDATE)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def one_step(ctx, name, path=0, search=None, copies=1):
    c = uc.case(name)
    xq, oq = icp_cases.csr([c["P"]]); xd, od = icp_cases.csr([c["Q"]])
    z = np.zeros(copies, np.int32)
    ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
    try:
        T, st = api.icp_refine(xq, oq, xd, od, z, z, np.tile(c["T0"], (copies, 1, 1)), max_iter=1, max_corr=c["max_corr"], tol_rmse=0.0,
                               tol_fitness=0.0, min_inliers=c["min_inliers"], ctx=ctx, search=search)
    finally:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
    return T, st


def same_pairs(ctx, name):
    """api.icp_nn under T0 == icp_np.nn, bit for bit: the device's pairs are the reference's."""
    c, pr = uc.case(name), uc.pairs(name)
    xq, oq = icp_cases.csr([c["P"]]); xd, od = icp_cases.csr([c["Q"]])
    _, gi, gd = api.icp_nn(xq, oq, xd, od, [0], [0], c["T0"][None], ctx=ctx)
    assert np.array_equal(gi, pr["idx"]) and bits_equal(gd, pr["d2"])


def held(name, what, T, ref):
    R = T[:, :3]
    (eR, et), (tR, tt) = uc.error(T, ref), uc.bound(ref)
    print("   %s %s: s2/s1 %.2e  |dR| %.2e / %.2e  |dt| %.2e / %.2e m  = %.3g of the bound" % (name, what, ref["ratio"], eR, tR, et, tt, uc.over(T, ref)))
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14
    assert eR <= tR and et <= tt


@pytest.mark.parametrize("name", UPDATES)
def test_one_step_update_against_the_extended_precision_kabsch(ctx, name):
    ref, rs = uc.reference(name), uc.restatement(name)
    same_pairs(ctx, name)
    runs = [("path %d" % p, p, None) for p in PATHS]
    if name in uc.COND or name in uc.RED:
        runs.append(("grid", 0, "grid"))
    for what, path, search in runs:
        T, st = one_step(ctx, name, path, search)
        assert (st[0]["status"], st[0]["iters"], st[0]["n_inl"]) == (_lib.ICP_MAX_ITER, 1, rs["n_inl"]) and rs["status"] == icp_np.MAX_ITER
        assert st[0]["fitness"] == rs["fitness"]
        held(name, what, T[0], ref)


@pytest.mark.parametrize("name", STOPS)
def test_degenerate_and_too_few_leave_the_seed_untouched(ctx, name):
    c, rs = uc.case(name), uc.restatement(name)
    same_pairs(ctx, name)
    want = _lib.ICP_DEGENERATE if c["expect"] == uc.DEGENERATE else _lib.ICP_TOO_FEW
    assert rs["status"] == want
    for path in PATHS:
        T, st = one_step(ctx, name, path)
        assert (st[0]["status"], st[0]["iters"]) == (want, 0), (path, st[0])
        assert bits_equal(T[0], c["T0"])
        assert st[0]["n_inl"] == rs["n_inl"] and st[0]["fitness"] == rs["fitness"]


@pytest.mark.parametrize("name", list(uc.FULL))
def test_full_refinement_of_a_thin_cloud_reaches_the_exact_motion(ctx, name):
    """Q is an exact rigid motion of P: the refinement ends on it, rmse <= 1e-12, with the restatement's status, iters and n_inl, and T
    within the bound (s1, s2 and the means of the last pass's pairs) of the restatement's T."""
    c = uc.case(name)
    rs = icp_np.icp(c["P"], c["Q"], c["T0"], **icp_cases.PARAMS)
    assert rs["status"] == icp_np.CONVERGED and rs["rmse"] <= 1e-12
    Pt = icp_np.transform(rs["T"], c["P"])
    idx, d2 = icp_np.nn(Pt, c["Q"])
    inl = d2 < icp_cases.MAX_CORR ** 2
    ref = icp_mp.kabsch_update(Pt[inl], c["Q"][idx[inl]], rs["T"])
    ref["T"] = rs["T"]                                            # the bound of the last pass, about the restatement's T
    xq, oq = icp_cases.csr([c["P"]]); xd, od = icp_cases.csr([c["Q"]])
    for path in PATHS:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
        try:
            T, st = api.icp_refine(xq, oq, xd, od, [0], [0], c["T0"][None], ctx=ctx, **icp_cases.PARAMS)
        finally:
            ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
        print("   %s path %d: status %d iters %d n_inl %d rmse %.3e (restatement %.3e)" % (name, path, st[0]["status"], st[0]["iters"], st[0]["n_inl"],
                                                                                      st[0]["rmse"], rs["rmse"]))
        assert (st[0]["status"], st[0]["iters"], st[0]["n_inl"]) == (rs["status"], rs["iters"], rs["n_inl"])
        held(name, "path %d" % path, T[0], ref)
        assert st[0]["rmse"] <= 1e-12


def test_many_pairs_update_in_the_four_points_per_lane_kernel(ctx):
    """4100 pairs of one 1025-point cloud pair: more than 4096 workgroups at one point per lane, so the kernel with four points per lane
    (chunks of 1024 points: one full chunk and a chunk of one point) forms the sums.  All results are the same bytes and hold the bound."""
    c = 4100
    ref, rs = uc.reference(uc.MANY), uc.restatement(uc.MANY)
    T, st = one_step(ctx, uc.MANY, copies=c)
    assert bits_equal(T, np.tile(T[0], (c, 1, 1))) and st.tobytes() == st[:1].tobytes() * c
    assert (st[0]["status"], st[0]["iters"], st[0]["n_inl"]) == (_lib.ICP_MAX_ITER, 1, rs["n_inl"]) and st[0]["fitness"] == rs["fitness"]
    held(uc.MANY, "x %d" % c, T[0], ref)
