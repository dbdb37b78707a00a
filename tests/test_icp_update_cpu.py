"""The ICP update cases' own proof (icp_update_cases.py; no device).  For every case: the correspondences and the inlier set are decided
by relative margins of at least 1e-9 (device and restatement then provably use the same pairs); the singular-value ratio s2 / s1 of H and
the Kabsch sign d are what the case states, by the 60-digit reference icp_mp.py; and the restatement's one step (icp_np.py: centred H,
LAPACK SVD) is within ONE TENTH of the bound the GPU test holds the device to - the bound is attainable in fp64.

Two NumPy ports of the device's finish arithmetic run on the same sums (test code: no kernel text):

  port_squared   what icp_finish_kernel did before these tests: H = sum p' q^T - (sum p')(sum q)^T / n about the coordinate origin, H scaled
                 by its largest entry, cyclic Jacobi on H^T H (frames.hpp), u = H v / |H v|, Gram-Schmidt, cross products.  It is the
                 documented MUTANT: it must exceed the bound on every conditioning case with s2 / s1 <= 1e-4 - which shows, without a GPU,
                 that test_gpu_icp_update.py fails on this class of error (eps (s1 / s2)^2 where eps s1 / s2 is attainable).
  port_onesided  what it does now: the sums per chunk of 256 source points about the chunk's PIVOT (the correspondence of its first
                 inlier), moved to the first chunk's pivot and added; one-sided Jacobi on the scaled H itself.  It must hold the bound
                 on every case, the far ones (1e3 and 1e4 m) included: the sums are pivoted, so the same bound is asserted there."""
import numpy as np
import pytest

import icp_np
import icp_update_cases as uc

SUM = icp_np._sum


def _jacobi_eig3(a):
    """frames.hpp's cyclic Jacobi of a symmetric 3 x 3 (a is overwritten by the rotated matrix; returns the eigenvector columns)."""
    v = np.eye(3)
    for _ in range(64):
        off = a[0, 1] * a[0, 1] + a[0, 2] * a[0, 2] + a[1, 2] * a[1, 2]
        dia = a[0, 0] * a[0, 0] + a[1, 1] * a[1, 1] + a[2, 2] * a[2, 2]
        if off == 0.0 or off <= 1e-36 * dia:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p, q] == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                for m in (a, a.T, v):                                # columns of a, rows of a, columns of v
                    x, y = m[:, p].copy(), m[:, q].copy()
                    m[:, p] = cs * x - sn * y
                    m[:, q] = sn * x + cs * y
    return v


def _finish(u, v, n1, n2):
    """Both ports' common end: u[0], u[1] unnormalised left vectors, v[0], v[1] right vectors -> dR (None: degenerate)."""
    if not (n2 > 1e-12 * n1):
        return None
    u0 = u[0] / n1
    u1 = u[1] - (u[1] @ u0) * u0
    u1 = u1 / np.linalg.norm(u1)
    v2 = np.cross(v[0], v[1])
    v2 = v2 / np.linalg.norm(v2)
    return np.outer(v[0], u0) + np.outer(v[1], u1) + np.outer(v2, np.cross(u0, u1))


def _kabsch_squared(H):
    hmax = np.abs(H).max()
    if not (0.0 < hmax < np.inf):
        return None
    G = H / hmax
    A = G.T @ G
    V = _jacobi_eig3(A)
    o = np.argsort(-np.diag(A), kind="stable")
    v = [V[:, o[0]], V[:, o[1]]]
    u = [G @ v[0], G @ v[1]]
    return _finish(u, v, np.linalg.norm(u[0]), np.linalg.norm(u[1]))


def _kabsch_onesided(H):
    hmax = np.abs(H).max()
    if not (0.0 < hmax < np.inf):
        return None
    G = H / hmax
    V = np.eye(3)
    rotate, sweep = True, 0
    while True:
        W = G @ V
        if not rotate or sweep == 12:
            break
        big = 0.0
        for p in range(2):
            for q in range(p + 1, 3):
                al, be, ga = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
                if not (ga * ga > 1e-31 * (al * be)):
                    continue
                zeta = (be - al) / (2.0 * ga)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                for m in (W, V):
                    x, y = m[:, p].copy(), m[:, q].copy()
                    m[:, p] = cs * x - sn * y
                    m[:, q] = sn * x + cs * y
                big = max(big, abs(t))
        rotate = big > 2.0 ** -50
        sweep += 1
    o = np.argsort(-(W * W).sum(0), kind="stable")
    u = [W[:, o[0]], W[:, o[1]]]
    v = [V[:, o[0]], V[:, o[1]]]
    return _finish(u, v, np.linalg.norm(u[0]), np.linalg.norm(u[1]))


CHUNK = 256                                                          # source points per chunk of the one-point-per-lane launches


def _chunked_sums(src, p, q):
    """The device's sums: per chunk of CHUNK source points (src: the inliers' source indices) about the chunk's pivot - the q of its first
    inlier -, then moved to the first chunk's pivot and added in chunk order.  Returns (pivot, n, Sp, Sq, Spq)."""
    piv, n, Sp, Sq, Spq = None, 0.0, np.zeros(3), np.zeros(3), np.zeros((3, 3))
    for k in np.unique(src // CHUNK):
        m = src // CHUNK == k
        ck = q[m][0]
        pc, qc, nk = p[m] - ck, q[m] - ck, float(m.sum())
        sp, sq, spq = SUM(pc, "pairwise"), SUM(qc, "pairwise"), SUM(pc[:, :, None] * qc[:, None, :], "pairwise")
        if piv is None:
            piv = ck
        d = ck - piv
        n += nk
        Sp = Sp + (sp + nk * d)
        Sq = Sq + (sq + nk * d)
        Spq = Spq + (spq + (np.outer(sp, d) + np.outer(d, sq)) + nk * np.outer(d, d))
    return piv, n, Sp, Sq, Spq


def port(name, onesided):
    """One update of the case by a port: (status, T) with status in uc.UPDATE | uc.DEGENERATE | uc.TOO_FEW; T = T0 where there is no update."""
    c, pr = uc.case(name), uc.pairs(name)
    p, q, T0 = pr["p"], pr["q"], c["T0"]
    n = len(p)
    if n < c["min_inliers"]:
        return uc.TOO_FEW, T0
    with np.errstate(all="ignore"):
        if onesided:
            piv, _, Sp, Sq, Spq = _chunked_sums(np.flatnonzero(pr["inl"]), p, q)
        else:
            piv, Sp, Sq, Spq = np.zeros(3), SUM(p, "pairwise"), SUM(q, "pairwise"), SUM(p[:, :, None] * q[:, None, :], "pairwise")
        H = Spq - np.outer(Sp, Sq) / n
        dR = (_kabsch_onesided if onesided else _kabsch_squared)(H)
    if dR is None:
        return uc.DEGENERATE, T0
    if onesided:
        t = dR @ ((T0[:, 3] - piv) - Sp / n) + (piv + Sq / n)
    else:
        t = dR @ T0[:, 3] + (Sq / n - dR @ Sp / n)
    return uc.UPDATE, np.hstack([dR @ T0[:, :3], t[:, None]])


STATUS = {icp_np.MAX_ITER: uc.UPDATE, icp_np.DEGENERATE: uc.DEGENERATE, icp_np.TOO_FEW: uc.TOO_FEW}


@pytest.mark.parametrize("name", uc.CASES + tuple(uc.FULL))
def test_case_is_sound_and_the_restatement_is_within_a_tenth_of_the_bound(name):
    c, pr, ref, rs = uc.case(name), uc.pairs(name), uc.reference(name), uc.restatement(name)
    assert pr["nn_margin"] >= 1e-9 and pr["corr_margin"] >= 1e-9, (pr["nn_margin"], pr["corr_margin"])
    assert rs["nn_margin"][0] == pr["nn_margin"] and min(rs["nn_margin"]) >= 1e-9 and min(rs["corr_margin"]) >= 1e-9      # the final pass too
    n = int(pr["inl"].sum())
    assert n == c.get("n_inl", n)
    assert STATUS[rs["status"]] == c["expect"], (rs["status"], c["expect"])
    if c["expect"] == uc.TOO_FEW:
        assert n == c["min_inliers"] - 1 or n < 3
        assert rs["iters"] == 0 and np.array_equal(rs["T"], c["T0"])
        return
    print(name, "n_inl", n, "s2/s1 %.3e s3/s1 %.3e d %+d" % (ref["ratio"], ref["s"][2] / ref["s"][0], ref["d"]))
    assert c["band"][0] <= ref["ratio"] <= c["band"][1], (ref["ratio"], c["band"])
    if c["expect"] == uc.DEGENERATE:
        assert ref["ratio"] <= 1e-13                                                  # 10 x below the rule's 1e-12, by the reference
        assert rs["iters"] == 0 and np.array_equal(rs["T"], c["T0"])
        return
    assert ref["ratio"] >= 1e-11                                                      # 10 x above it
    if ref["s"][2] > 1e-40 * ref["s"][0]:
        assert ref["d"] == c["d"]                                                     # (a flat pair set, s3 = 0, has no sign: dR is the same for both)
    assert rs["iters"] == 1
    (eR, et), (tR, tt) = uc.error(rs["T"], ref), uc.bound(ref)
    print("   restatement |dR| %.2e (bound %.2e)  |dt| %.2e m (bound %.2e): %.3f of the bound" % (eR, tR, et, tt, uc.over(rs["T"], ref)))
    assert eR <= 0.1 * tR and et <= 0.1 * tt
    if "update_deg" in c:                                                             # the update itself is the stated rotation
        dR = ref["T"][:, :3] @ c["T0"][:, :3].T
        ang = np.degrees(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0)
        assert abs(ang / c["update_deg"] - 1.0) < 1e-6, ang
    if name == "motion_cube8":
        assert ref["s"][2] / ref["s"][0] >= 0.999999
    if name == "motion_square":
        assert ref["s"][2] / ref["s"][0] <= 1e-15
    if name.startswith("reflect_"):
        assert ref["s"][2] <= 0.05 * ref["s"][1]                                      # d = -1 divides by s2 - s3, the bound by s2


@pytest.mark.parametrize("name", uc.CASES + tuple(uc.FULL))
def test_port_of_the_one_sided_finish_holds_the_bound(name):
    c, ref = uc.case(name), uc.reference(name)
    status, T = port(name, onesided=True)
    assert status == c["expect"]
    if status != uc.UPDATE:
        assert np.array_equal(T, c["T0"])
        return
    print(name, "one-sided port: %.3f of the bound" % uc.over(T, ref))
    assert uc.over(T, ref) <= 1.0
    R = T[:, :3]
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14


@pytest.mark.parametrize("name", [n for n in uc.COND if "1e-0" not in n and "1e-2" not in n])          # every one with s2 / s1 <= 1e-4
def test_port_of_the_squared_finish_is_rejected_on_thin_inlier_sets(name):
    """The mutant.  Measured here (its error over the bound, the four cases of a band): 1e-4: 11.5 - 132; 1e-6: 783 - 7.0e3; 1e-8: 3.9e4 -
    5.0e5; 1e-10: 540 - 8.4e3.  The kernel this port restates, measured on an MI355X: DESIGN.md 4.11."""
    ref = uc.reference(name)
    assert ref["ratio"] <= 1e-4
    status, T = port(name, onesided=False)
    ov = uc.over(T, ref) if status == uc.UPDATE else np.inf
    print(name, "squared port:", status, "%.3g of the bound" % ov)
    assert status != uc.UPDATE or ov > 1.0


def test_one_pass_sums_about_the_origin_fail_far_away_and_pivoted_ones_do_not():
    """What the pivot is for: the one-pass H about the coordinate origin, solved by the accurate one-sided finish, against the same with
    the pivot.  Far cases (1e3, 1e4 m): the origin form exceeds the bound, the pivoted one holds it."""
    for name in uc.FAR:
        c, pr, ref = uc.case(name), uc.pairs(name), uc.reference(name)
        p, q, n = pr["p"], pr["q"], len(pr["p"])
        H0 = SUM(p[:, :, None] * q[:, None, :], "pairwise") - np.outer(SUM(p, "pairwise"), SUM(q, "pairwise")) / n
        dR0 = _kabsch_onesided(H0)
        e0 = np.abs(dR0 @ c["T0"][:, :3] - ref["T"][:, :3]).max() / uc.bound(ref)[0]
        e1 = uc.over(port(name, onesided=True)[1], ref)
        print(name, "|dR| over its bound: origin sums %.3g, pivoted sums %.3g" % (e0, e1))
        assert e1 <= 1.0
        if name.endswith("_10000m"):
            assert e0 > 1.0


def test_far_exact_line_is_degenerate_only_with_pivoted_sums():
    """The exact line 1e3 and 1e4 m away: about the origin the one-pass H carries rounding noise of eps n |c|^2 and the squared finish
    takes it for a second singular value; about the pivot H is the line's own."""
    for name in ("degen_line_1000m", "degen_line_10000m"):
        old, new = port(name, onesided=False)[0], port(name, onesided=True)[0]
        print(name, "squared finish about the origin:", old, "| one-sided finish about the pivot:", new)
        assert new == uc.DEGENERATE
    assert old == uc.UPDATE                                          # at 1e4 m the earlier arithmetic updates from a line


@pytest.mark.parametrize("name", list(uc.FULL))
def test_full_cases_converge_on_the_exact_motion_with_margins(name):
    import icp_cases
    c = uc.case(name)
    rs = icp_np.icp(c["P"], c["Q"], c["T0"], **icp_cases.PARAMS)
    print(name, "iters", rs["iters"], "rmse %.2e nn margin %.2e corr margin %.2e stop margin %.2e" % (rs["rmse"], min(rs["nn_margin"]),
                                                                                                  min(rs["corr_margin"]), rs["stop_margin"]))
    assert rs["status"] == icp_np.CONVERGED and 2 <= rs["iters"] < icp_cases.PARAMS["max_iter"] and rs["n_inl"] == len(c["P"])
    assert min(rs["nn_margin"]) >= 1e-9 and min(rs["corr_margin"]) >= 1e-9 and rs["stop_margin"] >= 1e-6
    assert rs["rmse"] <= 1e-13                                       # ten times under what the GPU test asks of the device
