"""Normative arithmetic of the ICP refinement (csrc/icp.hip) as a NumPy restatement in fp64: the role gist_np.py, bow_np.py
and delight_np.py play for their kernels.  Point-to-point ICP of a source cloud P onto a target cloud Q from T0 = [R | t].

  transform        p' = ((R00 x + R01 y) + R02 z) + t0, every product and sum rounded (NumPy never fuses)
  correspondence   d2(i, j) = ((dx dx) + dy dy) + dz dz, the FIRST minimum over j: strict `best > d2` from (+Inf, -1), so a NaN or +Inf
                   distance never wins (run_test.m:5-16)
  inlier           d2 < max_corr^2
  update           Kabsch on the inliers: H = sum (p' - mu_p)(q - mu_q)^T = U S V^T, dR = V diag(1, 1, det(V U^T)) U^T, dt = mu_q - dR mu_p,
                   R <- dR R, t <- dR t + dt
  statistics       n_inl, rmse = sqrt(sum_inl d2 / n_inl) (0 without inliers), fitness = n_inl / |P| (0 for an empty P)
  stop             too_few: n_inl < min_inliers; degenerate: not (s2 > 1e-12 s1); converged: after an update, |rmse - rmse_prev| < tol_rmse
                   and |fitness - fitness_prev| < tol_fitness against the iteration before; max_iter updates done
  report           one more correspondence pass under the final T gives fitness, rmse, n_inl

The sums of an update (centroids, H, sum d2) have no normative ORDER: `order` selects forward, reversed or pairwise summation, and
test_icp_cpu.py bounds what the choice can move.  Correspondences, inlier sets, status, iters, n_inl and fitness are exact."""
import numpy as np

CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE, NO_PAIR = 0, 1, 2, 3, 4
STATS_DTYPE = np.dtype([("fitness", "<f8"), ("rmse", "<f8"), ("n_inl", "<i4"), ("iters", "<i4"), ("status", "<i4"), ("pad", "<i4")])


def transform(T, P):
    T = np.asarray(T, np.float64).reshape(3, 4)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[a, 0] * P[:, 0] + T[a, 1] * P[:, 1]) + T[a, 2] * P[:, 2]) + T[a, 3] for a in range(3)], 1)


def nn(Pt, Q, margins=False, block=512):
    """First-minimum nearest neighbour of every transformed source point: (idx int32, -1 = none; d2, +Inf = none) and with margins the
    smallest relative gap between the best and the second-best d2 of any point (Inf when no point has two finite candidates)."""
    Pt = np.asarray(Pt, np.float64).reshape(-1, 3)
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    n, m = len(Pt), len(Q)
    idx = np.full(n, -1, np.int32)
    d2 = np.full(n, np.inf)
    gap = np.inf
    for b0 in range(0, n if m else 0, block):
        p = Pt[b0:b0 + block]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = p[:, None, 0] - Q[None, :, 0]
            dy = p[:, None, 1] - Q[None, :, 1]
            dz = p[:, None, 2] - Q[None, :, 2]
            d = ((dx * dx) + dy * dy) + dz * dz
        d = np.where(np.isnan(d), np.inf, d)
        j = np.argmin(d, 1)                                        # the first index of the smallest value
        v = d[np.arange(len(p)), j]
        ok = v < np.inf
        idx[b0:b0 + block] = np.where(ok, j, -1)
        d2[b0:b0 + block] = v
        if margins and m > 1:
            e = d.copy()
            e[np.arange(len(p)), j] = np.inf
            s = e.min(1)
            both = ok & (s < np.inf)
            if both.any():
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.where(s[both] > 0, (s[both] - v[both]) / s[both], 0.0)
                gap = min(gap, float(rel.min()))
    return (idx, d2, gap) if margins else (idx, d2)


def _sum(x, order):
    """Column sums of x [n, ...] in the chosen order."""
    x = np.asarray(x, np.float64)
    if order == "pairwise":                                        # a balanced tree over the rows
        if len(x) == 0:
            return np.zeros(x.shape[1:])
        while len(x) > 1:
            if len(x) & 1:
                x = np.concatenate([x, np.zeros((1,) + x.shape[1:])])
            x = x[0::2] + x[1::2]
        return x[0]
    acc = np.zeros(x.shape[1:])
    for row in (x if order == "forward" else x[::-1]):
        acc = acc + row
    return acc


def _stats(d2, inl, n_src, order):
    n = int(inl.sum())
    rmse = float(np.sqrt(_sum(d2[inl], order) / n)) if n else 0.0
    return n, rmse, (n / n_src if n_src else 0.0)


def icp(P, Q, T0, max_iter=30, max_corr=1.0, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=3, order="pairwise"):
    """Returns dict(T [3, 4], fitness, rmse, n_inl, iters, status, nn_margin [per pass], corr_margin [per pass], stop_margin): the margins are
    the smallest relative gap best / second-best d2 and the smallest relative distance of any finite d2 to max_corr^2 in every pass (the
    final one included), and the smallest relative distance of a convergence test's two differences to their tolerances."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    T = np.array(T0, np.float64).reshape(3, 4)
    mc2 = max_corr * max_corr
    nn_margin, corr_margin, stop_margin = [], [], np.inf
    status, iters, prev = MAX_ITER, 0, None

    def one_pass(T):
        Pt = transform(T, P)
        idx, d2, gap = nn(Pt, Q, margins=True)
        fin = d2[d2 < np.inf]
        nn_margin.append(gap)
        corr_margin.append(float((np.abs(fin - mc2) / mc2).min()) if len(fin) else np.inf)
        return Pt, idx, d2, d2 < mc2

    for _ in range(max_iter):
        Pt, idx, d2, inl = one_pass(T)
        n, rmse, fit = _stats(d2, inl, len(P), order)
        if n < min_inliers:
            status = TOO_FEW
            break
        p, q = Pt[inl], Q[idx[inl]]
        mu_p, mu_q = _sum(p, order) / n, _sum(q, order) / n
        H = _sum((p - mu_p)[:, :, None] * (q - mu_q)[:, None, :], order)
        U, s, Vt = np.linalg.svd(H)
        if not (s[1] > 1e-12 * s[0]):
            status = DEGENERATE
            break
        dR = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
        dt = mu_q - dR @ mu_p
        T = np.hstack([dR @ T[:, :3], (dR @ T[:, 3] + dt)[:, None]])
        iters += 1
        if prev is not None:
            a, b = abs(rmse - prev[0]), abs(fit - prev[1])
            for diff, tol in ((a, tol_rmse), (b, tol_fitness)):
                if tol > 0:
                    stop_margin = min(stop_margin, abs(diff - tol) / tol)
            if a < tol_rmse and b < tol_fitness:
                status = CONVERGED
                break
        prev = (rmse, fit)
    _, idx, d2, inl = one_pass(T)
    n, rmse, fit = _stats(d2, inl, len(P), order)
    return dict(T=T, fitness=fit, rmse=rmse, n_inl=n, iters=iters, status=status, nn_margin=nn_margin, corr_margin=corr_margin,
                stop_margin=stop_margin)


def sequential_first_min(d):
    """run_test.m:5-16: strict `best > d` from (+Inf, -1)."""
    bd, bj = np.inf, -1
    for j, x in enumerate(d):
        if bd > x:
            bd, bj = x, j
    return bd, bj


def combine(a, b):
    """What every combine of two partial results does: the smaller d2, on equal d2 the smaller j; (+Inf, -1) is "no candidate"."""
    if b[1] >= 0 and (b[0] < a[0] or (b[0] == a[0] and b[1] < a[1])):
        return b
    return a
