"""NumPy restatement of the pose-proximity candidate search and of the batch add of the closure log (pr_proximity, pr_posegraphb_add; the
rules of include/place_recognition.h), operation by operation: the same products, the same association, the same blocked
order of the path length.  NumPy's elementwise + - x sqrt are IEEE operations without contraction, so the device must return these bytes.

search() returns the seven outputs of pr_proximity_search under their names, and under "aux" the centres, axes, validity and path length.
chain_scene() / chain_run() build and run the scene of the chain tests once for every test that needs it."""
import functools

import numpy as np

T = 256
QRANGE_CLAMPED = 1
OVERFLOW = 1
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def clamp(v, hi):
    return min(max(int(v), 0), int(hi))


# ------------------------------------------------------------------------------------------------ rows, centres, path length
def prepare(poses, n, cap):
    """-> (valid bool [cap], cen [cap, 3], axis [cap, 3]): steps 0 and 1; zeros for a row that is not valid"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)[:cap]
    n = clamp(n, cap)
    valid = (np.arange(cap) < n) & np.isfinite(P).all(1)
    A = np.where(valid[:, None], P, 0.0).reshape(cap, 3, 4)
    R, t = A[:, :, :3], A[:, :, 3]
    y = (R[:, 0, :] * t[:, 0, None] + R[:, 1, :] * t[:, 1, None]) + R[:, 2, :] * t[:, 2, None]          # R^T t
    with np.errstate(all="ignore"):
        cen = np.where(valid[:, None], -y, 0.0)
    return valid, cen, R[:, 2, :].copy()


def path_length(cen, valid):
    """step 2: 256 blocks of C rows, a running sum inside a block, the totals summed in block order, s = base + running sum"""
    cap = len(cen)
    C = -(-cap // T)
    w = np.zeros(cap)
    total = np.zeros(T)
    prev = -1
    with np.errstate(all="ignore"):
        for b in range(T):
            run = 0.0
            for i in range(min(b * C, cap), min(b * C + C, cap)):
                if valid[i]:
                    if prev >= 0:
                        d = cen[i] - cen[prev]
                        run = run + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                    prev = i
                w[i] = run
            total[b] = run
        base = 0.0
        s = np.zeros(cap)
        for b in range(T):
            lo, hi = min(b * C, cap), min(b * C + C, cap)
            s[lo:hi] = base + w[lo:hi]
            base = base + total[b]
    return s


# ------------------------------------------------------------------------------------------------ the 3 x 4 products
def _inv(P):
    R, t = P[:, :3], P[:, 3]
    y = (R[0, :] * t[0] + R[1, :] * t[1]) + R[2, :] * t[2]
    return np.concatenate([R.T, (-y)[:, None]], axis=1)


def _mul(A, B):
    RA, tA, RB, tB = A[:, :3], A[:, 3], B[:, :3], B[:, 3]
    R = (RA[:, 0, None] * RB[None, 0, :] + RA[:, 1, None] * RB[None, 1, :]) + RA[:, 2, None] * RB[None, 2, :]
    t = ((RA[:, 0] * tB[0] + RA[:, 1] * tB[1]) + RA[:, 2] * tB[2]) + tA
    return np.concatenate([R, t[:, None]], axis=1)


def seed(poses, i, q):
    """T0 = P_i P_q^-1 [12]"""
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        return _mul(P[i], _inv(P[q])).reshape(12)


# ------------------------------------------------------------------------------------------------ the search
def candidates(valid, cen, axis, s, n, q, radius, growth, radius_max, cos_min, min_gap):
    """step 3: (rows i ascending, their d2) of query row q (valid, 0 <= q < n)"""
    i = np.arange(n)
    with np.errstate(all="ignore"):
        dx = cen[:n] - cen[q]
        d2 = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
        rad = radius + growth * (s[q] - s[:n])
        rad = np.where(rad < radius_max, rad, radius_max)
        ok = valid[:n] & (i + int(min_gap) <= q) & (d2 < rad * rad)
        if cos_min > -1.0:
            dot = (axis[:n, 0] * axis[q, 0] + axis[:n, 1] * axis[q, 1]) + axis[:n, 2] * axis[q, 2]
            ok &= dot >= cos_min
    return i[ok], d2[ok]


def select(rows, d2, stride, k):
    """step 4: one representative per bucket, then the k best by (d2, row)"""
    b = rows // int(stride)
    order = np.lexsort((rows, d2, b))                              # bucket, then d2, then row
    first = np.ones(len(order), bool)
    first[1:] = b[order][1:] != b[order][:-1]
    rep = order[first]
    best = rep[np.lexsort((rows[rep], d2[rep]))][:k]
    return rows[best], d2[best]


def search(poses, n, qrange, node_capacity, query_capacity, *, radius, growth=0.0, radius_max=None, cos_min=-1.0, min_gap, stride=1, k=1,
           log=None, log_edge_capacity=0, known_window=0):
    """log: (edge_ij i32 [>= log_edge_capacity, 2], state i32 [>= 1]) or None"""
    cap, Q, k = int(node_capacity), int(query_capacity), int(k)
    radius_max = radius if radius_max is None else radius_max
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    n = clamp(n, cap)
    q0, mq_raw = int(qrange[0]), int(qrange[1])
    mq = clamp(mq_raw, Q)
    flags = QRANGE_CLAMPED if mq != mq_raw else 0
    if mq > 0 and (q0 < 0 or q0 + mq - 1 > n - 1):
        flags |= QRANGE_CLAMPED
    valid, cen, axis = prepare(poses, n, cap)
    s = path_length(cen, valid)
    idx = np.full((Q, k), -1, np.int32)
    d2o = np.full((Q, k), np.inf)
    T0 = np.tile(IDENTITY, (Q * k, 1))
    src = np.full(Q * k, -1, np.int32)
    dst = np.full(Q * k, -1, np.int32)
    known = np.zeros(Q * k, np.uint8)
    E = 0
    if log is not None:
        E = clamp(log[1][0], log_edge_capacity)
        e = np.asarray(log[0], np.int64).reshape(-1, 2)[:E]
        e_ok = (e >= 0).all(1)
        e_lo, e_hi = e.min(1), e.max(1)
    searched = filled = nknown = 0
    for r in range(mq):
        q = q0 + r
        if not (0 <= q < n and valid[q]):
            continue
        searched += 1
        rows, dd = select(*candidates(valid, cen, axis, s, n, q, radius, growth, radius_max, cos_min, min_gap), stride, k)
        for slot, (i, d) in enumerate(zip(rows, dd)):
            o = r * k + slot
            idx[r, slot], d2o[r, slot] = i, d
            filled += 1
            if E and (e_ok & (np.abs(e_lo - i) <= known_window) & (np.abs(e_hi - q) <= known_window)).any():
                known[o] = 1
                nknown += 1
                continue
            T0[o] = seed(poses, i, q)
            src[o], dst[o] = q, i
    return dict(idx=idx, d2=d2o, T0=T0.reshape(Q * k, 3, 4), pair_src=src, pair_dst=dst, known=known,
                info=np.array([searched, filled, nknown, flags], np.int32), aux=dict(valid=valid, cen=cen, axis=axis, s=s))


# ------------------------------------------------------------------------------------------------ the batch add
def add_batch(model, i, j, T, accepted, w=None, w_rot=1.0, w_trans=1.0):
    """the batch log rule on a posegraph_np.PoseGraphModel -> info i32 [4]"""
    i = np.asarray(i, np.int32).reshape(-1)
    j = np.asarray(j, np.int32).reshape(-1)
    c = len(i)
    T = np.asarray(T, np.float64).reshape(c, 12)
    acc = np.asarray(accepted, np.uint8).reshape(-1)
    W = np.tile(np.array([w_rot, w_trans], np.float64), (c, 1)) if w is None else np.asarray(w, np.float64).reshape(c, 2)
    e0 = clamp(model.state[0], model.cap)
    flags = int(model.state[1]) & OVERFLOW
    e = e0
    for p in range(c):
        if acc[p] == 0 or i[p] < 0 or j[p] < 0 or i[p] == j[p] or not np.isfinite(T[p]).all():
            continue
        if not (np.isfinite(W[p]).all() and (W[p] >= 0.0).all()):
            continue
        if e == model.cap:
            flags |= OVERFLOW
            continue
        model.edge_ij[e] = (i[p], j[p])
        model.edge_Z[e] = T[p]
        model.edge_w[e] = W[p]
        e += 1
    if (j >= 0).any():                                             # a single add with a negative query row leaves state as it is
        model.state[0], model.state[1] = e, flags
    return np.array([e - e0, e0 if e > e0 else -1, e, flags], np.int32)


# ------------------------------------------------------------------------------------------------ scenes
def lattice_poses(points, yaw=None):
    """W2C rows whose camera centres are exactly `points` (integers stay exact): R a rotation about z by a multiple of 90 degrees
    (yaw[i] quarter turns; entries 0, 1, -1), t = -R c"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    yaw = np.zeros(len(pts), np.int64) if yaw is None else np.asarray(yaw, np.int64)
    P = np.zeros((len(pts), 3, 4))
    for a, (c, y) in enumerate(zip(pts, yaw)):
        co, si = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(y) % 4]
        # camera looks along the world direction (co, si, 0): row 2 of R is the viewing axis
        R = np.array([[si, -co, 0.0], [0.0, 0.0, -1.0], [co, si, 0.0]])
        P[a, :, :3] = R
        P[a, :, 3] = -(R @ c)
    return P.reshape(-1, 12)


def two_lap_circle(n, seed=3, radius=30.0, rot=0.002, trans=0.03, flat=False):
    """a noisy two-lap circle of n keyframes (posegraph_np.circle_truth under odometry noise); flat: without circle_truth's climb of
    0.05 a keyframe, which at thousands of keyframes lifts the second lap out of any radius"""
    import posegraph_np as pg
    gt = pg.circle_truth(n, 2, radius=radius)
    if flat:
        G = gt.reshape(n, 3, 4).copy()
        G[:, :, 3] += G[:, :, 2] * (0.05 * np.arange(n))[:, None]   # c2w = [R | c]: t = -R^T c, so lowering c by z adds column z of R^T
        gt = G.reshape(n, 12)
    return pg.noisy(gt, seed, rot=rot, trans=trans)


CHAIN = dict(n=80, seed=7, landmarks=6000, see=14.0, keep=0.9, jitter=0.01,
             search=dict(radius=3.0, growth=0.03, radius_max=12.0, min_gap=20, stride=8, k=2),
             icp=dict(max_iter=20, max_corr=1.0), min_fitness=0.5, max_rmse=0.3, w=(100.0, 10.0),
             relax=dict(outer=6, inner=480, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0),
             gate=dict(max_gap=4, min_support=1, rounds=4))


@functools.lru_cache(maxsize=None)
def chain_scene(cloud_seed=11):
    """-> dict(gt, est [n, 12], clouds [list of [m, 3]]): the issue's chain scene"""
    import posegraph_np as pg
    c = CHAIN
    gt = pg.circle_truth(c["n"], 2, radius=20.0)
    est = pg.noisy(gt, c["seed"], rot=0.004, trans=0.05)
    rng = np.random.default_rng(cloud_seed)
    L = np.stack([rng.uniform(-32.0, 32.0, c["landmarks"]), rng.uniform(-32.0, 32.0, c["landmarks"]), rng.uniform(-2.0, 6.0, c["landmarks"])], 1)
    G = gt.reshape(-1, 3, 4)
    clouds = []
    for a in range(c["n"]):
        R, t = G[a, :, :3], G[a, :, 3]
        centre = -(R.T @ t)
        near = L[np.linalg.norm(L - centre, axis=1) < c["see"]]
        near = near[rng.random(len(near)) < c["keep"]]
        clouds.append(near @ R.T + t + rng.normal(0.0, c["jitter"], near.shape))
    return dict(gt=gt, est=est, clouds=clouds)


@functools.lru_cache(maxsize=None)
def chain_run(cloud_seed=11):
    """the chain on the CPU: search -> icp_np from T0 -> accept.  -> dict(search, slots, T [c, 12], fitness, rmse, status, iters, n_inl, accepted)
    over the slots that carry a pair"""
    import icp_np
    sc = chain_scene(cloud_seed)
    c = CHAIN
    n = c["n"]
    res = search(sc["est"], n, (0, n), n, n, **c["search"])
    slots = np.flatnonzero(res["pair_src"] >= 0)
    T, fit, rmse, ran, status, iters, n_inl = [], [], [], [], [], [], []
    for o in slots:
        q, i = int(res["pair_src"][o]), int(res["pair_dst"][o])
        r = icp_np.icp(sc["clouds"][q], sc["clouds"][i], res["T0"][o], **c["icp"])
        T.append(r["T"].reshape(12)); fit.append(r["fitness"]); rmse.append(r["rmse"])
        ran.append(r["status"] in (icp_np.CONVERGED, icp_np.MAX_ITER))
        status.append(r["status"]); iters.append(r["iters"]); n_inl.append(r["n_inl"])
    T, fit, rmse = np.array(T).reshape(-1, 12), np.array(fit), np.array(rmse)
    # verify's accept rule: a finished refinement with fitness >= min_fitness and rmse <= max_rmse (the 5 % margins the tests assert make
    # >= and > the same decision)
    return dict(search=res, slots=slots, T=T, fitness=fit, rmse=rmse, status=np.array(status), iters=np.array(iters), n_inl=np.array(n_inl),
                accepted=np.array(ran, bool) & (fit >= c["min_fitness"]) & (rmse <= c["max_rmse"]))
