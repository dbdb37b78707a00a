"""The rule of the loop-closure log and the pose-graph relaxation (pr_posegraph) restated in NumPy, fp64 throughout: what
the GPU tests compare posegraph.hip with.  A pose is [R | t], 12 doubles row-major (world to camera); products and inverses are of rigid
transforms.  relax() takes two switches that change only the ORDER of its sums (the per-node edge order reversed, the dot products summed
pairwise instead of sequentially): the difference between the restatement and itself under them is what the device tolerance is derived
from (test_gpu_posegraph.py), never the device's own output."""
import numpy as np

OVERFLOW = 1
MAX_K = 128
SMALL = 1e-4                                     # the one small-angle branch: theta < SMALL takes the series
# The restatement against itself with the per-node edge order reversed and the dot products summed pairwise, on noisy_case(12, 3, 1) and
# noisy_case(40, 4, 2) at their own budgets (measured on a CPU: largest pose entry difference 6.4e-15 / 2.2e-14, largest report
# difference 7.1e-15 / 3.4e-13).  The device bound is 100 times these figures (test_gpu_posegraph.py); test_posegraph_cpu.py measures
# them again.  The consistent graph's own error against ground truth: 8.9e-15.
SELF_POSE = {12: 6.4e-15, 40: 2.2e-14}
SELF_REPORT = {12: 7.1e-15, 40: 3.4e-13}
CONSISTENT_ERR = 8.9e-15


# ------------------------------------------------------------------------------------------------ rigid transforms, batched [..., 3, 4]
def as34(P):
    return np.asarray(P, np.float64).reshape(np.shape(P)[:-1] + (3, 4)) if np.shape(P)[-1] == 12 else np.asarray(P, np.float64)


def mul(A, B):
    A, B = as34(A), as34(B)
    R = A[..., :3] @ B[..., :3]
    t = (A[..., :3] @ B[..., 3:])[..., 0] + A[..., 3]
    return np.concatenate([R, t[..., None]], axis=-1)


def inv(A):
    A = as34(A)
    Rt = np.swapaxes(A[..., :3], -1, -2)
    t = -(Rt @ A[..., 3:])[..., 0]
    return np.concatenate([Rt, t[..., None]], axis=-1)


def skew(t):
    t = np.asarray(t, np.float64)
    K = np.zeros(t.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -t[..., 2], t[..., 1]
    K[..., 1, 0], K[..., 1, 2] = t[..., 2], -t[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -t[..., 1], t[..., 0]
    return K


def exp_so3(w):
    w = np.asarray(w, np.float64)
    t2 = (w * w).sum(-1)
    th = np.sqrt(t2)
    small = th < SMALL
    ths = np.where(small, 1.0, th)
    ka = np.where(small, 1.0 - t2 / 6.0, np.sin(ths) / ths)
    kb = np.where(small, 0.5 - t2 / 24.0, (1.0 - np.cos(ths)) / np.where(small, 1.0, t2))
    K2 = w[..., :, None] * w[..., None, :] - t2[..., None, None] * np.eye(3)
    return np.eye(3) + ka[..., None, None] * skew(w) + kb[..., None, None] * K2


def log_so3(R):
    """phi and the coefficient of the inverse left Jacobian I - [phi]x / 2 + cf [phi]x^2"""
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    sn = np.sqrt((v * v).sum(-1))
    cs = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = np.arctan2(sn, cs)
    small = th < SMALL
    ths, sns = np.where(small, 1.0, th), np.where(small, 1.0, sn)
    kf = np.where(small, 1.0 + th * th / 6.0, ths / sns)
    cf = np.where(small, 1.0 / 12.0 + th * th / 720.0, 1.0 / (ths * ths) - (1.0 + cs) / (2.0 * ths * sns))
    return kf[..., None] * v, cf


def update(P, delta):
    """R <- exp(w) R, t <- exp(w) t + v; a delta of six exact zeros is the identity, bit for bit"""
    P, delta = as34(P), np.asarray(delta, np.float64)
    E = exp_so3(delta[..., :3])
    with np.errstate(invalid="ignore"):                              # (a non-finite row is passed through below)
        out = np.concatenate([E @ P[..., :3], ((E @ P[..., 3:])[..., 0] + delta[..., 3:])[..., None]], axis=-1)
    keep = ~(delta != 0.0).any(-1)
    out[keep] = P[keep]
    return out


def linearize(Z, Pi, Pj, jac=True):
    """r [m, 6] (and A, B [m, 6, 6]) of E = Z^-1 P_i P_j^-1, r = [log_SO3(R_E); t_E]"""
    Z, Pi, Pj = as34(Z), as34(Pi), as34(Pj)
    Q = mul(Pi, inv(Pj))
    Rzt = np.swapaxes(Z[..., :3], -1, -2)
    RE = Rzt @ Q[..., :3]
    tE = (Rzt @ (Q[..., 3] - Z[..., 3])[..., None])[..., 0]
    phi, cf = log_so3(RE)
    r = np.concatenate([phi, tE], axis=-1)
    if not jac:
        return r
    p2 = (phi * phi).sum(-1)
    Jl = np.eye(3) - 0.5 * skew(phi) + cf[..., None, None] * (phi[..., :, None] * phi[..., None, :] - p2[..., None, None] * np.eye(3))
    A = np.zeros(r.shape[:-1] + (6, 6))
    B = np.zeros_like(A)
    A[..., :3, :3] = Jl @ Rzt
    A[..., 3:, :3] = -(Rzt @ skew(Q[..., 3]))
    A[..., 3:, 3:] = Rzt
    B[..., :3, :3] = -(Jl @ RE)
    B[..., 3:, 3:] = -RE
    return r, A, B


def edge_cost(r, w):
    return w[..., 0] * (r[..., :3] ** 2).sum(-1) + w[..., 1] * (r[..., 3:] ** 2).sum(-1)


# ------------------------------------------------------------------------------------------------ the log
class PoseGraphModel:
    """the four buffers and the add rule"""

    def __init__(self, edge_capacity):
        self.cap = int(edge_capacity)
        self.edge_ij = np.zeros((self.cap, 2), np.int32)
        self.edge_Z = np.zeros((self.cap, 12), np.float64)
        self.edge_w = np.zeros((self.cap, 2), np.float64)
        self.state = np.zeros(4, np.int32)

    def reset(self):
        self.state[:] = 0

    def add(self, idx, T, accepted, query_row, w_rot=1.0, w_trans=1.0):
        idx = np.asarray(idx, np.int32).reshape(-1)
        T = np.asarray(T, np.float64).reshape(len(idx), 12)
        acc = np.asarray(accepted, np.uint8).reshape(-1)
        e0 = min(max(int(self.state[0]), 0), self.cap)
        flags = int(self.state[1]) & OVERFLOW
        if query_row < 0:
            return np.array([0, -1, e0, flags], np.int32)
        e = e0
        for p in range(len(idx)):
            if acc[p] == 0 or idx[p] < 0 or idx[p] == query_row or not np.isfinite(T[p]).all():
                continue
            if e == self.cap:
                flags |= OVERFLOW
                continue
            self.edge_ij[e] = (idx[p], query_row)
            self.edge_Z[e] = T[p]
            self.edge_w[e] = (w_rot, w_trans)
            e += 1
        self.state[0], self.state[1] = e, flags
        return np.array([e - e0, e0 if e > e0 else -1, e, flags], np.int32)


# ------------------------------------------------------------------------------------------------ the relaxation
def _dot(a, b, pairwise):
    s = (a * b).reshape(-1)
    if not pairwise:
        return float(np.cumsum(s)[-1]) if len(s) else 0.0            # sequential
    while len(s) > 1:
        if len(s) % 2:
            s = np.concatenate([s, [0.0]])
        s = s[0::2] + s[1::2]
    return float(s[0]) if len(s) else 0.0


def _gather(n, node, rank, deg, contrib, start, reverse):
    """out[a] = start[a] + the contributions of node a's entries, added one at a time in rank order (reversed: from the last)"""
    out = start.copy()
    r = deg[node] - 1 - rank if reverse else rank
    for q in range(int(deg.max()) if len(deg) and len(node) else 0):
        sel = r == q
        out[node[sel]] += contrib[sel]                               # a node has one entry of each rank
    return out


def _block_inverse(D):
    """Gauss-Jordan without pivoting over [n, 6, 6]; a pivot that is not positive makes the inverse the zero block"""
    D = D.copy()
    n = len(D)
    Inv = np.tile(np.eye(6), (n, 1, 1))
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for k in range(6):
            piv = D[:, k, k].copy()
            ok &= (piv > 0.0) & np.isfinite(piv)
            ip = 1.0 / piv
            D[:, k, :] *= ip[:, None]
            Inv[:, k, :] *= ip[:, None]
            for r in range(6):
                if r == k:
                    continue
                f = D[:, r, k].copy()
                D[:, r, :] -= f[:, None] * D[:, k, :]
                Inv[:, r, :] -= f[:, None] * Inv[:, k, :]
    Inv[~ok] = 0.0
    return Inv


def used_edges(poses, n, edge_ij, edge_Z, edge_w, edges, w_odo_rot, w_odo_trans):
    """(I, J, Z [m, 3, 4], W [m, 2], logged used): the odometry edges of the finite input poses, then the logged edges in log order"""
    P = as34(poses)
    fin = np.isfinite(P[:n].reshape(n, 12)).all(1) if n > 0 else np.zeros(0, bool)
    I = [i for i in range(n - 1) if fin[i] and fin[i + 1]]
    J = [i + 1 for i in I]
    Z = [mul(P[i], inv(P[i + 1])) for i in I]
    W = [(w_odo_rot, w_odo_trans)] * len(I)
    logged = 0
    for l in range(int(edges)):
        i, j = int(edge_ij[l][0]), int(edge_ij[l][1])
        if not (0 <= i < n and 0 <= j < n) or i == j or not (fin[i] and fin[j]):
            continue
        if not (np.isfinite(edge_Z[l]).all() and np.isfinite(edge_w[l]).all()):
            continue
        I.append(i); J.append(j); Z.append(np.asarray(edge_Z[l], np.float64).reshape(3, 4)); W.append(tuple(edge_w[l]))
        logged += 1
    return (np.array(I, np.int64), np.array(J, np.int64), np.array(Z, np.float64).reshape(-1, 3, 4), np.array(W, np.float64).reshape(-1, 2),
            logged)


def relax(poses, n, edge_ij, edge_Z, edge_w, edges, outer, inner, lam, w_odo_rot, w_odo_trans, reverse=False, pairwise=False):
    """-> (poses_out [N, 12] - rows >= n untouched -, report [outer + 2])"""
    poses = np.array(poses, np.float64).reshape(-1, 12)
    n = min(max(int(n), 0), len(poses))
    edges = min(max(int(edges), 0), len(edge_ij))
    out = poses.copy()
    report = np.zeros(outer + 2)
    I, J, Z, W, logged = used_edges(poses, n, edge_ij, edge_Z, edge_w, edges, w_odo_rot, w_odo_trans)
    m = len(I)
    report[outer + 1] = m
    if n < 2 or logged == 0:
        return out, report                                          # nothing to relax: the bytes of the input, every cost 0
    X = poses[:n].reshape(n, 3, 4).copy()
    # the incidence entries (edge e, side): node a's entries in ascending e = odometry a - 1, odometry a, its logged edges in log order
    node = np.concatenate([I, J])
    eidx = np.concatenate([np.arange(m), np.arange(m)])
    order = np.lexsort((eidx, node))
    deg = np.bincount(node, minlength=n)
    first = np.concatenate([[0], np.cumsum(deg)[:-1]])
    rank = np.empty(2 * m, np.int64)
    rank[order] = np.arange(2 * m) - first[node[order]]
    gauge = node == 0
    Wd = np.repeat(W, 3, axis=1)                                     # [m, 6]
    for s in range(outer):
        r, A, B = linearize(Z, X[I], X[J])
        report[s] = _dot(edge_cost(r, W), np.ones(m), pairwise)
        Jt = np.concatenate([np.swapaxes(A, 1, 2), np.swapaxes(B, 1, 2)])                      # [2m, 6, 6] = J^T per entry
        Jn = np.concatenate([A, B])
        W2 = np.concatenate([Wd, Wd])
        gc = -(Jt @ (W2 * np.concatenate([r, r]))[..., None])[..., 0]
        Dc = Jt @ (W2[:, :, None] * Jn)
        gc[gauge] = 0.0; Dc[gauge] = 0.0
        g = _gather(n, node, rank, deg, gc, np.zeros((n, 6)), reverse)
        D = _gather(n, node, rank, deg, Dc, np.tile(lam * np.eye(6), (n, 1, 1)), reverse)
        Dinv = _block_inverse(D)
        Dinv[0] = np.eye(6)

        def matvec(p):
            u = Wd * ((A @ p[I][..., None])[..., 0] + (B @ p[J][..., None])[..., 0])
            c = (Jt @ np.concatenate([u, u])[..., None])[..., 0]
            c[gauge] = 0.0
            start = lam * p
            start[0] = 0.0
            return _gather(n, node, rank, deg, c, start, reverse)

        x = np.zeros((n, 6))
        res = g.copy()
        z = (Dinv @ res[..., None])[..., 0]
        p = z.copy()
        rz = _dot(res, z, pairwise)
        for _ in range(inner):
            q = matvec(p)
            pq = _dot(p, q, pairwise)
            alpha = rz / pq if pq > 0.0 else 0.0
            x += alpha * p
            res -= alpha * q
            z = (Dinv @ res[..., None])[..., 0]
            rzn = _dot(res, z, pairwise)
            beta = rzn / rz if rz > 0.0 else 0.0
            p = z + beta * p
            rz = rzn
        x[0] = 0.0
        X = update(X, x)
    report[outer] = _dot(edge_cost(linearize(Z, X[I], X[J], jac=False), W), np.ones(m), pairwise)
    out[:n] = X.reshape(n, 12)
    return out, report


# ------------------------------------------------------------------------------------------------ committed cases
def circle_truth(n=12, laps=2, radius=10.0):
    """world-to-camera poses of a camera on `laps` laps of a circle, looking along the tangent, with a slow climb"""
    P = np.zeros((n, 3, 4))
    for a in range(n):
        ang = 2.0 * np.pi * laps * a / n
        c2w = np.eye(4)
        c2w[:3, :3] = exp_so3(np.array([0.0, 0.0, ang]))
        c2w[:3, 3] = (radius * np.cos(ang), radius * np.sin(ang), 0.05 * a)
        P[a] = inv(c2w[:3])
    return P.reshape(n, 12)


def noisy(P, seed, rot=0.02, trans=0.1):
    """ground truth composed with seeded odometry noise: the relative motions are perturbed and re-chained from node 0"""
    rng = np.random.default_rng(seed)
    P = as34(P)
    out = np.empty_like(P)
    out[0] = P[0]
    for a in range(1, len(P)):
        step = mul(P[a], inv(P[a - 1]))                              # P_a = step P_{a-1}
        d = np.concatenate([rng.normal(0.0, rot, 3), rng.normal(0.0, trans, 3)])
        out[a] = mul(update(step[None], d[None])[0], out[a - 1])
    return out.reshape(len(P), 12)


def measure(P, i, j):
    """Z_ij = P_i P_j^-1"""
    P = as34(P)
    return mul(P[i], inv(P[j])).reshape(12)


def consistent_case():
    """the issue's consistent graph: a two-lap circle of 12 nodes, every measurement (the chain included, as logged edges over a
    zero-weight odometry) from ground truth, the input poses noisy"""
    gt = circle_truth(12, 2)
    pairs = [(a, a + 1) for a in range(11)] + [(0, 6), (1, 7), (2, 8), (3, 9), (4, 10), (5, 11)]
    return dict(gt=gt, poses=noisy(gt, 5), pairs=pairs, Z=np.array([measure(gt, i, j) for i, j in pairs]),
                params=dict(outer=6, inner=72, lam=0.0, w_odo_rot=0.0, w_odo_trans=0.0))


def noisy_case(n, closures, seed):
    """the issue's noisy graphs: odometry-noisy input poses, closures measured from ground truth with their own small noise"""
    gt = circle_truth(n, 2, radius=10.0 + n / 4.0)
    rng = np.random.default_rng(seed + 100)
    half = n // 2
    starts = np.linspace(0, half - 1, closures).astype(int)
    pairs = [(int(a), int(a) + half) for a in starts]
    Z = []
    for i, j in pairs:
        d = np.concatenate([rng.normal(0.0, 0.002, 3), rng.normal(0.0, 0.01, 3)])
        Z.append(update(measure(gt, i, j).reshape(1, 12), d[None])[0].reshape(12))
    return dict(gt=gt, poses=noisy(gt, seed), pairs=pairs, Z=np.array(Z), w=(100.0, 10.0),
                params=dict(outer=10, inner=6 * n, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0))


def log_of(case, cap=None, w=(1.0, 1.0)):
    """a PoseGraphModel holding the case's edges"""
    m = PoseGraphModel(cap or len(case["pairs"]))
    w = case.get("w", w)
    for (i, j), Z in zip(case["pairs"], case["Z"]):
        m.add([i], Z, [1], j, *w)
    return m


def relax_case(case, **kw):
    m = log_of(case)
    p = dict(case["params"]); p.update(kw)
    return relax(case["poses"], len(case["poses"]), m.edge_ij, m.edge_Z, m.edge_w, m.state[0], **p)


SWEEP_NODES = (0, 1, 2, 3, 12, 40, 257)                              # 257: a 256-lane block wraps
SWEEP_LOGS = ("none", "one", "four", "hub")


def sweep_case(n, log):
    """the relax sweep of the GPU test: n nodes of a noisy two-lap circle inside a larger pose buffer, and a log of 0, 1 or 4 closures or
    of one node carrying 5 edges (as i and as j) - each non-empty log with one more edge that points at a row >= n"""
    N = n + 3
    gt = circle_truth(N, 2, radius=10.0 + N / 8.0)
    rng = np.random.default_rng(1000 * n + SWEEP_LOGS.index(log))
    pairs = []
    if log != "none":
        if n >= 2:
            if log == "hub":
                h = n // 2
                others = [a for a in range(n) if a != h]
                picks = [others[int(q)] for q in rng.integers(0, len(others), 5)]
                pairs = [(h, a) if t % 2 else (a, h) for t, a in enumerate(picks)]
            else:
                for _ in range(1 if log == "one" else 4):
                    i, j = sorted(int(q) for q in rng.choice(n, 2, replace=False))
                    pairs.append((i, j))
        else:
            pairs = [(0, 1)]
        pairs.append((0, n + 1))                                     # points behind n: never used
    Z = []
    for i, j in pairs:
        d = np.concatenate([rng.normal(0.0, 0.002, 3), rng.normal(0.0, 0.01, 3)])
        Z.append(update(measure(gt, i, j).reshape(1, 12), d[None])[0].reshape(12))
    sc = min(1.0, 12.0 / max(n, 1)) ** 0.5                           # the drift of a longer chain stays that of 12 nodes
    return dict(n=n, gt=gt, poses=noisy(gt, 77 + n, rot=0.01 * sc, trans=0.05 * sc), pairs=pairs, Z=np.array(Z).reshape(-1, 12), w=(100.0, 10.0),
                params=dict(outer=4, inner=max(1, min(6 * n, 600)), lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0))


def relax_sweep(case, **kw):
    m = log_of(case, cap=8)
    p = dict(case["params"]); p.update(kw)
    return relax(case["poses"], case["n"], m.edge_ij, m.edge_Z, m.edge_w, m.state[0], **p)
