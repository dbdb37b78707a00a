"""The rule of the closure consistency gate (pr_gate; the text of include/place_recognition.h) restated in NumPy, fp64
throughout: what the GPU tests compare gate.hip with, byte for byte.  Every product is written out as explicit scalar products in the
stated order - (a0 b0 + a1 b1) + a2 b2 - vectorised over edges and over pairs; there is no `@`, whose summation order NumPy does not
promise.  (NumPy's elementwise + and x round once each and are never contracted into a fused multiply-add.)  The case builders stand on
posegraph_np's circle_truth / measure / noisy / log_of."""
import numpy as np

import posegraph_np as pg

SRC_OVERFLOW, UNSETTLED = 1, 2
LOG_OVERFLOW = pg.OVERFLOW


# ------------------------------------------------------------------------------------------------ rigid transforms [..., 3, 4], explicit order
def mul33(A, B):
    C = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for r in range(3):
        for c in range(3):
            C[..., r, c] = (A[..., r, 0] * B[..., 0, c] + A[..., r, 1] * B[..., 1, c]) + A[..., r, 2] * B[..., 2, c]
    return C


def mv3(A, x):
    y = np.empty(np.broadcast_shapes(A.shape[:-1], x.shape))
    for r in range(3):
        y[..., r] = (A[..., r, 0] * x[..., 0] + A[..., r, 1] * x[..., 1]) + A[..., r, 2] * x[..., 2]
    return y


def rmul(A, B):
    """A B = [R_A R_B | R_A t_B + t_A]"""
    R = mul33(A[..., :3], B[..., :3])
    t = mv3(A[..., :3], B[..., 3]) + A[..., 3]
    return np.concatenate([R, t[..., None]], axis=-1)


def rinv(A):
    """A^-1 = [R^T | -(R^T t)]"""
    Rt = np.ascontiguousarray(np.swapaxes(A[..., :3], -1, -2))
    t = -mv3(Rt, A[..., 3])
    return np.concatenate([Rt, t[..., None]], axis=-1)


def default_tables(max_gap, rot_deg=2.0, rot_deg_per_kf=0.05, trans=0.5, trans_per_kf=0.02):
    g = np.arange(max_gap + 1, dtype=np.float64)
    return 2.0 * (1.0 - np.cos(np.radians(rot_deg + g * rot_deg_per_kf))), (trans + g * trans_per_kf) ** 2


# ------------------------------------------------------------------------------------------------ the rule
def gate(poses, n, log, node_capacity, max_gap, min_support, rounds, rot_tab, trans2_tab, dst=None, margins=False):
    """log: a PoseGraphModel (edge_ij, edge_Z, edge_w, state; its capacity is edge_capacity).  dst: a PoseGraphModel to write, or None.
    -> dict(keep u8 [EC], support i32 [EC], map i32 [EC], info i32 [4]) and, with margins=True, `margin`: the smallest relative distance
    |c - entry| / entry of any comparable pair's c_rot / c_trans from its (finite, positive) table entry."""
    EC = log.cap
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    rot_tab, trans2_tab = np.asarray(rot_tab, np.float64), np.asarray(trans2_tab, np.float64)
    E = min(max(int(log.state[0]), 0), EC)                                                      # 1. counts
    n = min(max(int(n), 0), int(node_capacity))
    ij = log.edge_ij[:E].astype(np.int64)
    i, j = ij[:, 0], ij[:, 1]
    valid = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j)                                  # 2. valid edges
    valid &= np.isfinite(log.edge_Z[:E]).all(1) & np.isfinite(log.edge_w[:E]).all(1)
    ic, jc = np.where(valid, i, 0), np.where(valid, j, 0)
    fin = np.isfinite(poses).all(1)                                                             # (node_capacity >= 1 rows)
    valid &= fin[ic] & fin[jc]
    V = np.flatnonzero(valid)
    m = len(V)
    S = np.zeros((m, m), bool)
    margin = np.inf
    if m:
        with np.errstate(all="ignore"):
            Z = log.edge_Z[V].reshape(m, 3, 4)
            Pi, Pj = poses[i[V]].reshape(m, 3, 4), poses[j[V]].reshape(m, 3, 4)
            L = rmul(rinv(Z), Pi)                                                               # 3. per valid edge
            M = rmul(rmul(rinv(Pi), Z), Pj)
            N = rinv(Pj)
            iv, jv = i[V], j[V]
            gap = np.abs(iv[:, None] - iv[None, :]) + np.abs(jv[:, None] - jv[None, :])         # 4. ordered pairs [a, b]
            comparable = (gap <= max_gap) & (jv[:, None] != jv[None, :]) & ~np.eye(m, dtype=bool)
            Y = rmul(L[:, None], M[None, :])                                                    # L_a M_b
            Na = N[:, None]
            x00 = (Y[..., 0, 0] * Na[..., 0, 0] + Y[..., 0, 1] * Na[..., 1, 0]) + Y[..., 0, 2] * Na[..., 2, 0]
            x11 = (Y[..., 1, 0] * Na[..., 0, 1] + Y[..., 1, 1] * Na[..., 1, 1]) + Y[..., 1, 2] * Na[..., 2, 1]
            x22 = (Y[..., 2, 0] * Na[..., 0, 2] + Y[..., 2, 1] * Na[..., 1, 2]) + Y[..., 2, 2] * Na[..., 2, 2]
            t = mv3(Y[..., :3], np.broadcast_to(Na[..., 3], Y.shape[:-2] + (3,))) + Y[..., 3]
            c_rot = 3.0 - ((x00 + x11) + x22)
            c_trans = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
            g = np.where(comparable, gap, 0)
            S = comparable & (c_rot <= rot_tab[g]) & (c_trans <= trans2_tab[g])                 # a NaN compares false
            if margins and comparable.any():
                for c, tab in ((c_rot, rot_tab[g]), (c_trans, trans2_tab[g])):
                    ok = comparable & np.isfinite(tab) & (tab > 0.0)
                    if ok.any():
                        margin = min(margin, float((np.abs(c[ok] - tab[ok]) / tab[ok]).min()))
    keep_v = np.ones(m, bool)                                                                   # 5. rounds
    s = np.zeros(m, np.int64)
    prev = keep_v
    for _ in range(rounds):
        prev = keep_v
        s = (S & prev[None, :]).sum(1)
        keep_v = prev & (s >= min_support)
    keep = np.zeros(EC, np.uint8)
    support = np.full(EC, -1, np.int32)
    keep[V] = keep_v
    support[V] = s
    kept = int(keep.sum())
    mp = np.where(keep != 0, np.cumsum(keep != 0) - 1, -1).astype(np.int32)                     # 6. copy
    over = int(log.state[1]) & LOG_OVERFLOW
    flags = (SRC_OVERFLOW if over else 0) | (UNSETTLED if (keep_v != prev).any() else 0)
    if dst is not None:
        rows = np.flatnonzero(keep)
        dst.edge_ij[:kept] = log.edge_ij[rows]
        dst.edge_Z[:kept] = log.edge_Z[rows]
        dst.edge_w[:kept] = log.edge_w[rows]
        dst.state[:] = (kept, over, 0, 0)
    out = dict(keep=keep, support=support, map=mp, info=np.array([m, kept, E, flags], np.int32))
    if margins:
        out["margin"] = margin
    return out


# ------------------------------------------------------------------------------------------------ committed cases
def _case(poses, n, node_capacity, edges, cap, max_gap, min_support, rounds, tabs=None, **extra):
    """edges: (i, j, Z [12], (w_rot, w_trans)); written into the log as they are (an add would refuse some of the invalid ones)"""
    log = pg.PoseGraphModel(cap)
    for e, (i, j, Z, w) in enumerate(edges):
        log.edge_ij[e] = (i, j); log.edge_Z[e] = Z; log.edge_w[e] = w
    log.state[0] = len(edges)
    buf = np.zeros((node_capacity, 12))
    buf[:len(poses)] = np.asarray(poses).reshape(-1, 12)[:node_capacity]
    rot_tab, trans2_tab = tabs if tabs is not None else default_tables(max_gap)
    return dict(poses=buf, n=n, node_capacity=node_capacity, log=log, cap=cap,
                gate=dict(max_gap=max_gap, min_support=min_support, rounds=rounds, rot_tab=np.asarray(rot_tab, np.float64),
                          trans2_tab=np.asarray(trans2_tab, np.float64)), **extra)


def run_case(case, dst_cap=None, **kw):
    """the restatement on a case -> (result dict, dst model)"""
    dst = pg.PoseGraphModel(dst_cap or case["cap"])
    prm = dict(case["gate"]); prm.update(kw)
    return gate(case["poses"], case["n"], case["log"], case["node_capacity"], dst=dst, **prm), dst


NOISE = dict(rot=0.004, trans=0.02)                                # odometry noise a keyframe of the noisy cases
W = (100.0, 10.0)


def _noisy_Z(gt, i, j, rng):
    d = np.concatenate([rng.normal(0.0, 0.002, 3), rng.normal(0.0, 0.01, 3)])
    return pg.update(pg.measure(gt, i, j).reshape(1, 12), d[None])[0].reshape(12)


SWEEP_EDGES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 513)         # 64: the LDS tile of a round; 256: a workgroup
SWEEP_SEED = 11


def sweep_case(E, n=40, cap=600, seed=SWEEP_SEED):
    """E closures between the two laps of an n-node noisy circle inside a 44-row pose buffer: i on the first lap, j near i + n / 2, most
    measured from ground truth with their own small noise, one in seven from a row 3 places off.  Gate: max_gap 6, min_support 2, 3 rounds."""
    N = 44
    gt = pg.circle_truth(N, 2, radius=20.0)
    poses = pg.noisy(gt, seed, **NOISE)
    rng = np.random.default_rng(1000 * seed + E + 7 * n)
    half = 20
    edges = []
    for e in range(E):
        i = int(rng.integers(0, half))
        j = min(i + half + int(rng.integers(-1, 2)), 39)
        src = min(i + 3, half - 1) if e % 7 == 3 else i
        edges.append((i, j, _noisy_Z(gt, src, j, rng), W))
    return _case(poses, n, N, edges, cap, 6, 2, 3)


def validity_case():
    """five true closures in a run and, between them, one edge each with i = -1, j = n, i == j, a NaN in Z, an Inf weight and a NaN in
    P_i - every one of them with the Z of a true closure next to the run, so that it would support its neighbours if it were counted"""
    n, N = 40, 44
    gt = pg.circle_truth(N, 2, radius=20.0)
    poses = pg.noisy(gt, 21, **NOISE).copy()
    rng = np.random.default_rng(2100)
    good = [(a, a + 20) for a in (6, 7, 8, 9, 10)]
    poses[12, 5] = np.nan                                            # node 12 is used by no good edge
    zn = _noisy_Z(gt, 8, 29, rng); zn[7] = np.nan
    bad = [(-1, 27, _noisy_Z(gt, 7, 27, rng), W), (8, n, _noisy_Z(gt, 8, 28, rng), W), (9, 9, _noisy_Z(gt, 9, 29, rng), W), (8, 29, zn, W),
           (9, 31, _noisy_Z(gt, 9, 31, rng), (np.inf, 1.0)), (12, 31, _noisy_Z(gt, 11, 31, rng), W)]
    edges = []
    for k, (i, j) in enumerate(good):
        edges.append((i, j, _noisy_Z(gt, i, j, rng), W))
        edges.append(bad[k])
    edges.append(bad[5])
    return _case(poses, n, N, edges, 16, 6, 2, 2, good_rows=list(range(0, 10, 2)), bad_rows=[1, 3, 5, 7, 9, 10])


def path_case(rounds):
    """the issue's path: edges (s, 100 + s), s = 0 .. 11, all from ground truth; only log neighbours are comparable (max_gap 2)"""
    N = 120
    gt = pg.circle_truth(N, 2, radius=30.0)
    edges = [(s, 100 + s, pg.measure(gt, s, 100 + s), (1.0, 1.0)) for s in range(12)]
    return _case(gt, N, N, edges, 16, 2, 2, rounds)


OUTLIER_SEED = 31


def outlier_case(seed=OUTLIER_SEED):
    """the 40-node two-lap circle with noisy poses: eight true closures in a run of consecutive keyframes (rows 5 .. 12 against 25 .. 32)
    and, between them in the log, three wrong ones - a true Z attached to a row 7 places off, a Z turned by 20 degrees, a Z shifted by 5 m"""
    n = 40
    gt = pg.circle_truth(n, 2, radius=20.0)
    poses = pg.noisy(gt, seed, **NOISE)
    rng = np.random.default_rng(seed + 100)
    true = [(a, a + 20, _noisy_Z(gt, a, a + 20, rng), W) for a in range(5, 13)]
    off = (7, 34, _noisy_Z(gt, 14, 34, rng), W)
    turned = (13, 33, pg.update(_noisy_Z(gt, 13, 33, rng).reshape(1, 12), np.array([[0.0, 0.0, np.radians(20.0), 0.0, 0.0, 0.0]]))[0].reshape(12), W)
    shifted_Z = _noisy_Z(gt, 4, 24, rng); shifted_Z[3] += 5.0
    shifted = (4, 24, shifted_Z, W)
    edges = true[:2] + [off] + true[2:5] + [turned] + true[5:7] + [shifted] + true[7:]
    return _case(poses, n, n, edges, 16, 8, 2, 8, gt=gt, true_rows=[0, 1, 3, 4, 5, 7, 8, 10], true_edges=true,
                 relax=dict(outer=10, inner=240, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0))


# ---- thresholds in exact arithmetic: identity and 90-degree rotations, integer translations, so every product is exact
RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
INF = np.inf


def _exact_poses(N=16):
    P = np.zeros((N, 3, 4))
    R = np.eye(3)
    for k in range(N):
        P[k, :, :3] = R
        P[k, :, 3] = (-3.0 * k, 2.0 * (k % 3), 1.0 * k)
        R = RZ90 @ R                                                 # (0 / +-1 entries: exact)
    return P


def _exact_Z(P, i, j, shift=(0.0, 0.0, 0.0), turn=False):
    Z = rmul(P[i], rinv(P[j]))
    if turn:
        Z = rmul(np.concatenate([RZ90, np.zeros((3, 1))], axis=1), Z)
    Z = Z.copy()
    Z[:, 3] += shift
    return Z.reshape(12)


def exact_cases():
    """name -> (case, expected support of the edges in log order); min_support 1, one round, so keep = support >= 1"""
    P = _exact_poses()
    one = (1.0, 1.0)
    a = (0, 10, _exact_Z(P, 0, 10), one)
    b_shift = (1, 11, _exact_Z(P, 1, 11, shift=(1.0, 2.0, 2.0)), one)            # c_trans = 9 exactly
    b_turn = (1, 11, _exact_Z(P, 1, 11, turn=True), one)                         # c_rot = 3 - 1 = 2 exactly
    b_both = (1, 11, _exact_Z(P, 1, 11, shift=(1.0, 2.0, 2.0), turn=True), one)
    z3, nine, two = np.zeros(3), np.full(3, 9.0), np.full(3, 2.0)
    mk = lambda edges, rot, tr: _case(P.reshape(-1, 12), 16, 16, edges, 8, 2, 1, 1, tabs=(rot, tr))
    out = {
        "trans_equal": (mk([a, b_shift], z3, nine), [1, 1]),
        "trans_one_ulp_lower": (mk([a, b_shift], z3, np.nextafter(nine, 0.0)), [0, 0]),
        "rot_equal": (mk([a, b_turn], two, np.full(3, INF)), [1, 1]),
        "rot_one_ulp_lower": (mk([a, b_turn], np.nextafter(two, 0.0), np.full(3, INF)), [0, 0]),
        "inf_switches_both_off": (mk([a, b_both], np.full(3, INF), np.full(3, INF)), [1, 1]),
        "inf_rot_only": (mk([a, b_both], np.full(3, INF), z3), [0, 0]),
        # all four agree exactly and both tables are 0: a-b has gap 2 = max_gap and counts; a-c, a-d, b-d have gap 3; b-c share j (gap 1)
        "gap_and_same_j": (mk([a, (1, 11, _exact_Z(P, 1, 11), one), (2, 11, _exact_Z(P, 2, 11), one), (0, 13, _exact_Z(P, 0, 13), one)], z3, z3),
                           [1, 1, 0, 0]),
    }
    return out
