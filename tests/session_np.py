"""The rule of the drive sessions (pr_session; the text of include/place_recognition.h) restated in NumPy, fp64
throughout: what the GPU tests compare session.hip with.  Conventions as for pr_posegraph and pr_gate: a pose is [R | t], 12 doubles
row-major, world to camera; a closure (i, j, Z) measures Z ~ P_i P_j^-1; products and inverses are gate_np's rmul / rinv, written out as
explicit scalar products in the stated order - (a0 b0 + a1 b1) + a2 b2 -, so everything up to the choice of a*, every hypothesis G_a and
every copied row is what the device leaves BYTE FOR BYTE.  The refinement (log_SO3, exp, the means) is posegraph_np's log_so3 / exp_so3
with sequential sums; the device sums by a tree and has its own sin / cos / atan2, so G and the moved rows are compared within a bound
that refine_mp (50 digits) measures on the restatement itself, never on the device.

    1. counts     E, n, S clamped before use; t = session, -1 means S - 1; t <= 0, t >= S or no row of t below n: NO_TARGET
    2. candidates valid by the relaxation's skip rule, exactly one end in t and the other in a session < t
    3. hypotheses j in t: G_a = (P_i^-1 Z_a) P_j;  i in t: G_a = (P_j^-1 Z_a^-1) P_i;  q_a the row in t, c_a = -(R^T t) of P_qa
    4. support    b supports a iff candidates, a != b, q_a != q_b, 3 - tr(R_Ga^T R_Gb) <= rot_c_max, |G_a c_b - G_b c_b|^2 <= trans2_max
    5. choice     a* = the largest support, ties to the lowest index; none: NO_CANDIDATE; support + 1 < min_inliers: WEAK
    6. refinement over I = {a*} + its supporters: R = R_Ga* exp(mean log_SO3(R_Ga*^T R_Gb)), t = mean(G_b c_b) - R mean(c_b)
    7. apply      every finite row of t becomes P_r G^-1, every other row < n keeps its bytes, rows >= n are not written
    8. outputs    hyp (zeros for a non-candidate), support (-1), inlier, info = {status, a* | -1, support, candidates, |I|, E, n, flags}

relax() is posegraph_np.relax with the odometry slots whose row s + 1 is a break removed from used_edges."""
import numpy as np

import gate_np as gn
import posegraph_np as pg

OVERFLOW, REUSED, LOG_OVERFLOW = 1, 2, 4
ALIGNED, NO_TARGET, NO_CANDIDATE, WEAK, NONFINITE = 0, 1, 2, 3, 4
MAX_SESSIONS = 1024
MARGIN = 100.0                                   # device bound = MARGIN x the restatement's own distance from the 50-digit evaluation
EPS = 2.0 ** -52


def scratch_bytes(nc, ec, sc):
    """the formula of the header"""
    if not (1 <= nc <= 1 << 20 and 1 <= ec <= 65536 and 1 <= sc <= MAX_SESSIONS):
        return 0
    r = lambda b: (b + 15) & ~15
    return (2 * r(4 * nc) + 2 * r(4 * ec) + r(96 * ec) + 2 * r(24 * ec) + 2 * r(4 * ec) + 192 + 48) + \
           (96 + r(96 * ec) + r(4 * ec) + r(ec) + 32 + 16)


# ------------------------------------------------------------------------------------------------ the table
class SessionModel:
    """the two buffers and the begin rule"""

    def __init__(self, node_capacity, session_capacity):
        self.nc, self.cap = int(node_capacity), int(session_capacity)
        self.start = np.zeros(self.cap, np.int32)
        self.state = np.array([1, 0, 0, 0], np.int32)

    def reset(self):
        self.start[0] = 0
        self.state[:] = (1, 0, 0, 0)

    @property
    def S(self):
        return min(max(int(self.state[0]), 1), self.cap)

    def sid(self, r):
        """#{q in 1 .. S-1 : start[q] <= r}: a count, defined for any start"""
        r = np.asarray(r, np.int64)
        st = self.start[1:self.S].astype(np.int64)
        return (st[None, :] <= r.reshape(-1, 1)).sum(1).reshape(r.shape).astype(np.int64)

    def breaks(self, rows):
        """bool [rows]: row r >= 1 is a break iff sid(r) != sid(r - 1)"""
        s = self.sid(np.arange(rows))
        b = np.zeros(rows, bool)
        b[1:] = s[1:] != s[:-1]
        return b

    def begin(self, n):
        S = self.S
        n = min(max(int(n), 0), self.nc)
        flags = int(self.state[1]) & OVERFLOW
        last = int(self.start[S - 1]) if S > 1 else 0
        if n == last:
            return np.array([S - 1, last, S, flags | REUSED], np.int32)
        if S == self.cap:
            flags |= OVERFLOW
            self.state[1] = flags
            return np.array([S - 1, last, S, flags], np.int32)
        self.start[S] = n
        self.state[0] = S + 1
        return np.array([S, n, S + 1, flags], np.int32)


def thresholds(rot_deg=3.0, trans=1.0):
    """(rot_c_max, trans2_max) of the Python class's defaults"""
    return 2.0 * (1.0 - float(np.cos(np.radians(float(rot_deg))))), float(trans) ** 2


# ------------------------------------------------------------------------------------------------ the alignment
def _support_matrix(G, c, p, q, rot_c_max, trans2_max):
    """S[a, b]: b supports a, over the candidates; and the smallest relative distance of a c_rot / c_trans from its threshold"""
    m = len(G)
    Ra, Rb = G[:, None, :, :3], G[None, :, :, :3]
    x = [(Ra[..., 0, k] * Rb[..., 0, k] + Ra[..., 1, k] * Rb[..., 1, k]) + Ra[..., 2, k] * Rb[..., 2, k] for k in range(3)]
    c_rot = 3.0 - ((x[0] + x[1]) + x[2])
    d = (gn.mv3(Ra, np.broadcast_to(c[None, :, :], (m, m, 3))) + G[:, None, :, 3]) - p[None, :, :]
    c_trans = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    comparable = (q[:, None] != q[None, :]) & ~np.eye(m, dtype=bool)
    S = comparable & (c_rot <= rot_c_max) & (c_trans <= trans2_max)                             # a NaN compares false
    margin = np.inf
    for v, thr in ((c_rot, rot_c_max), (c_trans, trans2_max)):
        if comparable.any() and np.isfinite(thr) and thr > 0.0:
            margin = min(margin, float((np.abs(v[comparable] - thr) / thr).min()))
    return S, margin


def refine(Gs, GI, cI, pI):
    """step 6 in fp64: Gs = G_a* [3, 4]; GI [k, 3, 4], cI, pI [k, 3] of the members of I in log order -> G [3, 4]"""
    k = len(GI)
    RE = gn.mul33(np.ascontiguousarray(np.swapaxes(Gs[None, :, :3], -1, -2)), GI[:, :, :3])
    phi, _ = pg.log_so3(RE)
    seq = lambda v: np.cumsum(v, axis=0)[-1]                                                    # sequential, in log order
    w, mp_, mc = seq(phi) / float(k), seq(pI) / float(k), seq(cI) / float(k)
    R = gn.mul33(Gs[:, :3], pg.exp_so3(w))
    t = mp_ - gn.mv3(R, mc)
    return np.concatenate([R, t[:, None]], axis=1)


def refine_mp(Gs, GI, cI, pI, dps=50):
    """step 6 with 50 digits from the same fp64 hypotheses (exact log and exp: no small-angle series) -> G [3, 4] rounded to fp64"""
    import mpmath as mp
    with mp.workdps(dps):
        M = lambda A: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(A)])
        Rs = M(Gs[:, :3])
        acc, sp, sc = mp.zeros(3, 1), mp.zeros(3, 1), mp.zeros(3, 1)
        for Gb, cb, pb in zip(GI, cI, pI):
            RE = Rs.T * M(Gb[:, :3])
            v = mp.matrix([(RE[2, 1] - RE[1, 2]) / 2, (RE[0, 2] - RE[2, 0]) / 2, (RE[1, 0] - RE[0, 1]) / 2])
            sn = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
            th = mp.atan2(sn, (RE[0, 0] + RE[1, 1] + RE[2, 2] - 1) / 2)
            acc += (th / sn if sn != 0 else mp.mpf(1)) * v
            sp += mp.matrix([mp.mpf(float(x)) for x in pb]); sc += mp.matrix([mp.mpf(float(x)) for x in cb])
        k = mp.mpf(len(GI))
        w, mpp, mcc = acc / k, sp / k, sc / k
        th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
        K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Ex = mp.eye(3) + ((mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K) if th != 0 else mp.zeros(3))
        R = Rs * Ex
        t = mpp - R * mcc
        return np.array([[float(R[r, c]) for c in range(3)] + [float(t[r])] for r in range(3)])


def apply_mp(P, G, dps=50):
    """P G^-1 with 50 digits, rounded to fp64: P [k, 3, 4], G [3, 4]"""
    import mpmath as mp
    with mp.workdps(dps):
        M = lambda A: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(A)])
        Rg, tg = M(G[:, :3]), M(G[:, 3:])
        Ri, ti = Rg.T, -(Rg.T * tg)
        out = np.empty((len(P), 3, 4))
        for k, Pk in enumerate(P):
            R, t = M(Pk[:, :3]), M(Pk[:, 3:])
            Rn, tn = R * Ri, R * ti + t
            out[k] = [[float(Rn[r, c]) for c in range(3)] + [float(tn[r])] for r in range(3)]
        return out


def align(model, poses, n, log, edge_capacity, session=-1, min_inliers=3, rot_c_max=None, trans2_max=None, margins=False, exact=False):
    """model: a SessionModel; log: a PoseGraphModel (its capacity is log_edge_capacity <= edge_capacity).  -> dict(poses [N, 12] - rows
    >= n untouched -, G [12], hyp [EC, 12], support i32 [EC], inlier u8 [EC], info i32 [8]); margins=True adds `margin`, the smallest
    relative distance of a compared c_rot / c_trans from its threshold; exact=True adds G_mp and poses_mp, step 6 and 7 with 50 digits."""
    d0 = thresholds()
    rot_c_max = d0[0] if rot_c_max is None else float(rot_c_max)
    trans2_max = d0[1] if trans2_max is None else float(trans2_max)
    EC = int(edge_capacity)
    poses = np.array(poses, np.float64).reshape(-1, 12)
    out = poses.copy()
    n = min(max(int(n), 0), model.nc)                                                           # 1. counts
    E = min(max(int(log.state[0]), 0), log.cap)
    S = model.S
    t = S - 1 if session == -1 else int(session)
    flags = (int(model.state[1]) & OVERFLOW) | (LOG_OVERFLOW if int(log.state[1]) & pg.OVERFLOW else 0)
    hyp, support, inlier = np.zeros((EC, 12)), np.full(EC, -1, np.int32), np.zeros(EC, np.uint8)
    ident = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    res = dict(poses=out, G=ident, hyp=hyp, support=support, inlier=inlier)
    if margins:
        res["margin"] = np.inf
    sid_rows = model.sid(np.arange(n))
    in_t = sid_rows == t
    if t <= 0 or t >= S or not in_t.any():
        res["info"] = np.array([NO_TARGET, -1, 0, 0, 0, E, n, flags], np.int32)
        return res
    ij = log.edge_ij[:E].astype(np.int64)                                                       # 2. candidates
    i, j = ij[:, 0], ij[:, 1]
    valid = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j)
    valid &= np.isfinite(log.edge_Z[:E]).all(1) & np.isfinite(log.edge_w[:E]).all(1)
    ic, jc = np.where(valid, i, 0), np.where(valid, j, 0)
    fin = np.isfinite(poses).all(1)
    valid &= fin[ic] & fin[jc]
    si, sj = model.sid(ic), model.sid(jc)
    j_in_t = valid & (sj == t) & (si < t)
    i_in_t = valid & (si == t) & (sj < t)
    V = np.flatnonzero(j_in_t | i_in_t)
    m = len(V)
    if m == 0:
        res["info"] = np.array([NO_CANDIDATE, -1, 0, 0, 0, E, n, flags], np.int32)
        return res
    with np.errstate(all="ignore"):
        Z = log.edge_Z[V].reshape(m, 3, 4)                                                      # 3. hypotheses
        Pi, Pj = poses[i[V]].reshape(m, 3, 4), poses[j[V]].reshape(m, 3, 4)
        jt = j_in_t[V]
        G = np.where(jt[:, None, None], gn.rmul(gn.rmul(gn.rinv(Pi), Z), Pj), gn.rmul(gn.rmul(gn.rinv(Pj), gn.rinv(Z)), Pi))
        q = np.where(jt, j[V], i[V])
        c = gn.rinv(poses[q].reshape(m, 3, 4))[..., 3]
        p = gn.mv3(G[..., :3], c) + G[..., 3]
        Sm, margin = _support_matrix(G, c, p, q, rot_c_max, trans2_max)                         # 4. support
    sup = Sm.sum(1)
    hyp[V] = G.reshape(m, 12)
    support[V] = sup
    best = int(np.argmax(sup))                                                                  # 5. choice: the first of the largest
    members = np.flatnonzero(Sm[best] | (np.arange(m) == best))
    inlier[V[members]] = 1
    if margins:
        res["margin"] = margin
    status = WEAK if int(sup[best]) + 1 < int(min_inliers) else ALIGNED
    Gr = None
    if status == ALIGNED:
        with np.errstate(all="ignore"):
            Gr = refine(G[best], G[members], c[members], p[members])                            # 6. refinement
        if not np.isfinite(Gr).all():
            status, Gr = NONFINITE, None
    res["info"] = np.array([status, V[best], sup[best], m, len(members), E, n, flags], np.int32)
    if Gr is None:
        return res
    res["G"] = Gr.reshape(12)
    rows = np.flatnonzero(in_t & fin[:n])                                                       # 7. apply
    out[rows] = gn.rmul(poses[rows].reshape(-1, 3, 4), gn.rinv(Gr)).reshape(-1, 12)
    if exact:
        Gm = refine_mp(G[best], G[members], c[members], p[members])
        pm = poses.copy()
        pm[rows] = apply_mp(poses[rows].reshape(-1, 3, 4), Gm).reshape(-1, 12)
        res["G_mp"], res["poses_mp"], res["rows"] = Gm.reshape(12), pm, rows
    return res


def device_bound(res):
    """(bound on |G - G_device|, bound on |moved rows - device rows|) from a result of align(exact=True): MARGIN x the restatement's own
    distance from the 50-digit evaluation, floored at MARGIN roundings of the largest entry compared"""
    if "G_mp" not in res:
        return 0.0, 0.0
    rows = res["rows"]
    dG = float(np.abs(res["G"] - res["G_mp"]).max())
    dP = float(np.abs(res["poses"][rows] - res["poses_mp"][rows]).max(initial=0.0))
    fG = EPS * max(1.0, float(np.abs(res["G_mp"]).max()))
    fP = EPS * max(1.0, float(np.abs(res["poses_mp"][rows]).max(initial=0.0)))
    return MARGIN * max(dG, fG), MARGIN * max(dP, fP)


# ------------------------------------------------------------------------------------------------ the relaxation across breaks
def used_edges(model, poses, n, edge_ij, edge_Z, edge_w, edges, w_odo_rot, w_odo_trans, base=None):
    """posegraph_np.used_edges without the odometry slots s whose row s + 1 is a break"""
    I, J, Z, W, logged = (base or pg.used_edges)(poses, n, edge_ij, edge_Z, edge_w, edges, w_odo_rot, w_odo_trans)
    brk = model.breaks(max(int(n), 1))
    odo = len(I) - logged
    keep = np.ones(len(I), bool)
    keep[:odo] = ~brk[J[:odo]]
    return I[keep], J[keep], Z[keep], W[keep], logged


def relax(model, poses, n, edge_ij, edge_Z, edge_w, edges, **kw):
    """posegraph_np.relax over used_edges above (the module's function is swapped for the call)"""
    orig = pg.used_edges
    pg.used_edges = lambda *a: used_edges(model, *a, base=orig)
    try:
        return pg.relax(poses, n, edge_ij, edge_Z, edge_w, edges, **kw)
    finally:
        pg.used_edges = orig


# ------------------------------------------------------------------------------------------------ committed cases
ODO = dict(rot=1e-4, trans=1e-3)                 # odometry noise a keyframe of the cases: a twentieth of the closures' (2e-3 rad, 1e-2 m),
#                                                  because a drive that drifts has no single transform onto another drive - G_true would
#                                                  be defined only to the drift
W = gn.W
ROT_NOISE, TRANS_NOISE = 0.002, 0.01             # gate_np._noisy_Z's sigmas


def frame(k):
    """the known transform of session k's world frame into session 0's: a rotation of about 2 rad and tens of metres"""
    if k == 0:
        return np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    w = np.array([0.3 + 0.1 * k, -0.4, 1.93 - 0.05 * k])
    return np.concatenate([pg.exp_so3(w), np.array([[35.0 + 3 * k], [-22.0 - k], [4.0]])], axis=1)


def _log(edges, cap):
    log = pg.PoseGraphModel(cap)
    for e, (i, j, Z, w) in enumerate(edges):
        log.edge_ij[e] = (i, j); log.edge_Z[e] = Z; log.edge_w[e] = w
    log.state[0] = len(edges)
    return log


def drives(gt, starts, n, seed, noise):
    """the rows [starts[k], starts[k + 1]) of gt as session k in its own frame: P' = P G_k, with seeded odometry noise per session"""
    N = len(gt)
    P = pg.as34(gt)
    out = np.zeros((N, 12))
    ends = list(starts[1:]) + [n]
    for k, (a, b) in enumerate(zip(starts, ends)):
        if b <= a:
            continue
        own = pg.mul(P[a:b], frame(k)).reshape(b - a, 12)
        out[a:b] = pg.noisy(own, seed + 17 * k, **noise) if noise else own
    out[n:] = gt[n:]
    return out


SWEEP_CANDIDATES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)      # 64: the LDS tile of the pairs kernel; 256: a workgroup; 513: grid.y
SWEEP_STARTS = {1: [0], 2: [0, 20], 3: [0, 14, 27], 5: [0, 8, 16, 24, 32]}


def sweep_case(C, S=2, target=-1, seed=3, cap=800, session_capacity=None, one_q=False, rows=(44, 40), starts=None):
    """C candidates between session `target` and the earlier sessions of 40 rows in a 44-row buffer, both orientations, one in seven
    measured from a row 3 places off; between them edges that are no candidates: inside one session, to a later session, with a NaN in Z,
    with a row >= n.  one_q: every candidate ends in the same row of the target."""
    N, n = rows                                                         # (rows beyond 256: more than one workgroup of row lanes)
    starts = list(starts or SWEEP_STARTS[S])
    t = S - 1 if target == -1 else target
    gt = pg.circle_truth(N, 2, radius=20.0)
    poses = drives(gt, starts, n, seed, ODO)
    model = SessionModel(N, session_capacity or max(S, 2))
    for k in range(1, S):
        model.begin(starts[k])
    rng = np.random.default_rng(1000 * seed + C + 7 * S + t)
    ends = starts[1:] + [n]
    edges = []
    if 0 < t < S:
        lo, hi = starts[t], ends[t]
        for e in range(C):
            i = int(rng.integers(0, lo))
            j = lo if one_q else int(rng.integers(lo, hi))
            src = (i + 3) % lo if e % 7 == 3 else i
            Z = gn._noisy_Z(gt, src, j, rng)
            edges.append((j, i, gn.rinv(Z.reshape(3, 4)).reshape(12), W) if e % 2 else (i, j, Z, W))
            if e % 4 == 1:                                               # a non-candidate between the candidates
                kind = (e // 4) % 4
                if kind == 0:
                    a, b = sorted(int(x) for x in rng.choice(np.arange(lo, hi), 2, replace=False)) if hi - lo >= 2 else (0, 1)
                    edges.append((a, b, gn._noisy_Z(gt, a, b, rng), W))                          # inside one session
                elif kind == 1 and t + 1 < S:
                    b = int(rng.integers(starts[t + 1], n))
                    edges.append((j, b, gn._noisy_Z(gt, j, b, rng), W))                          # to a later session
                elif kind == 2:
                    Zn = gn._noisy_Z(gt, i, j, rng); Zn[5] = np.nan
                    edges.append((i, j, Zn, W))
                else:
                    edges.append((i, n + 1, gn._noisy_Z(gt, i, n + 1, rng), W))                  # a row >= n
    edges += [(1, 2, gn._noisy_Z(gt, 1, 2, rng), W), (3, 3, gn._noisy_Z(gt, 3, 4, rng), W), (-1, 5, gn._noisy_Z(gt, 0, 5, rng), W)]
    assert len(edges) <= cap
    return dict(poses=poses, n=n, node_capacity=N, model=model, log=_log(edges, cap), cap=cap, gt=gt, starts=starts, target=target,
                align=dict(session=target, min_inliers=3))


def run_case(case, **kw):
    prm = dict(case["align"]); prm.update(kw)
    return align(case["model"], case["poses"], case["n"], case["log"], case["cap"], **prm)


# ---- thresholds in exact arithmetic: identity and 90-degree rotations, integer translations, so every product is exact
def exact_cases():
    """name -> (case, expected support of the two candidates); min_inliers 1"""
    P = gn._exact_poses()                                               # [16, 3, 4]
    Gt = np.concatenate([gn.RZ90 @ gn.RZ90 @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]), np.array([[30.0], [-20.0], [4.0]])], axis=1)
    poses = P.copy()
    poses[8:] = gn.rmul(P[8:], Gt)                                      # session 1 = rows 8 .. 15 in its own frame (exact)
    one = (1.0, 1.0)
    a = (0, 10, gn._exact_Z(P, 0, 10), one)
    b_shift = (1, 11, gn._exact_Z(P, 1, 11, shift=(1.0, 2.0, 2.0)), one)          # c_trans = 9 exactly
    b_turn = (1, 11, gn._exact_Z(P, 1, 11, turn=True), one)                       # c_rot = 3 - 1 = 2 exactly
    flip = lambda e: (e[1], e[0], gn.rinv(e[2].reshape(3, 4)).reshape(12), e[3])  # the other orientation (exact too)
    INF = np.inf

    def mk(edges, rot, tr):
        model = SessionModel(16, 2)
        model.begin(8)
        return dict(poses=poses.reshape(16, 12), n=16, node_capacity=16, model=model, log=_log(edges, 8), cap=8, Gt=Gt,
                    align=dict(session=-1, min_inliers=1, rot_c_max=rot, trans2_max=tr))
    return {
        "trans_equal": (mk([a, b_shift], 0.0, 9.0), [1, 1]),
        "trans_one_ulp_lower": (mk([a, b_shift], 0.0, float(np.nextafter(9.0, 0.0))), [0, 0]),
        "rot_equal": (mk([a, b_turn], 2.0, INF), [1, 1]),
        "rot_one_ulp_lower": (mk([a, b_turn], float(np.nextafter(2.0, 0.0)), INF), [0, 0]),
        "inf_switches_both_off": (mk([a, flip(b_turn)], INF, INF), [1, 1]),
        "flipped_trans_equal": (mk([flip(a), b_shift], 0.0, 9.0), [1, 1]),
        "same_q": (mk([a, (2, 10, gn._exact_Z(P, 2, 10), one)], INF, INF), [0, 0]),
    }


def tie_case():
    """two consensus groups of two closures each, noise-free, 9 m apart: every support is 1.  The group at the HIGHER log rows (513, 514)
    is met first by a walk over lanes (rows 513 and 514 belong to lanes 1 and 2 of a 256-lane stride, rows 300 and 301 to lanes 44 and
    45), so the tie rule - the lowest log index, 300 - has to hold across lanes, not only inside one."""
    N, n = 44, 40
    gt = pg.circle_truth(N, 2, radius=20.0)
    poses = drives(gt, [0, 20], n, 0, None)
    model = SessionModel(N, 2)
    model.begin(20)
    Gs = frame(1).copy(); Gs[0, 3] += 9.0
    shifted = lambda i, j: pg.mul(pg.mul(pg.as34(gt[i]), Gs), pg.inv(pg.as34(poses[j]))).reshape(12)
    filler = (1, 2, pg.measure(gt, 1, 2), W)                           # inside session 0: no candidate
    edges = [filler] * 300 + [(3, 25, pg.measure(gt, 3, 25), W), (4, 26, pg.measure(gt, 4, 26), W)] + [filler] * 211 + \
            [(5, 30, shifted(5, 30), W), (6, 31, shifted(6, 31), W)]
    return dict(poses=poses, n=n, node_capacity=N, model=model, log=_log(edges, 800), cap=800, gt=gt, align=dict(session=-1, min_inliers=2))


def nonfinite_case():
    """two candidates whose hypotheses are finite but whose transported centres (about -1.2e308 each) overflow in the refinement's sum:
    PR_SESSION_NONFINITE, the poses copied, G the identity; both thresholds +Inf, so the two support each other"""
    P = gn._exact_poses()
    poses = P.copy()
    poses[0, :, :3] = np.eye(3); poses[1, :, :3] = np.eye(3)
    poses[0, :, 3] = (1.2e308, 0.0, 0.0); poses[1, :, 3] = (1.2e308, 1.0, 0.0)
    Z = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12)
    model = SessionModel(16, 2)
    model.begin(8)
    return dict(poses=poses.reshape(16, 12), n=16, node_capacity=16, model=model, log=_log([(0, 10, Z, W), (1, 11, Z, W)], 8), cap=8,
                align=dict(session=-1, min_inliers=1, rot_c_max=np.inf, trans2_max=np.inf))


# ---- the two-drive scene
SCENE_SEED = 5
SCENE_ROWS = 80
SCENE_GATE = dict(max_gap=8, min_support=2, rounds=8)
SCENE_RELAX = dict(outer=6, inner=240, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
SCENE_G_ROT = 3.0 * ROT_NOISE                    # G_true is recovered within 3 x the planted measurement noise: the angle of
SCENE_G_TRANS = 3.0 * TRANS_NOISE                # G_true^-1 G, and |G c - G_true c| at the inliers' mean camera centre
# every row after align -> gate -> session relax: an alignment error of 3 sigma in rotation seen from the closures at the far side of the
# lap (its diameter, 40 m) plus 3 sigma in translation
SCENE_ROW_BOUND = 3.0 * ROT_NOISE * 40.0 + 3.0 * TRANS_NOISE


def scene(seed=SCENE_SEED, noise=True):
    """one lap of posegraph_np.circle_truth as session 0 and the second lap as session 1 in the frame frame(1); odometry noise ODO; 12
    closures of consecutive keyframes (rows 4 .. 15 against 44 .. 55) with gate_np._noisy_Z's noise, three of them planted outliers - a
    true Z attached to a row 7 places off, a Z turned by 20 degrees, a Z shifted by 5 m."""
    N = SCENE_ROWS
    gt = pg.circle_truth(N, 2, radius=20.0)
    poses = drives(gt, [0, 40], N, seed, ODO if noise else None)
    rng = np.random.default_rng(seed + 100)
    Zof = (lambda i, j: gn._noisy_Z(gt, i, j, rng)) if noise else (lambda i, j: pg.measure(gt, i, j))
    true = {a: (a, a + 40, Zof(a, a + 40), W) for a in range(4, 16)}
    edges, outliers = [], [2, 6, 9]
    for k, a in enumerate(range(4, 16)):
        if k == 2:
            edges.append((a, a + 40, Zof(a + 7, a + 40), W))
        elif k == 6:
            edges.append((a, a + 40, pg.update(true[a][2].reshape(1, 12), np.array([[0.0, 0.0, np.radians(20.0), 0.0, 0.0, 0.0]]))[0].reshape(12), W))
        elif k == 9:
            Zs = true[a][2].copy(); Zs[3] += 5.0
            edges.append((a, a + 40, Zs, W))
        else:
            edges.append(true[a])
    model = SessionModel(N, 4)
    model.begin(40)
    return dict(poses=poses, n=N, node_capacity=N, model=model, log=_log(edges, 16), cap=16, gt=gt, Gt=frame(1),
                true_rows=[k for k in range(12) if k not in outliers], align=dict(session=-1, min_inliers=3))


def centres(P):
    """camera centres -(R^T t) of poses [k, 12]"""
    return gn.rinv(np.asarray(P, np.float64).reshape(-1, 3, 4))[..., 3]


def scene_chain(c):
    """the restatement of align -> gate -> relax across breaks on a scene -> (align result, gate result, relaxed poses, report)"""
    a = align(c["model"], c["poses"], c["n"], c["log"], c["cap"], margins=True, **c["align"])
    rot_tab, trans2_tab = gn.default_tables(SCENE_GATE["max_gap"])
    dst = pg.PoseGraphModel(c["cap"])
    g = gn.gate(a["poses"], c["n"], c["log"], c["node_capacity"], rot_tab=rot_tab, trans2_tab=trans2_tab, dst=dst, margins=True, **SCENE_GATE)
    out, rep = relax(c["model"], a["poses"], c["n"], dst.edge_ij, dst.edge_Z, dst.edge_w, dst.state[0], **SCENE_RELAX)
    return a, g, dst, out, rep
