"""NumPy restatement of the trajectory evaluation (pr_trajeval; the rule of include/place_recognition.h), operation by
operation: the same products, the same association, the same tree for every sum, the Jacobi rotation by rotation in Python floats.  NumPy's
elementwise + - x / sqrt are IEEE operations without contraction, so apart from atan2 the device must return these bytes.

evaluate() returns the arrays of pr_trajeval_out under the same names, and under "aux" the rotation matrices E that every theta was taken
from, so that a test can bound the one libm call (theta_tol)."""
import math

import numpy as np

T = 256
SWEEPS = 10
NONE, FIRST, SE3, SIM3 = 0, 1, 2, 3
W2C, C2W, POSITIONS = 0, 1, 2
FEW, DEGENERATE, NO_SCALE = 1, 2, 4
ALIGN = dict(none=NONE, first=FIRST, se3=SE3, sim3=SIM3)
GT = dict(w2c=W2C, c2w=C2W, positions=POSITIONS)
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the tree and the 3 x 3 helpers
def tree_sum(x):
    """the sum over axis 0 of the rule's tree: lane t adds terms t, t + 256, .. in order to +0.0, then the lanes are folded by halving"""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    C = -(-M // T)
    pad = np.zeros((max(C, 1) * T,) + x.shape[1:])
    pad[:M] = x
    lanes = np.zeros((T,) + x.shape[1:])
    for c in range(C):
        lanes = lanes + pad[c * T:(c + 1) * T]
    s = T // 2
    while s:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return lanes[0]


def mul33(A, B):
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def mv3(A, x):
    return (A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1]) + A[..., :, 2] * x[..., None, 2]


def mtv3(A, x):
    return (A[..., 0, :] * x[..., 0, None] + A[..., 1, :] * x[..., 1, None]) + A[..., 2, :] * x[..., 2, None]


def split(p):
    p = np.asarray(p, np.float64).reshape(p.shape[:-1] + (3, 4))
    return p[..., :3], p[..., 3]


def rigid_mul(RA, tA, RB, tB):
    return mul33(RA, RB), mv3(RA, tB) + tA


def rigid_inv(R, t):
    return np.swapaxes(R, -1, -2), -mtv3(R, t)


def norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def gt_rel(gt, gt_kind, i, j):
    Ri, ti = split(gt[i])
    Rj, tj = split(gt[j])
    if gt_kind == W2C:
        return rigid_mul(Ri, ti, *rigid_inv(Rj, tj))
    return rigid_mul(*rigid_inv(Ri, ti), Rj, tj)


def rel_error(RA, tA, RQ, tQ):
    """E = A^-1 Q -> (c_rot, theta, d, R_E)"""
    RE, tE = rigid_mul(*rigid_inv(RA, tA), RQ, tQ)
    tr = (RE[..., 0, 0] + RE[..., 1, 1]) + RE[..., 2, 2]
    v = np.stack([0.5 * (RE[..., 2, 1] - RE[..., 1, 2]), 0.5 * (RE[..., 0, 2] - RE[..., 2, 0]), 0.5 * (RE[..., 1, 0] - RE[..., 0, 1])], -1)
    return 3.0 - tr, np.arctan2(norm3(v), 0.5 * (tr - 1.0)), norm3(tE), RE


def pair_error(est_b, gt, gt_kind, i, j, s):
    Ri, ti = split(est_b[i])
    Rj, tj = split(est_b[j])
    RQ, tQ = rigid_mul(Ri, ti, *rigid_inv(Rj, tj))
    tQ = s * tQ
    return rel_error(*gt_rel(gt, gt_kind, i, j), RQ, tQ)


def theta_mp(RE):
    """theta of the rule from the fp64 entries of R_E in 50-digit arithmetic (what the libm call and the three roundings in front of it
    are measured against)"""
    import mpmath
    RE = np.asarray(RE, np.float64).reshape(-1, 3, 3)
    out = np.zeros(len(RE))
    with mpmath.workdps(50):
        for k, E in enumerate(RE):
            m = [[mpmath.mpf(float(x)) for x in r] for r in E]
            v = [(m[2][1] - m[1][2]) / 2, (m[0][2] - m[2][0]) / 2, (m[1][0] - m[0][1]) / 2]
            tr = m[0][0] + m[1][1] + m[2][2]
            out[k] = float(mpmath.atan2(mpmath.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), (tr - 1) / 2))
    return out


def theta_tol(RE, theta):
    """the bound of one theta: 100 x |restatement - 50-digit evaluation| over the thetas of this case, floored at 100 roundings of the
    largest; taken when the test runs, never from the device.  A mean, a maximum and an rmse of values each moved by at most tol move by
    at most tol (plus the sums' own rounding, which the restatement shares bit for bit)."""
    theta = np.asarray(theta, np.float64).reshape(-1)
    if theta.size == 0:
        return 0.0
    d = np.abs(theta - theta_mp(RE))
    return max(100.0 * float(d.max()), 100.0 * (EPS / 2) * float(np.abs(theta).max()))


# ------------------------------------------------------------------------------------------------ Umeyama's rotation, in Python floats
def umeyama_rot(A):
    """A [3][3] -> (R [3][3], sigma [3], deg, dsign) by the header's fixed-sweep one-sided Jacobi"""
    A = [[float(A[a][b]) for b in range(3)] for a in range(3)]
    hmax = 0.0
    for a in range(3):
        for b in range(3):
            hmax = max(hmax, abs(A[a][b])) if not math.isnan(A[a][b]) else hmax
    R = [[1.0 if a == b else 0.0 for b in range(3)] for a in range(3)]
    if not (hmax > 0.0) or not math.isfinite(hmax):
        return R, [0.0, 0.0, 0.0], 1, 1.0
    G = [[A[a][b] / hmax for b in range(3)] for a in range(3)]
    V = [[1.0 if a == b else 0.0 for b in range(3)] for a in range(3)]
    sweep = 0
    while True:
        W = [[(G[a][0] * V[0][k] + G[a][1] * V[1][k]) + G[a][2] * V[2][k] for k in range(3)] for a in range(3)]
        if sweep == SWEEPS:
            break
        sweep += 1
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = (W[0][p] * W[0][p] + W[1][p] * W[1][p]) + W[2][p] * W[2][p]
            be = (W[0][q] * W[0][q] + W[1][q] * W[1][q]) + W[2][q] * W[2][q]
            ga = (W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q]
            if not (ga * ga > 1e-31 * (al * be)):
                continue
            zeta = (be - al) / (2.0 * ga)
            t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(zeta * zeta + 1.0))
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            for a in range(3):
                x, y, vx, vy = W[a][p], W[a][q], V[a][p], V[a][q]
                W[a][p] = cs * x - sn * y
                W[a][q] = sn * x + cs * y
                V[a][p] = cs * vx - sn * vy
                V[a][q] = sn * vx + cs * vy
    w = [[W[a][k] for a in range(3)] for k in range(3)]
    vv = [[V[a][k] for a in range(3)] for k in range(3)]
    m = [(w[k][0] * w[k][0] + w[k][1] * w[k][1]) + w[k][2] * w[k][2] for k in range(3)]
    for j, k in ((0, 1), (1, 2), (0, 1)):
        if m[j] < m[k]:
            w[j], w[k] = w[k], w[j]
            vv[j], vv[k] = vv[k], vv[j]
            m[j], m[k] = m[k], m[j]
    n1, n2, n3 = math.sqrt(m[0]), math.sqrt(m[1]), math.sqrt(m[2])
    sig = [n1 * hmax, n2 * hmax, n3 * hmax]
    deg = 0 if n2 > 1e-12 * n1 else 1
    u0 = [w[0][a] / n1 for a in range(3)]
    if not deg:
        u1 = list(w[1])
    else:
        k = 0
        if abs(u0[1]) < abs(u0[k]):
            k = 1
        if abs(u0[2]) < abs(u0[k]):
            k = 2
        u1 = [1.0 if a == k else 0.0 for a in range(3)]
    dot = (u1[0] * u0[0] + u1[1] * u0[1]) + u1[2] * u0[2]
    u1 = [u1[a] - dot * u0[a] for a in range(3)]
    m2 = math.sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2])
    u1 = [u1[a] / m2 for a in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    u2 = cross(u0, u1)
    v3 = cross(vv[0], vv[1])
    m3 = math.sqrt((v3[0] * v3[0] + v3[1] * v3[1]) + v3[2] * v3[2])
    v3 = [v3[a] / m3 for a in range(3)]
    dsign = 1.0
    if not deg:
        pu = (u2[0] * w[2][0] + u2[1] * w[2][1]) + u2[2] * w[2][2]
        pv = (v3[0] * vv[2][0] + v3[1] * vv[2][1]) + v3[2] * vv[2][2]
        dsign = -1.0 if pu * pv < 0.0 else 1.0
    R = [[(u0[a] * vv[0][b] + u1[a] * vv[1][b]) + u2[a] * v3[b] for b in range(3)] for a in range(3)]
    return R, sig, deg, dsign


# ------------------------------------------------------------------------------------------------ the prefixes and the segment search
def blocked_prefix(steps, cap):
    """dist[i] of the rule from the per-row additions (0 for a row that adds nothing): T blocks of C rows"""
    C = -(-cap // T)
    pad = np.zeros(T * C)
    pad[:cap] = steps
    w = np.cumsum(pad.reshape(T, C), axis=1)                       # a running sum in row order (np.add.accumulate is sequential)
    base = np.zeros(T)
    for t in range(1, T):
        base[t] = base[t - 1] + w[t - 1, C - 1]
    return (base[:, None] + w).reshape(-1)[:cap]


def path_steps(cen, used):
    """|c_i - c_prev used| per used row with a used row before it, else 0"""
    steps = np.zeros(len(cen))
    rows = np.flatnonzero(used)
    if len(rows) > 1:
        steps[rows[1:]] = norm3(cen[rows[1:]] - cen[rows[:-1]])
    return steps


def segment_end(dist, n, f, length):
    """the first row j > f, j < n, with dist[j] > dist[f] + length, or n: the device's binary search"""
    return int(np.searchsorted(dist[:n], dist[f] + length, side="right"))


def segment_end_scan(dist, n, f, length):
    """the same by the rule's own words: a linear scan"""
    target = dist[f] + length
    for j in range(f + 1, n):
        if dist[j] > target:
            return j
    return n


# ------------------------------------------------------------------------------------------------ the whole rule
def evaluate(est, n, gt, valid=None, align="sim3", gt_kind="c2w", deltas=(), lengths=(), step=1, log=None, edge_capacity=0, rot_thr=0.0,
             trans_thr=0.0):
    """est [B][cap][12], gt [cap][12 | 3], valid [cap] or None, log = (edge_ij [EC][2], edge_Z [EC][12], state [>= 1]) or None"""
    align = ALIGN[align] if isinstance(align, str) else align
    gt_kind = GT[gt_kind] if isinstance(gt_kind, str) else gt_kind
    est = np.asarray(est, np.float64)
    if est.ndim == 2:
        est = est[None]
    gt = np.asarray(gt, np.float64)
    B, cap = est.shape[0], est.shape[1]
    K, L = len(deltas), len(lengths)
    slots = -(-cap // step)
    n = min(max(int(n), 0), cap)
    rows = np.arange(cap)
    old = np.seterr(all="ignore")
    try:
        gtok = (rows < n) & (np.ones(cap, bool) if valid is None else np.asarray(valid).astype(bool)) & np.isfinite(gt).all(axis=1)
        used = gtok[None, :] & np.isfinite(est).all(axis=2)
        cen = np.zeros((B + 1, cap, 3))
        if gt_kind == POSITIONS:
            cg = gt.copy()
        elif gt_kind == C2W:
            cg = gt[:, [3, 7, 11]].copy()
        else:
            cg = -mtv3(*split(gt))
        cen[B][gtok] = cg[gtok]
        for b in range(B):
            ce = -mtv3(*split(est[b]))
            cen[b][used[b]] = ce[used[b]]
        out = dict(ate=np.zeros((B, 24)), err=np.full((B, cap), -1.0), centres=cen, prefix=np.zeros((B, 2, cap)), used=used, gtok=gtok)
        aux = dict(rpe_E=[], rpe_theta=[], seg_E=[], seg_theta=[], clo_E=np.zeros((0, 3, 3)), clo_theta=np.zeros(0))
        if K:
            out["rpe"] = np.zeros((B, K, 8))
        if L:
            out["seg"] = np.zeros((B, L + 1, 4))
            out["seg_end"] = np.full((B, slots, L), -1, np.int32)
        y = cen[B]
        for b in range(B):
            u, x = used[b], cen[b]
            N = int(u.sum())
            ate = out["ate"][b]
            s, R, t, sig, varx = 1.0, np.eye(3), np.zeros(3), [0.0, 0.0, 0.0], 0.0
            flags = FEW if N < 3 else 0
            mx = my = np.zeros(3)
            if N > 0:
                mx = tree_sum(np.where(u[:, None], x, 0.0)) / float(N)
                my = tree_sum(np.where(u[:, None], y, 0.0)) / float(N)
            if align in (SE3, SIM3) and N >= 3:
                dx, dy = x - mx, y - my
                A = tree_sum(np.where(u[:, None, None], dy[:, :, None] * dx[:, None, :], 0.0)) / float(N)
                varx = float(tree_sum(np.where(u, (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2], 0.0)) / float(N))
                Rl, sig, deg, dsign = umeyama_rot(A)
                R = np.array(Rl)
                if deg:
                    flags |= DEGENERATE
                if not (varx > 0.0):
                    flags |= NO_SCALE
                elif align == SIM3:
                    s = ((sig[0] + sig[1]) + dsign * sig[2]) / varx
                t = my - s * mv3(R, mx)
            elif align == FIRST and N >= 1:
                f = int(np.flatnonzero(u)[0])
                Re, te = split(est[b][f])
                Rg, tg = split(gt[f])
                if gt_kind == W2C:
                    R, t = rigid_mul(*rigid_inv(Rg, tg), Re, te)
                else:
                    R, t = rigid_mul(Rg, tg, Re, te)
            e3 = y - (s * mv3(R, x) + t)
            e2 = (e3[:, 0] * e3[:, 0] + e3[:, 1] * e3[:, 1]) + e3[:, 2] * e3[:, 2]
            e = np.sqrt(e2)
            out["err"][b][u] = e[u]
            sse = float(tree_sum(np.where(u, e2, 0.0)))
            se = float(tree_sum(np.where(u, e, 0.0)))
            ate[0], ate[1] = N, sse
            if N > 0:
                ate[2], ate[3] = math.sqrt(sse / float(N)), se / float(N)
                ate[4] = e[u].max()
                ate[5] = int(np.flatnonzero(u & (e == ate[4]))[0])
            else:
                ate[5] = -1.0
            ate[6], ate[7:16], ate[16:19], ate[19], ate[20:23], ate[23] = s, np.asarray(R).reshape(-1), t, flags, sig, varx
            # the prefixes
            dg = blocked_prefix(path_steps(y, u), cap)
            de = blocked_prefix(path_steps(x, u), cap)
            out["prefix"][b, 0], out["prefix"][b, 1] = dg, de
            # RPE
            for k, delta in enumerate(deltas):
                i = np.arange(max(n - int(delta), 0))
                if len(i):
                    i = i[u[i] & u[i + int(delta)]]
                P = len(i)
                if P == 0:
                    continue
                c_rot, th, d, RE = pair_error(est[b], gt, gt_kind, i, i + int(delta), s)
                aux["rpe_E"].append(RE); aux["rpe_theta"].append(th)
                full = lambda v: tree_sum(_scatter(v, i, max(n - int(delta), 0)))
                o = out["rpe"][b, k]
                o[0] = P
                o[1], o[2], o[3] = math.sqrt(full(d * d) / float(P)), full(d) / float(P), d.max()
                o[4], o[5], o[6] = math.sqrt(full(th * th) / float(P)), full(th) / float(P), th.max()
                o[7] = full(c_rot) / float(P)
            # segments
            if L:
                tot, totn = np.zeros(3), 0
                for l, length in enumerate(lengths):
                    length = float(length)
                    ks, fs, js = [], [], []
                    for k in range(slots):
                        f = k * step
                        if f < n and u[f]:
                            j = segment_end(dg, n, f, length)
                            if j < n and u[j]:
                                ks.append(k); fs.append(f); js.append(j)
                                out["seg_end"][b, k, l] = j
                    S = len(ks)
                    o = out["seg"][b, l]
                    o[0] = S
                    if S:
                        fs, js, ks = np.array(fs), np.array(js), np.array(ks)
                        c_rot, th, d, RE = pair_error(est[b], gt, gt_kind, fs, js, s)
                        aux["seg_E"].append(RE); aux["seg_theta"].append(th)
                        terms = np.stack([d / length, th / length, (de[js] - de[fs]) / (dg[js] - dg[fs])], 1)
                        sm = tree_sum(_scatter(terms, ks, slots))
                        o[1:4] = sm / float(S)
                        tot = tot + sm
                        totn += S
                    else:
                        tot = tot + 0.0
                o = out["seg"][b, L]
                o[0] = totn
                if totn:
                    o[1:4] = tot / float(totn)
        # closures
        if log is not None and edge_capacity > 0:
            eij, eZ, state = (np.asarray(a) for a in log)
            EC = edge_capacity
            E = min(max(int(state[0]), 0), EC)
            out["edge_err"] = np.full((EC, 2), -1.0)
            out["clo"] = np.zeros(8)
            a = np.arange(E)
            i, j = eij[:E, 0].astype(np.int64), eij[:E, 1].astype(np.int64)
            ok = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j) & np.isfinite(eZ[:E]).all(axis=1)
            ok[ok] &= gtok[i[ok]] & gtok[j[ok]]
            a, i, j = a[ok], i[ok], j[ok]
            Ne = len(a)
            out["clo"][6] = E
            if Ne:
                RZ, tZ = split(eZ[a])
                c_rot, th, d, RE = rel_error(*gt_rel(gt, gt_kind, i, j), RZ, tZ)
                aux["clo_E"], aux["clo_theta"] = RE, th
                out["edge_err"][a, 0], out["edge_err"][a, 1] = th, d
                c = out["clo"]
                c[0], c[1] = Ne, int(((th > rot_thr) | (d > trans_thr)).sum())
                c[2], c[3] = math.sqrt(float(tree_sum(_scatter(th * th, a, EC))) / float(Ne)), th.max()
                c[4], c[5] = math.sqrt(float(tree_sum(_scatter(d * d, a, EC))) / float(Ne)), d.max()
    finally:
        np.seterr(**old)
    for nm in ("rpe", "seg"):
        aux[nm + "_E"] = np.concatenate(aux[nm + "_E"]) if aux[nm + "_E"] else np.zeros((0, 3, 3))
        aux[nm + "_theta"] = np.concatenate(aux[nm + "_theta"]) if aux[nm + "_theta"] else np.zeros(0)
    out["aux"] = aux
    return out


def _scatter(v, idx, M):
    """the terms v at their own indices of an M-term sum, +0.0 elsewhere"""
    v = np.asarray(v, np.float64)
    full = np.zeros((M,) + v.shape[1:])
    full[idx] = v
    return full


# ------------------------------------------------------------------------------------------------ cases shared by the tests
def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def drive(n, seed, spacing=1.0, standstill=()):
    """a smooth drive of n camera-to-world poses [n][12]: a curving path with `spacing` metres a row; rows in `standstill` repeat the row
    before them exactly"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, 12))
    R, p = rot(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3) * 10
    for i in range(n):
        if i and i not in standstill:
            R = R @ rot([0.1, 1.0, 0.05], 0.03 + 0.01 * math.sin(0.1 * i))
            p = p + R @ np.array([0.0, 0.0, spacing])
        G[i] = np.hstack([R, p[:, None]]).reshape(-1)
    return G


def invert_rows(G):
    R, t = split(G)
    Ri, ti = rigid_inv(R, t)
    return np.concatenate([Ri, ti[..., None]], -1).reshape(len(G), 12)


def perturb(G_c2w, seed, noise=0.02, scale=1.0, rigid=None):
    """world-to-camera estimates of a drive: per-row noise on the camera-to-world pose, then a similarity of the world"""
    rng = np.random.default_rng(seed)
    R, t = split(G_c2w)
    out = np.zeros_like(G_c2w)
    Rw, tw = (np.eye(3), np.zeros(3)) if rigid is None else rigid
    for i in range(len(G_c2w)):
        Ri = Rw @ R[i] @ rot(rng.normal(size=3), noise * rng.normal())
        pi = scale * (Rw @ (t[i] + noise * rng.normal(size=3))) + tw
        out[i] = np.hstack([Ri.T, (-Ri.T @ pi)[:, None]]).reshape(-1)
    return out


def case(n, cap=None, B=1, seed=0, gt_kind="c2w", holes=False, bad=False, standstill=(), spacing=1.0):
    """est [B][cap][12] (W2C), gt [cap][12 | 3], valid [cap] u8 | None for n rows of a drive inside cap rows; the rows behind n hold
    finite garbage.  holes: every seventh row is not valid.  bad: a NaN row in est of the LAST b only, an Inf row in gt."""
    cap = cap or n
    rng = np.random.default_rng(1000 + seed)
    G = drive(max(cap, 1), seed, spacing, standstill)
    est = np.stack([perturb(G, 10 * seed + b, scale=1.0 - 0.03 * (b + 1), rigid=(rot([1, 2, 3], 0.5 + b), np.array([5.0, -3.0, 2.0]) * (b + 1)))
                    for b in range(B)])
    gt = G if gt_kind == "c2w" else (invert_rows(G) if gt_kind == "w2c" else np.ascontiguousarray(G[:, [3, 7, 11]]))
    gt = gt.copy()
    valid = None
    if holes:
        valid = np.ones(cap, np.uint8)
        valid[3::7] = 0
    if bad and n > 6:
        est[B - 1, 5, rng.integers(0, 12)] = np.nan
        gt[2, 0] = np.inf
        if n > 40:
            est[B - 1, 33, 3] = -np.inf
    return est, gt, valid
