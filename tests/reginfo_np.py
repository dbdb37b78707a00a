"""The registration information's rule (pr_reginfo_*, pr_posegraphw_add*) restated in fp64 - written from the
rule's text in include/place_recognition.h, not from the kernels: scalar Python floats wherever the order of operations matters (a
point's terms, the L D L^T, the six solves, the Jacobi sweeps), numpy for the tree of the sums.

  point_terms / plane_terms   a slot's per-point terms [ns, 11] / [ns, 25] (zeros where a point adds nothing)
  tree_sum                    the device's order: 64-lane shuffle tree per wave, the four waves in order, the chunks in index order
  finish                      steps 2 .. 8 of the rule from a slot's sums
  run                         every slot of a call -> dict(H, cov, spec, w, stat, ok)
  finish_mp                   steps 4 .. 8 in mpmath (inverse, symmetric eigen-decomposition): the other half of the measured bound
  add_weighted                the weighted add rule on a posegraph_np.PoseGraphModel
and the committed cases of test_reginfo_cpu.py / test_gpu_reginfo.py."""
import math

import numpy as np

import icp_np
import mapplane_np as pnp
import posegraph_np as pg

OFF, NONFINITE, TOO_FEW, SINGULAR, WEAK_ROT, WEAK_TRANS = 1, 2, 4, 8, 16, 32
POINT_SUMS, PLANE_SUMS, NS = 11, 25, 25
PIVOT = 1e-12
COND_MAX = 1e8                                   # the cases whose cov / spec / w are compared by the measured bound


# ------------------------------------------------------------------------------------------------ the sums
def _u_of(T, s):
    """(p', u) of one source point as Python floats: p' = T s in pr_icp_pairs_dev's association, u = p' - t"""
    x, y, z = (float(v) for v in s)
    p = [((float(T[a, 0]) * x + float(T[a, 1]) * y) + float(T[a, 2]) * z) + float(T[a, 3]) for a in range(3)]
    return p, [p[a] - float(T[a, 3]) for a in range(3)]


def point_terms(T, P, idx, d2, max_corr):
    T = np.asarray(T, np.float64).reshape(3, 4)
    mc2 = float(max_corr) * float(max_corr)
    terms = np.zeros((len(P), POINT_SUMS))
    for i in range(len(P)):
        if not (idx[i] >= 0 and d2[i] < mc2):
            continue
        _, u = _u_of(T, P[i])
        terms[i] = [1.0, d2[i], u[0], u[1], u[2], u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2]]
    return terms


def plane_terms(T, P, idx, d2, max_corr, world, normals, ninfo):
    T = np.asarray(T, np.float64).reshape(3, 4)
    mc2 = float(max_corr) * float(max_corr)
    oc = len(world)
    terms = np.zeros((len(P), PLANE_SUMS))
    for i in range(len(P)):
        j = int(idx[i])
        if not (j >= 0 and d2[i] < mc2 and j < oc):
            continue
        terms[i, 0], terms[i, 1] = 1.0, d2[i]
        if ninfo[j] > 0:
            J, r = pnp.point_terms(T, P[i], world[j], normals[j])
            terms[i, 2], terms[i, 3] = 1.0, r * r
            m = 4
            for a in range(6):
                for b in range(a, 6):
                    terms[i, m] = J[a] * J[b]
                    m += 1
    return terms


def tree_sum(terms):
    """terms [n, k] -> the slot's k sums in the device's order"""
    terms = np.asarray(terms, np.float64)
    k = terms.shape[1]
    total = np.zeros(k)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(terms), 256):
            a = np.zeros((256, k))
            blk = terms[c0:c0 + 256]
            a[:len(blk)] = blk
            a = a.reshape(4, 64, k)
            d = 32
            while d:
                a[:, :d] = a[:, :d] + a[:, d:2 * d]
                d >>= 1
            w = a[:, 0]
            total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


def reversed_sum(terms):
    """the same sums added one by one from the LAST point to the first: another order of the same terms"""
    terms = np.asarray(terms, np.float64)
    total = np.zeros(terms.shape[1])
    with np.errstate(all="ignore"):
        for t in terms[::-1]:
            total = total + t
    return total


# ------------------------------------------------------------------------------------------------ the finish
def assemble(plane, sums):
    """(H as nested lists, SSE, n_inl, n_used, dof)"""
    s = [float(v) for v in sums]
    H = [[0.0] * 6 for _ in range(6)]
    n_inl = int(s[0])
    if plane:
        m = 4
        for r in range(6):
            for c in range(r, 6):
                H[r][c] = H[c][r] = s[m]
                m += 1
        n_used = int(s[2])
        return H, s[3], n_inl, n_used, n_used - 6
    n, s0, s1, s2 = s[0], s[2], s[3], s[4]
    H[0][0], H[1][1], H[2][2] = s[8] + s[10], s[5] + s[10], s[5] + s[8]
    H[0][1] = H[1][0] = -s[6]; H[0][2] = H[2][0] = -s[7]; H[1][2] = H[2][1] = -s[9]
    H[0][4] = H[4][0] = -s2; H[0][5] = H[5][0] = s1; H[1][3] = H[3][1] = s2
    H[1][5] = H[5][1] = -s0; H[2][3] = H[3][2] = -s1; H[2][4] = H[4][2] = s0
    H[3][3] = H[4][4] = H[5][5] = n
    return H, s[1], n_inl, n_inl, 3 * n_inl - 6


def ldl(H, detail=False):
    """(L, d) of the L D L^T without pivoting, or None when a d_k is not finite or not > 1e-12 H_kk.  detail: (L, d, ok, the smallest
    d_k / H_kk) with no early exit"""
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ok, margin = True, math.inf
    for k in range(6):
        v = H[k][k]
        for m in range(k):
            v = v - (L[k][m] * d[m]) * L[k][m]
        d[k] = v
        if not math.isfinite(v) or not (v > PIVOT * H[k][k]):
            ok = False
            if not detail:
                return None
        if H[k][k] > 0 and math.isfinite(v):
            margin = min(margin, v / H[k][k])
        for i in range(k + 1, 6):
            l = H[i][k]
            for m in range(k):
                l = l - (L[i][m] * d[m]) * L[k][m]
            L[i][k] = l / v if v != 0.0 else math.nan
    return (L, d, ok, margin) if detail else (L, d)


def sigma_of(L, d):
    """Sigma = H^-1 by six solves (column j from e_j), as nested lists"""
    Sg = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        x = [0.0] * 6
        for i in range(6):
            y = 1.0 if i == j else 0.0
            for m in range(i):
                y = y - L[i][m] * x[m]
            x[i] = y
        for i in range(6):
            x[i] = x[i] / d[i]
        for i in range(5, -1, -1):
            z = x[i]
            for m in range(i + 1, 6):
                z = z - L[m][i] * x[m]
            x[i] = z
        for i in range(6):
            Sg[i][j] = x[i]
    return Sg


def _signed_unit(e):
    nrm = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    e = [v / nrm for v in e]
    mag, lead = abs(e[0]), e[0]
    if abs(e[1]) > mag:
        mag, lead = abs(e[1]), e[1]
    if abs(e[2]) > mag:
        lead = e[2]
    return [-v for v in e] if lead < 0.0 else e


def block_spectrum(Sg, o):
    """(l0 <= l1 <= l2, the unit eigenvector of l2 with its largest component positive) of the block at o: the upper triangle, mirrored"""
    A = [[Sg[o + min(r, c)][o + max(r, c)] for c in range(3)] for r in range(3)]
    l, V = pnp.jacobi(A)
    l0, l1, l2, _, _, i2 = pnp.sorted_eigen(l)
    return [l0, l1, l2], _signed_unit([V[a][i2] for a in range(3)])


def weights(flags, SSE, dof, cr2, ct2, sigma_min, w_max):
    q, sm2 = SSE / float(dof), sigma_min * sigma_min
    s2 = q if q > sm2 else sm2
    if flags:
        return s2, 0.0, 0.0
    xr, xt = 1.0 / (s2 * cr2), 1.0 / (s2 * ct2)
    return s2, (xr if xr < w_max else w_max), (xt if xt < w_max else w_max)


def finish(plane, sums, T, min_inliers, min_ratio, sigma_min, w_max):
    """a slot that is not OFF -> dict(H [6, 6], cov [6, 6], spec [16], w [2], stat [4])"""
    H0, cov, spec, w = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(16), np.zeros(2)
    k = PLANE_SUMS if plane else POINT_SUMS
    n_inl = int(sums[0])
    n_used = int(sums[2]) if plane else n_inl
    dof = n_used - 6 if plane else 3 * n_used - 6
    if not (np.isfinite(np.asarray(T, np.float64)).all() and np.isfinite(sums[:k]).all()):
        return dict(H=H0, cov=cov, spec=spec, w=w, stat=np.array([n_inl, n_used, dof, NONFINITE], np.int32))
    H, SSE, n_inl, n_used, dof = assemble(plane, sums)
    H0 = np.array(H)
    spec[12] = SSE
    flags = 0
    if n_used < min_inliers or dof <= 0:
        flags = TOO_FEW
    else:
        f = ldl(H)
        Sg = sigma_of(*f) if f is not None else None
        if Sg is None or not all(math.isfinite(v) for row in Sg for v in row):
            flags = SINGULAR
        else:
            cov = np.array(Sg)
            cr, dr = block_spectrum(Sg, 0)
            ct, dt = block_spectrum(Sg, 3)
            if not (cr[0] >= min_ratio * cr[2]):
                flags |= WEAK_ROT
            if not (ct[0] >= min_ratio * ct[2]):
                flags |= WEAK_TRANS
            s2, w[0], w[1] = weights(flags, SSE, dof, cr[2], ct[2], sigma_min, w_max)
            spec[:12] = cr + ct + dr + dt
            spec[13] = s2
    return dict(H=H0, cov=cov, spec=spec, w=w, stat=np.array([n_inl, n_used, dof, flags], np.int32))


def finish_mp(plane, sums, min_ratio, sigma_min, w_max, dps=50):
    """steps 5 .. 8 from the sums with the inverse and the eigen-decompositions in mpmath -> dict(cov, spec, w) as float64 arrays (the
    flags of the weakness test are recomputed; the caller compares clean and weak cases only)"""
    import mpmath as mp
    mp.mp.dps = dps
    H, SSE, _, _, dof = assemble(plane, sums)
    Sg = mp.inverse(mp.matrix(H))
    spec = np.zeros(16)
    flags = 0
    out = []
    for o in (0, 3):
        B = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                B[r, c] = (Sg[o + r, o + c] + Sg[o + c, o + r]) / 2
        E, Q = mp.eigsy(B)
        order = sorted(range(3), key=lambda i: E[i])
        l = [E[i] for i in order]
        e = [Q[a, order[2]] for a in range(3)]
        nrm = mp.sqrt(sum(v * v for v in e))
        e = [v / nrm for v in e]
        lead = max(e, key=abs)
        if lead < 0:
            e = [-v for v in e]
        out.append(([float(v) for v in l], [float(v) for v in e]))
        if not (l[0] >= mp.mpf(min_ratio) * l[2]):
            flags |= WEAK_ROT if o == 0 else WEAK_TRANS
    (cr, dr), (ct, dt) = out
    s2, wr, wt = weights(flags, SSE, dof, cr[2], ct[2], sigma_min, w_max)
    spec[:12] = cr + ct + dr + dt
    spec[12], spec[13] = SSE, s2
    return dict(cov=np.array([[float(Sg[r, c]) for c in range(6)] for r in range(6)]), spec=spec, w=np.array([wr, wt]), flags=flags)


# ------------------------------------------------------------------------------------------------ a call
def slot_points(xyz_q, offs_q, pair_src, accepted, out_offs, p, max_src_pts):
    """(first source row, first correspondence row, points read) of slot p, or None: OFF"""
    Nq = len(offs_q) - 1
    src = int(pair_src[p])
    if src < 0 or src >= Nq or (accepted is not None and accepted[p] == 0):
        return None
    o0 = int(out_offs[p]); span = int(out_offs[p + 1]) - o0
    if span <= 0:
        return None
    q0 = int(offs_q[src]); cloud = int(offs_q[src + 1]) - q0
    return q0, o0, max(min(span, cloud, max_src_pts), 0)


def slot_terms(plane, xyz_q, T, q0, o0, ns, nn_idx, nn_d2, max_corr, world=None, normals=None, ninfo=None):
    P, idx, d2 = xyz_q[q0:q0 + ns], nn_idx[o0:o0 + ns], nn_d2[o0:o0 + ns]
    with np.errstate(all="ignore"):
        return plane_terms(T, P, idx, d2, max_corr, world, normals, ninfo) if plane else point_terms(T, P, idx, d2, max_corr)


def run(plane, xyz_q, offs_q, pair_src, T, accepted, nn, max_src_pts, max_corr, min_inliers, min_ratio, sigma_min, w_max, world=None,
        normals=None, ninfo=None, summer=tree_sum, detail=False):
    """every slot -> dict(H [c, 6, 6], cov [c, 6, 6], spec [c, 16], w [c, 2], stat [c, 4] i32, ok [c] bool); detail: also the per-slot
    terms and sums (None for an OFF slot)"""
    xyz_q = np.asarray(xyz_q, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3, 4)
    c = len(pair_src)
    out = dict(H=np.zeros((c, 6, 6)), cov=np.zeros((c, 6, 6)), spec=np.zeros((c, 16)), w=np.zeros((c, 2)), stat=np.zeros((c, 4), np.int32))
    terms_of, sums_of = [], []
    for p in range(c):
        sp = slot_points(xyz_q, offs_q, pair_src, accepted, nn[0], p, max_src_pts)
        if sp is None:
            out["stat"][p] = (0, 0, 0, OFF)
            terms_of.append(None); sums_of.append(None)
            continue
        terms = slot_terms(plane, xyz_q, T[p], *sp, nn[1], nn[2], max_corr, world, normals, ninfo)
        sums = summer(terms)
        r = finish(plane, sums, T[p], min_inliers, min_ratio, sigma_min, w_max)
        for k in ("H", "cov", "spec", "w", "stat"):
            out[k][p] = r[k]
        terms_of.append(terms); sums_of.append(sums)
    out["ok"] = out["stat"][:, 3] == 0
    if detail:
        out["terms"], out["sums"] = terms_of, sums_of
    return out


def scratch_bytes(pair_capacity, max_src_pts):
    """the header's formula"""
    if not (1 <= pair_capacity <= 65535 and 0 <= max_src_pts <= 1 << 26):
        return 0
    pc, ld = pair_capacity, max(max_src_pts, 1)
    nch = (ld + 255) // 256
    parts = [200 * pc * nch, 24 * pc * ld, 8 * (pc + 1), 4 * pc, 96 * pc, pc, 8 * (pc + 1), 4 * pc * ld, 8 * pc * ld, 24 * pc * ld, 24 * pc * ld,
             4 * pc * ld, 288 * pc, 288 * pc, 128 * pc, 16 * pc, 16 * pc, pc]
    return sum((b + 15) // 16 * 16 for b in parts)


# ------------------------------------------------------------------------------------------------ the weighted add
def add_weighted(model, idx, T, accepted, query_row, w):
    """posegraph_np.PoseGraphModel.add slot for slot with (w_rot, w_trans) = w[p] and one more condition: both finite and >= 0"""
    idx = np.asarray(idx, np.int32).reshape(-1)
    T = np.asarray(T, np.float64).reshape(len(idx), 12)
    acc = np.asarray(accepted, np.uint8).reshape(-1)
    w = np.asarray(w, np.float64).reshape(len(idx), 2)
    e0 = min(max(int(model.state[0]), 0), model.cap)
    flags = int(model.state[1]) & pg.OVERFLOW
    if query_row < 0:
        return np.array([0, -1, e0, flags], np.int32)
    e = e0
    for p in range(len(idx)):
        if acc[p] == 0 or idx[p] < 0 or idx[p] == query_row or not np.isfinite(T[p]).all():
            continue
        if not (np.isfinite(w[p]).all() and w[p, 0] >= 0.0 and w[p, 1] >= 0.0):
            continue
        if e == model.cap:
            flags |= pg.OVERFLOW
            continue
        model.edge_ij[e] = (idx[p], query_row)
        model.edge_Z[e] = T[p]
        model.edge_w[e] = w[p]
        e += 1
    model.state[0], model.state[1] = e, flags
    return np.array([e - e0, e0 if e > e0 else -1, e, flags], np.int32)


# ------------------------------------------------------------------------------------------------ the committed cases
POINT = dict(max_corr=0.5, min_inliers=3, min_ratio=1e-6, sigma_min=0.01, w_max=1e9)
PLANE = dict(max_corr=0.499, min_inliers=6, min_ratio=5e-5, sigma_min=0.01, w_max=1e9)
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 513)


def pose(deg, axis, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.hstack([np.array(pnp.exp_so3(list(axis * np.deg2rad(deg)))), np.asarray(t, np.float64).reshape(3, 1)])


def d2_of(T, P, Q):
    """the pass's d2 = ((dx dx) + dy dy) + dz dz between T P and Q, row by row"""
    E = icp_np.transform(T, np.asarray(P, np.float64).reshape(-1, 3)) - np.asarray(Q, np.float64).reshape(-1, 3)
    return (E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1]) + E[:, 2] * E[:, 2]


def box_cloud(n=60, seed=11):
    """n points on the faces of a 4 x 3 x 2 box around the sensor"""
    rng = np.random.default_rng(seed)
    P = (rng.random((n, 3)) - 0.5) * (4.0, 3.0, 2.0)
    face = rng.integers(0, 3, n)
    half = np.array([2.0, 1.5, 1.0])
    P[np.arange(n), face] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * half[face]
    return P


def point_case():
    """The point metric's call: one CSR set of source clouds, slots over it with hand-made correspondences (row i of the span belongs to
    source point i; the targets are T s plus a small offset, so d2 is what a pass would report).  Returns dict(xq, oq, src, T, acc, nn,
    max_src_pts, names)."""
    rng = np.random.default_rng(23)
    T = pose(20.0, (1.0, 2.0, 2.0), (30.0, -12.0, 4.0))
    clouds, names = [], []
    big = box_cloud(513, seed=5)
    for s in SIZES:                                                # clouds 0 .. 10: the sizes
        clouds.append(big[:s]); names.append("size %d" % s)
    clouds.append(box_cloud(60)); names.append("the 60-point box")                               # 11
    grid = np.array([(float(i), 2.0 * i, -1.0 * i) for i in range(-5, 6)])
    clouds.append(grid); names.append("collinear on an integer grid")                           # 12
    clouds.append(box_cloud(700, seed=6)); names.append("a span longer than max_src_pts")       # 13
    bad = box_cloud(60, seed=7); bad[17, 1] = np.nan; bad[40, 0] = np.inf
    clouds.append(bad); names.append("a NaN / Inf source point")                                # 14
    oq = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    xq = np.vstack(clouds)
    Nq = len(clouds)
    # slots: one per cloud, then the edge cases on the 60-point box
    src = list(range(Nq))
    extra = ["all outliers", "n = 2", "a point at max_corr and one ulp inside", "a NaN in T", "nn_idx >= out_capacity", "SSE = 0",
             "pair_src -1", "pair_src Nq", "accepted 0"]
    src += [11] * 6 + [-1, Nq, 11]
    names += extra
    c = len(src)
    Ts = np.tile(T, (c, 1, 1))
    Ts[12] = np.hstack([np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), [[3.0], [-7.0], [2.0]]])      # an integer T
    Ts[Nq + 3, 1, 2] = np.nan
    acc = np.ones(c, np.uint8); acc[c - 1] = 0
    spans, idxs, d2s = [], [], []
    mc = POINT["max_corr"]
    for p in range(c):
        s = src[p]
        if not (0 <= s < Nq):
            spans.append(0); continue
        P = xq[oq[s]:oq[s + 1]]
        n = len(P)
        off = rng.normal(0.0, 0.02, (n, 3))
        with np.errstate(all="ignore"):
            d2 = (off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2]
        idx = np.arange(n, dtype=np.int32)
        name = names[p]
        if name == "all outliers":
            idx[:] = -1; d2[:] = np.inf
        if name == "n = 2":
            idx[2:] = -1; d2[2:] = np.inf
        if name == "a point at max_corr and one ulp inside":
            idx[8:] = -1; d2[8:] = np.inf
            d2[0] = mc * mc; d2[1] = float(np.nextafter(mc * mc, 0.0))          # 7 inliers: rows 1 .. 7
        if name == "nn_idx >= out_capacity":
            idx[:] = 1 << 30                                       # the point metric forms no address from it: every row is an inlier
        if name == "SSE = 0":
            d2[:] = 0.0
        if name == "collinear on an integer grid":
            d2[:] = 0.25 * 0.25
        spans.append(n); idxs.append(idx); d2s.append(d2)
    out_offs = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
    return dict(xq=xq, oq=oq, src=np.array(src, np.int32), T=Ts, acc=acc, nn=(out_offs, np.concatenate(idxs).astype(np.int32), np.concatenate(d2s)),
                max_src_pts=600, names=names)


def nearest(Pt, world):
    """brute-force first minimum of d2 = ((dx dx) + dy dy) + dz dz: (idx int32, d2)"""
    D = Pt[:, None, :] - world[None, :, :]
    d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    j = d2.argmin(axis=1)
    return j.astype(np.int32), d2[np.arange(len(Pt)), j]


def corridor(jitter, seed=3, half=1.5, cone_deg=15.0):
    """Two walls (y = -1, y = 1) and a floor (z = -1) along x for |x| <= half, world rows 0.25 apart; every row has a normal: the
    plane's own, or - jitter > 0 - that normal turned by exactly `jitter` rad towards a direction within cone_deg of the in-plane
    perpendicular of the corridor axis (a tilt mostly ACROSS the corridor: the normals' components along the axis are about jitter
    sin(15 deg) / sqrt(3), which keeps cond(H) under 1e8 while the pose along the axis is noise).  A source of 300 points on the three
    planes seen from a sensor near the middle.  Returns dict(world, normals, ninfo, src, T)."""
    rng = np.random.default_rng(seed)
    xs = np.arange(-half, half + 1e-9, 0.25)
    ts = np.arange(-1.0, 1.0 + 1e-9, 0.25)
    rows, nrm, across = [], [], []
    for x in xs:
        for t in ts:
            rows += [(x, -1.0, t), (x, 1.0, t), (x, t, -1.0)]
            nrm += [(0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
            across += [(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)]
    world, nrm, across = np.array(rows), np.array(nrm), np.array(across)
    if jitter > 0:
        for j in range(len(nrm)):
            phi = np.deg2rad(90.0 + cone_deg * (2.0 * rng.random() - 1.0)) * (1.0 if rng.random() < 0.5 else -1.0)
            t = np.cos(phi) * np.array([1.0, 0.0, 0.0]) + np.sin(phi) * across[j]
            v = np.cos(jitter) * nrm[j] + np.sin(jitter) * t
            nrm[j] = v / np.linalg.norm(v)
    T = pose(8.0, (0.2, -0.3, 1.0), (0.2, 0.1, -0.2))
    pts = []
    for plane, val in ((1, -1.0), (1, 1.0), (2, -1.0)):
        uv = np.column_stack([(rng.random(100) - 0.5) * (2.0 * half - 0.4), (rng.random(100) - 0.5) * 1.8])
        pts.append(np.insert(uv, plane, val, axis=1))
    W = np.vstack(pts) + rng.normal(0.0, 0.004, (300, 3))
    src = (W - T[:, 3]) @ T[:, :3]
    return dict(world=world, normals=nrm, ninfo=np.full(len(world), 5, np.int32), src=src, T=T)


def plane_case():
    """The plane metric's call over ONE world: the corner scene of mapplane_np (its rows, normals and ninfo), and far from it a floor
    alone, the exact corridor, the jittered corridor and a patch whose rows have ninfo <= 0.  Sources: the scene's cloud at its truth, the
    sizes cut from it, six plane correspondents, a cloud on the patch, the floor, the two corridors.  Returns dict(world, normals, ninfo,
    xq, oq, src, T, acc, nn, max_src_pts, names, scene_rows)."""
    import maploc_np as mnp
    sc = pnp.corner_scene()
    ix = mnp.index(sc["xyz"], len(sc["xyz"]), sc["cell"])
    n0, i0 = pnp.normals(ix, sc["xyz"], **pnp.SCENE_NORMALS)
    ex, jt = corridor(0.0), corridor(1e-3)
    g = np.array([(0.25 * a, 0.25 * b, 0.0) for a in range(24) for b in range(24)])
    worlds = [sc["xyz"], g + (100.0, 100.0, 100.0), ex["world"] + (200.0, 0.0, 0.0), jt["world"] + (300.0, 0.0, 0.0), g[:100] + (400.0, 0.0, 0.0)]
    up = np.tile((0.0, 0.0, 1.0), (len(g), 1))
    normals = np.vstack([n0, up, ex["normals"], jt["normals"], up[:100]])
    ninfo = np.concatenate([i0, np.full(len(g), 5), ex["ninfo"], jt["ninfo"], np.full(100, -4)]).astype(np.int32)
    world = np.vstack(worlds)
    rng = np.random.default_rng(31)
    perm = rng.permutation(len(sc["src"]))
    clouds, Ts, names = [], [], []
    for s in SIZES:
        clouds.append(sc["src"][perm[:s]]); Ts.append(sc["truth"]); names.append("scene, size %d" % s)
    clouds.append(sc["src"]); Ts.append(sc["truth"]); names.append("the corner scene")
    shift = lambda T, d: np.hstack([T[:, :3], (T[:, 3] + d)[:, None]])
    Tf = pose(5.0, (1.0, 0.5, 0.2), (103.0, 103.0, 101.5))
    fl = np.column_stack([100.3 + 5.0 * rng.random((120, 2)), np.full(120, 100.0) + rng.normal(0.0, 0.004, 120)])
    clouds.append((fl - Tf[:, 3]) @ Tf[:, :3]); Ts.append(Tf); names.append("one floor")
    clouds.append(ex["src"]); Ts.append(shift(ex["T"], (200.0, 0.0, 0.0))); names.append("the exact corridor")
    clouds.append(jt["src"]); Ts.append(shift(jt["T"], (300.0, 0.0, 0.0))); names.append("the jittered corridor")
    Tp = pose(0.0, (0.0, 0.0, 1.0), (401.0, 1.0, 1.0))
    pa = g[:40] + (400.0, 0.0, 0.0) + (0.03, 0.02, 0.05)
    clouds.append((pa - Tp[:, 3]) @ Tp[:, :3]); Ts.append(Tp); names.append("ninfo <= 0 on every correspondent")
    js, _ = nearest(icp_np.transform(sc["truth"], sc["src"]), sc["xyz"])
    six = [i for i in range(len(sc["src"])) if i0[js[i]] > 0][:6]
    clouds.append(sc["src"][six]); Ts.append(sc["truth"]); names.append("n_pl = 6")
    oq = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    xq = np.vstack(clouds)
    c = len(clouds)
    spans, idxs, d2s = [], [], []
    mc = PLANE["max_corr"]
    for p in range(c):
        Pt = icp_np.transform(Ts[p], clouds[p])
        j, d2 = nearest(Pt, world) if len(Pt) else (np.zeros(0, np.int32), np.zeros(0))
        out = ~(d2 < mc * mc)
        j = np.where(out, -1, j).astype(np.int32); d2 = np.where(out, np.inf, d2)
        spans.append(len(Pt)); idxs.append(j); d2s.append(d2)
    out_offs = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
    return dict(world=world, normals=normals, ninfo=ninfo, xq=xq, oq=oq, src=np.arange(c, dtype=np.int32), T=np.array(Ts),
                acc=np.ones(c, np.uint8), nn=(out_offs, np.concatenate(idxs).astype(np.int32), np.concatenate(d2s)), max_src_pts=900, names=names,
                scene_rows=len(sc["xyz"]))


def run_point_case(case, summer=tree_sum, detail=False, **kw):
    """run()'s dict of the point case under POINT (kw overrides a parameter: w_max=50.0 is the 'w_max reached' run)"""
    return run(0, case["xq"], case["oq"], case["src"], case["T"], case["acc"], case["nn"], case["max_src_pts"], summer=summer, detail=detail,
               **dict(POINT, **kw))


def run_plane_case(case, summer=tree_sum, detail=False):
    return run(1, case["xq"], case["oq"], case["src"], case["T"], case["acc"], case["nn"], case["max_src_pts"], world=case["world"],
               normals=case["normals"], ninfo=case["ninfo"], summer=summer, detail=detail, **PLANE)
