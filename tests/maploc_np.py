"""The map localiser's rule (pr_maploc_*) restated in fp64 NumPy - written from the rule's text in
include/place_recognition.h, not from the kernels: no hash table, a dict from the voxel's index triple to its smallest row.  `nn` walks
the 27 voxels around a transformed point; `nn_brute` is the plain first-minimum scan over the indexed, non-excluded rows masked to the
radius - the containment claim says the two agree on every input (test_maploc_cpu.py).  `icp` is icp_grid_np.icp_masked on the candidate
rows; `seed` is the seed rule elementwise in the rule's association (no `@`: a BLAS may fuse).  `voxel_quot` / `voxel_coord` restate the
two formulas of the index as the source states them (the test pins them to the source text)."""
import numpy as np

import icp_grid_np
import icp_np

SKIPPED, RANGE, DUPLICATE, TABLE = 1, 2, 4, 8
LIM = 1 << 20
SLACK = 1.0 + 2.0 ** -10          # MAPLOC_SLACK: cell >= max_corr * SLACK


def voxel_quot(x, cell):
    """x / cell"""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64) / np.float64(cell)


def voxel_coord(x, cell):
    """floor(voxel_quot(x, cell))"""
    return np.floor(voxel_quot(x, cell))


def index(xyz, state0, cell, out_capacity=None):
    """The index of the world rows xyz [out_capacity, 3] under the count word state0.  Returns dict(first: voxel triple -> smallest row,
    rows: the indexed rows ascending (int64), R, flags, info i64 [4] = rows indexed, R, flags, 0)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    ocap = len(xyz) if out_capacity is None else out_capacity
    R = min(max(int(state0), 0), ocap)
    x = xyz[:R]
    finite = np.isfinite(x).all(axis=1)
    c = voxel_coord(x, cell)
    inside = ((c >= -float(LIM)) & (c < float(LIM))).all(axis=1)
    flags = 0
    if (~finite).any():
        flags |= SKIPPED
    if (finite & ~inside).any():
        flags |= RANGE
    first = {}
    for j in np.nonzero(finite & inside)[0]:
        k = (int(c[j, 0]), int(c[j, 1]), int(c[j, 2]))
        if k in first:
            flags |= DUPLICATE
        else:
            first[k] = int(j)
    rows = np.array(sorted(first.values()), np.int64)
    return dict(first=first, rows=rows, R=R, flags=flags, cell=float(cell), info=np.array([len(rows), R, flags, 0], np.int64))


def candidates(ix, row, excl=None):
    """the indexed rows that the window excl = (lo, hi) on world.row leaves: ascending"""
    rows = ix["rows"]
    if excl is None or len(rows) == 0:
        return rows
    r = np.asarray(row)[rows]
    return rows[~((excl[0] <= r) & (r <= excl[1]))]


def _first_min(p, Q, js):
    """smaller d2, then smaller j over the rows js of Q (any order); a NaN or +Inf distance never wins"""
    bd, bj = np.inf, -1
    for j in js:
        with np.errstate(all="ignore"):
            dx, dy, dz = p[0] - Q[j, 0], p[1] - Q[j, 1], p[2] - Q[j, 2]
            d = ((dx * dx) + dy * dy) + dz * dz
        if d < bd or (d == bd and j < bj):
            bd, bj = d, j
    return bd, bj


def nn(ix, xyz, row, Pt, max_corr, excl=None):
    """One pass for the transformed points Pt [n, 3]: (idx int32, d2) through the 27 voxels around each point."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    Pt = np.asarray(Pt, np.float64).reshape(-1, 3)
    cell, first = ix["cell"], ix["first"]
    mc2 = np.float64(max_corr) * np.float64(max_corr)
    idx = np.full(len(Pt), -1, np.int32)
    d2 = np.full(len(Pt), np.inf)
    t = voxel_quot(Pt, cell)
    ok = np.isfinite(Pt).all(axis=1) & ((t >= -(LIM + 1.0)) & (t < LIM + 1.0)).all(axis=1)
    for i in np.nonzero(ok)[0]:
        f = [int(np.floor(t[i, a])) for a in range(3)]
        js = []
        for d0 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                for d2_ in (-1, 0, 1):
                    k = (f[0] + d0, f[1] + d1, f[2] + d2_)
                    if all(-LIM <= v < LIM for v in k) and k in first:
                        j = first[k]
                        if excl is None or not (excl[0] <= row[j] <= excl[1]):
                            js.append(j)
        bd, bj = _first_min(Pt[i], xyz, js)
        if bd < mc2:
            idx[i], d2[i] = bj, bd
    return idx, d2


def nn_brute(ix, xyz, row, Pt, max_corr, excl=None):
    """The plain scan: the first minimum over the indexed, non-excluded rows, masked to d2 < max_corr^2."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cand = candidates(ix, row, excl)
    j, d2 = icp_grid_np.nn_radius(Pt, xyz[cand], max_corr)
    return np.where(j >= 0, cand[np.maximum(j, 0)] if len(cand) else -1, -1).astype(np.int32), d2


def icp(ix, xyz, row, P, T0, excl=None, max_corr=0.9, **kw):
    """A refinement of the source cloud P against the world rows: icp_grid_np.icp_masked on the candidate rows.  To keep a pass over a
    large world quick, every pass scans only the candidates inside the box of its finite transformed points widened by max_corr
    (1 + 2^-10) - a row outside it differs from every point by more than max_corr along one axis, so it is nobody's masked
    correspondent, and the kept rows stay in ascending order: the masked result is the full scan's, bit for bit."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    Q = xyz[candidates(ix, row, excl)]
    plain = icp_np.nn
    r = max_corr * SLACK

    def boxed(Pt, Q_, margins=False, block=512):
        fin = Pt[np.isfinite(Pt).all(axis=1)]
        if len(fin) and len(Q_):
            with np.errstate(all="ignore"):
                sel = np.nonzero(((Q_ >= fin.min(0) - r) & (Q_ <= fin.max(0) + r)).all(axis=1))[0]
        else:
            sel = np.zeros(0, np.int64)
        res = plain(Pt, Q_[sel], margins=margins, block=block)
        idx = np.where(res[0] >= 0, sel[np.maximum(res[0], 0)] if len(sel) else -1, -1).astype(np.int32)
        return (idx,) + tuple(res[1:])

    icp_np.nn = boxed
    try:
        return icp_grid_np.icp_masked(P, Q, T0, max_corr=max_corr, **kw)
    finally:
        icp_np.nn = plain


def accept(res, min_fitness, max_rmse):
    return bool(res["status"] in (icp_np.CONVERGED, icp_np.MAX_ITER) and res["fitness"] >= min_fitness and res["rmse"] <= max_rmse)


def seed(poses, n, idx, accepted=None, T_rel=None, src=None):
    """(T0 [c, 3, 4], pair_src int32 [c]) of the seed rule."""
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    kcap = len(poses)
    n = min(max(int(n), 0), kcap)
    idx = np.asarray(idx).reshape(-1)
    c = len(idx)
    T0 = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (c, 1, 1))
    ps = np.full(c, -1, np.int32)
    for p in range(c):
        r = int(idx[p])
        if not (0 <= r < n) or (accepted is not None and not accepted[p]):
            continue
        P = poses[r]
        if not np.isfinite(P).all():
            continue
        Tr = None
        if T_rel is not None:
            Tr = np.asarray(T_rel, np.float64).reshape(-1, 12)[p]
            if not np.isfinite(Tr).all():
                continue
        with np.errstate(all="ignore"):
            Ri = [[P[4 * b + a] for b in range(3)] for a in range(3)]
            ti = [-((P[a] * P[3] + P[4 + a] * P[7]) + P[8 + a] * P[11]) for a in range(3)]
            for a in range(3):
                if Tr is None:
                    for b in range(3):
                        T0[p, a, b] = Ri[a][b]
                    T0[p, a, 3] = ti[a]
                else:
                    for b in range(3):
                        T0[p, a, b] = (Ri[a][0] * Tr[b] + Ri[a][1] * Tr[4 + b]) + Ri[a][2] * Tr[8 + b]
                    T0[p, a, 3] = ((Ri[a][0] * Tr[3] + Ri[a][1] * Tr[7]) + Ri[a][2] * Tr[11]) + ti[a]
        ps[p] = p if src is None else int(src[p])
    return T0, ps


# ------------------------------------------------------------------------------------------------ the table's key and home slot
def key_of(c):
    """the three biased 21-bit indices packed into 63 bits (c_0 highest)"""
    return ((int(c[0]) + LIM) << 42) | ((int(c[1]) + LIM) << 21) | (int(c[2]) + LIM)


def home_slot(key, log2T):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - log2T)


def log2T(out_capacity):
    l = 6
    while (1 << l) < 2 * out_capacity:
        l += 1
    return l


def scratch_bytes(out_capacity, pair_capacity, max_src_pts):
    """the header's formula"""
    if not (1 <= out_capacity <= 1 << 29 and 1 <= pair_capacity <= 65535 and 0 <= max_src_pts <= 1 << 26):
        return 0
    T, pc, ld = 1 << log2T(out_capacity), pair_capacity, max(max_src_pts, 1)
    nch = (ld + 255) // 256
    parts = [16 * T, 16, 16, 4 * pc, 8 * pc * ld, 4 * pc * ld, 160 * pc * nch, 4 * pc, 16 * pc,
             24 * pc * ld, 8 * (pc + 1), 4 * pc, 96 * pc, 8 * pc, 8 * (pc + 1), 32 * pc, 32]
    return sum((b + 15) // 16 * 16 for b in parts)


# 32 distinct voxels for a table of T = 64 slots: the first ten have the home slot 62, so their chain runs 62, 63, 0, 1, ... across the
# table's end; the other 22 are spread (test_maploc_cpu.py asserts this of the list as committed)
COLLIDING_CELLS = [(0, 0, c) for c in (-1944, -1889, -1800, -1745, -1711, -1656, -1567, -1512, -1423, -1368)] + [(1, 0, c) for c in range(22)]
