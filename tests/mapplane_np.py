"""The plane-metric map localiser's rule (pr_mapplane_*) restated in fp64 - written from the rule's text in
include/place_recognition.h, not from the kernels: no hash table (maploc_np's dict from the voxel triple to its smallest row), scalar
Python floats wherever the order of operations matters (the sums of a row's neighbours, the Jacobi sweeps, the L D L^T solve).

  normals          per-row normals and ninfo of the world rows
  plane_pass_sums  one pass: pr_maploc_nn_dev's correspondences and a pair's 30 sums in the device's tree (a 64-lane shuffle tree per
                   wave, the four waves in order, the chunks of 256 points in index order)
  plane_update     the update from those sums: L D L^T, Rodrigues
  icp_plane        the rounds, stop rules and the final pass"""
import math

import numpy as np

import icp_grid_np
import icp_np
import maploc_np as mnp

SWEEPS = 8
SUMS = 30
SERIES_BELOW = 1e-4              # th2 below which Exp(w) uses the series
RUNNING = -1


def jacobi(C):
    """Cyclic Jacobi on the symmetric 3 x 3 C (nested lists of floats): (the three diagonal entries, V as nested lists)."""
    A = [[float(C[a][b]) for b in range(3)] for a in range(3)]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for a in range(3):
                vp, vq = V[a][p], V[a][q]
                V[a][p] = c * vp - s * vq
                V[a][q] = s * vp + c * vq
    return [A[0][0], A[1][1], A[2][2]], V


def sorted_eigen(l):
    """(l0, l1, l2, i0, i1, i2): three compare-exchanges (1,0), (2,1), (1,0) on strict <"""
    v, i = list(l), [0, 1, 2]
    for a, b in ((1, 0), (2, 1), (1, 0)):
        if v[a] < v[b]:
            v[a], v[b] = v[b], v[a]
            i[a], i[b] = i[b], i[a]
    return v[0], v[1], v[2], i[0], i[1], i[2]


def row_neighbours(ix, xyz, j, radius):
    """the kept rows around indexed row j in visit order with their offsets d = q - x_j: [(row, (dx, dy, dz), d2)] and every visited
    (row, d2), kept or not"""
    cell, first = ix["cell"], ix["first"]
    x = [float(v) for v in xyz[j]]
    f = [int(math.floor(x[a] / cell)) for a in range(3)]
    r2 = float(radius) * float(radius)
    kept, seen = [], []
    for d0 in (-1, 0, 1):
        for k in range(9):
            key = (f[0] + d0, f[1] + (k // 3 - 1), f[2] + (k % 3 - 1))
            if not all(-mnp.LIM <= v < mnp.LIM for v in key) or key not in first:
                continue
            row = first[key]
            q = xyz[row]
            dx, dy, dz = float(q[0]) - x[0], float(q[1]) - x[1], float(q[2]) - x[2]
            d2 = ((dx * dx) + dy * dy) + dz * dz
            seen.append((row, d2))
            if d2 < r2:
                kept.append((row, (dx, dy, dz), d2))
    return kept, seen


def row_covariance(kept):
    """(k, C as nested lists): the sums from 0.0 in visit order, C_ab = S_ab - (s_a s_b) / k"""
    k = len(kept)
    s = [0.0, 0.0, 0.0]
    S = [[0.0] * 3 for _ in range(3)]
    for _, d, _ in kept:
        for a in range(3):
            s[a] += d[a]
        for a in range(3):
            for b in range(a, 3):
                S[a][b] += d[a] * d[b]
    C = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            C[a][b] = C[b][a] = S[a][b] - (s[a] * s[b]) / float(k)
    return k, C


def row_normal(ix, xyz, j, radius, min_nbrs, max_ratio, detail=False):
    """(ninfo, normal) of the INDEXED row j"""
    kept, seen = row_neighbours(ix, xyz, j, radius)
    k, C = row_covariance(kept)
    l, V = jacobi(C)
    l0, l1, l2, i0, _, _ = sorted_eigen(l)
    valid = k >= min_nbrs and all(math.isfinite(v) for v in l) and l1 > 0.0 and l0 <= max_ratio * l1
    n = (0.0, 0.0, 0.0)
    if valid:
        e = [V[a][i0] for a in range(3)]
        nrm = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        e = [v / nrm for v in e]
        mag, lead = abs(e[0]), e[0]
        if abs(e[1]) > mag:
            mag, lead = abs(e[1]), e[1]
        if abs(e[2]) > mag:
            lead = e[2]
        n = tuple(-v for v in e) if lead < 0.0 else tuple(e)
    if detail:
        return (k if valid else -k), n, dict(k=k, C=C, l=(l0, l1, l2), seen=seen, valid=valid)
    return (k if valid else -k), n


def normals(ix, xyz, radius, min_nbrs, max_ratio, out_capacity=None):
    """(normals [out_capacity, 3], ninfo int32 [out_capacity]) under the index ix = maploc_np.index(xyz, state0, cell, out_capacity)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    oc = len(xyz) if out_capacity is None else out_capacity
    nrm, info = np.zeros((oc, 3)), np.zeros(oc, np.int32)
    for j in ix["rows"]:
        info[j], nrm[j] = row_normal(ix, xyz, int(j), radius, min_nbrs, max_ratio)
    return nrm, info


class LazyNormals:
    """normals()'s rows computed when first asked for: what a refinement against a large world needs"""

    def __init__(self, ix, xyz, radius, min_nbrs, max_ratio):
        self.ix, self.xyz, self.args, self.cache = ix, np.asarray(xyz, np.float64).reshape(-1, 3), (radius, min_nbrs, max_ratio), {}
        self.indexed = set(int(j) for j in ix["rows"])

    def __call__(self, j):
        j = int(j)
        if j not in self.cache:
            self.cache[j] = row_normal(self.ix, self.xyz, j, *self.args) if j in self.indexed else (0, (0.0, 0.0, 0.0))
        return self.cache[j]


def table(nrm, info):
    """arrays -> the callable j -> (ninfo, normal) the pass takes"""
    return lambda j: (int(info[j]), nrm[j])


def nn_boxed(ix, xyz, row, Pt, max_corr, excl=None):
    """maploc_np.nn_brute over the candidates inside the box of the finite points widened by max_corr (1 + 2^-10): the same (j, d2) as
    maploc_np.nn (test_maploc_cpu.py holds nn to nn_brute; a row outside the box is nobody's masked correspondent), quick on a large world"""
    cand = mnp.candidates(ix, row, excl)
    Pt = np.asarray(Pt, np.float64).reshape(-1, 3)
    fin = Pt[np.isfinite(Pt).all(axis=1)]
    r = max_corr * mnp.SLACK
    if len(fin) and len(cand):
        Q = xyz[cand]
        with np.errstate(all="ignore"):
            cand = cand[((Q >= fin.min(0) - r) & (Q <= fin.max(0) + r)).all(axis=1)]
    else:
        cand = cand[:0]
    j, d2 = icp_grid_np.nn_radius(Pt, xyz[cand], max_corr)
    return np.where(j >= 0, cand[np.maximum(j, 0)] if len(cand) else -1, -1).astype(np.int32), d2


def point_terms(T, p_src, q, n):
    """one plane correspondent's (J [6], r) as Python floats; T [3, 4]"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    x, y, z = (float(v) for v in p_src)
    p = [((float(T[a, 0]) * x + float(T[a, 1]) * y) + float(T[a, 2]) * z) + float(T[a, 3]) for a in range(3)]
    u = [p[a] - float(T[a, 3]) for a in range(3)]
    e = [p[a] - float(q[a]) for a in range(3)]
    n = [float(v) for v in n]
    r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
    J = [u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0], n[0], n[1], n[2]]
    return J, r


def tree_sum(terms):
    """terms [n, SUMS] per source point (zeros where a point adds nothing) -> the pair's sums: per chunk of 256 the 64-lane shuffle tree of
    each wave, the four waves in order; then the chunks in index order from 0.0"""
    terms = np.asarray(terms, np.float64).reshape(-1, SUMS)
    total = np.zeros(SUMS)
    for c0 in range(0, len(terms), 256):
        a = np.zeros((256, SUMS))
        blk = terms[c0:c0 + 256]
        a[:len(blk)] = blk
        a = a.reshape(4, 64, SUMS)
        d = 32
        while d:
            a[:, :d] = a[:, :d] + a[:, d:2 * d]
            d >>= 1
        w = a[:, 0]
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


def plane_pass_sums(ix, xyz, row, P, T, normal_of, max_corr, excl=None, search=None):
    """One pass of the source cloud P under T: (sums [30], idx, d2).  sums = inliers, sum d2, plane correspondents, the 21 entries of
    sum J J^T (upper triangle, row-major), the 6 of sum J r."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    Pt = icp_np.transform(T, P)
    idx, d2 = (search or nn_boxed)(ix, xyz, row, Pt, max_corr, excl)
    terms = np.zeros((len(P), SUMS))
    for i in np.nonzero(idx >= 0)[0]:
        j = int(idx[i])
        terms[i, 0], terms[i, 1] = 1.0, d2[i]
        info, n = normal_of(j)
        if info > 0:
            J, r = point_terms(T, P[i], xyz[j], n)
            terms[i, 2] = 1.0
            m = 3
            for a in range(6):
                for b in range(a, 6):
                    terms[i, m] = J[a] * J[b]
                    m += 1
            for a in range(6):
                terms[i, 24 + a] = J[a] * r
    return tree_sum(terms), idx, d2


def system_of(sums):
    """(A [6][6], b [6]) as nested lists of floats"""
    A = [[0.0] * 6 for _ in range(6)]
    m = 3
    for r in range(6):
        for c in range(r, 6):
            A[r][c] = A[c][r] = float(sums[m])
            m += 1
    return A, [float(v) for v in sums[24:30]]


def ldl_solve(A, b):
    """x of A x = -b by L D L^T without pivoting, or None: a d_k not finite or <= 1e-12 A_kk, or an x_i not finite"""
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for k in range(6):
        v = A[k][k]
        for m in range(k):
            v = v - (L[k][m] * d[m]) * L[k][m]
        d[k] = v
        if not math.isfinite(v) or not (v > 1e-12 * A[k][k]):
            return None
        for i in range(k + 1, 6):
            l = A[i][k]
            for m in range(k):
                l = l - (L[i][m] * d[m]) * L[k][m]
            L[i][k] = l / v
    x = [0.0] * 6
    for i in range(6):
        y = -b[i]
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
    return x if all(math.isfinite(v) for v in x) else None


def exp_so3(w):
    """Exp(w) = (1 - b th2) I + b w w^T + a [w]x as nested lists"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if th2 < SERIES_BELOW:
        ca = 1.0 - (th2 / 6.0) * (1.0 - (th2 / 20.0) * (1.0 - th2 / 42.0))
        cb = 0.5 - (th2 / 24.0) * (1.0 - (th2 / 30.0) * (1.0 - th2 / 56.0))
    else:
        th = math.sqrt(th2)
        ca = math.sin(th) / th
        cb = (1.0 - math.cos(th)) / th2
    E = [[cb * (w[r] * w[c]) for c in range(3)] for r in range(3)]
    for r in range(3):
        E[r][r] = (1.0 - cb * th2) + E[r][r]
    E[0][1] -= ca * w[2]; E[0][2] += ca * w[1]
    E[1][0] += ca * w[2]; E[1][2] -= ca * w[0]
    E[2][0] -= ca * w[1]; E[2][1] += ca * w[0]
    return E


def plane_update(sums, T, min_inliers):
    """(status or None, T'): TOO_FEW / DEGENERATE leave T as it is"""
    T = np.array(T, np.float64).reshape(3, 4)
    if sums[2] < min_inliers:
        return icp_np.TOO_FEW, T
    A, b = system_of(sums)
    x = ldl_solve(A, b)
    if x is None:
        return icp_np.DEGENERATE, T
    E = exp_so3(x[:3])
    Tn = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            Tn[r, c] = (E[r][0] * float(T[0, c]) + E[r][1] * float(T[1, c])) + E[r][2] * float(T[2, c])
        Tn[r, 3] = float(T[r, 3]) + x[3 + r]
    return None, Tn


def _stats(sums, ns):
    n = float(sums[0])
    return int(n), (n / ns if ns > 0 else 0.0), (math.sqrt(float(sums[1]) / n) if n > 0 else 0.0)


def icp_plane(ix, xyz, row, P, T0, normal_of, excl=None, max_iter=30, max_corr=0.9, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=6,
              search=None):
    """dict(T, fitness, rmse, n_inl, iters, status, n_plane [per pass]) of the plane-metric refinement of P (already cut to max_src_pts)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    T = np.array(T0, np.float64).reshape(3, 4)
    status, iters, prev, planes = RUNNING, 0, (0.0, 0.0), []
    for _ in range(max_iter):
        sums, _, _ = plane_pass_sums(ix, xyz, row, P, T, normal_of, max_corr, excl, search)
        planes.append(int(sums[2]))
        _, fit, rmse = _stats(sums, len(P))
        stop, T = plane_update(sums, T, min_inliers)
        if stop is not None:
            status = stop
            break
        iters += 1
        if iters > 1 and abs(rmse - prev[0]) < tol_rmse and abs(fit - prev[1]) < tol_fitness:
            status = icp_np.CONVERGED
            break
        prev = (rmse, fit)
    sums, _, _ = plane_pass_sums(ix, xyz, row, P, T, normal_of, max_corr, excl, search)
    n, fit, rmse = _stats(sums, len(P))
    return dict(T=T, fitness=fit, rmse=rmse, n_inl=n, iters=iters, status=icp_np.MAX_ITER if status == RUNNING else status, n_plane=planes)


def scratch_bytes(pair_capacity, max_src_pts):
    """the header's formula"""
    if not (1 <= pair_capacity <= 65535 and 0 <= max_src_pts <= 1 << 26):
        return 0
    pc, ld = pair_capacity, max(max_src_pts, 1)
    nch = (ld + 255) // 256
    parts = [8 * pc * ld, 4 * pc * ld, 240 * pc * nch, 4 * pc, 16 * pc, 24 * pc * ld, 8 * (pc + 1), 4 * pc, 96 * pc, 8 * pc, 32 * pc,
             24 * pc * ld, 4 * pc * ld]
    return sum((b + 15) // 16 * 16 for b in parts)


# ------------------------------------------------------------------------------------------------ the committed scene
def corner_scene(seed=7, cell=0.5, extent=6.0):
    """A floor and two perpendicular walls - the planes z, x, y = 0.1 cell -, extent m each way.  World rows: one per voxel of `cell`
    along each plane, at irregular in-plane positions inside the voxel.  A source cloud of 810 points on the same planes at other
    in-plane positions, seen from a sensor at (2.5, 2.5, 1.5); the truth maps it into the world, the seed is the truth turned by
    1 degree and shifted by 0.15 m.  Returns dict(xyz, row, src, truth, seed, cell)."""
    rng = np.random.default_rng(seed)
    n = int(round(extent / cell))
    rows = []
    for plane in (2, 0, 1):
        for a in range(n):
            for b in range(n):
                uv = (np.array([a, b]) + 0.15 + 0.7 * rng.random(2)) * cell
                rows.append(np.insert(uv, plane, 0.1 * cell))
    xyz = np.array(rows)
    keep = {}
    for j, p in enumerate(xyz):                                   # one per voxel: the rows along the edges share voxels
        keep.setdefault(tuple(np.floor(p / cell).astype(int)), j)
    xyz = xyz[sorted(keep.values())]
    pts = []
    for plane in (2, 0, 1):
        uv = 0.4 + (extent - 0.8) * rng.random((270, 2))
        pts.append(np.insert(uv, plane, 0.1 * cell, axis=1))
    world_pts = np.vstack(pts)
    ang = np.deg2rad(25.0)
    Rt = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    truth = np.hstack([Rt, np.array([[2.5], [2.5], [1.5]])])
    src = (world_pts - truth[:, 3]) @ Rt                          # inv(truth) applied: the sensor's frame
    axis = np.array([1.0, 2.0, 2.0]) / 3.0
    dR = np.array(exp_so3(list(axis * np.deg2rad(1.0))))
    shift = 0.15 * np.array([2.0, -1.0, 2.0]) / 3.0
    seed_T = np.hstack([dR @ Rt, (truth[:, 3] + shift)[:, None]])
    return dict(xyz=xyz, row=np.zeros(len(xyz), np.int32), src=src, truth=truth, seed=seed_T, cell=cell)


SCENE_NORMALS = dict(radius=0.499, min_nbrs=4, max_ratio=0.01)
REFINE_SIZES = (0, 1, 255, 256, 257, 513)


def refine_case():
    """The corner scene's world and, far from it, a single plane (12 x 12 rows around (100, 100, 100)) and a sparse patch whose rows
    have no neighbour within the radius (around 200): one world of cell 0.5, keyframe rows j % 4.  Sources, a CSR set in the sensor's
    frame: clouds of REFINE_SIZES points cut from the scene's source cloud (0 .. 5), a cloud on the single plane (6), one on the sparse
    patch (7), five points next to five rows of the floor that have a normal (8).  seeds[s]: the scene's seed for 0 .. 5, the truth for
    6 .. 8.  Returns dict(xyz, row, cell, xq, oq, seeds, truth, ix, normals, ninfo)."""
    sc = corner_scene()
    rng = np.random.default_rng(17)
    cell = sc["cell"]
    g = np.array([(a, b) for a in range(12) for b in range(12)], np.float64)
    plane = np.hstack([(g + 0.15 + 0.7 * rng.random((144, 2))) * cell + 100.0, np.full((144, 1), 100.0 + 0.1 * cell)])
    sparse = np.array([(200.0 + 1.5 * a + 0.1, 200.0 + 1.5 * b + 0.1, 200.05) for a in range(8) for b in range(8)])
    xyz = np.vstack([sc["xyz"], plane, sparse])
    row = (np.arange(len(xyz)) % 4).astype(np.int32)
    ix = mnp.index(xyz, len(xyz), cell)
    nrm, info = normals(ix, xyz, **SCENE_NORMALS)
    src = sc["src"]
    perm = rng.permutation(len(src))
    clouds = [src[perm[:s]] for s in REFINE_SIZES]
    inv = lambda P: (np.asarray(P) - sc["truth"][:, 3]) @ sc["truth"][:, :3]                      # world points into the sensor's frame
    uv = 100.6 + 4.5 * rng.random((120, 2))
    clouds.append(inv(np.hstack([uv, np.full((120, 1), 100.0 + 0.1 * cell)])))
    clouds.append(inv(sparse[:40] + 0.05))
    floor = [j for j in range(len(sc["xyz"])) if info[j] > 0 and xyz[j, 2] == 0.1 * cell and xyz[j, 0] > 1.0 and xyz[j, 1] > 1.0]
    clouds.append(inv(xyz[floor[::max(len(floor) // 5, 1)][:5]] + (0.03, 0.02, 0.0)))
    oq = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    seeds = [sc["seed"]] * 6 + [sc["truth"]] * 3
    return dict(xyz=xyz, row=row, cell=cell, xq=np.vstack(clouds), oq=oq, seeds=seeds, truth=sc["truth"], ix=ix, normals=nrm, ninfo=info)


def plane_rows(rng, normal, size, samples, cell, noise=0.0, quantum=None, origin=(0.0, 0.0, 0.0)):
    """world rows as a fuse with keep = first leaves them: `samples` random points of a size x size patch of the plane through `origin`
    with the given normal, `noise` along it; the first point of every voxel of `cell`; coordinates rounded to multiples of `quantum`"""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    a = np.cross(n, (1.0, 0.0, 0.0) if abs(n[0]) < 0.9 else (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    uv = size * rng.random((samples, 2))
    P = np.asarray(origin) + uv[:, :1] * a + uv[:, 1:] * b + noise * rng.standard_normal((samples, 1)) * n
    if quantum:
        P = np.round(P / quantum) * quantum
    keep = {}
    for j, p in enumerate(P):
        keep.setdefault(tuple(np.floor(p / cell).astype(int)), j)
    return P[sorted(keep.values())]


def normal_cases():
    """The committed normal cases: name -> (xyz rows, cell, radius, min_nbrs, max_ratio).  No validity decision lies within 1e-6 relative
    of its threshold outside the deliberate radius edge (test_mapplane_cpu.py asserts it)."""
    rng = np.random.default_rng(3)
    cases = {}
    tilt = (0.5, 0.6, 0.62)
    jit = plane_rows(rng, tilt, 7.0, 4000, 1.0, noise=0.02, origin=(1.0, 0.5, 2.0))
    cases["jittered plane"] = (jit, 1.0, 0.99, 5, 0.2)
    flat = plane_rows(rng, tilt, 56.0, 4000, 8.0, noise=0.001, quantum=2.0 ** -17, origin=(8.0, 4.0, 16.0))
    cases["plane unshifted"] = (flat, 8.0, 7.9, 5, 0.2)
    cases["plane shifted by 5e6"] = (flat + np.array([5e6, 0.0, 0.0]), 8.0, 7.9, 5, 0.2)
    fl = plane_rows(rng, (0.0, 0.0, 1.0), 6.0, 2000, 1.0, origin=(0.0, 0.0, 0.3))
    wall = plane_rows(rng, (1.0, 0.0, 0.0), 6.0, 2000, 1.0, origin=(0.3, 0.0, 0.0))
    cases["two planes meeting in an edge"] = (np.vstack([fl, wall[wall[:, 2] > 1.0]]), 1.0, 0.99, 4, 0.05)
    cases["a line"] = (np.array([(0.75 * i + 0.1, 0.5, 0.5) for i in range(10)]), 1.0, 0.99, 3, 0.5)
    cases["an isolated row"] = (np.vstack([jit[:40], [(40.5, 40.5, 40.5)]]), 1.0, 0.99, 5, 0.2)
    few = np.array([(0.5, 0.5, 0.5), (1.3, 0.6, 0.5), (0.6, 1.4, 0.5), (1.4, 1.3, 0.52),
                    (10.5, 10.5, 0.5), (11.3, 10.6, 0.5), (10.6, 11.4, 0.5), (11.2, 11.1, 0.52), (9.7, 10.4, 0.49)])
    cases["k = min_nbrs - 1 and k = min_nbrs"] = (few, 1.0, 0.99, 4, 0.5)
    edge = np.array([(0.5, 0.5, 0.5), (1.25, 0.5, 0.5), (0.5, float(np.nextafter(1.25, 0.0)), 0.5), (0.5, 0.5, 1.0), (-0.25, 0.5, 0.5),
                     (0.5, -0.2, 0.6)])
    cases["a neighbour at exactly radius and one ulp inside"] = (edge, 1.0, 0.75, 3, 1.0)
    bad = jit[:60].copy()
    bad[3] = (np.nan, 1.0, 1.0); bad[7] = (2.0, np.inf, 0.5)
    cases["NaN and Inf rows"] = (bad, 1.0, 0.99, 5, 0.2)
    tri = np.vstack([jit[:60], jit[4] + (0.01, 0.01, 0.0), jit[4] + (-0.01, 0.01, 0.0)])
    cases["three rows in one voxel"] = (tri, 1.0, 0.99, 5, 0.2)
    L = float(mnp.LIM)
    ends = np.array([(L - 0.5, 0.5, 0.5), (L - 1.4, 0.6, 0.5), (L - 0.6, 1.4, 0.5), (L - 1.5, 1.5, 0.55), (L - 0.5, -0.4, 0.5),
                     (-L + 0.5, 0.5, 0.5), (-L + 1.4, 0.6, 0.5), (-L + 0.6, 1.4, 0.5), (-L + 1.5, 1.5, 0.55), (-L + 0.5, -0.4, 0.5)])
    cases["the first and last voxel of the range"] = (ends, 1.0, 0.99, 4, 0.5)
    neg = np.array([(-0.0, -0.0, -0.0), (0.9, 0.1, 0.0), (0.1, 0.9, -0.0), (-0.9, 0.2, 0.0), (0.2, -0.9, 0.0), (-0.8, -0.7, -0.0)])
    cases["-0.0 coordinates"] = (neg, 1.0, 0.99, 4, 0.5)
    cells = np.array(mnp.COLLIDING_CELLS, np.float64)
    cases["the colliding keys"] = (cells + 0.3 + 0.4 * rng.random((32, 3)), 1.0, 0.99, 3, 1.0)
    return cases
