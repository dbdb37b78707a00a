"""Normative arithmetic of the pose seed and of the choice among refined hypotheses (csrc/pose.hip, pose_seed.hpp) as a
NumPy restatement in fp64: the role icp_np.py plays for the refinement.

A frame is the [16]-double record pr_cloud_frames_dev writes: mean mu [0:3], E = [v0 v1 v2] by ascending eigenvalue [3:12] (vector by
vector), 0, the point count [13].  Aligned coordinates are p' = E^T (p - mu) (utils/pts_align.h:7-46).  For every type
    R = E_db S E_q^T,  t = mu_db - R mu_q,  T = [R | t] maps query-frame points into the DB entry's frame
with S from the pair's best-aligning variant v:
    SC       v = 2 s + r < 120   S = diag(sigma, B), D = 2 pi / 60: r = 0: B = Rot(-s D); r = 1: B = [[cos f, sin f], [sin f, -cos f]],
                                 f = (s + 1) D; sigma = sign(det(E_db) det(E_q) det(B))
    M2DP     v = 4 a + b < 16    S0 = D_b D_a, D_u = diag(dx, dy, dx dy), (dx, dy) = (-1,-1), (-1,+1), (+1,-1), (+1,+1) for u = 0..3
                                 (the loop order of test_m2dp.cpp:46-57); the match says D_a q' ~ D_b d'
    DELIGHT  v = k < 4           row k of Mut (processDELIGHT.m:2-5) is the octant XOR 0, 5, 6, 3 with octant = 4 (z>0) + 2 (y>0) + (x>0)
                                 (DELIGHT.cpp:21): S0 = I, diag(-1,1,-1), diag(1,-1,-1), diag(-1,-1,1)
    M2DP and DELIGHT: S = diag(sigma, 1, 1) S0, sigma = sign(det E_db) sign(det E_q) - the repair goes on x', the least-variance axis, as
    SC's does, so R is always proper.
Products are formed as (E_db S) E_q^T with three-term sums left to right, as the library does; NumPy never fuses."""
import numpy as np

SC, M2DP, DELIGHT = 0, 1, 2
VARIANTS = {SC: 120, M2DP: 16, DELIGHT: 4}
DELTA = 2.0 * np.pi / 60.0
M2DP_DIRS = ((-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0))
DELIGHT_XOR = (0, 5, 6, 3)
CONVERGED, MAX_ITER = 0, 1
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def frame(xyz, signs=(1, 1, 1)):
    """The frame of a cloud: pts_align.h's mean and the eigenvectors of the scatter matrix by ascending eigenvalue, each multiplied by
    signs[e] (an eigen-solver may return either sign, and so either handedness)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    mu = xyz.mean(0)
    c = xyz - mu
    w, V = np.linalg.eigh(c.T @ c)
    f = np.zeros(16)
    f[:3] = mu
    f[3:12] = (V * np.asarray(signs, np.float64)).T.reshape(-1)
    f[13] = len(xyz)
    return f


def E_of(f):
    return np.asarray(f[3:12], np.float64).reshape(3, 3).T          # [component][eigenvector]


def aligned(xyz, f):
    return (np.asarray(xyz, np.float64) - f[:3]) @ E_of(f)


def m2dp_D(u):
    dx, dy = M2DP_DIRS[u]
    return np.diag([dx, dy, dx * dy])


def delight_S0(k):
    x = DELIGHT_XOR[k]
    return np.diag([-1.0 if x & 1 else 1.0, -1.0 if x & 2 else 1.0, -1.0 if x & 4 else 1.0])


def _sgn(x):
    return -1.0 if x < 0 else 1.0


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def S_of(type_, v, Eq, Ed):
    if type_ == SC:
        s, r = v >> 1, v & 1
        a = (s + 1) * DELTA if r else s * DELTA
        ca, sa = np.cos(a), np.sin(a)
        sigma = -1.0 if _det3(Ed) * _det3(Eq) * (-1.0 if r else 1.0) < 0 else 1.0
        return np.array([[sigma, 0, 0], [0, ca, sa], [0, sa if r else -sa, -ca if r else ca]])
    S0 = m2dp_D(v & 3) @ m2dp_D(v >> 2) if type_ == M2DP else delight_S0(v)
    return np.diag([_sgn(_det3(Ed)) * _sgn(_det3(Eq)), 1.0, 1.0]) @ S0


def _mm(A, B):
    """3 x 3 product with the three-term sums left to right."""
    return np.array([[(A[j, 0] * B[0, e] + A[j, 1] * B[1, e]) + A[j, 2] * B[2, e] for e in range(3)] for j in range(3)])


def relative_pose(type_, fq, fd, v):
    """One pair: frames [16], variant -> T [3, 4]."""
    assert 0 <= v < VARIANTS[type_] and fq[13] >= 3 and fd[13] >= 3
    Eq, Ed = E_of(fq), E_of(fd)
    R = _mm(_mm(Ed, S_of(type_, int(v), Eq, Ed)), Eq.T)
    t = np.array([fd[j] - ((R[j, 0] * fq[0] + R[j, 1] * fq[1]) + R[j, 2] * fq[2]) for j in range(3)])
    return np.hstack([R, t[:, None]])


def seed_slots(type_, frames_q, frames_db, db_row0, idx, variant, H):
    """pose_seed_kernel: idx [m, k] global rows, variant [m, k, >= H] -> (T0 [m, k, H, 3, 4], pair_src, pair_dst [m, k, H])."""
    m, k = idx.shape
    T0 = np.tile(IDENT, (m, k, H, 1, 1))
    src = np.full((m, k, H), -1, np.int32)
    dst = np.full((m, k, H), -1, np.int32)

    def usable(f):
        return bool(np.all(np.isfinite(f[:12])) and np.isfinite(f[13]) and f[13] >= 3)
    for q in range(m):
        for j in range(k):
            for h in range(H):
                g, v = int(idx[q, j]), int(variant[q, j, h])
                loc = g - db_row0
                if g < 0 or loc < 0 or loc >= len(frames_db) or v < 0 or v >= VARIANTS[type_]:
                    continue
                if h > 0 and int(variant[q, j, 0]) == v:
                    continue
                if not (usable(frames_q[q]) and usable(frames_db[loc])):
                    continue
                T0[q, j, h] = relative_pose(type_, frames_q[q], frames_db[loc], v)
                src[q, j, h], dst[q, j, h] = q, loc
    return T0, src, dst


def _better(a, b):
    """Whether a beats the kept b: the larger fitness, then the smaller rmse; IEEE comparisons, a kept NaN loses to a number."""
    fa, fb, ra, rb = float(a["fitness"]), float(b["fitness"]), float(a["rmse"]), float(b["rmse"])
    if fa > fb:
        return True
    if fb != fb and fa == fa:
        return True
    if fa == fb:
        return ra < rb or (rb != rb and ra == ra)
    return False


def select(stats_h, min_fitness, max_rmse):
    """verify_select_kernel for one pair: stats_h [H] records (fitness, rmse, status) -> (hyp, accepted)."""
    best = -1
    for h in range(len(stats_h)):
        if int(stats_h[h]["status"]) not in (CONVERGED, MAX_ITER):
            continue
        if best < 0 or _better(stats_h[h], stats_h[best]):
            best = h
    if best < 0:
        return 0, False
    s = stats_h[best]
    return best, bool(s["fitness"] >= min_fitness and s["rmse"] <= max_rmse)


def m2dp_variant(q4, d4, channel=0):
    """processM2DP.m:12-22 for one pair: the first minimum of the 4 x 4 block (1 - q d^T) / 2 in row-major order: v = 4 a + b.
    q4 / d4: the pair's [4, 384] signature rows; channel 0 = count, 1 = intensity."""
    h = q4.shape[1] // 2
    sl = slice(0, h) if channel == 0 else slice(h, 2 * h)
    blk = (1.0 - q4[:, sl] @ d4[:, sl].T) / 2.0
    return int(np.argmin(blk.reshape(-1))), blk


def delight_variant(A, B):
    """processDELIGHT.m:7-37 for one pair ([16, 256] each): chi-square over the bins with A + B > 0, mean over those, strict first minimum
    over the rows of Mut (row k, 0-based: row o of Bk = row o ^ XOR[k] within each half of 8)."""
    best, bk, dist = np.inf, -1, []
    for k, x in enumerate(DELIGHT_XOR):
        perm = [(o & 8) | ((o & 7) ^ x) for o in range(16)]
        Bk = B[perm]
        s = A + Bk
        on = s > 0
        ts = (2.0 * (A[on] - Bk[on]) ** 2 / s[on]).sum() / on.sum() if on.any() else np.inf
        dist.append(ts)
        if best > ts:
            best, bk = ts, k
    return bk, dist
