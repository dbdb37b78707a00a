"""The world map's rule (pr_worldmap_fuse_dev) restated in fp64 NumPy - written from the rule's text in
include/place_recognition.h, not from the kernels: no hash table, a dict from the voxel's index triple to its points.  The products and
sums of the world position are written out elementwise in the rule's association (no `@`, no einsum: a BLAS may fuse), so the bits are
the device's.  Also the restated key and home slot of the table, for the cases that aim at its probe chains."""
import numpy as np

OVERFLOW, SKIPPED, RANGE, TABLE = 1, 2, 4, 8
LIM = 1 << 20
KEEP = {"first": 0, "last": 1, 0: 0, 1: 1}


def world_positions(xyz, poses, rows):
    """step 1 for the points xyz [P, 3] of the rows `rows` [P]: w_a = (R[0][a] d0 + R[1][a] d1) + R[2][a] d2, d = p - t"""
    q = np.asarray(poses, np.float64).reshape(-1, 12)[rows]
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = p[:, 0] - q[:, 3], p[:, 1] - q[:, 7], p[:, 2] - q[:, 11]
        w = np.empty((len(p), 3), np.float64)
        for a in range(3):
            w[:, a] = (q[:, a] * d0 + q[:, 4 + a] * d1) + q[:, 8 + a] * d2
    return w


def fuse(m_xyz, m_inten, m_offs, poses, n, cell, min_count=1, keep="first", out_capacity=None):
    """One fuse of a map (its xyz [point_capacity, 3], inten, offs [keyframe_capacity + 1]) under poses [keyframe_capacity, 12] with the
    count word n.  Returns dict(xyz, inten, src, row, count: the rows WRITTEN; state i32 [4]; info i64 [4])."""
    m_xyz = np.asarray(m_xyz, np.float64).reshape(-1, 3)
    m_inten = np.asarray(m_inten, np.float32).reshape(-1)
    m_offs = np.asarray(m_offs, np.int64).reshape(-1)
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    kcap, pcap, keep = len(m_offs) - 1, len(m_xyz), KEEP[keep]
    assert len(poses) == kcap and min_count >= 1 and np.isfinite(cell) and cell > 0
    n = min(max(int(n), 0), kcap)
    P = min(max(int(m_offs[n]), 0), pcap) if n > 0 else 0
    out_capacity = pcap if out_capacity is None else out_capacity
    flags = 0
    g = np.arange(P, dtype=np.int64)
    rows = np.searchsorted(m_offs[:n + 1], g, side="right") - 1 if P else np.zeros(0, np.int64)    # offs[r] <= g < offs[r + 1]
    w = world_positions(m_xyz[:P], poses, rows)
    finite = np.isfinite(poses).all(axis=1)[rows] & np.isfinite(w).all(axis=1)
    with np.errstate(all="ignore"):
        c = np.floor(w / cell)                                      # IEEE division, then floor; compared as doubles
    inside = ((c >= -float(LIM)) & (c < float(LIM))).all(axis=1)
    if (~finite).any():
        flags |= SKIPPED
    if (finite & ~inside).any():
        flags |= RANGE
    voxels = {}                                                     # (c0, c1, c2) -> its valid points in ascending g
    valid = np.nonzero(finite & inside)[0]
    for i in valid:
        voxels.setdefault((int(c[i, 0]), int(c[i, 1]), int(c[i, 2])), []).append(int(i))
    reps = sorted((pts[-1] if keep else pts[0], len(pts)) for pts in voxels.values() if len(pts) >= min_count)
    qualifying = len(reps)
    if qualifying > out_capacity:
        flags |= OVERFLOW
    written = min(qualifying, out_capacity)
    src = np.array([r[0] for r in reps[:written]], np.int64)
    return dict(xyz=w[src].reshape(-1, 3), inten=m_inten[src], src=src, row=rows[src].astype(np.int32),
                count=np.array([r[1] for r in reps[:written]], np.int32), state=np.array([written, flags, 0, 0], np.int32),
                info=np.array([written, qualifying, len(valid), flags], np.int64), keys=set(voxels))


# ------------------------------------------------------------------------------------------------ the table's key and home slot
def key_of(c):
    """the three biased 21-bit indices packed into 63 bits"""
    return ((int(c[0]) + LIM) << 42) | ((int(c[1]) + LIM) << 21) | (int(c[2]) + LIM)


def home_slot(key, log2T):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - log2T)


def log2T(point_capacity):
    l = 6
    while (1 << l) < 2 * point_capacity:
        l += 1
    return l


# 32 distinct voxels for a table of T = 64 slots: the first ten have the home slot 62, so their chain runs 62, 63, 0, 1, ... across the
# table's end; the other 22 are spread (test_worldmap_cpu.py asserts this of the list as committed)
COLLIDING_CELLS = [(0, 0, c) for c in (-1944, -1889, -1800, -1745, -1711, -1656, -1567, -1512, -1423, -1368)] + [(1, 0, c) for c in range(22)]


def identity_poses(kcap):
    p = np.zeros((kcap, 12), np.float64)
    p[:, 0] = p[:, 5] = p[:, 10] = 1.0
    return p
