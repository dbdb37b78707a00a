"""The incremental world map's rule (pr_mapgrow_*) restated in fp64 NumPy - written from the rule's text in
include/place_recognition.h, not from the kernels: no hash table, a dict from the voxel's index triple to its row.  The world position
of a point is worldmap_np.world_positions (the device's bits); a normal is mapplane_np.row_normal.  `Model` holds what the device holds -
the five world arrays, state, the index as a dict, the two normal arrays and the handle's words fused, rows_seen and [a, b) - and
restates sync, extend with its three refusals, the dirty-row set of the normals and the normals call.  `drive` is the committed case."""
import numpy as np

import maploc_np as mnp
import mapplane_np as pnp
import worldmap_np as wnp

ORDER, STALE, FULL = 16, 32, 64
LIM = 1 << 20


def scratch_bytes(max_cloud_points):
    """the header's formula"""
    m = max_cloud_points
    if not 1 <= m <= 1 << 26:
        return 0
    nblk = (m + 255) // 256
    parts = [64, 4 * m, 8 * nblk, 96, 16, 32, 648 * m, 108 * m, 108 * m]
    return sum((b + 15) // 16 * 16 for b in parts)


class Model:
    """the state a pr_mapgrow works on, over a map's arrays (m_xyz [pcap, 3], m_inten [pcap], m_offs [kcap + 1])"""

    def __init__(self, m_xyz, m_inten, m_offs, out_capacity, cell, max_cloud_points):
        self.m_xyz = np.asarray(m_xyz, np.float64).reshape(-1, 3)
        self.m_inten = np.asarray(m_inten, np.float32).reshape(-1)
        self.m_offs = np.asarray(m_offs, np.int64).reshape(-1)
        self.kcap, self.pcap, self.ocap, self.cell, self.mcp = len(self.m_offs) - 1, len(self.m_xyz), int(out_capacity), float(cell), int(max_cloud_points)
        oc = self.ocap
        self.xyz, self.inten, self.src = np.zeros((oc, 3)), np.zeros(oc, np.float32), np.zeros(oc, np.int64)
        self.row, self.count, self.state = np.zeros(oc, np.int32), np.zeros(oc, np.int32), np.zeros(4, np.int32)
        self.first = {}
        self.normals_, self.ninfo = np.zeros((oc, 3)), np.zeros(oc, np.int32)
        self.fused = self.rows_seen = self.a = self.b = 0

    # ---- the rebuild: the committed restatements, one after the other, then sync
    def rebuild(self, poses, n, normals_kw=None):
        w = wnp.fuse(self.m_xyz, self.m_inten, self.m_offs, poses, n, self.cell, 1, "first", out_capacity=self.ocap)
        R = int(w["state"][0])
        for name in ("xyz", "inten", "src", "row", "count"):
            getattr(self, name)[:R] = w[name]
        self.state = w["state"].copy()
        ix = mnp.index(self.xyz, R, self.cell, self.ocap)
        self.first = dict(ix["first"])
        if normals_kw is not None:
            self.normals_, self.ninfo = pnp.normals(ix, self.xyz, out_capacity=self.ocap, **normals_kw)
        self.sync(n)
        return w

    def rows(self):
        return min(max(int(self.state[0]), 0), self.ocap)

    def sync(self, n):
        self.fused = min(max(int(n), 0), self.kcap)
        self.rows_seen = self.a = self.b = self.rows()

    def snapshot(self):
        return (self.xyz.tobytes(), self.inten.tobytes(), self.src.tobytes(), self.row.tobytes(), self.count.tobytes(), self.state.tobytes(),
                tuple(sorted(self.first.items())), self.normals_.tobytes(), self.ninfo.tobytes(), self.fused, self.rows_seen, self.a, self.b)

    # ---- extend
    def extend(self, poses, r, map_n):
        """one call with d_row[0] = r under the map's count map_n; -> info i64 [4]"""
        r, R = int(r), self.rows()
        if r < 0:
            return np.array([0, R, 0, 0], np.int64)
        n = min(max(int(map_n), 0), self.kcap)
        flags = 0
        if r != self.fused or r >= n:
            flags |= ORDER
        if R != self.rows_seen:
            flags |= STALE
        if int(self.state[1]) & wnp.OVERFLOW:
            flags |= FULL
        if flags:
            return np.array([0, R, 0, flags], np.int64)
        poses = np.asarray(poses, np.float64).reshape(-1, 12)
        P = min(max(int(self.m_offs[r + 1]), 0), self.pcap)
        g0 = min(max(int(self.m_offs[r]), 0), P)
        g1 = min(P, g0 + self.mcp)
        g = np.arange(g0, g1, dtype=np.int64)
        w = wnp.world_positions(self.m_xyz[g0:g1], poses, np.full(len(g), r, np.int64))
        finite = np.isfinite(poses[r]).all() & np.isfinite(w).all(axis=1)
        with np.errstate(all="ignore"):
            c = np.floor(w / self.cell)
        inside = ((c >= -float(LIM)) & (c < float(LIM))).all(axis=1)
        if (~finite).any():
            flags |= wnp.SKIPPED
        if (finite & ~inside).any():
            flags |= wnp.RANGE
        valid = np.nonzero(finite & inside)[0]
        fresh = {}                                                  # key -> [its smallest point (index into g), its points]; ascending by insertion
        for i in valid:
            key = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
            if key in self.first:
                self.count[self.first[key]] += 1
            elif key in fresh:
                fresh[key][1] += 1
            else:
                fresh[key] = [int(i), 1]
        stored = 0
        for key, (i, cnt) in fresh.items():                         # ascending representative g
            j = R + stored
            if j >= self.ocap:
                flags |= wnp.OVERFLOW
                break
            self.xyz[j], self.inten[j], self.src[j], self.row[j], self.count[j] = w[i], self.m_inten[g[i]], g[i], r, cnt
            self.first[key] = j
            stored += 1
        R2 = R + stored
        self.state = np.array([R2, int(self.state[1]) | flags, 0, 0], np.int32)
        self.fused, self.rows_seen, self.a, self.b = r + 1, R2, R, R2
        return np.array([stored, R2, len(valid), flags], np.int64)

    # ---- normals
    def index(self):
        """the index in maploc_np's form (what mapplane_np's functions take)"""
        return dict(first=self.first, rows=np.array(sorted(self.first.values()), np.int64), R=self.rows(), flags=0, cell=self.cell)

    def dirty_rows(self):
        """the rows whose normal the call recomputes: those the index holds for the 27 keys around the voxel of a row in [a, b)"""
        dirty = set()
        for s in range(self.a, self.b):
            with np.errstate(all="ignore"):
                f = np.floor(self.xyz[s] / self.cell)
            if not (np.isfinite(self.xyz[s]).all() and ((f >= -LIM) & (f < LIM)).all()):
                continue
            f = [int(v) for v in f]
            for d0 in (-1, 0, 1):
                for d1 in (-1, 0, 1):
                    for d2 in (-1, 0, 1):
                        key = (f[0] + d0, f[1] + d1, f[2] + d2)
                        if all(-LIM <= v < LIM for v in key) and key in self.first:
                            dirty.add(self.first[key])
        return dirty

    def normals(self, radius, min_nbrs, max_ratio):
        ix = self.index()
        for j in sorted(self.dirty_rows()):
            self.ninfo[j], self.normals_[j] = pnp.row_normal(ix, self.xyz, int(j), radius, min_nbrs, max_ratio)


# ------------------------------------------------------------------------------------------------ the committed case
SIZES = (0, 1, 255, 256, 257, 0, 513, 40)
CELL = 0.5
NORMALS = dict(radius=0.499, min_nbrs=4, max_ratio=0.05)


# a normal that flips from invalid to valid: row 0 has two neighbours within the radius after keyframe 0 (k = min_nbrs - 1) and the
# one point of keyframe 1, in a new voxel next to it, completes them (k = min_nbrs).  (map xyz [8, 3], offs [4], the normals' arguments)
FLIP = (np.array([(0.5, 0.5, 0.5), (1.3, 0.6, 0.5), (0.6, 1.4, 0.5), (-0.3, 0.45, 0.52)] + [(0.0, 0.0, 0.0)] * 4), np.array([0, 3, 4, 4], np.int64),
        dict(radius=0.99, min_nbrs=4, max_ratio=0.5))


def rigid(rng, rot, shift):
    """a world-to-camera pose row [12] near the identity"""
    w = rng.normal(0, rot, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rm = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)
    return np.hstack([Rm, rng.normal(0, shift, (3, 1))]).reshape(12)


def camera_points(world, pose):
    """p with world_positions(p, pose) = world to rounding: p = R w + t"""
    P = np.asarray(pose).reshape(3, 4)
    return np.asarray(world) @ P[:, :3].T + P[:, 3]


def drive(seed=5, sizes=SIZES, cell=CELL, kcap=None, slack=8):
    """A map of len(sizes) keyframes on a floor and a wall, each seen under its own pose from a window that moves along the floor, so a
    keyframe's cloud overlaps the one before.  The last keyframe lies entirely inside voxels the earlier ones occupy (the centres of
    occupied voxels).  Returns dict(m_xyz [pcap, 3], m_inten, m_offs [kcap + 1], poses [kcap, 12], n, sizes, cell)."""
    rng = np.random.default_rng(seed)
    kcap = len(sizes) + 2 if kcap is None else kcap
    poses = np.zeros((kcap, 12))
    clouds, seen = [], []
    for k, s in enumerate(sizes):
        poses[k] = rigid(rng, 0.2, 1.0)
        if k == len(sizes) - 1 and len(seen):
            occ = np.unique(np.floor(np.vstack(seen) / cell), axis=0)
            world = (occ[rng.permutation(len(occ))[:s]] + 0.5) * cell
        else:
            uv = rng.random((s, 2)) * (6.0, 4.0) + (1.5 * k, 0.0)
            on_wall = rng.random(s) < 0.35
            world = np.where(on_wall[:, None], np.column_stack([np.full(s, 1.5 * k + 0.07), uv[:, 1], uv[:, 0] - 1.5 * k]),
                             np.column_stack([uv[:, 0], uv[:, 1], np.full(s, 0.06)]))
        seen.append(world.reshape(-1, 3))
        clouds.append(camera_points(world.reshape(-1, 3), poses[k]))
    offs = np.zeros(kcap + 1, np.int64)
    offs[1:len(sizes) + 1] = np.cumsum([len(c) for c in clouds])
    offs[len(sizes) + 1:] = 0                                       # rows behind the count read as empty or negative sizes
    total = int(offs[len(sizes)])
    m_xyz = np.zeros((total + slack, 3))
    m_xyz[:total] = np.vstack(clouds)
    m_inten = np.zeros(total + slack, np.float32)
    m_inten[:total] = rng.random(total).astype(np.float32)
    return dict(m_xyz=m_xyz, m_inten=m_inten, m_offs=offs, poses=poses, n=len(sizes), sizes=tuple(len(c) for c in clouds), cell=cell,
                clouds=clouds)
