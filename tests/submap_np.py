"""The rule of the local submaps (pr_submap; include/place_recognition.h) restated in NumPy fp64, operation by operation:
the device equals build() byte for byte.  Elementwise NumPy fp64 arithmetic rounds every product and sum (no contraction), so the vector
form below is the scalar rule applied to every point."""
import numpy as np

TRUNCATED, NO_CENTER, OVERFLOW = 1, 2, 4


def walk(centre: int, w: int, past_only: bool = False):
    """the rows of a slot in walk order: centre, centre - 1, centre + 1, centre - 2, ... (Python integers: nothing wraps)"""
    rows = [centre]
    for d in range(1, w + 1):
        rows.append(centre - d)
        if not past_only:
            rows.append(centre + d)
    return rows


def pose_finite(poses, r) -> bool:
    return bool(np.isfinite(np.asarray(poses, np.float64).reshape(-1, 12)[r]).all())


def plan_slot(offs, poses, n, centre, avoid, *, w, past_only, avoid_gap, max_pts, max_cloud_points):
    """(entries, flags): entries = [(row, source start, length)] of the rows taken, in walk order"""
    centre = int(centre)
    if centre < 0:
        return [], 0
    if centre >= n or not pose_finite(poses, centre):
        return [], NO_CENTER
    entries, total = [], 0
    for k, r in enumerate(walk(centre, w, past_only)):
        if not (0 <= r < n) or not pose_finite(poses, r):
            continue
        if k > 0 and avoid is not None and not abs(r - int(avoid)) > avoid_gap:
            continue
        a, b = int(offs[r]), int(offs[r + 1])
        if a < 0 or b < a or b - a > max_cloud_points:
            continue
        if total + (b - a) > max_pts:
            return entries, TRUNCATED
        entries.append((r, a, b - a))
        total += b - a
    return entries, 0


def transform(x, P_r, P_c):
    """y = R_c (R_r^T (x - t_r)) + t_c in the rule's order, for points x [m, 3]"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    Pr, Pc = np.asarray(P_r, np.float64).reshape(3, 4), np.asarray(P_c, np.float64).reshape(3, 4)
    Rr, tr, Rc, tc = Pr[:, :3], Pr[:, 3], Pc[:, :3], Pc[:, 3]
    with np.errstate(all="ignore"):
        d = [x[:, k] - tr[k] for k in range(3)]
        u = [(Rr[0, k] * d[0] + Rr[1, k] * d[1]) + Rr[2, k] * d[2] for k in range(3)]
        y = [((Rc[k, 0] * u[0] + Rc[k, 1] * u[1]) + Rc[k, 2] * u[2]) + tc[k] for k in range(3)]
    return np.stack(y, axis=1)


def build(xyz, offs, poses, n, centers, avoid=None, *, slot_capacity, point_capacity, max_cloud_points, keyframe_capacity, w, past_only=False,
          avoid_gap=0, max_pts):
    """dict(xyz [offs[c], 3] f64, offs [slot_capacity + 1] i64, rows [slot_capacity, 2] i32, info [4] i32)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    n = min(max(int(n), 0), keyframe_capacity)
    centers = np.asarray(centers, np.int64).reshape(-1)
    c = len(centers)
    assert 0 <= c <= slot_capacity
    out_offs = np.zeros(slot_capacity + 1, np.int64)
    rows = np.zeros((slot_capacity, 2), np.int32)
    parts, cur, nonempty, flags_or = [], 0, 0, 0
    for p in range(c):
        entries, flags = plan_slot(offs, poses, n, centers[p], None if avoid is None else avoid[p], w=w, past_only=bool(past_only),
                                   avoid_gap=avoid_gap, max_pts=max_pts, max_cloud_points=max_cloud_points)
        total = sum(e[2] for e in entries)
        out_offs[p] = cur
        if cur + total > point_capacity:
            entries, flags = [], flags | OVERFLOW
        for k, (r, a, ln) in enumerate(entries):
            src = xyz[a:a + ln]
            parts.append(src.copy() if k == 0 and r == int(centers[p]) else transform(src, poses[r], poses[int(centers[p])]))
            cur += ln
        rows[p] = (len(entries), flags)
        nonempty += 1 if entries else 0
        flags_or |= flags
    out_offs[c:] = cur
    info = np.array([nonempty, cur & 0xffffffff, cur >> 32, flags_or], np.int64).astype(np.uint32).view(np.int32)
    out_xyz = np.concatenate(parts, axis=0) if parts else np.zeros((0, 3))
    return dict(xyz=np.ascontiguousarray(out_xyz, np.float64).reshape(-1, 3), offs=out_offs, rows=rows, info=info)
