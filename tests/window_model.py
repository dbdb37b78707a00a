"""A numpy restatement of the reference's "nearby" set (utils/pts_preprocess.h:187-216) for the window tests: per pose the points the cursor
delivers, the set before and after the range test - with the reference's expression order, so that membership is bit-exact."""
import numpy as np


def cursor_cuts(pose_ids, point_ids):
    """Ten lines of pts_preprocess.h:196-200: cuts[p + 1] = cursor after pose p."""
    cuts, c = [0], 0
    for pid in pose_ids:
        while c < len(point_ids) and point_ids[c] <= pid:
            c += 1
        cuts.append(c)
    return np.array(cuts, np.int64)


def to_camera(w, g):
    """camera-frame points of world points g [n, 3] under w [12] (:141-142), and |p| (:144)"""
    w = np.asarray(w, np.float64).reshape(3, 4)
    l = np.stack([((w[r, 0] * g[:, 0] + w[r, 1] * g[:, 1]) + w[r, 2] * g[:, 2]) + w[r, 3] * 1.0 for r in range(3)], axis=1)
    return l, np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2])


def replay(pose_w, cuts, xyz, lidar_range):
    """Per pose: dict(emit, need = set size after the append (what point_capacity must hold), alive = set size after the push,
    cam = camera-frame survivors [*, 3] of an emitting pose, idx = their file indices)."""
    alive = np.zeros(0, np.int64)
    since, out = 0, []
    for p, w in enumerate(pose_w):
        w = np.asarray(w, np.float64).reshape(12)
        if np.sqrt(w[3] * w[3] + w[7] * w[7] + w[11] * w[11]) < 1.0:
            since, alive = 0, np.zeros(0, np.int64)
        alive = np.concatenate([alive, np.arange(cuts[p], cuts[p + 1])])
        need = len(alive)
        if since < 30:
            since += 1
            out.append(dict(emit=False, need=need, alive=len(alive), cam=None, idx=None))
            continue
        l, nrm = to_camera(w, xyz[alive])
        keep = nrm < lidar_range
        alive = alive[keep]
        out.append(dict(emit=True, need=need, alive=len(alive), cam=l[keep], idx=alive.copy()))
    return out
