"""Inputs shared by the submap tests (test_submap_cpu.py, test_gpu_submap.py): small maps with chosen cloud sizes, and the
corner scene - keyframes that each see a small seeded sample of the SAME three planes, with a revisit under drift."""
import numpy as np

import posegraph_np as pg
import submap_np as sn


def look_pose(centre, yaw, pitch=0.0):
    """a world-to-camera pose [3, 4] of a camera at `centre` turned by yaw about z and pitch about y"""
    R = pg.exp_so3(np.array([0.0, pitch, 0.0])) @ pg.exp_so3(np.array([0.0, 0.0, yaw]))
    return np.hstack([R, (-R @ np.asarray(centre, np.float64))[:, None]])


def random_map(sizes, seed, spread=3.0, shift=0.0):
    """(xyz [sum, 3], offs [len + 1], poses [len, 12]) of keyframes with the given cloud sizes on a gentle curve; shift: a translation
    added to every camera centre (UTM-sized coordinates)"""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xyz = rng.normal(size=(int(offs[-1]), 3)) * spread
    poses = [look_pose([0.7 * i + shift, 0.1 * i * i - shift, 0.05 * i + 0.5 * shift], 0.07 * i, 0.02 * i) for i in range(len(sizes))]
    return xyz, offs, np.asarray(poses, np.float64).reshape(len(sizes), 12)


CORNER = dict(per_keyframe=14, side=3.0, lattice=6, noise=0.005, w=3, first=3, revisit=13, rows=17,
              icp=dict(max_iter=30, max_corr=0.25, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=10), min_fitness=0.4, max_rmse=0.05)


def corner_scene(seed=5):
    """17 keyframes: rows 0 .. 6 pass the corner of the planes x = 0, y = 0, z = 0 once, rows 7 .. 9 are far along the path, rows
    10 .. 16 pass the corner again.  The planes carry a lattice of lattice^2 landmarks each inside [0, side]^2; every keyframe holds
    per_keyframe of the 3 lattice^2 landmarks (a seeded choice, each with noise of `noise` m), in its camera frame: two keyframes share a
    handful of landmarks at most, two submaps of 4 and 7 keyframes share dozens.  The map's poses of the second pass carry a common
    drift D (P_map = P_true D), so the clouds inside a pass stay consistent while the seed T0 = P_i P_q^-1 from the map's poses is off
    by the drift.  Returns dict(xyz, offs, poses [17, 12] (the map's), T_true [3, 4] = P_i P_q^-1 of the TRUE poses for (i, q) = (first,
    revisit), T0 [3, 4] the seed from the map's poses, pair)."""
    rng = np.random.default_rng(seed)
    K, side, G, n = CORNER["per_keyframe"], CORNER["side"], CORNER["lattice"], CORNER["rows"]
    true = []
    for r in range(n):
        s = r if r < 7 else (r - 10 if r >= 10 else 40 + r)
        lap = 0.0 if r < 7 else 0.15
        true.append(look_pose([2.0 + 0.12 * s + lap, 1.6 - 0.08 * s + lap, 1.5 + 0.03 * s], 0.4 + 0.03 * s + lap, 0.1 - 0.01 * s))
    true = np.stack(true)
    g = (np.arange(G) + 0.5) * side / G
    uu, vv = np.meshgrid(g, g, indexing="ij")
    lat = np.zeros((3, G * G, 3))
    for a in range(3):
        lat[a][:, [b for b in range(3) if b != a]] = np.stack([uu.ravel(), vv.ravel()], 1)
    lat = lat.reshape(-1, 3)
    clouds = []
    for r in range(n):
        pick = rng.choice(len(lat), K, replace=False)
        wpts = lat[pick] + rng.normal(size=(K, 3)) * CORNER["noise"]
        clouds.append(wpts @ true[r][:, :3].T + true[r][:, 3])
    D = np.hstack([pg.exp_so3(np.array([0.01, -0.015, 0.03])), np.array([[0.12], [-0.08], [0.05]])])
    mapped = true.copy()
    mapped[10:] = pg.mul(true[10:], D)
    i, q = CORNER["first"], CORNER["revisit"]
    return dict(xyz=np.concatenate(clouds), offs=(np.arange(n + 1) * K).astype(np.int64), poses=mapped.reshape(n, 12),
                T_true=pg.mul(true[i], pg.inv(true[q])), T0=pg.mul(mapped[i], pg.inv(mapped[q])), pair=(i, q))


def corner_sets(sc, w):
    """(query cloud, DB cloud) of the scene's pair as pair_torch builds them: the DB side centred on i avoiding q, the query side centred
    on q avoiding i with past_only"""
    i, q = sc["pair"]
    kw = dict(slot_capacity=1, point_capacity=1 << 12, max_cloud_points=CORNER["per_keyframe"], keyframe_capacity=CORNER["rows"], w=w,
              avoid_gap=w, max_pts=1 << 12)
    db = sn.build(sc["xyz"], sc["offs"], sc["poses"], CORNER["rows"], [i], [q], past_only=False, **kw)
    qs = sn.build(sc["xyz"], sc["offs"], sc["poses"], CORNER["rows"], [q], [i], past_only=True, **kw)
    return qs["xyz"], db["xyz"]


def pose_error(T, T_true):
    """(rotation angle [rad], translation distance) of T against T_true"""
    E = pg.mul(T, pg.inv(T_true))
    c = min(1.0, max(-1.0, (np.trace(E[:, :3]) - 1.0) / 2.0))
    return float(np.arccos(c)), float(np.linalg.norm(E[:, 3]))
