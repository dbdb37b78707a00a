"""The generated drive of the M2DP / DELIGHT end-to-end test (test_gpu_pose.py): c places of the anisotropic box scene
(synth.scene_cloud), each seen twice - the DB cloud and the query, which is the same place moved by a planted rigid motion (any yaw, a
tilt of up to 2 degrees, a few metres), both 90 % subsets with 2 cm jitter.  Every physical point keeps its intensity in both views."""
import numpy as np

from so_dso_place_recognition_amd import synth

PLACES, POINTS, SEED = 6, 2000, 411


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def drive(c=PLACES, P=POINTS, seed=SEED):
    """(query clouds, DB clouds, query intensities, DB intensities, R, t): DB frame = R query frame + t for place i."""
    rng = np.random.default_rng(seed)
    qs, ds, iqs, ids, Rs, ts = [], [], [], [], [], []
    for i in range(c):
        base, inten = synth.scene_cloud(seed, i, P)
        R = _rot((0, -1, 0), rng.random() * 360.0) @ _rot((rng.normal(), 0, rng.normal()), 2.0 * rng.random())
        t = np.array([rng.normal(0, 3), rng.normal(0, 0.2), rng.normal(0, 3)])
        keep = rng.random(P) < 0.9
        q = base[keep]
        qs.append(q + rng.normal(0, 0.02, q.shape)); iqs.append(inten[keep])
        keep = rng.random(P) < 0.9
        d = base[keep]
        ds.append(d @ R.T + t + rng.normal(0, 0.02, d.shape)); ids.append(inten[keep])
        Rs.append(R); ts.append(t)
    return qs, ds, np.concatenate(iqs), np.concatenate(ids), Rs, ts
