"""The committed cases of the ICP tests (test_icp_cpu.py, test_gpu_icp.py): a scene seen twice - the query cloud and the DB cloud are
independent 85 % subsets of it with 2 cm jitter each, the DB cloud moved by a planted rigid motion - and the seed the refinement starts
from.  Scenes: the box scene of synth.scene_cloud (anisotropic) and the whitened ground disk with boxes of test_align._scene.
Seeds: hand-set (identity against a planted yaw of up to 3 degrees and a (0.3, 0.02, -0.2) m offset) or pr_sc_relative_pose's from the
oracle's SC signatures and PCA frames (any planted yaw: the seed is then good to about half a sector and the centroids' alignment).

The seeds below were picked so that the restatement alone (icp_np.icp) keeps, in every pass, the best / second-best d2 of every point and
every d2 / max_corr^2 at least 1e-9 apart relative (test_icp_cpu.py asserts it): device and restatement then provably choose the same
correspondences and inlier sets."""
import functools

import numpy as np

import icp_np
from so_dso_place_recognition_amd import synth

MAX_CORR = 1.0
PARAMS = dict(max_iter=30, max_corr=MAX_CORR, tol_rmse=1e-7, tol_fitness=1e-7, min_inliers=3)
OFFSET = np.array([0.3, 0.02, -0.2])

# name: (scene, points of the scene, rng seed, planted yaw in degrees, seed kind)
CASES = {
    "box300_hand": ("box", 300, 11, 3.0, "hand"),
    "box2000_hand": ("box", 2000, 12, 3.0, "hand"),
    "disk300_hand": ("disk", 300, 13, -2.0, "hand"),
    "disk2000_hand": ("disk", 2000, 14, 3.0, "hand"),
    "box2000_sc": ("box", 2000, 15, 137.0, "sc"),
    "disk2000_sc": ("disk", 2000, 16, -71.0, "sc"),
}


def yaw(theta):
    """Rotation about the camera's up axis (-y), as test_align._yaw."""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])


def sc_seed(q, d):
    """pr_sc_relative_pose's seed from the oracle's SC signatures and PCA frames (the chain of test_align.py, no device)."""
    import oracle_lib
    from test_align import _frame, _sc_variant
    from so_dso_place_recognition_amd import api
    xyz = np.concatenate([q, d])
    inten = np.ones(len(xyz), np.float32)
    sig = oracle_lib.sc_generate(xyz, inten, np.array([0, len(q), len(xyz)], np.int64))
    return api.sc_relative_pose(_frame(q)[None], _frame(d)[None], np.array([_sc_variant(sig[0], sig[1])], np.int32))[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(P query cloud, Q DB cloud, T0 seed, R / t planted: Q's frame = R P's frame + t)."""
    scene, npts, seed, deg, kind = CASES[name]
    rng = np.random.default_rng(seed)
    if scene == "box":
        base = synth.scene_cloud(seed, 0, npts)[0]
    else:
        from test_align import _scene
        base = _scene(rng, npts)
    R, t = yaw(np.radians(deg)), OFFSET.copy()
    P = base[rng.random(npts) < 0.85]
    P = P + rng.normal(0, 0.02, P.shape)
    Q = base[rng.random(npts) < 0.85]
    Q = Q @ R.T + t + rng.normal(0, 0.02, Q.shape)
    T0 = np.hstack([np.eye(3), np.zeros((3, 1))]) if kind == "hand" else sc_seed(P, Q)
    return dict(P=np.ascontiguousarray(P), Q=np.ascontiguousarray(Q), T0=np.ascontiguousarray(T0), R=R, t=t)


@functools.lru_cache(maxsize=None)
def reference(name, order="pairwise"):
    """The restatement's answer for a case (computed once per process, shared by the tests, never modified)."""
    c = case(name)
    return icp_np.icp(c["P"], c["Q"], c["T0"], order=order, **PARAMS)


def pose_error(T, R, t):
    """(rotation error in degrees, translation error in metres) of [R | t] against the planted motion."""
    T = np.asarray(T).reshape(3, 4)
    ang = np.degrees(np.arccos(np.clip((np.trace(T[:, :3].T @ R) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(T[:, 3] - t))


def csr(clouds):
    """list of [n, 3] clouds -> (xyz [sum n, 3], offs [N + 1])."""
    offs = np.zeros(len(clouds) + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    xyz = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3))
    return np.ascontiguousarray(xyz), offs
