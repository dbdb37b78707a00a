"""CPU checks of the alignment layer: pr_sc_relative_pose recovers a known rigid motion from the reference's own SC signatures and PCA
frames (the oracle), with the winning sector shift found by a numpy argmin over the 120 variants of processSC.m:22-33; bad inputs fail."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from so_dso_place_recognition_amd import _lib, api

DELTA = 2 * np.pi / 60


def _scene(rng, P=12000):
    """A camera-frame cloud (x right, y down, z forward): a ground disk of radius 40 m 1.6 m below the sensor and 40 boxes of 1 - 8 m
    height standing on it."""
    n_g = P // 2
    r = 40.0 * np.sqrt(rng.random(n_g))
    a = rng.random(n_g) * 2 * np.pi
    ground = np.stack([r * np.cos(a), np.full(n_g, 1.6), r * np.sin(a)], 1)
    nb = 40
    ctr_r = 6.0 + 26.0 * np.sqrt(rng.random(nb))
    ctr_a = rng.random(nb) * 2 * np.pi
    cx, cz = ctr_r * np.cos(ctr_a), ctr_r * np.sin(ctr_a)
    hx, hz = 0.5 + rng.random(nb), 0.5 + rng.random(nb)
    h = 1.0 + 7.0 * rng.random(nb)
    b = rng.integers(0, nb, P - n_g)
    u = rng.random((P - n_g, 3))
    boxes = np.stack([cx[b] + (2 * u[:, 0] - 1) * hx[b], 1.6 - u[:, 1] * h[b], cz[b] + (2 * u[:, 2] - 1) * hz[b]], 1)
    xyz = np.concatenate([ground, boxes])
    # in-plane spread made exactly isotropic (the boxes' anisotropy whitened away): PCA's in-plane axes then carry no information - the
    # jitter alone picks them, independently in the two clouds - and the yaw must come from the sector shift
    g = xyz[:, [0, 2]]
    mu = g.mean(0)
    w, V = np.linalg.eigh(np.cov((g - mu).T))
    xyz[:, [0, 2]] = (g - mu) @ (V @ np.diag(np.sqrt(w.mean() / w)) @ V.T) + mu
    return xyz


def _yaw(theta):
    """Rotation about the camera's up axis (-y)."""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])


def _frame(xyz):
    _, ev = oracle_lib.align_pca(xyz)                    # columns v0 | v1 | v2 by ascending eigenvalue
    f = np.zeros(16)
    f[:3] = xyz.mean(0)
    f[3:12] = ev.T.reshape(-1)
    f[13] = len(xyz)
    return f


def _sc_variant(q, d):
    """numpy argmin over the 120 variants of processSC.m:22-33 (structure channel): v = 2 s + r."""
    qn = q[:1200] / np.linalg.norm(q[:1200])
    dn = d[:1200] / np.linalg.norm(d[:1200])
    img, dim = qn.reshape(60, 20), dn.reshape(60, 20)
    c = np.arange(60)
    dist = np.empty(120)
    for s in range(60):
        dist[2 * s] = (1 - (img[(s + c) % 60] * dim).sum()) / 2
        dist[2 * s + 1] = (1 - (img[(s - c) % 60] * dim).sum()) / 2
    return int(np.argmin(dist))


def _rot_err_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_sc_relative_pose_recovers_yaw_and_translation():
    rng = np.random.default_rng(7)
    cases = 40
    yaws = rng.random(cases) * 2 * np.pi
    fq, fd, var, Rt, tt = [], [], [], [], []
    for i in range(cases):
        base = _scene(rng)
        R, t = _yaw(yaws[i]), np.array([rng.normal(0, 3), rng.normal(0, 0.2), rng.normal(0, 3)])
        q = base + rng.normal(0, 0.02, base.shape)
        d = base @ R.T + t + rng.normal(0, 0.02, base.shape)
        inten = np.ones(len(base), np.float32)
        xyz = np.concatenate([q, d])
        sig = oracle_lib.sc_generate(xyz, np.concatenate([inten, inten]), np.array([0, len(q), 2 * len(q)], np.int64))
        fq.append(_frame(q)); fd.append(_frame(d))
        var.append(_sc_variant(sig[0], sig[1]))
        Rt.append(R); tt.append(t)
    T = api.sc_relative_pose(np.array(fq), np.array(fd), np.array(var, np.int32))
    assert T.shape == (cases, 3, 4)
    rerr = np.array([_rot_err_deg(T[i, :, :3], Rt[i]) for i in range(cases)])
    terr = np.array([np.linalg.norm(T[i, :, 3] - tt[i]) for i in range(cases)])
    for i in range(cases):
        assert abs(np.linalg.det(T[i, :, :3]) - 1) < 1e-9
    assert rerr.max() <= 4.0, (rerr.max(), np.median(rerr))
    assert terr.max() <= 0.5, terr.max()
    v = np.array(var)
    assert np.any(~np.isin(v % 60, (0, 30)))              # the sector shift itself carries yaw in some case
    assert len(set((v >> 1).tolist())) > 4


def test_sc_relative_pose_rejects_bad_inputs():
    lib = _lib.load()
    f = np.zeros((1, 16)); f[0, 3:12] = np.eye(3).reshape(-1); f[0, 13] = 100
    T = np.empty((1, 3, 4))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for bad in (-1, 120, 1000):
        v = np.array([bad], np.int32)
        assert lib.pr_sc_relative_pose(p(f), p(f), p(v), 1, p(T)) == _lib.PR_EINVAL
        assert b"variant" in lib.pr_last_error(None)
    few = f.copy(); few[0, 13] = 2
    v = np.array([7], np.int32)
    assert lib.pr_sc_relative_pose(p(f), p(few), p(v), 1, p(T)) == _lib.PR_EINVAL
    assert lib.pr_sc_relative_pose(p(few), p(f), p(v), 1, p(T)) == _lib.PR_EINVAL
    assert lib.pr_sc_relative_pose(p(f), p(f), p(v), 1, p(T)) == _lib.PR_OK
    with pytest.raises(_lib.PRError):
        api.sc_relative_pose(f, f, [120])


def test_sc_relative_pose_identity_frames():
    """Identity frames: v = 2 s is a yaw of -s sectors in the y'z' plane, v = 2 s + 1 the reflection with det(R) kept at +1."""
    f = np.zeros((4, 16)); f[:, 3:12] = np.eye(3).reshape(-1); f[:, 13] = 10
    f[:, :3] = [1.0, 2.0, 3.0]
    T = api.sc_relative_pose(f, f, [0, 2 * 15, 1, 2 * 7 + 1])
    assert np.allclose(T[0], np.hstack([np.eye(3), np.zeros((3, 1))]), atol=1e-15)
    a = 15 * DELTA
    assert np.allclose(T[1, 1:, 1:3], [[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], atol=1e-15)
    for i in range(4):
        assert abs(np.linalg.det(T[i, :, :3]) - 1) < 1e-12
        assert np.allclose(T[i, :, :3] @ f[i, :3] + T[i, :, 3], f[i, :3])     # the centroid maps onto the centroid
    assert T[2, 0, 0] == -1.0 and T[3, 0, 0] == -1.0                           # a reflection in y'z' flips the height axis


def test_cli_align_out_needs_a_type_with_variants():
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "so_dso_place_recognition_amd", "bin", "match_signatures")
    for t in ("gist", "bow"):
        r = subprocess.run([exe, "--type", t, "--hist1", "a", "--hist2", "b", "--out", "c", "--align_out", "d"], capture_output=True, text=True)
        assert r.returncode == 1 and "--align_out" in r.stderr
