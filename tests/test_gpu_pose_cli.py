"""match_signatures --icp_out beyond the SC single-hypothesis form (test_gpu_icp.py covers that one): --type delight, and --icp_hyp 2 for
SC with the kept hypothesis appended, on the first poses of the committed seq07 fixture.  The executable's lines against the same chain
through the Python forms (match_align -> relative_pose / sc_relative_pose -> icp_refine, hypotheses chosen by pose_np.select): integer
columns equal, fitness equal, rmse and [R | t] within 1e-10 (DESIGN.md 4.11's bound between launch geometries: the executable refines
all hypotheses in one call, the comparison one hypothesis per call).  --type m2dp stays refused (test_gpu_icp.py pins that)."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import pose_np
from so_dso_place_recognition_amd import _lib, api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")
TOL = 1e-10


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_cli")
    full = open(os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")).read().split("\n")
    poses, pts = str(d / "poses_history_file.txt"), str(d / "pts_history_file.txt")
    open(poses, "w").write("\n".join(full[:60]) + "\n")
    helpers.write_synthetic_points(poses, pts, per_pose=60)
    return d, poses, pts


def generate(exe, key, d, poses, pts):
    sig = str(d / f"history_{exe}.txt")
    r = subprocess.run([os.path.join(BIN, exe), f"_poses_history_file:={poses}", f"_pts_history_file:={pts}", f"_{key}:={sig}",
                        f"_incoming_id_file:={d / ('ids_' + exe + '.txt')}", "_lidarRange:=45.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return sig


def run_cli(type_, sig, d, poses, pts, k, extra=()):
    out, icp = str(d / f"out_{type_}.txt"), str(d / f"icp_{type_}.txt")
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", type_, "--hist1", sig, "--hist2", sig, "--mask_width", "5", "--topk", str(k),
                        "--out", out, "--icp_out", icp, "--poses1", poses, "--pts1", pts, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    h = np.loadtxt(sig)
    return h, np.loadtxt(out), np.loadtxt(icp, ndmin=2)


def expected(type_, h, ix, xyz, offs, fr, H):
    """Per hypothesis the Python chain, then the select rule: rows [m k, 18 (+ hyp)]."""
    m, k = ix.shape
    var, _ = api.match_align(type_, h, h, ix)
    per = []
    for hh in range(H):
        v = var[..., hh].copy()
        if hh > 0:
            v[v == var[..., 0]] = -1
        has = ((ix >= 0) & (v >= 0)).reshape(-1)
        src = np.where(has, np.repeat(np.arange(m), k), -1).astype(np.int32); dst = np.where(has, ix.reshape(-1), -1).astype(np.int32)
        T0 = np.tile(pose_np.IDENT, (m * k, 1, 1))
        if has.any():
            T0[has] = api.relative_pose(type_, fr[src[has]], fr[dst[has]], v.reshape(-1)[has])
        T, st = api.icp_refine(xyz, offs, xyz, offs, src, dst, T0)
        per.append((T, st, dst))
    rows = []
    for e in range(m * k):
        sh = np.array([per[hh][1][e] for hh in range(H)])
        kept, _ = pose_np.select(sh, 0.0, np.inf)
        T, st, dst = per[kept]
        row = [e // k, dst[e], st[e]["status"], st[e]["iters"], st[e]["fitness"], st[e]["rmse"], *T[e].reshape(-1)]
        rows.append(row + ([kept] if H == 2 else []))
    return np.array(rows, np.float64), per


def compare(got, want):
    assert got.shape == want.shape
    ints = [0, 1, 2, 3] + ([18] if want.shape[1] == 19 else [])
    assert np.array_equal(got[:, ints], want[:, ints]), np.flatnonzero((got[:, ints] != want[:, ints]).any(1))[:8]
    assert np.array_equal(got[:, 4], want[:, 4])
    d = np.abs(got[:, 5:18] - want[:, 5:18]).max()
    print("   executable against the Python chain: max |d rmse, dT| %.2e" % d)
    assert d <= TOL


def test_cli_icp_out_delight(files):
    d, poses, pts = files
    sig = generate("test_delight", "delight_file", d, poses, pts)
    k = 2
    h, out, got = run_cli("delight", sig, d, poses, pts, k)
    m = len(h) // 16
    ix = out.reshape(m, k, 2)[..., 0].astype(np.int32)
    xyz, it, offs, _ = api.pts_preprocess(poses, pts, None, 45.0, True, gpu=True)       # DELIGHT's generator reads the polar-filtered clouds
    assert len(offs) - 1 == m
    want, per = expected("delight", h, ix, xyz, offs, api.cloud_frames(xyz, it, offs), 1)
    assert got.shape == (m * k, 18)
    compare(got, want)
    assert (per[0][1]["status"] != _lib.ICP_NO_PAIR).sum() > m


def test_cli_icp_hyp_2_sc_appends_the_kept_hypothesis(files):
    d, poses, pts = files
    sig = generate("test_sc", "sc_file", d, poses, pts)
    k = 2
    h, out, got = run_cli("sc", sig, d, poses, pts, k, ("--icp_hyp", "2"))
    m = len(h)
    ix = out.reshape(m, k, 2)[..., 0].astype(np.int32)
    xyz, it, offs, _ = api.pts_preprocess(poses, pts, None, 45.0, False, gpu=True)
    want, per = expected("sc", h, ix, xyz, offs, api.cloud_frames(xyz, it, offs), 2)
    assert got.shape == (m * k, 19)
    compare(got, want)
    second = per[1][1]["status"] != _lib.ICP_NO_PAIR
    print("   second hypotheses refined:", int(second.sum()), "kept:", int(want[:, 18].sum()))
    assert second.any()                                                        # the channels disagree somewhere: a second hypothesis ran
    h1 = np.loadtxt(str(d / "icp_sc.txt"), ndmin=2)
    _, _, got1 = run_cli("sc", sig, d, poses, pts, k)                          # without the flag: the 18 columns, hypothesis 0
    assert got1.shape == (m * k, 18) and h1.shape == (m * k, 19)


def test_cli_icp_out_refusals():
    base = [os.path.join(BIN, "match_signatures"), "--hist1", "a", "--hist2", "b", "--out", "c", "--icp_out", "d", "--poses1", "p", "--pts1", "q"]
    for extra in (["--type", "m2dp"], ["--type", "gist"], ["--type", "delight", "--icp_hyp", "2"], ["--type", "sc", "--icp_hyp", "3"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "--icp_out" in r.stderr, extra
