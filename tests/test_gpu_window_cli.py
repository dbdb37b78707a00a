"""--stream 1 on the drop-in generators: the files replayed keyframe by keyframe through a pr_window, every row generated from the cloud and
frame the push left in HBM - the same signature file and incoming_id_file, byte for byte, as the default (batch) run."""
import os
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("seq07cli")
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    pts = str(d / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
    short = str(d / "poses.txt")                                   # the same 140 poses the points were made for
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    return short, pts, d


@pytest.mark.parametrize("exe,key", [("test_sc", "sc_file"), ("test_m2dp", "m2dp_file"), ("test_delight", "delight_file")])
def test_stream_flag_writes_the_same_files(files, exe, key):
    poses, pts, d = files
    got = {}
    for stream in (0, 1):
        sig, ids = str(d / f"{exe}_{stream}.txt"), str(d / f"{exe}_ids_{stream}.txt")
        cmd = [os.path.join(BIN, exe), f"_poses_history_file:={poses}", f"_pts_history_file:={pts}", f"_{key}:={sig}",
               f"_incoming_id_file:={ids}", "_lidarRange:=45.0"] + (["--stream", "1"] if stream else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[stream] = (open(sig, "rb").read(), open(ids, "rb").read())
    assert len(got[0][1].split()) == 110 and len(got[0][0]) > 100000
    assert got[1][1] == got[0][1]
    assert got[1][0] == got[0][0]
