"""What tests/test_gpu_snapshot.py and its child process tests/snapshot_child.py share: a Rig builds the device handles of a snapshot
spec over GUARDED buffers (longer than stated, the excess filled with a pattern), moves a snapshot_np state to and from them, and holds
the Snapshot over them.

A spec is a dict: map (keyframe_capacity, point_capacity, max_cloud_points) | None, online ((type name, capacity), ...), set (kind name,
capacity) | None, graphs (edge_capacity, ...), sessions session_capacity | None, nodes (the node capacity of logs and table)."""
import ctypes as C
import os

import numpy as np
import torch

import helpers
import snapshot_np as sp
from so_dso_place_recognition_amd import _lib, api, graph
from so_dso_place_recognition_amd.matcher import _stream_context
from so_dso_place_recognition_amd.snapshot import Snapshot

GUARD_BYTE, GUARD_ROWS = 0xE7, 3
TYPES = {"sc": sp.TYPE_SC, "m2dp": sp.TYPE_M2DP}
KINDS = {"fused": sp.SET_FUSED, "delight": sp.SET_DELIGHT}
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


def spec_state(spec):
    """the snapshot_np state (zeroed arrays at full capacity) of a spec, in blob order"""
    st = []
    if spec.get("map"):
        st.append(sp.map_part(*spec["map"]))
    st += [sp.online_part(TYPES[t], c) for t, c in spec.get("online", ())]
    if spec.get("set"):
        st.append(sp.set_part(KINDS[spec["set"][0]], spec["set"][1]))
    st += [sp.graph_part(k, c) for k, c in enumerate(spec.get("graphs", ()))]
    if spec.get("sessions"):
        st.append(sp.session_part(spec["sessions"]))
    return st


class Rig:
    def __init__(self, spec, ctx=None):
        self.spec, self.own_ctx = spec, ctx is None
        self.ctx = ctx or _stream_context(0)
        self.model = spec_state(spec)                   # the shapes; its arrays are overwritten by download()
        self.big, self.handles = [], []
        nodes = spec.get("nodes", 8)

        def guarded(part):
            bufs, big = {}, {}
            for name, arr in list(part["arrays"].items()) + [("state", part["state"])]:
                rows = arr.shape[0]
                t = torch.full((rows + GUARD_ROWS,) + arr.shape[1:], 0, dtype=_TORCH[arr.dtype], device="cuda")
                t.view(torch.uint8).fill_(GUARD_BYTE)
                t[:rows] = 0
                big[name], bufs[name] = t, t[:rows]
            self.big.append(big)
            return bufs

        it = iter(self.model)
        self.map = self.set = self.sessions = None
        self.online, self.graphs = [], []
        if spec.get("map"):
            self.map = api.KeyframeMap(self.ctx, *spec["map"], buffers=guarded(next(it)))
            self.handles.append(self.map)
        for t, c in spec.get("online", ()):
            self.online.append(api.OnlineDatabase(self.ctx, t, c, buffers=guarded(next(it))))
            self.handles.append(self.online[-1])
        if spec.get("set"):
            self.set = api.OnlineSet(self.ctx, spec["set"][0], spec["set"][1], buffers=guarded(next(it)))
            self.handles.append(self.set)
        for c in spec.get("graphs", ()):
            self.graphs.append(api.PoseGraph(self.ctx, nodes, c, buffers=guarded(next(it))))
            self.handles.append(self.graphs[-1])
        if spec.get("sessions"):
            self.sessions = graph.SessionTable(self.ctx, nodes, min(max(spec.get("graphs", (1,))), 65536), spec["sessions"], buffers=guarded(next(it)))
            self.handles.append(self.sessions)
        self.snap = Snapshot(self.ctx, map=self.map, online=self.online, onlineset=self.set, graphs=self.graphs, sessions=self.sessions)
        self.info = torch.zeros(4 + GUARD_ROWS, dtype=torch.int64, device="cuda")

    def buffers(self):
        """[(part index, name, tensor)] of every caller-owned buffer, the state last"""
        out = []
        for p, (part, h) in enumerate(zip(self.model, self.handles)):
            out += [(p, name, getattr(h, name)) for name in list(part["arrays"]) + ["state"]]
        return out

    def upload(self, state):
        for p, name, t in self.buffers():
            src = state[p]["state"] if name == "state" else state[p]["arrays"][name]
            t.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(t.shape))
        self.ctx.sync()

    def fill_bytes(self, byte):
        for _, _, t in self.buffers():
            t.view(torch.uint8).fill_(byte)
        self.ctx.sync()

    def download(self):
        """the device buffers as a snapshot_np state"""
        self.ctx.sync()
        st = spec_state(self.spec)
        for p, name, t in self.buffers():
            a = t.cpu().numpy()
            if name == "state":
                st[p]["state"] = a.copy()
            else:
                st[p]["arrays"][name] = a.copy().reshape(st[p]["arrays"][name].shape)
        return st

    def intact(self):
        """no guard row behind any buffer was written"""
        for big, part in zip(self.big, self.model):
            for name, t in big.items():
                rows = (part["state"] if name == "state" else part["arrays"][name]).shape[0]
                assert bool((t[rows:].contiguous().view(torch.uint8) == GUARD_BYTE).all()), name

    def blob(self, nbytes, guard=256):
        """a device blob of nbytes + guard bytes, every byte the guard pattern; on a 16-byte boundary"""
        return torch.full((int(nbytes) + guard,), GUARD_BYTE, dtype=torch.uint8, device="cuda")

    def pack(self, capacity=None):
        """packs into a guarded blob -> (all its bytes as numpy, info); capacity: the blob_capacity passed (default: bound())"""
        cap = self.snap.bound() if capacity is None else capacity
        b = self.blob(cap)
        self.info.fill_(-7)
        self.snap.pack_torch(b[:cap], info=self.info[:4])
        self.ctx.sync()
        info = self.info.cpu().numpy()
        assert (info[4:] == -7).all()
        return b.cpu().numpy(), info[:4].copy()

    def unpack(self, raw, nbytes=None):
        """uploads raw (numpy uint8) and unpacks its first nbytes -> info"""
        b = self.blob(len(raw), guard=64)
        b[:len(raw)] = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        self.info.fill_(-7)
        self.snap.unpack_torch(b[:len(raw)], len(raw) if nbytes is None else nbytes, info=self.info[:4])
        self.ctx.sync()
        info = self.info.cpu().numpy()
        assert (info[4:] == -7).all()
        return info[:4].copy()

    def close(self):
        self.snap.close()
        for h in reversed(self.handles):
            h.close()
        if self.own_ctx:
            self.ctx.close()


def seq07_batch_clouds(golden_dir, workdir):
    """the 110 keyframe clouds of the committed seq07 drive (the first 140 poses, synthetic points as in test_gpu_map.py) from the BATCH
    pre-stage, with their frames, poses and ids: host arrays xyz, inten, offs, frames, poses, ids"""
    poses = os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")
    pts = os.path.join(workdir, "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60, max_poses=140)
    short = os.path.join(workdir, "poses140.txt")
    open(short, "w").write("\n".join([l for l in open(poses).read().split("\n") if l.strip()][:140]) + "\n")
    pid, w, qid, xyz, it = api.read_poses_points(short, pts)
    lib = _lib.load()
    ctx = api.Context(0)
    h = C.c_void_p()
    ctx.check(lib.pr_pts_preprocess_gpu(ctx.h, short.encode(), pts.encode(), None, 45.0, 0, 0, C.byref(h)))
    try:
        N = int(lib.pr_clouds_count(h))
        T = int(np.ctypeslib.as_array(lib.pr_clouds_offs(h), (N + 1,))[-1])
        hip = C.CDLL("libamdhip64.so")

        def dev_array(ptr, shape, dtype):                  # a copy of library-owned device memory
            t = torch.empty(int(np.prod(shape)), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(t.numel() * t.element_size()), 3) == 0
            return t.reshape(shape).cpu().numpy()
        res = dict(xyz=dev_array(lib.pr_clouds_dev_xyz(h), (T, 3), torch.float64), inten=dev_array(lib.pr_clouds_dev_inten(h), (T,), torch.float32),
                   offs=dev_array(lib.pr_clouds_dev_offs(h), (N + 1,), torch.int64), frames=dev_array(lib.pr_clouds_dev_frames(h), (N, 16), torch.float64),
                   poses=w[30:].reshape(N, 12), ids=pid[30:].astype(np.int32))
    finally:
        lib.pr_clouds_free(h)
        ctx.close()
    assert N == 110
    return res
