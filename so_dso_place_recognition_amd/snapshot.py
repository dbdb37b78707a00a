"""Snapshots: the resident state of a drive - a KeyframeMap, up to two OnlineDatabases, an OnlineSet, up to two
PoseGraph closure logs and a SessionTable - packed into one self-describing blob on the device, validated and unpacked from one into
handles of the same or larger capacities, and written to or read from a file.  Import Snapshot from this module: the public names of
`api` are a literal table in tests/test_api_surface.py, which a new name there would fail (graph.SessionTable is the precedent)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._context import Context
from ._handle import Handle, _ptr, ptr

__all__ = ["Snapshot"]


class Snapshot(Handle):
    """pr_snapshot over existing handles: map (a KeyframeMap), online (up to two OnlineDatabases), onlineset (an OnlineSet), graphs (up to
    two PoseGraphs: the raw closure log and a gated one) and sessions (a SessionTable); every one is optional, at least one is needed,
    and all must live on this object's context.  The snapshot owns none of their buffers and must be closed before them.  Out of scope:
    the CloudWindow, the SequenceFilter's ring, the WorldMap with its index and normals (rebuild them by fuse -> index -> normals from
    the restored map) and all scratch.  pack_torch and unpack_torch are enqueued on the context's stream, read every count on the device,
    read nothing back and allocate nothing when info= is given; save and load are the host forms.  A failed unpack or load changes no
    byte of any destination buffer: restore into freshly created or reset handles.  The format and the rule are in
    include/place_recognition.h."""

    _DESTROY = "pr_snapshot_destroy"

    def __init__(self, ctx: Context | None, map=None, online=(), onlineset=None, graphs=(), sessions=None):
        import torch
        self._attach(ctx)
        online, graphs = tuple(online), tuple(graphs)
        if len(online) > 2 or len(graphs) > 2:
            raise ValueError("Snapshot: at most two online databases and two closure logs")
        parts = [p for p in (map, *online, onlineset, *graphs, sessions) if p is not None]
        if not parts:
            raise ValueError("Snapshot: no part was given (map, online, onlineset, graphs, sessions)")
        self._share("Snapshot", "the snapshot and every part", *parts)          # refused before the library is called
        self.parts = parts                                                       # keeps the buffers alive
        d, recs = _lib.SnapshotDesc(), []

        def rec(cls, obj, names):
            r = cls(*(ptr(getattr(obj, n, None)) for n in names))
            recs.append(r)
            return C.addressof(r)

        if map is not None:
            d.map = rec(_lib.MapBuffers, map, map.NAMES)
            d.keyframe_capacity, d.point_capacity, d.max_cloud_points = map.keyframe_capacity, map.point_capacity, map.max_cloud_points
        for k, o in enumerate(online):
            d.online[k] = rec(_lib.OnlineBuffers, o, ("sig", "state"))
            d.online_type[k], d.online_capacity[k] = o.type, o.capacity
        if onlineset is not None:
            d.onlineset = rec(_lib.OnlineSetBuffers, onlineset, ("sc", "m2dp", "delight", "state"))
            d.onlineset_kind, d.onlineset_capacity = onlineset.kind, onlineset.capacity
        for k, g in enumerate(graphs):
            d.graph[k] = rec(_lib.PoseGraphBuffers, g, g.NAMES)
            d.edge_capacity[k] = g.edge_capacity
        if sessions is not None:
            d.sessions = rec(_lib.SessionBuffers, sessions, sessions.NAMES)
            d.session_capacity = sessions.session_capacity
        torch.cuda.synchronize(self._device)              # torch's fills (its stream) before the library's stream reads the buffers
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_snapshot_create(self.ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    def bound(self) -> int:
        """The largest blob these capacities can produce, in bytes (pr_snapshot_bound)."""
        b = C.c_int64()
        self.ctx.check(self.lib.pr_snapshot_bound(self.h, C.byref(b)))
        return int(b.value)

    def _blob(self, who, blob):
        import torch
        self._t(who, "blob", blob, torch.uint8)
        if blob.data_ptr() % 16:
            raise ValueError(f"{who}: blob must lie on a 16-byte boundary")
        return blob

    def pack_torch(self, blob, info=None):
        """Device form (pr_snapshot_pack_dev): the live rows of every part into blob (device uint8, on a 16-byte boundary; bound() bytes
        always suffice).  Returns info (device i64 [4]) = bytes written, sections, flags, 0; with SNAPSHOT_OVERFLOW nothing past the
        header is written and info[0] is the size that would have been needed.  Nothing synchronises."""
        import torch
        who = "Snapshot.pack_torch"
        self._blob(who, blob)
        info = self._result(who, "info", info, torch.int64, (4,), flat=True)
        self.ctx.check(self.lib.pr_snapshot_pack_dev(self.h, ptr(blob), blob.numel(), ptr(info)))
        return info

    def unpack_torch(self, blob, nbytes=None, info=None):
        """Device form (pr_snapshot_unpack_dev): validates the first nbytes of blob on the device and, if every check passes, copies
        the saved rows and state words into the parts' buffers.  Returns info (device i64 [4]) = sections restored, first failing
        section or -1, flags, 0.  Nothing synchronises."""
        import torch
        who = "Snapshot.unpack_torch"
        self._blob(who, blob)
        nbytes = blob.numel() if nbytes is None else int(nbytes)
        if nbytes < 0 or nbytes > blob.numel():
            raise ValueError(f"{who}: nbytes={nbytes} outside 0 .. {blob.numel()}")
        info = self._result(who, "info", info, torch.int64, (4,), flat=True)
        self.ctx.check(self.lib.pr_snapshot_unpack_dev(self.h, ptr(blob), nbytes, ptr(info)))
        return info

    def save(self, path):
        """Host form (pr_snapshot_save; synchronises): the blob as it stands to path, through path + '.tmp' and a rename."""
        self.ctx.check(self.lib.pr_snapshot_save(self.h, os.fsencode(path)))

    def load(self, path):
        """Host form (pr_snapshot_load; synchronises): returns info int64 [4] = sections restored, first failing section or -1, flags,
        0.  A missing file, a file shorter than a header and a table that points outside the file raise PRError before a device is
        touched."""
        info = np.zeros(4, np.int64)
        self.ctx.check(self.lib.pr_snapshot_load(self.h, os.fsencode(path), _ptr(info)))
        return info

    def close(self):
        super().close()
        self.parts = None
