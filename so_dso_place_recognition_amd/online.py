"""The online signature databases and the sequence filter: device-resident handles whose count lives on
the device, so that one captured step serves every keyframe of a drive.  `api` re-exports every name."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._context import Context
from ._handle import Handle, _ptr, ptr

__all__ = ["OnlineDatabase", "OnlineSet", "SequenceFilter", "seq_steps", "seq_tile"]

def seq_steps(L: int, velocities) -> np.ndarray:
    """The step table of the sequence matcher, i32 [V, L]: row v holds, for query lag l, how many DB rows behind the
    candidate the trajectory of velocity velocities[v] lies: sign(v) * floor(|v| l + 0.5).  Negative velocities are a reverse traversal,
    0 a standstill.  Identical rows are dropped, keeping the first."""
    L = int(L)
    if not 1 <= L <= _lib.SEQ_MAX_L:
        raise ValueError(f"seq_steps: L must be in 1 .. {_lib.SEQ_MAX_L}")
    rows = []
    for v in velocities:
        v = float(v)
        if not np.isfinite(v):
            raise ValueError("seq_steps: a velocity is not finite")
        sg = (v > 0) - (v < 0)
        row = [int(sg * np.floor(abs(v) * l + 0.5)) for l in range(L)]
        if max(abs(s) for s in row) > _lib.SEQ_MAX_STEP:
            raise ValueError(f"seq_steps: velocity {v} reaches beyond {_lib.SEQ_MAX_STEP} rows within {L} lags")
        if row not in rows:
            rows.append(row)
    if not 1 <= len(rows) <= _lib.SEQ_MAX_V:
        raise ValueError(f"seq_steps: 1 .. {_lib.SEQ_MAX_V} distinct velocities")
    return np.array(rows, np.int32).reshape(len(rows), L)


def seq_tile():
    """(rows, cols) of the batch kernel's tile (pr_seq_tile); needs no device."""
    lib = _lib.load()
    r, c = C.c_int32(), C.c_int32()
    lib.pr_seq_tile(C.byref(r), C.byref(c))
    return int(r.value), int(c.value)


def _check_steps(steps, who):
    st = np.ascontiguousarray(steps, np.int32)
    if st.ndim != 2 or not (1 <= st.shape[0] <= _lib.SEQ_MAX_V and 1 <= st.shape[1] <= _lib.SEQ_MAX_L) or (st[:, 0] != 0).any() \
            or np.abs(st).max() > _lib.SEQ_MAX_STEP:
        raise ValueError(f"{who}: steps must be i32 [V <= {_lib.SEQ_MAX_V}, L <= {_lib.SEQ_MAX_L}] with steps[:, 0] == 0 and "
                         f"|steps| <= {_lib.SEQ_MAX_STEP} (api.seq_steps builds one)")
    return st


class _OnlineEngine(Handle):
    """What OnlineDatabase and OnlineSet share - the two front ends of ONE engine (online.hip): the buffers, made or validated from
    .parts = ((name, rows per entry, row length), ...); the checks of emitted= / out= / rows= / info=; match, append, step, reset and
    count.  A subclass names itself (_WHO), its C family (_C, and _DESTROY for the base), its buffers record (_REC) and the order in which the family's calls
    take the part pointers (_ORDER; None for a part this object does not have), and sets .parts and .channels before _create."""

    def _create(self, ctx, code, capacity, max_k, buffers):
        import torch
        self._attach(ctx)
        self.capacity, self.max_k = int(capacity), int(max_k)
        cap = max(self.capacity, 0)
        shapes = {**{n: ((cap * r, L), torch.float64) for n, r, L in self.parts}, "state": ((4,), torch.int32)}
        self._buffers(self._WHO, shapes, buffers)
        torch.cuda.synchronize(self._device)              # torch's fills (its stream) before the library's stream writes the buffers
        rec = self._REC(*(ptr(getattr(self, n)) if n in shapes else None for n, _ in self._REC._fields_))
        h = C.c_void_p()
        self.ctx.check(self._fn("create")(self.ctx.h, code, C.byref(rec), self.capacity, self.max_k, C.byref(h)))
        self.h = h

    def _fn(self, name):
        return getattr(self.lib, f"{self._C}_{name}")

    def _sigs(self, sigs, who, emitted=None):
        """the call's part tensors, checked (as is emitted=), and their pointers in the C family's order"""
        import torch
        ts = tuple(sigs) if isinstance(sigs, (tuple, list)) else (sigs,)
        if len(ts) != len(self.parts):
            raise ValueError(f"{who}: sigs must hold {len(self.parts)} tensor(s): " + ", ".join(n for n, _, _ in self.parts))
        for t, (n, r, L) in zip(ts, self.parts):
            self._t(who, n, t, torch.float64, numel=r * L, msg=f"{who}: {n} must be a contiguous CUDA tensor f64 [{r}, {L}]")
        if emitted is not None:
            self._t(who, "emitted", emitted, torch.int32, numel_min=1, msg=f"{who}: emitted must be a CUDA tensor i32 [>= 1]")
        at = {n: ptr(t) for t, (n, _, _) in zip(ts, self.parts)}
        return ts, tuple(at.get(n) for n in self._ORDER)

    def _idx(self, who, idx):
        """align's idx i32 [1, k], checked; -> k"""
        import torch
        msg = f"{who}: idx must be a contiguous CUDA tensor i32 [1, k]"
        self._t(who, "idx", idx, torch.int32, msg=msg)
        if idx.dim() != 2 or idx.shape[0] != 1:
            raise ValueError(msg)
        return idx.shape[1]

    def match_torch(self, sigs, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, emitted=None, out=None, rows=None):
        """Device form (<family>_match_dev): the query's part(s) against the rows held NOW (the count is read on the device); the query
        counts as row `count` for the mask.  emitted i32 [>= 1] | None: emitted[0] == 0 switches the call off on the device (idx = -1,
        score = NaN).  Returns (idx int32 [1, k], score float64 [1, k]) - the shape verify takes; out: an earlier call's pair, written
        again.  rows f64 [channels, capacity] | None receives the distances (the first `count` of each row): 'sc' structure, intensity;
        'm2dp' count, intensity; 'fused' those four; 'delight' its one (no p_weight).  Nothing synchronises or, given out=, allocates."""
        import torch
        who = f"{self._WHO}.match_torch"
        _, parts = self._sigs(sigs, who, emitted)
        k = int(k)
        if rows is not None:
            self._t(who, "rows", rows, torch.float64, shape=(self.channels, self.capacity),
                    msg=f"{who}: rows must be a contiguous CUDA tensor f64 [{self.channels}, capacity]")
        o, msg = out or (None, None), f"{who}: out must be (idx i32 [1, k], score f64 [1, k]) CUDA tensors"
        shape = (1, max(k, 0) if out is None else k)
        out = (self._result(who, "out[0]", o[0], torch.int32, shape, msg=msg), self._result(who, "out[1]", o[1], torch.float64, shape, msg=msg))
        self.ctx.check(self._fn("match_dev")(self.h, *parts, ptr(emitted), int(mask_width), float(p_weight), k, ptr(out[0]), ptr(out[1]), ptr(rows)))
        return out

    def append_torch(self, sigs, emitted=None, info=None):
        """Device form (<family>_append_dev, one launch): every part becomes row `count`, then the one count is committed (emitted as in
        match_torch).  Returns info (device i32 [4]) = appended, row | -1, count after, flags."""
        import torch
        who = f"{self._WHO}.append_torch"
        _, parts = self._sigs(sigs, who, emitted)
        info = self._result(who, "info", info, torch.int32, (4,), flat=True, msg=f"{who}: info must be a CUDA tensor i32 [4]")
        self.ctx.check(self._fn("append_dev")(self.h, *parts, ptr(emitted), ptr(info)))
        return info

    def step_torch(self, sigs, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, emitted=None, out=None, rows=None, info=None):
        """One keyframe: match_torch against the rows seen so far, then append_torch of the same part(s).  Returns (idx, score, info)."""
        idx, score = self.match_torch(sigs, mask_width, p_weight, k, emitted=emitted, out=out, rows=rows)
        return idx, score, self.append_torch(sigs, emitted=emitted, info=info)

    def append(self, sigs):
        """Host form (<family>_append; synchronises): sigs numpy array(s) of the parts' sizes.  Returns info int32 [4]."""
        hs = tuple(sigs) if isinstance(sigs, (tuple, list)) else (sigs,)
        if len(hs) != len(self.parts):
            raise ValueError(f"{self._WHO}.append: sigs must hold {len(self.parts)} array(s)")
        arr = {n: np.ascontiguousarray(a, np.float64).reshape(-1) for a, (n, _, _) in zip(hs, self.parts)}
        for n, r, L in self.parts:
            if len(arr[n]) != r * L:
                raise ValueError(f"{self._WHO}.append: {n} must hold {r} x {L} numbers")
        info = np.empty(4, np.int32)
        self.ctx.check(self._fn("append")(self.h, *(_ptr(arr[n]) if n in arr else None for n in self._ORDER), _ptr(info)))
        return info

    def reset(self):
        self.ctx.check(self._fn("reset")(self.h))

    def count(self):
        """(count, flags); synchronises (<family>_count)."""
        n, f = C.c_int32(), C.c_int32()
        self.ctx.check(self._fn("count")(self.h, C.byref(n), C.byref(f)))
        return int(n.value), int(f.value)


class OnlineDatabase(_OnlineEngine):
    """pr_online: the raw SC or M2DP rows of the keyframes seen so far with a DEVICE-side count, matched exactly in fp64 and grown on the
    stream - the sibling of KeyframeMap for signatures.  type_ 'sc' | 'm2dp'; the two buffers are zeroed torch tensors
    on the context's device (or the caller's: buffers = dict(sig=, state=)): .sig [capacity * rows_per_sig, sig_len] f64 (1 x 2400 /
    4 x 384) and .state [4] i32 = count, flags, 0, 0.  Every call's launch geometry depends on capacity and max_k only and the count is
    read on the device, so ONE captured step_torch serves every keyframe of a drive.  At count == capacity an append stores nothing and
    sets ONLINE_OVERFLOW in info[3] until reset().  There is no error: nothing is read back.  All *_torch calls are enqueued on the
    context's stream (the caller orders it against the producers of the inputs, e.g. a Context made on torch's current stream)."""

    NAMES = ("sig", "state")
    _WHO, _C, _DESTROY, _REC, _ORDER = "OnlineDatabase", "pr_online", "pr_online_destroy", _lib.OnlineBuffers, ("sig",)

    def __init__(self, ctx: Context | None, type_: str, capacity: int, max_k: int = 8, buffers: dict | None = None):
        if type_ not in ("sc", "m2dp"):
            raise ValueError("OnlineDatabase: type_ is 'sc' or 'm2dp'")
        self.type_name, self.type = type_, {"sc": _lib.TYPE_SC, "m2dp": _lib.TYPE_M2DP}[type_]
        self.rows_per_sig, self.sig_len = (1, 2400) if type_ == "sc" else (4, 384)
        self.parts, self.channels = (("sig", self.rows_per_sig, self.sig_len),), 2
        self._create(ctx, self.type, capacity, max_k, buffers)

    # The engine's calls (documented there) of the one part: sig f64 [rows_per_sig, sig_len], rows f64 [2, capacity].
    def match_torch(self, sig, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, emitted=None, out=None, rows=None):
        return super().match_torch(sig, mask_width, p_weight, k, emitted=emitted, out=out, rows=rows)

    def append_torch(self, sig, emitted=None, info=None):
        return super().append_torch(sig, emitted=emitted, info=info)

    def step_torch(self, sig, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, emitted=None, out=None, rows=None, info=None):
        return super().step_torch(sig, mask_width, p_weight, k, emitted=emitted, out=out, rows=rows, info=info)

    def append(self, sig):
        return super().append((sig,))                     # (a list of numbers is one part, not a list of parts)

    def align(self, idx, sig, out=None):
        """The best-aligning variant of the pairs (query sig, row idx[0, j]) from the raw rows in place (pr_align_pairs_dev with n_local =
        capacity): (variant int32 [1, k, 2], dist float64 [1, k, 2]) per channel, as Matcher.align returns them - the variants are what
        KeyframeMap.verify_variants takes.  idx int32 [1, k] as match_torch returns it (-1: no pair).  out: an earlier call's pair."""
        import torch
        who = "OnlineDatabase.align"
        self._sigs(sig, who)
        k = self._idx(who, idx)
        ch = slice(0, 2) if self.type == _lib.TYPE_SC else slice(2, 4)
        if out is None:
            var = torch.empty((1, k, 4), dtype=torch.int32, device=idx.device)
            dist = torch.empty((1, k, 4), dtype=torch.float64, device=idx.device)
        else:
            var, dist = out[0]._base, out[1]._base
            if var is None or dist is None or tuple(var.shape) != (1, k, 4) or tuple(dist.shape) != (1, k, 4):
                raise ValueError(f"{who}: out must be the pair an earlier align() of the same k returned")
        sc = (ptr(sig), ptr(self.sig), _lib.F64) if self.type == _lib.TYPE_SC else (None, None, 0)
        m2 = (ptr(sig), ptr(self.sig), _lib.F64) if self.type == _lib.TYPE_M2DP else (None, None, 0)
        self.ctx.check(self.lib.pr_align_pairs_dev(self.ctx.h, *sc, *m2, 1, self.capacity, 0, k, ptr(idx), ptr(var), ptr(dist)))
        return var[..., ch], dist[..., ch]


class OnlineSet(_OnlineEngine):
    """pr_onlineset: the online signature database for the two configurations one OnlineDatabase cannot hold - kind
    'fused' (BASELINE config 5: the SC and the M2DP rows of every keyframe, the four row z-scores in one selection) or 'delight' - with
    ONE device-side count for all parts.  The buffers are zeroed torch tensors on the context's device (or the caller's: buffers = dict
    of NAMES[kind]): .sc [capacity, 2400] and .m2dp [capacity * 4, 384] f64, or .delight [capacity * 16, 256] f64, and .state [4] i32 =
    count, flags, 0, 0.  `sigs` is the keyframe's (sc [1, 2400], m2dp [4, 384]) pair for 'fused' and the DELIGHT tensor [16, 256] for
    'delight'.  Everything else is OnlineDatabase's, the calls included (one engine); at count == capacity an append stores NO part."""

    NAMES = {"fused": ("sc", "m2dp", "state"), "delight": ("delight", "state")}
    PARTS = {"fused": (("sc", 1, 2400), ("m2dp", 4, 384)), "delight": (("delight", 16, 256),)}
    CHANNELS = {"fused": 4, "delight": 1}
    _WHO, _C, _DESTROY, _REC, _ORDER = "OnlineSet", "pr_onlineset", "pr_onlineset_destroy", _lib.OnlineSetBuffers, ("sc", "m2dp", "delight")

    def __init__(self, ctx: Context | None, kind: str, capacity: int, max_k: int = 8, buffers: dict | None = None):
        if kind not in ("fused", "delight"):
            raise ValueError("OnlineSet: kind is 'fused' or 'delight'")
        self.kind_name, self.kind = kind, {"fused": _lib.ONLINESET_FUSED, "delight": _lib.ONLINESET_DELIGHT}[kind]
        self.parts, self.channels = self.PARTS[kind], self.CHANNELS[kind]
        self._align_tmp = {}
        self._create(ctx, self.kind, capacity, max_k, buffers)

    def align(self, idx, sigs, out=None):
        """The best-aligning variant of the pairs (query, row idx[0, j]) from the raw rows in place.  'fused': (variant int32 [1, k, 4],
        dist float64 [1, k, 4]) through ONE pr_align_pairs_dev, channels as rows= (var[..., :2] and var[..., 2:] are what
        KeyframeMap.verify_variants('sc' | 'm2dp', ...) takes).  'delight': [1, k, 2] through pr_delight_align_pairs_dev in Matcher.align's
        convention ([..., 0] the octant permutation, [..., 1] = -1 / NaN).  idx int32 [1, k] as match_torch returns it (-1: no pair).
        out: an earlier call's pair, written again (nothing is allocated then)."""
        import torch
        who = "OnlineSet.align"
        ts, _ = self._sigs(sigs, who)
        k = self._idx(who, idx)
        C_ = 4 if self.kind == _lib.ONLINESET_FUSED else 2
        o, msg = out or (None, None), f"{who}: out must be the pair an earlier align() of the same k returned"
        var = self._result(who, "out[0]", o[0], torch.int32, (1, k, C_), msg=msg)
        dist = self._result(who, "out[1]", o[1], torch.float64, (1, k, C_), msg=msg)
        if self.kind == _lib.ONLINESET_FUSED:
            self.ctx.check(self.lib.pr_align_pairs_dev(self.ctx.h, ptr(ts[0]), ptr(self.sc), _lib.F64, ptr(ts[1]), ptr(self.m2dp), _lib.F64, 1, self.capacity, 0, k,
                                                       ptr(idx), ptr(var), ptr(dist)))
            return var, dist
        tmp = self._align_tmp.get(k)                      # the library writes [1][k] contiguous: staged, then copied into slot 0
        if tmp is None:
            tmp = self._align_tmp[k] = (torch.empty((1, k), dtype=torch.int32, device=idx.device), torch.empty((1, k), dtype=torch.float64, device=idx.device))
        self.ctx.check(self.lib.pr_delight_align_pairs_dev(self.ctx.h, ptr(ts[0]), ptr(self.delight), _lib.F64, 1, self.capacity, 0, k, ptr(idx), ptr(tmp[0]), ptr(tmp[1])))
        var[..., 0].copy_(tmp[0]); var[..., 1].fill_(-1)
        dist[..., 0].copy_(tmp[1]); dist[..., 1].fill_(float("nan"))
        return var, dist


class SequenceFilter(Handle):
    """pr_seqmatch: the online form of the sequence matcher - a ring of the last L fused score rows of a drive.  Every
    keyframe, push_torch takes the distance rows an OnlineDatabase / OnlineSet match wrote (rows=) and the database's .state, fuses them
    into one row (the row z-scores weighted, or the one row as it is with normalize=False), stores it and returns the k rows whose
    scores summed along the step table's trajectories over the earlier pushed rows are smallest.  steps: api.seq_steps(L, velocities).
    Calls are enqueued on the context's stream, read the count on the device and allocate nothing; ONE captured push_torch serves every
    keyframe (the weights' values are part of the capture)."""

    _DESTROY = "pr_seqmatch_destroy"

    def __init__(self, ctx: Context | None, capacity: int, channels: int, steps, max_k: int = 8):
        self._attach(ctx)
        self.steps = _check_steps(steps, "SequenceFilter")
        self.capacity, self.channels, self.max_k = int(capacity), int(channels), int(max_k)
        self.V, self.L = self.steps.shape
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_seqmatch_create(self.ctx.h, self.capacity, self.channels, _ptr(self.steps), self.V, self.L, self.max_k,
                                                   C.byref(h)))
        self.h = h

    def _weights(self, weights, who):
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        if len(w) != self.channels:
            raise ValueError(f"{who}: weights must hold {self.channels} numbers")
        return w

    def push_torch(self, rows, state, weights, normalize: bool = True, mask_width: int = 0, k: int = 1, emitted=None, out=None):
        """Device form (pr_seqmatch_push_dev): rows f64 [channels, capacity], state i32 [>= 1] (word 0: the database's count = this
        keyframe's row id), weights [channels] host numbers (SC / M2DP rows: (p_weight, 1)).  emitted i32 [>= 1] | None: emitted[0] == 0
        switches the push off on the device.  Returns (idx i32 [1, k], score f64 [1, k], vel i32 [1, k], info i32 [4] = pushed, lags used,
        pushes after, 0); out: an earlier call's tuple, written again."""
        import torch
        who = "SequenceFilter.push_torch"
        k = int(k)
        self._t(who, "rows", rows, torch.float64, numel=self.channels * self.capacity,
                msg=f"{who}: rows must be a contiguous CUDA tensor f64 [{self.channels}, {self.capacity}]")
        for name, t in (("state", state), ("emitted", emitted)):
            if t is not None:
                self._t(who, name, t, torch.int32, numel_min=1, msg=f"{who}: {name} must be a CUDA tensor i32 [>= 1]")
        w = self._weights(weights, who)
        msg = f"{who}: out must be (idx i32 [1, k], score f64 [1, k], vel i32 [1, k], info i32 [4]) CUDA tensors"
        if out is not None and len(out) != 4:
            raise ValueError(msg)
        o, shape = out or (None,) * 4, (1, max(k, 0) if out is None else k)
        out = (self._result(who, "out[0]", o[0], torch.int32, shape, msg=msg), self._result(who, "out[1]", o[1], torch.float64, shape, msg=msg),
               self._result(who, "out[2]", o[2], torch.int32, shape, msg=msg), self._result(who, "out[3]", o[3], torch.int32, (4,), flat=True, msg=msg))
        self.ctx.check(self.lib.pr_seqmatch_push_dev(self.h, ptr(rows), ptr(state), ptr(emitted), _ptr(w), int(bool(normalize)), int(mask_width), k,
                                                     ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])))
        return out

    def push(self, rows, count: int, weights, normalize: bool = True, mask_width: int = 0, k: int = 1):
        """Host form (pr_seqmatch_push; synchronises): rows a NumPy array [channels, capacity].  Returns NumPy (idx [k], score [k],
        vel [k], info [4])."""
        who = "SequenceFilter.push"
        r = np.ascontiguousarray(rows, np.float64).reshape(-1)
        if len(r) != self.channels * self.capacity:
            raise ValueError(f"{who}: rows must hold {self.channels} x {self.capacity} numbers")
        w = self._weights(weights, who)
        k = int(k)
        idx, score, vel, info = np.empty(max(k, 0), np.int32), np.empty(max(k, 0), np.float64), np.empty(max(k, 0), np.int32), np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_seqmatch_push(self.h, _ptr(r), int(count), _ptr(w), int(bool(normalize)), int(mask_width), k, _ptr(idx),
                                                 _ptr(score), _ptr(vel), _ptr(info)))
        return idx, score, vel, info

    def read(self):
        """(ring f64 [L, capacity], row ids i32 [L], pushes) on the host; synchronises (pr_seqmatch_read)."""
        ring, ids, n = np.empty((self.L, self.capacity), np.float64), np.empty(self.L, np.int32), C.c_int32()
        self.ctx.check(self.lib.pr_seqmatch_read(self.h, _ptr(ring), _ptr(ids), C.byref(n)))
        return ring, ids, int(n.value)

    def reset(self):
        self.ctx.check(self.lib.pr_seqmatch_reset(self.h))
