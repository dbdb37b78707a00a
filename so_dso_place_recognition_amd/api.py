"""Host-side mirror of the reference's interface for the hot path, on top of the C ABI (libpr_amd.so).

Same names, argument meaning and error behaviour as the reference:
  SC / M2DP classes            SC/SC.h:10-23, M2DP/M2DP.h:12-30  (getSignatureSize / getSignature)
  GIST class, gist_generate    GIST/include/gist.h, gist.cpp:54-94  (getSignatureSize / extract)
  ORBVocabulary, bow_generate  BoW/ORBVocabulary.h, DBoW2 TemplatedVocabulary.h (loadFromTextFile / transform), test_bow.cpp:127-163
  processSC / processM2DP      match_signatures/processSC.m:1, processM2DP.m:1
  run_test                     match_signatures/run_test.m:1  (fusion, mask, top-1; PR/AUC evaluation in eval.py)
Arrays are numpy on the host; the device-resident path used by bench.py / dist.py is `Matcher`.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import PRError, TYPE_BOW, TYPE_DELIGHT, TYPE_GIST, TYPE_M2DP, TYPE_SC  # noqa: F401


class GISTParams(NamedTuple):
    """cls::GISTParams (GIST/include/gist.h): use_color, width, height, blocks, scale, orients."""
    use_color: bool = False
    width: int = 256
    height: int = 256
    blocks: int = 4
    scale: int = 4
    orients: tuple = (8, 8, 8, 8)

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One HIP device + stream (pr_ctx)."""

    def __init__(self, device: int = 0, sc_arith: str | None = None, stream: int | None = None, nan_policy: str | None = None,
                 exact_statistics: bool | None = None, sc_binary: bool | None = None):
        """sc_arith: None (library default: "f16x2", or PR_SC_MATCH=f32 from the environment), "f16x2" or "f32".
        exact_statistics: True = every query of a top-k call gets fp64 row statistics (pr_set_exact_statistics: scores are the reference's
        doubles to rounding, at 2.3 ms per query and 100k entries).
        stream: a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream; 0 = the null stream): the
        context's kernels are enqueued there (pr_create_on_stream).  nan_policy: "exclude" (default, MATLAB's behaviour for
        zero-norm SC rows) or "fail" (PR_ENAN)."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            rc = self.lib.pr_create(device, C.byref(h))
        else:
            rc = self.lib.pr_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise PRError(rc, self.lib.pr_last_error(None).decode())
        self.h = h
        self.device = device
        if sc_arith is not None:
            self.check(self.lib.pr_set_sc_arith(h, {"f16x2": _lib.SC_ARITH_F16X2, "f32": _lib.SC_ARITH_F32, "f16": _lib.SC_ARITH_F16}[sc_arith]))
        if nan_policy is not None:
            self.check(self.lib.pr_set_nan_policy(h, {"exclude": _lib.NAN_EXCLUDE, "fail": _lib.NAN_FAIL}[nan_policy]))
        self.exact_statistics = bool(exact_statistics) if exact_statistics is not None else os.environ.get("PR_FORCE_ORDER_FLAGS") == "1"
        if exact_statistics is not None:
            self.check(self.lib.pr_set_exact_statistics(h, int(bool(exact_statistics))))
        if sc_binary is not None:      # False: a binary intensity channel goes through the split-f16 kernel like any other (pr_set_sc_binary)
            self.check(self.lib.pr_set_sc_binary(h, int(bool(sc_binary))))

    def kernel_timing(self, on: bool):
        """HIP events around the matcher launches of pr_distances_dev (pr_set_kernel_timing)."""
        self.check(self.lib.pr_set_kernel_timing(self.h, int(bool(on))))

    def last_distance_timing(self):
        """(ms channel-0 or only launch, ms channel-1 single-product launch, ms channel-1 split-f16 launch) of the last timed call."""
        ms = (C.c_float * 3)()
        self.check(self.lib.pr_last_distance_timing(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def take_warnings(self) -> int:
        """PR_WARN_* bits raised since the last call (1: zero-norm SC rows excluded, 2: an M2DP singular pair did not converge)."""
        return int(self.lib.pr_take_warnings(self.h))

    @property
    def sc_arith(self) -> str:
        return {_lib.SC_ARITH_F32: "f32", _lib.SC_ARITH_F16: "f16"}.get(self.lib.pr_get_sc_arith(self.h), "f16x2")

    def close(self):
        if getattr(self, "h", None):
            self.lib.pr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        _lib.check(self.h, rc)

    def sync(self):
        self.check(self.lib.pr_sync(self.h))

    @property
    def stream(self) -> int:
        return int(self.lib.pr_stream(self.h) or 0)


class Group:
    """pr_group: hist2 row-sharded over the GPUs `devices` of this node inside the C ABI (RCCL all-gathers between the kernels;
    repeated device ids = several shards on one GPU, exchanged by device copies)."""

    def __init__(self, devices):
        self.lib = _lib.load()
        d = np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        rc = self.lib.pr_group_create(_ptr(d), len(d), C.byref(h))
        if rc != 0:
            raise PRError(rc, self.lib.pr_group_last_error(None).decode())
        self.h = h
        self.div, self.width = None, None

    @property
    def uses_rccl(self) -> bool:
        return bool(self.lib.pr_group_uses_rccl(self.h))

    @property
    def rccl_ranks(self) -> int:
        """Ranks the group's RCCL communicator reports (ncclCommCount); 0 when the group exchanges by device copies."""
        return int(self.lib.pr_group_rccl_ranks(self.h))

    PHASES = ("upload+pack(q)", "distances", "moments", "all_gather A (moments)", "select", "all_gather B (candidates)", "merge+rerank",
              "all_gather C (evaluations)", "finish+checks", "exact rows (flagged queries)")

    def set_timing(self, on: bool):
        """HIP events between the phases of every following match_topk, on every shard's stream (pr_group_set_timing)."""
        self._check(self.lib.pr_group_set_timing(self.h, int(bool(on))))

    def last_timing(self):
        """[{phase: ms}] per shard for the last timed match_topk (pr_group_last_timing)."""
        G = int(self.lib.pr_group_size(self.h))
        ms = (C.c_float * (G * len(self.PHASES)))()
        self._check(self.lib.pr_group_last_timing(self.h, ms, G * len(self.PHASES)))
        return [{name: float(ms[r * len(self.PHASES) + p]) for p, name in enumerate(self.PHASES)} for r in range(G)]

    @property
    def last_flagged(self) -> int:
        """Queries of the last match_topk that were answered from their exact fp64 rows (order / containment checks)."""
        return int(self.lib.pr_group_last_flagged(self.h))

    def _check(self, rc):
        if rc != 0:
            raise PRError(rc, self.lib.pr_group_last_error(self.h).decode())

    def set_database(self, type_: str, hist2, extra_capacity: int = 0):
        """extra_capacity > 0: room for that many more signatures, added later in place by append_database (the online loop of
        SC/test_sc.cpp:40-56 + run_test.m:57 through host buffers)."""
        t = {"sc": TYPE_SC, "m2dp": TYPE_M2DP}[type_]
        self.div, self.width = {TYPE_SC: (1, 2400), TYPE_M2DP: (4, 384)}[t]
        h2 = np.ascontiguousarray(hist2, np.float64)
        if h2.ndim != 2 or h2.shape[1] != self.width or h2.shape[0] % self.div:
            raise ValueError(f"expected a [{self.div}*n, {self.width}] signature matrix")
        if extra_capacity:
            self._check(self.lib.pr_group_set_database_growable(self.h, t, _ptr(h2), h2.shape[0] // self.div, int(extra_capacity)))
        else:
            self._check(self.lib.pr_group_set_database(self.h, t, _ptr(h2), h2.shape[0] // self.div))

    def append_database(self, hist_new):
        h = np.ascontiguousarray(hist_new, np.float64)
        if h.ndim != 2 or h.shape[1] != self.width or h.shape[0] % self.div:
            raise ValueError(f"expected a [{self.div}*n_new, {self.width}] signature matrix")
        self._check(self.lib.pr_group_append_database(self.h, _ptr(h), h.shape[0] // self.div))

    @property
    def database_rows(self) -> int:
        return int(self.lib.pr_group_database_rows(self.h))

    def match_topk(self, hist1, mask_width=0, p_weight=2.0, k=1):
        """run_test.m:26-57 against the sharded database -> (idx int32 [m,k] global rows, score float64 [m,k])."""
        h1 = np.ascontiguousarray(hist1, np.float64)
        if h1.ndim != 2 or h1.shape[1] != self.width or h1.shape[0] % self.div:
            raise ValueError(f"expected a [{self.div}*m, {self.width}] signature matrix")
        m = h1.shape[0] // self.div
        idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float64)
        self._check(self.lib.pr_group_match_topk(self.h, _ptr(h1), m, int(mask_width), float(p_weight), int(k), _ptr(idx), _ptr(sc)))
        return idx, sc

    def take_warnings(self) -> int:
        """PR_WARN_* bits raised on any shard since the last call."""
        return int(self.lib.pr_group_take_warnings(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pr_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class _exact_statistics:
    """`with _exact_statistics(ctx):` - pr_set_exact_statistics(ctx, 1) around a call, the context's own setting back afterwards."""

    def __init__(self, ctx: Context):
        self.ctx, self.prev = ctx, ctx.exact_statistics

    def __enter__(self):
        self.ctx.check(self.ctx.lib.pr_set_exact_statistics(self.ctx.h, 1))
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.check(self.ctx.lib.pr_set_exact_statistics(self.ctx.h, int(self.prev)))
        return False


def _csr(pts_list):
    """list of (xyz [P,3], intensity [P]) -> CSR arrays."""
    offs = np.zeros(len(pts_list) + 1, np.int64)
    for i, (p, _) in enumerate(pts_list):
        offs[i + 1] = offs[i] + len(p)
    xyz = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p, _ in pts_list])
                               if pts_list else np.zeros((0, 3)))
    it = np.ascontiguousarray(np.concatenate([np.asarray(i, np.float32).reshape(-1) for _, i in pts_list])
                              if pts_list else np.zeros((0,), np.float32))
    return xyz, it, offs


def sc_generate(xyz, inten, offs, max_rho=45.0, ctx: Context | None = None) -> np.ndarray:
    """test_sc.cpp:40-56 over clouds in CSR layout -> [N, 2400]."""
    ctx = ctx or default_context()
    xyz = np.ascontiguousarray(xyz, np.float64)
    inten = np.ascontiguousarray(inten, np.float32)
    offs = np.ascontiguousarray(offs, np.int64)
    N = len(offs) - 1
    out = np.empty((N, 2400))
    ctx.check(ctx.lib.pr_sc_generate(ctx.h, _ptr(xyz), _ptr(inten), _ptr(offs), N, float(max_rho), _ptr(out)))
    return out


def m2dp_generate(xyz, inten, offs, max_rho=45.0, ctx: Context | None = None) -> np.ndarray:
    """test_m2dp.cpp:41-68 over clouds in CSR layout -> [4N, 384]."""
    ctx = ctx or default_context()
    xyz = np.ascontiguousarray(xyz, np.float64)
    inten = np.ascontiguousarray(inten, np.float32)
    offs = np.ascontiguousarray(offs, np.int64)
    N = len(offs) - 1
    out = np.empty((4 * N, 384))
    ctx.check(ctx.lib.pr_m2dp_generate(ctx.h, _ptr(xyz), _ptr(inten), _ptr(offs), N, float(max_rho), _ptr(out)))
    return out


def m2dp_svd_rows(ctx: Context | None = None) -> np.ndarray:
    """Rows (cloud * 4 + variant) of the context's last m2dp_generate call whose leading singular pair is not unique (pr_m2dp_svd_rows):
    the rows PR_WARN_M2DP_SVD is about."""
    ctx = ctx or default_context()
    rows = np.empty(1024, np.int32)
    cnt = np.zeros(1, np.int32)
    ctx.check(ctx.lib.pr_m2dp_svd_rows(ctx.h, _ptr(rows), len(rows), _ptr(cnt)))
    return rows[: int(cnt[0])].copy()


def delight_generate(xyz, inten, offs, ctx: Context | None = None) -> np.ndarray:
    """test_delight.cpp:41-56 over clouds in CSR layout -> [16N, 256]."""
    ctx = ctx or default_context()
    xyz = np.ascontiguousarray(xyz, np.float64)
    inten = np.ascontiguousarray(inten, np.float32)
    offs = np.ascontiguousarray(offs, np.int64)
    N = len(offs) - 1
    out = np.empty((16 * N, 256))
    ctx.check(ctx.lib.pr_delight_generate(ctx.h, _ptr(xyz), _ptr(inten), _ptr(offs), N, _ptr(out)))
    return out


def gist_signature_size(nblocks: int = 4, orients=(8, 8, 8, 8)) -> int:
    """nblocks^2 x sum(orients) (GIST::setParams, gist.cpp:40-50, grayscale)."""
    o = np.ascontiguousarray(orients, np.int32)
    rc = _lib.load().pr_gist_signature_size(int(nblocks), len(o), _ptr(o))
    if rc < 0:
        raise ValueError(f"invalid GIST parameters: nblocks={nblocks}, orients={tuple(orients)}")
    return rc


def _gist_images(images, where: str):
    if images.ndim == 2:
        images = images[None]
    if images.ndim != 3:
        raise ValueError(f"expected [N, 256, 256] images ({where})")
    return images


def gist_generate(images, nblocks: int = 4, orients=(8, 8, 8, 8), ctx: Context | None = None) -> np.ndarray:
    """GIST::extract (gist.cpp:54-94) of 256 x 256 grayscale images, uint8 (mono8) or float32, [N, 256, 256] or one [256, 256]
    -> float32 [N, nblocks^2 sum(orients)].  Other sizes raise PRError (PR_EINVAL): resize and crop them first.
    A descriptor with a NaN / Inf raises PRError (PR_ENAN), as the reference returns NULL for it."""
    ctx = ctx or default_context()
    img = np.asarray(images)
    dtype = _lib.U8 if img.dtype == np.uint8 else _lib.F32
    img = _gist_images(np.ascontiguousarray(img, np.uint8 if dtype == _lib.U8 else np.float32), "gist_generate")
    o = np.ascontiguousarray(orients, np.int32)
    N, H, W = img.shape
    out = np.empty((N, gist_signature_size(nblocks, orients)), np.float32)
    ctx.check(ctx.lib.pr_gist_generate(ctx.h, _ptr(img), dtype, N, H, W, int(nblocks), len(o), _ptr(o), _ptr(out)))
    return out


def gist_generate_torch(images, nblocks: int = 4, orients=(8, 8, 8, 8), ctx: Context | None = None, out=None):
    """Device form (pr_gist_generate_dev) for images already on the GPU: a torch uint8 / float32 tensor [N, 256, 256] (or [256, 256])
    -> float32 tensor [N, D] on the same device (or `out`, preallocated).  No host wait, and after the first call with these parameters
    and a batch at least this size nothing is allocated by the library (graph-capturable with a preallocated `out`).  A row whose
    descriptor is not finite is left as NaN.
    ctx given: the kernels run on ctx's stream and the caller orders it with the tensors' producers and consumers (e.g. a context created
    on the stream the work runs on).  ctx None: one library context per device, on a stream of its own, joined to torch's current stream
    by stream waits on both sides (no host wait); the tensors are marked as used on that stream for torch's caching allocator."""
    import torch
    if images.dtype not in (torch.uint8, torch.float32) or not images.is_cuda:
        raise ValueError("gist_generate_torch: expected a CUDA tensor of dtype uint8 or float32")
    img = _gist_images(images.contiguous(), "gist_generate_torch")
    o = np.ascontiguousarray(orients, np.int32)
    N, H, W = img.shape
    D = gist_signature_size(nblocks, orients)
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=img.device)
    elif out.shape != (N, D) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"gist_generate_torch: out must be a contiguous float32 tensor [{N}, {D}]")
    dtype = _lib.U8 if img.dtype == torch.uint8 else _lib.F32
    lib_stream = cur = None
    if ctx is None:
        ctx, lib_stream = _torch_default_context(img.device.index or 0)
        cur = torch.cuda.current_stream(img.device)
        lib_stream.wait_stream(cur)                # the images (and out) are ready on torch's stream before the library reads / writes them
    ctx.check(ctx.lib.pr_gist_generate_dev(ctx.h, C.c_void_p(img.data_ptr()), dtype, N, H, W, int(nblocks), len(o), _ptr(o),
                                           C.c_void_p(out.data_ptr())))
    if lib_stream is not None:
        cur.wait_stream(lib_stream)                # torch's later work sees the rows
        img.record_stream(lib_stream)
        out.record_stream(lib_stream)
    return out


_torch_ctx = {}      # device -> (Context on its own stream, that stream as a torch.cuda.ExternalStream): one per device, for the process


def _torch_default_context(device: int):
    import torch
    if device not in _torch_ctx:
        c = Context(device)
        _torch_ctx[device] = (c, torch.cuda.ExternalStream(c.stream, device=device))
    return _torch_ctx[device]


class ORBVocabulary:
    """ORB_SLAM2::ORBVocabulary (DBoW2 TemplatedVocabulary<FORB::TDescriptor, FORB>): the vocabulary tree, held by the library
    (pr_bow_vocab, no device needed until transform).  Scoring / weighting values as DBoW2's enums: scoring L1_NORM, L2_NORM, CHI_SQUARE,
    KL, BHATTACHARYYA, DOT_PRODUCT = 0..5; weighting TF_IDF, TF, IDF, BINARY = 0..3."""

    def __init__(self, path: str | None = None):
        self.lib = _lib.load()
        self.h = None
        if path is not None:
            self.loadFromTextFile(path)

    def _own(self, h):
        self.close()
        self.h = h

    def loadFromTextFile(self, path: str) -> bool:
        """ORBvoc-style text (TemplatedVocabulary.h:1338-1424) or the binary side-car of save(); raises PRError (PR_EINVAL / PR_EIO)
        where the reference would fail or read out of bounds."""
        h = C.c_void_p()
        rc = self.lib.pr_bow_vocab_load(os.fsencode(path), C.byref(h))
        if rc != 0:
            raise PRError(rc, self.lib.pr_host_last_error().decode())
        self._own(h)
        return True

    @classmethod
    def from_arrays(cls, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        """Node arrays with the root at index 0 (its entries ignored): parent int32 [n] (< own index), is_leaf [n] (> 0: a word),
        desc uint8 [n, 32], weight float64 [n]."""
        parent = np.ascontiguousarray(parent, np.int32)
        n = parent.shape[0]
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64)
        if is_leaf.shape != (n,) or desc.shape != (n, 32) or weight.shape != (n,):
            raise ValueError("from_arrays: parent [n], is_leaf [n], desc [n, 32], weight [n]")
        v = cls()
        h = C.c_void_p()
        rc = v.lib.pr_bow_vocab_create(int(k), int(L), int(scoring), int(weighting), n, _ptr(parent), _ptr(is_leaf), _ptr(desc),
                                       _ptr(weight), C.byref(h))
        if rc != 0:
            raise PRError(rc, v.lib.pr_host_last_error().decode())
        v._own(h)
        return v

    def save(self, path: str):
        """The binary side-car (loads ~100x faster than the text)."""
        rc = self.lib.pr_bow_vocab_save_bin(self._handle(), os.fsencode(path))
        if rc != 0:
            raise PRError(rc, self.lib.pr_host_last_error().decode())

    def _handle(self):
        if not self.h:
            raise ValueError("ORBVocabulary: nothing loaded")
        return self.h

    def info(self):
        """dict of k, L, scoring, weighting, nodes (the root included), words."""
        i = np.zeros(4, np.int32)
        nn, nw = C.c_int64(), C.c_int64()
        self.lib.pr_bow_vocab_info(self._handle(), _ptr(i), C.byref(nn), C.byref(nw))
        return {"k": int(i[0]), "L": int(i[1]), "scoring": int(i[2]), "weighting": int(i[3]), "nodes": nn.value, "words": nw.value}

    def size(self) -> int:
        return self.info()["words"]

    def empty(self) -> bool:
        return self.size() == 0

    def arrays(self):
        """(parent, is_leaf, desc, weight) as from_arrays takes them (pr_bow_vocab_export)."""
        n = self.info()["nodes"]
        parent, is_leaf = np.empty(n, np.int32), np.empty(n, np.uint8)
        desc, weight = np.empty((n, 32), np.uint8), np.empty(n, np.float64)
        self.lib.pr_bow_vocab_export(self._handle(), _ptr(parent), _ptr(is_leaf), _ptr(desc), _ptr(weight))
        return parent, is_leaf, desc, weight

    def transform(self, descriptors, ctx: Context | None = None):
        """BowVector of one image's ORB descriptors (uint8 [n, 32]): (word ids int64 ascending, values float64)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        out, nw = bow_generate((d, np.array([0, d.shape[0]], np.int64)), self, cols=max(d.shape[0], 1), ctx=ctx, return_counts=True)
        return out[0, :nw[0]].astype(np.int64), out[1, :nw[0]].copy()

    def close(self):
        if getattr(self, "h", None):
            self.lib.pr_bow_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bow_csr(descriptors):
    if isinstance(descriptors, tuple):
        desc, offs = descriptors
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        offs = np.ascontiguousarray(offs, np.int64)
    else:
        parts = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptors]
        offs = np.zeros(len(parts) + 1, np.int64)
        offs[1:] = np.cumsum([p.shape[0] for p in parts])
        desc = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    if offs.ndim != 1 or offs.shape[0] < 1 or offs[0] != 0 or offs[-1] != desc.shape[0]:
        raise ValueError("bow_generate: offs must run from 0 to the descriptor count")
    return desc, offs


def bow_generate(descriptors, vocab: ORBVocabulary, cols: int = 4000, ctx: Context | None = None, return_counts: bool = False):
    """ORBVocabulary::transform of each image (test_bow.cpp:127-135) -> float64 [2N, cols] as test_bow writes history_bow.txt and
    processBoW reads it: per image a row of word ids (ascending) and a row of values, padded with -1.  descriptors: a list of uint8
    [n_i, 32] arrays, or (desc [F, 32], offs [N + 1]).  An image with more than cols words raises PRError (PR_EINVAL).
    return_counts: also return each image's distinct-word count (int32 [N])."""
    ctx = ctx or default_context()
    desc, offs = _bow_csr(descriptors)
    N = offs.shape[0] - 1
    out = np.empty((2 * N, int(cols)), np.float64)
    nw = np.empty(N, np.int32)
    ctx.check(ctx.lib.pr_bow_generate(ctx.h, vocab._handle(), _ptr(desc), _ptr(offs), N, int(cols), _ptr(out), _ptr(nw)))
    return (out, nw) if return_counts else out


def bow_generate_torch(desc, offs, vocab: ORBVocabulary, cols: int = 4000, ctx: Context | None = None, out=None, n_words=None,
                       feature_words=None):
    """Device form (pr_bow_generate_dev): desc a CUDA uint8 tensor [F, 32], offs a CUDA int64 tensor [N + 1] -> float64 tensor [2N, cols]
    (or `out`).  n_words (int32 [N]) and feature_words (int32 [F], each descriptor's word id) are optional outputs.  No host wait; after
    the first call with this vocabulary and at least F descriptors the library allocates nothing (graph-capturable with preallocated
    outputs).  A row with more than cols words keeps its first cols and raises _lib.WARN_BOW_TRUNCATED (Context.take_warnings).
    ctx as in gist_generate_torch: None joins a per-device library context to torch's current stream."""
    import torch
    if desc.dtype != torch.uint8 or not desc.is_cuda or offs.dtype != torch.int64 or not offs.is_cuda:
        raise ValueError("bow_generate_torch: expected CUDA tensors desc uint8 [F, 32] and offs int64 [N + 1]")
    desc = desc.contiguous().reshape(-1, 32)
    offs = offs.contiguous()
    F, N = desc.shape[0], offs.shape[0] - 1
    if N < 0:
        raise ValueError("bow_generate_torch: offs needs N + 1 entries")
    if out is None:
        out = torch.empty((2 * N, int(cols)), dtype=torch.float64, device=desc.device)
    elif out.shape != (2 * N, cols) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"bow_generate_torch: out must be a contiguous float64 tensor [{2 * N}, {cols}]")
    for name, t, n in (("n_words", n_words, N), ("feature_words", feature_words, F)):
        if t is not None and (t.shape != (n,) or t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f"bow_generate_torch: {name} must be a contiguous int32 tensor [{n}]")
    lib_stream = cur = None
    if ctx is None:
        ctx, lib_stream = _torch_default_context(desc.device.index or 0)
        cur = torch.cuda.current_stream(desc.device)
        lib_stream.wait_stream(cur)

    def dp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    ctx.check(ctx.lib.pr_bow_generate_dev(ctx.h, vocab._handle(), dp(desc), F, dp(offs), N, int(cols), dp(out), dp(n_words),
                                          dp(feature_words)))
    if lib_stream is not None:
        cur.wait_stream(lib_stream)
        for t in (desc, offs, out, n_words, feature_words):
            if t is not None:
                t.record_stream(lib_stream)
    return out


class DELIGHT:
    """DELIGHT/DELIGHT.h:11-18."""

    def __init__(self, ctx: Context | None = None):
        self.ctx = ctx

    def getSignatureSize(self) -> int:
        return 256

    def getSignature(self, pts, intensity):
        xyz, it, offs = _csr([(pts, intensity)])
        return delight_generate(xyz, it, offs, self.ctx)


class SC:
    """SC/SC.h:10-23."""

    def __init__(self, max_rho: float, ctx: Context | None = None):
        self.max_rho = float(max_rho)
        self.ctx = ctx

    def getSignatureSize(self) -> int:
        return 1200

    def getSignature(self, pts, intensity):
        """pts [P,3] camera frame (PCA alignment happens inside, SC.cpp:17) -> (structure[1200], intensity[1200])."""
        xyz, it, offs = _csr([(pts, intensity)])
        row = sc_generate(xyz, it, offs, self.max_rho, self.ctx)[0]
        return row[:1200].copy(), row[1200:].copy()


class M2DP:
    """M2DP/M2DP.h:12-30.  The reference driver aligns once and loops the 4 sign variants (test_m2dp.cpp:44-68);
    getSignatures returns all 4 rows of that loop."""

    def __init__(self, max_rho: float, ctx: Context | None = None):
        self.max_rho = float(max_rho)
        self.ctx = ctx

    def getSignatureSize(self) -> int:
        return 192

    def getSignatures(self, pts, intensity):
        xyz, it, offs = _csr([(pts, intensity)])
        return m2dp_generate(xyz, it, offs, self.max_rho, self.ctx)


class GIST:
    """cls::GIST (GIST/include/gist.h, gist.cpp:40-94), grayscale.  params: a GISTParams or None for test_gist.cpp:57's
    DEFAULT_PARAMS{false, 256, 256, 4, 4, {8, 8, 8, 8}}."""

    def __init__(self, params=None, ctx: Context | None = None):
        self.params = params if params is not None else GISTParams()
        p = self.params
        if p.use_color:
            raise ValueError("GIST: colour GIST is not supported (test_gist uses use_color = false)")
        if (p.width, p.height) != (256, 256) or p.scale != len(p.orients):
            raise ValueError("GIST: width = height = 256 and scale = len(orients) are supported")
        self.ctx = ctx

    def getSignatureSize(self) -> int:
        return gist_signature_size(self.params.blocks, self.params.orients)

    def extract(self, img) -> np.ndarray:
        """One 256 x 256 image (uint8 or float32) -> float32 [getSignatureSize()] (the resize / crop of extract is the caller's)."""
        return gist_generate(np.asarray(img)[None], self.params.blocks, self.params.orients, self.ctx)[0]


def _distance(fn_name, div, width, hist1, hist2, ctx):
    ctx = ctx or default_context()
    h1 = np.ascontiguousarray(hist1, np.float64)
    h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != width or h2.shape[1] != width or h1.shape[0] % div or h2.shape[0] % div:
        raise ValueError(f"expected [{div}*m, {width}] and [{div}*n, {width}] signature matrices")
    m, n = h1.shape[0] // div, h2.shape[0] // div
    dp = np.empty((m, n), np.float32)
    di = np.empty((m, n), np.float32)
    ctx.check(getattr(ctx.lib, fn_name)(ctx.h, _ptr(h1), m, _ptr(h2), n, _ptr(dp), _ptr(di)))
    return dp, di


def processSC(hist1, hist2, ctx: Context | None = None):
    """[diff_m_p, diff_m_i] = processSC(hist1, hist2)  (processSC.m:1); float32 [m, n] each."""
    return _distance("pr_sc_distance", 1, 2400, hist1, hist2, ctx)


def processM2DP(hist1, hist2, ctx: Context | None = None):
    """[diff_m_p, diff_m_i] = processM2DP(hist1, hist2)  (processM2DP.m:1); hist rows come in groups of 4 variants."""
    return _distance("pr_m2dp_distance", 4, 384, hist1, hist2, ctx)


def processDELIGHT(hist1, hist2, ctx: Context | None = None):
    """dist = processDELIGHT(hist1, hist2)  (processDELIGHT.m:1); 16 rows per signature; float32 [m, n]."""
    ctx = ctx or default_context()
    h1 = np.ascontiguousarray(hist1, np.float64)
    h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != 256 or h2.shape[1] != 256 or h1.shape[0] % 16 or h2.shape[0] % 16:
        raise ValueError("expected [16*m, 256] and [16*n, 256] histogram matrices")
    m, n = h1.shape[0] // 16, h2.shape[0] // 16
    d = np.empty((m, n), np.float32)
    ctx.check(ctx.lib.pr_delight_distance(ctx.h, _ptr(h1), m, _ptr(h2), n, _ptr(d)))
    return d


def processGIST(hist1, hist2, ctx: Context | None = None):
    """diff_m = processGIST(hist1, hist2)  (processGIST.m:1): squared Euclidean distances, float32 [m, n]."""
    ctx = ctx or default_context()
    h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.shape[1] != h2.shape[1]:
        raise ValueError("hist1 and hist2 must have the same number of columns")
    d = np.empty((h1.shape[0], h2.shape[0]), np.float32)
    ctx.check(ctx.lib.pr_gist_distance(ctx.h, _ptr(h1), h1.shape[0], _ptr(h2), h2.shape[0], h1.shape[1], _ptr(d)))
    return d


def processBoW(hist1, hist2, ctx: Context | None = None):
    """diff_m = processBoW(hist1, hist2)  (processBoW.m:1): rows alternate word ids / weights (padded with -1); float32 [m, n]."""
    ctx = ctx or default_context()
    h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.shape[1] != h2.shape[1] or h1.shape[0] % 2 or h2.shape[0] % 2:
        raise ValueError("BoW files hold two rows of the same width per image")
    m, n = h1.shape[0] // 2, h2.shape[0] // 2
    d = np.empty((m, n), np.float32)
    ctx.check(ctx.lib.pr_bow_distance(ctx.h, _ptr(h1), m, _ptr(h2), n, h1.shape[1], _ptr(d)))
    return d


def _bow_pair(hist1, hist2):
    h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != h2.shape[1] or h1.shape[0] % 2 or h2.shape[0] % 2:
        raise ValueError("BoW files hold two rows of the same width per image")
    return h1, h2, h1.shape[0] // 2, h2.shape[0] // 2


def bow_distance_f64(hist1, hist2, ctx: Context | None = None):
    """processBoW(hist1, hist2) in fp64 as the reference evaluates it (processBoW.m:1-38), through the inverted file
    (pr_bow_distance_f64): float64 [m, n], bit for bit the merge's values for conforming rows; PRError (PR_EINVAL) for a row that is not."""
    ctx = ctx or default_context()
    h1, h2, m, n = _bow_pair(hist1, hist2)
    d = np.empty((m, n), np.float64)
    ctx.check(ctx.lib.pr_bow_distance_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, h1.shape[1], _ptr(d)))
    return d


def bow_match_topk(hist1, hist2, mask_width=0, k=1, ctx: Context | None = None):
    """run_test.m:32-57 for 'bow' in fp64 through the inverted file (pr_bow_match_topk_f64): (idx int32 [m,k], score float64 [m,k]),
    the reference's double-precision ranking (ties -> lower index, -1 / NaN when fewer than k candidates).  k <= 128.
    match_topk('bow', ...) keeps the fp32 all-pairs path."""
    ctx = ctx or default_context()
    h1, h2, m, n = _bow_pair(hist1, hist2)
    idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float64)
    ctx.check(ctx.lib.pr_bow_match_topk_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, h1.shape[1], int(mask_width), int(k), _ptr(idx), _ptr(sc)))
    return idx, sc


def _gist_pair(hist1, hist2):
    h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != h2.shape[1] or h1.shape[1] < 1:
        raise ValueError("GIST files hold one row of the same width per image")
    return h1, h2, h1.shape[0], h2.shape[0]


def gist_distance_f64(hist1, hist2, ctx: Context | None = None):
    """processGIST(hist1, hist2) in fp64 as the reference evaluates it (processGIST.m:7: differences, squares, sum in ascending column
    order, no contraction; pr_gist_distance_f64): float64 [m, n], bit for bit."""
    ctx = ctx or default_context()
    h1, h2, m, n = _gist_pair(hist1, hist2)
    d = np.empty((m, n), np.float64)
    ctx.check(ctx.lib.pr_gist_distance_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, h1.shape[1], _ptr(d)))
    return d


def gist_match_topk(hist1, hist2, mask_width=0, k=1, ctx: Context | None = None):
    """run_test.m:32-57 for 'gist' in fp64 (pr_gist_match_topk_f64): (idx int32 [m,k], score float64 [m,k]), the reference's
    double-precision ranking (ties -> lower index, -1 / NaN when fewer than k candidates).  k <= 128.
    match_topk('gist', ...) keeps the fp32 all-pairs path."""
    ctx = ctx or default_context()
    h1, h2, m, n = _gist_pair(hist1, hist2)
    idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float64)
    ctx.check(ctx.lib.pr_gist_match_topk_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, h1.shape[1], int(mask_width), int(k), _ptr(idx), _ptr(sc)))
    return idx, sc


def _delight_pair(hist1, hist2):
    h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != 256 or h2.shape[1] != 256 or h1.shape[0] % 16 or h2.shape[0] % 16:
        raise ValueError("DELIGHT files hold 16 rows of 256 bins per cloud")
    return h1, h2, h1.shape[0] // 16, h2.shape[0] // 16


def delight_distance_f64(hist1, hist2, ctx: Context | None = None):
    """processDELIGHT(hist1, hist2) in fp64 as the reference evaluates it (processDELIGHT.m:7-37: per permutation the terms of the
    occupied bins added in column-major order, divided by their count, the smallest of the four; no contraction;
    pr_delight_distance_f64): float64 [m, n], bit for bit."""
    ctx = ctx or default_context()
    h1, h2, m, n = _delight_pair(hist1, hist2)
    d = np.empty((m, n), np.float64)
    ctx.check(ctx.lib.pr_delight_distance_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, _ptr(d)))
    return d


def delight_match_topk(hist1, hist2, mask_width=0, k=1, ctx: Context | None = None):
    """run_test.m:32-57 for 'delight' in fp64 (pr_delight_match_topk_f64): (idx int32 [m,k], score float64 [m,k]), the reference's
    double-precision ranking (ties -> lower index, -1 / NaN when fewer than k candidates).  k <= 128.
    match_topk('delight', ...) keeps the fp32 all-pairs path."""
    ctx = ctx or default_context()
    h1, h2, m, n = _delight_pair(hist1, hist2)
    idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float64)
    ctx.check(ctx.lib.pr_delight_match_topk_f64(ctx.h, _ptr(h1), m, _ptr(h2), n, int(mask_width), int(k), _ptr(idx), _ptr(sc)))
    return idx, sc


def match_topk(type_, hist1, hist2, mask_width=0, p_weight=2.0, k=1, ctx: Context | None = None):
    """run_test.m:26-57 generalised to top-k: returns (idx int32 [m,k] 0-based, score float64 [m,k] as MATLAB holds it;
    float32 for gist / bow, whose distances are a single fp32 matrix)."""
    ctx = ctx or default_context()
    t = {"sc": TYPE_SC, "m2dp": TYPE_M2DP, "delight": TYPE_DELIGHT, "gist": TYPE_GIST, "bow": TYPE_BOW}.get(type_, type_)
    if t in (TYPE_GIST, TYPE_BOW):
        h1 = np.ascontiguousarray(hist1, np.float64); h2 = np.ascontiguousarray(hist2, np.float64)
        div = 2 if t == TYPE_BOW else 1
        if h1.shape[1] != h2.shape[1] or h1.shape[0] % div or h2.shape[0] % div:
            raise ValueError("hist1 / hist2 shapes do not fit the type")
        m, n = h1.shape[0] // div, h2.shape[0] // div
        idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float32)
        ctx.check(ctx.lib.pr_match_topk_cols(ctx.h, t, _ptr(h1), m, _ptr(h2), n, h1.shape[1], int(mask_width), int(k), _ptr(idx), _ptr(sc)))
        return idx, sc
    if t not in (TYPE_SC, TYPE_M2DP, TYPE_DELIGHT):
        raise ValueError("type must be 'sc', 'm2dp', 'delight', 'gist' or 'bow'")
    div, width = {TYPE_SC: (1, 2400), TYPE_M2DP: (4, 384), TYPE_DELIGHT: (16, 256)}[t]
    h1 = np.ascontiguousarray(hist1, np.float64)
    h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != width or h2.shape[1] != width:
        raise ValueError(f"signature width must be {width}")
    if h1.shape[0] % div or h2.shape[0] % div:
        raise ValueError(f"signature matrices of this type hold {div} rows per signature")
    m, n = h1.shape[0] // div, h2.shape[0] // div
    idx = np.empty((m, k), np.int32)
    sc = np.empty((m, k), np.float64)
    ctx.check(ctx.lib.pr_match_topk_f64(ctx.h, t, _ptr(h1), m, _ptr(h2), n, int(mask_width), float(p_weight), int(k),
                                        _ptr(idx), _ptr(sc)))
    return idx, sc


def match_topk_fused(sc1, m2dp1, sc2, m2dp2, mask_width=0, p_weight=2.0, k=1, ctx: Context | None = None):
    """BASELINE config 5 (build-defined, no reference counterpart): SC [m, 2400] and M2DP [4 m, 384] signatures of the same
    places scored together - the four row z-scores added with weights p, 1, p, 1.  Returns (idx int32 [m,k], score float64)."""
    ctx = ctx or default_context()
    a1 = np.ascontiguousarray(sc1, np.float64); a2 = np.ascontiguousarray(sc2, np.float64)
    b1 = np.ascontiguousarray(m2dp1, np.float64); b2 = np.ascontiguousarray(m2dp2, np.float64)
    m, n = a1.shape[0], a2.shape[0]
    if b1.shape != (4 * m, 384) or b2.shape != (4 * n, 384) or a1.shape[1] != 2400 or a2.shape[1] != 2400:
        raise ValueError("need SC [m, 2400] and M2DP [4 m, 384] signatures of the same m (n) places")
    idx = np.empty((m, k), np.int32); sc = np.empty((m, k), np.float64)
    ctx.check(ctx.lib.pr_match_topk_fused_f64(ctx.h, _ptr(a1), _ptr(b1), m, _ptr(a2), _ptr(b2), n, int(mask_width), float(p_weight),
                                          int(k), _ptr(idx), _ptr(sc)))
    return idx, sc


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


def seq_select_torch(d_p, d_i, mom, steps, q_row0: int = 0, db_row0: int = 0, mask_width: int = 0, p_weight: float = 2.0, k: int = 1,
                     dense: bool = False, ctx: Context | None = None, out=None):
    """Device form of the sequence selection (pr_seq_select_dev): d_p, d_i f32 [m, n] and mom f64 [m, 2, 3] as
    pr_distances_dev / pr_row_moments_dev wrote them (d_i = None: one matrix, no normalisation, mom unused), steps a CUDA i32 [V, L]
    tensor.  Returns (idx i32 [m, k] global DB rows, score f64 [m, k], vel i32 [m, k][, S f64 [m, n] with dense=True]); out: an earlier
    call's tuple, written again.  Enqueued on the context's stream; nothing synchronises or, given out=, allocates."""
    import torch
    ctx = ctx or _torch_default_context(d_p.device.index)
    who = "seq_select_torch"
    if (not d_p.is_cuda) or d_p.dtype != torch.float32 or d_p.dim() != 2 or not d_p.is_contiguous():
        raise ValueError(f"{who}: d_p must be a contiguous CUDA tensor f32 [m, n]")
    m, n = d_p.shape
    if d_i is not None:
        if (not d_i.is_cuda) or d_i.dtype != torch.float32 or tuple(d_i.shape) != (m, n) or not d_i.is_contiguous():
            raise ValueError(f"{who}: d_i must be a contiguous CUDA tensor f32 [m, n]")
        if mom is None or (not mom.is_cuda) or mom.dtype != torch.float64 or mom.numel() != 6 * m or not mom.is_contiguous():
            raise ValueError(f"{who}: mom must be a contiguous CUDA tensor f64 [m, 2, 3]")
    if (not steps.is_cuda) or steps.dtype != torch.int32 or steps.dim() != 2 or not steps.is_contiguous():
        raise ValueError(f"{who}: steps must be a contiguous CUDA tensor i32 [V, L]")
    V, L = steps.shape
    k = int(k)
    dev = d_p.device
    if out is None:
        out = (torch.empty((m, max(k, 0)), dtype=torch.int32, device=dev), torch.empty((m, max(k, 0)), dtype=torch.float64, device=dev),
               torch.empty((m, max(k, 0)), dtype=torch.int32, device=dev)) + ((torch.empty((m, n), dtype=torch.float64, device=dev),) if dense else ())
    elif len(out) != (4 if dense else 3) or any(tuple(t.shape) != (m, k) or not t.is_contiguous() or not t.is_cuda for t in out[:3]) \
            or (out[0].dtype, out[1].dtype, out[2].dtype) != (torch.int32, torch.float64, torch.int32) \
            or (dense and (tuple(out[3].shape) != (m, n) or out[3].dtype != torch.float64 or not out[3].is_contiguous())):
        raise ValueError(f"{who}: out must be (idx i32 [m, k], score f64 [m, k], vel i32 [m, k][, S f64 [m, n]]) CUDA tensors")
    if m == 0:
        return out
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ctx.check(ctx.lib.pr_seq_select_dev(ctx.h, p(d_p), p(d_i), m, n, p(mom) if d_i is not None else None, p(steps), V, L, int(q_row0),
                                        int(db_row0), int(mask_width), float(p_weight), k, p(out[0]), p(out[1]), p(out[2]),
                                        p(out[3]) if dense else None))
    return out


def match_topk_seq(type_, hist1, hist2, steps, mask_width=0, p_weight=2.0, k=1, ctx: Context | None = None):
    """Sequence matching over host buffers (pr_match_topk_seq_f64): hist1's rows are consecutive keyframes of a drive.  type_ 'sc',
    'm2dp' or 'delight'; steps as api.seq_steps builds it.  Returns (idx int32 [m, k], score float64 [m, k], vel int32 [m, k])."""
    ctx = ctx or default_context()
    t = {"sc": TYPE_SC, "m2dp": TYPE_M2DP, "delight": TYPE_DELIGHT}.get(type_, type_)
    if t not in (TYPE_SC, TYPE_M2DP, TYPE_DELIGHT):
        raise ValueError("type must be 'sc', 'm2dp' or 'delight'")
    st = _check_steps(steps, "match_topk_seq")
    div, width = {TYPE_SC: (1, 2400), TYPE_M2DP: (4, 384), TYPE_DELIGHT: (16, 256)}[t]
    h1 = np.ascontiguousarray(hist1, np.float64)
    h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != width or h2.shape[1] != width:
        raise ValueError(f"signature width must be {width}")
    if h1.shape[0] % div or h2.shape[0] % div:
        raise ValueError(f"signature matrices of this type hold {div} rows per signature")
    m, n = h1.shape[0] // div, h2.shape[0] // div
    idx, sc, vel = np.empty((m, k), np.int32), np.empty((m, k), np.float64), np.empty((m, k), np.int32)
    ctx.check(ctx.lib.pr_match_topk_seq_f64(ctx.h, t, _ptr(h1), m, _ptr(h2), n, int(mask_width), float(p_weight), int(k), _ptr(st),
                                            st.shape[0], st.shape[1], _ptr(idx), _ptr(sc), _ptr(vel)))
    return idx, sc, vel


def match_align(type_, hist1, hist2, idx, ctx: Context | None = None):
    """The best-aligning variant of every matched pair (pr_match_align): idx [m,k] as match_topk returns it (-1 = none).  Returns
    (variant int32 [m,k,2], dist float64 [m,k,2]) per channel - SC: structure, intensity, v = 2 * shift + mirror; M2DP: count, intensity,
    v = 4 * query row + DB row; DELIGHT: [..., 0] the octant permutation, [..., 1] = -1 / NaN.  -1 / NaN where there is no variant."""
    ctx = ctx or default_context()
    t = {"sc": TYPE_SC, "m2dp": TYPE_M2DP, "delight": TYPE_DELIGHT}.get(type_, type_)
    if t not in (TYPE_SC, TYPE_M2DP, TYPE_DELIGHT):
        raise ValueError("alignment needs type 'sc', 'm2dp' or 'delight' (gist / bow have no variants)")
    div, width = {TYPE_SC: (1, 2400), TYPE_M2DP: (4, 384), TYPE_DELIGHT: (16, 256)}[t]
    h1 = np.ascontiguousarray(hist1, np.float64)
    h2 = np.ascontiguousarray(hist2, np.float64)
    if h1.ndim != 2 or h2.ndim != 2 or h1.shape[1] != width or h2.shape[1] != width or h1.shape[0] % div or h2.shape[0] % div:
        raise ValueError(f"expected [{div}*m, {width}] and [{div}*n, {width}] signature matrices")
    m, n = h1.shape[0] // div, h2.shape[0] // div
    ix = np.ascontiguousarray(idx, np.int32)
    if ix.ndim != 2 or ix.shape[0] != m:
        raise ValueError("idx must be [m, k]")
    k = ix.shape[1]
    var = np.empty((m, k, 2), np.int32); dist = np.empty((m, k, 2), np.float64)
    ctx.check(ctx.lib.pr_match_align(ctx.h, t, _ptr(h1), m, _ptr(h2), n, k, _ptr(ix), _ptr(var), _ptr(dist)))
    return var, dist


def match_align_fused(sc1, m2dp1, sc2, m2dp2, idx, ctx: Context | None = None):
    """match_align for the pairs of match_topk_fused (pr_match_align_fused) -> (variant int32 [m,k,4], dist float64 [m,k,4]): SC structure,
    SC intensity, M2DP count, M2DP intensity."""
    ctx = ctx or default_context()
    a1 = np.ascontiguousarray(sc1, np.float64); a2 = np.ascontiguousarray(sc2, np.float64)
    b1 = np.ascontiguousarray(m2dp1, np.float64); b2 = np.ascontiguousarray(m2dp2, np.float64)
    m, n = a1.shape[0], a2.shape[0]
    if b1.shape != (4 * m, 384) or b2.shape != (4 * n, 384) or a1.shape[1] != 2400 or a2.shape[1] != 2400:
        raise ValueError("need SC [m, 2400] and M2DP [4 m, 384] signatures of the same m (n) places")
    ix = np.ascontiguousarray(idx, np.int32)
    if ix.ndim != 2 or ix.shape[0] != m:
        raise ValueError("idx must be [m, k]")
    k = ix.shape[1]
    var = np.empty((m, k, 4), np.int32); dist = np.empty((m, k, 4), np.float64)
    ctx.check(ctx.lib.pr_match_align_fused(ctx.h, _ptr(a1), _ptr(b1), m, _ptr(a2), _ptr(b2), n, k, _ptr(ix), _ptr(var), _ptr(dist)))
    return var, dist


def cloud_frames(xyz, inten, offs, ctx: Context | None = None) -> np.ndarray:
    """PCA frames of clouds in CSR layout (pr_cloud_frames_dev: utils/pts_align.h:7-46 on the GPU) -> host float64 [N, 16]: mean[3], the
    eigenvectors by ascending eigenvalue [3][3], 0, point count, and with intensities the cloud's float average and 1.0 (else 0, 0).
    Numpy arrays or device tensors; the clouds go through device memory of the context's GPU."""
    import torch
    ctx = ctx or default_context()
    dev = torch.device("cuda", ctx.device)
    x = torch.as_tensor(xyz, dtype=torch.float64).to(dev).contiguous()
    o = torch.as_tensor(offs, dtype=torch.int64).to(dev).contiguous()
    it = None if inten is None else torch.as_tensor(inten, dtype=torch.float32).to(dev).contiguous()
    N = o.numel() - 1
    fr = torch.empty((max(N, 0), 16), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)                       # the uploads (torch's stream) before the library's stream reads them
    ctx.check(ctx.lib.pr_cloud_frames_dev(ctx.h, C.c_void_p(x.data_ptr()), None if it is None else C.c_void_p(it.data_ptr()),
                                          C.c_void_p(o.data_ptr()), N, C.c_void_p(fr.data_ptr())))
    ctx.sync()
    return fr.cpu().numpy()


def sc_relative_pose(frames_q, frames_db, variant) -> np.ndarray:
    """[R | t] float64 [c, 3, 4] mapping query-camera-frame points into the DB entry's camera frame, from the two clouds' frames
    ([c, 16] as cloud_frames returns them) and the SC structure-channel variant of the pair ([c], match_align / Matcher.align):
    pr_sc_relative_pose, host only.  An initial guess for ICP (DESIGN.md "Alignment")."""
    fq = np.ascontiguousarray(frames_q, np.float64).reshape(-1, 16)
    fd = np.ascontiguousarray(frames_db, np.float64).reshape(-1, 16)
    v = np.ascontiguousarray(variant, np.int32).reshape(-1)
    if fq.shape[0] != v.shape[0] or fd.shape[0] != v.shape[0]:
        raise ValueError("frames_q, frames_db and variant must describe the same pairs")
    T = np.empty((v.shape[0], 3, 4), np.float64)
    lib = _lib.load()
    rc = lib.pr_sc_relative_pose(_ptr(fq), _ptr(fd), _ptr(v), v.shape[0], _ptr(T))
    if rc != 0:
        raise PRError(rc, lib.pr_last_error(None).decode())
    return T


# ------------------------------------------------------------------------------- ICP refinement and verification (icp.hip)
ICP_STATS = np.dtype([("fitness", "<f8"), ("rmse", "<f8"), ("n_inl", "<i4"), ("iters", "<i4"), ("status", "<i4"), ("pad", "<i4")])   # pr_icp_stats


def icp_tile_rows() -> int:
    """Target rows a workgroup of the correspondence kernel stages at a time (pr_icp_tile_rows)."""
    return int(_lib.load().pr_icp_tile_rows())


def _icp_sets(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T):
    xq = np.ascontiguousarray(xyz_q, np.float64).reshape(-1, 3); oq = np.ascontiguousarray(offs_q, np.int64).reshape(-1)
    xd = np.ascontiguousarray(xyz_db, np.float64).reshape(-1, 3); od = np.ascontiguousarray(offs_db, np.int64).reshape(-1)
    ps = np.ascontiguousarray(pair_src, np.int32).reshape(-1); pd = np.ascontiguousarray(pair_dst, np.int32).reshape(-1)
    if len(oq) < 1 or len(od) < 1 or oq[-1] != len(xq) or od[-1] != len(xd):
        raise ValueError("clouds are CSR sets: xyz [offs[-1], 3] and offs [N + 1]")
    if len(ps) != len(pd):
        raise ValueError("pair_src and pair_dst must have the same length")
    c = len(ps)
    T = np.ascontiguousarray(T, np.float64)
    if T.size != 12 * c:
        raise ValueError("T must be [c, 3, 4]")
    return xq, oq, xd, od, ps, pd, c, T.reshape(c, 3, 4)


_ICP_SEARCH = {"brute": _lib.ICP_SEARCH_BRUTE, "grid": _lib.ICP_SEARCH_GRID}


@contextlib.contextmanager
def icp_search(ctx: Context, search: str | None):
    """The `search=` keyword of the ICP calls: None leaves the context's correspondence search (pr_set_icp_search, or PR_ICP_SEARCH in
    the environment) alone; "brute" | "grid" sets it for the body and restores what it was.  "grid"  finds the same
    correspondences from a uniform grid over the target: a refinement returns the bytes "brute" returns under pr_set_icp_path(ctx, 2).
    Measured on one MI355X with 30 forced iterations ("Measured"): 1 pair of 50 000-point clouds 4.7 ms against 33.3 ms,
    64 pairs of 4096-point clouds 8.5 ms against 13.8 ms; "grid" loses where most of the target falls into a source's 27 cells."""
    if search is None:
        yield ctx
        return
    if search not in _ICP_SEARCH:
        raise ValueError("search must be None, 'brute' or 'grid'")
    before = ctx.lib.pr_get_icp_search(ctx.h)
    ctx.check(ctx.lib.pr_set_icp_search(ctx.h, _ICP_SEARCH[search]))
    try:
        yield ctx
    finally:
        ctx.check(ctx.lib.pr_set_icp_search(ctx.h, before))


def icp_nn_radius(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T, max_corr: float = 1.0, ctx: Context | None = None,
                  search: str | None = None):
    """icp_nn restricted to the radius (pr_icp_nn_radius): the brute-force (nn_idx, nn_d2) where d2 < max_corr^2, -1 / +Inf elsewhere - the
    correspondences a refinement uses.  The context's search mode (or search=, see icp_search) chooses the scan-and-mask or the uniform
    grid; the two return the same bits."""
    ctx = ctx or default_context()
    xq, oq, xd, od, ps, pd, c, T = _icp_sets(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T)
    total = int(sum(oq[s + 1] - oq[s] for s, d in zip(ps, pd) if 0 <= s < len(oq) - 1 and d >= 0))
    out_offs = np.zeros(c + 1, np.int64); idx = np.empty(total, np.int32); d2 = np.empty(total, np.float64)
    with icp_search(ctx, search):
        ctx.check(ctx.lib.pr_icp_nn_radius(ctx.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(xd), _ptr(od), len(od) - 1, _ptr(ps), _ptr(pd), c, _ptr(T),
                                           float(max_corr), _ptr(out_offs), _ptr(idx), _ptr(d2)))
    return out_offs, idx, d2


def icp_nn(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T, ctx: Context | None = None):
    """One correspondence pass (pr_icp_nn) for the pairs (pair_src[i] of the query clouds, pair_dst[i] of the DB clouds; -1 = none) under
    T [c, 3, 4]: returns (out_offs int64 [c + 1], nn_idx int32, nn_d2 float64): pair i's source points are rows out_offs[i] .. out_offs[i + 1];
    -1 / +Inf where a point has no finite candidate."""
    ctx = ctx or default_context()
    xq, oq, xd, od, ps, pd, c, T = _icp_sets(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T)
    total = int(sum(oq[s + 1] - oq[s] for s, d in zip(ps, pd) if 0 <= s < len(oq) - 1 and d >= 0))
    out_offs = np.zeros(c + 1, np.int64); idx = np.empty(total, np.int32); d2 = np.empty(total, np.float64)
    ctx.check(ctx.lib.pr_icp_nn(ctx.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(xd), _ptr(od), len(od) - 1, _ptr(ps), _ptr(pd), c, _ptr(T),
                                _ptr(out_offs), _ptr(idx), _ptr(d2)))
    return out_offs, idx, d2


def icp_refine(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0, max_iter: int = 30, max_corr: float = 1.0, tol_rmse: float = 1e-6,
               tol_fitness: float = 1e-6, min_inliers: int = 3, ctx: Context | None = None, search: str | None = None):
    """Point-to-point ICP of every pair from its seed T0 [c, 3, 4] (pr_icp_pairs; the arithmetic is in the header): returns
    (T float64 [c, 3, 4], stats [c] of dtype ICP_STATS: fitness, rmse, n_inl, iters, status = _lib.ICP_*).  search: None | "brute" | "grid",
    the correspondence search of this call (icp_search)."""
    ctx = ctx or default_context()
    xq, oq, xd, od, ps, pd, c, T0 = _icp_sets(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0)
    T = np.empty((c, 3, 4)); stats = np.zeros(c, ICP_STATS)
    with icp_search(ctx, search):
        ctx.check(ctx.lib.pr_icp_pairs(ctx.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(xd), _ptr(od), len(od) - 1, _ptr(ps), _ptr(pd), c, _ptr(T0),
                                       int(max_iter), float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), _ptr(T), _ptr(stats)))
    return T, stats


def icp_refine_torch(xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0, max_src_pts: int, max_dst_pts: int, max_iter: int = 30,
                     max_corr: float = 1.0, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3, ctx: Context | None = None,
                     out=None, search: str | None = None):
    """Device form (pr_icp_pairs_dev): CUDA tensors xyz float64 [*, 3], offs int64 [N + 1], pairs int32 [c], T0 float64 [c, 3, 4];
    max_src_pts / max_dst_pts: the most points a source / target cloud of a pair has (host numbers: nothing is read back).  Returns
    (T float64 [c, 3, 4], stats uint8 [c, 32] - view it on the host with ICP_STATS), device tensors; nothing synchronises.  out: the pair
    (T, stats) an earlier call returned for the same c - written again (fixed addresses: what a captured graph needs).
    ctx given: its stream is the caller's to order; ctx None: the per-device default context, joined to torch's current stream.
    search: None | "brute" | "grid", the correspondence search of this call (icp_search)."""
    import torch
    from .eval import _on_stream, _p
    ts = (xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0)
    want = (torch.float64, torch.int64, torch.float64, torch.int64, torch.int32, torch.int32, torch.float64)
    if any((not t.is_cuda) or t.dtype != w or not t.is_contiguous() for t, w in zip(ts, want)):
        raise ValueError("icp_refine_torch: expected contiguous CUDA tensors xyz f64, offs i64, pairs i32, T0 f64")
    c = pair_src.numel()
    if pair_dst.numel() != c or T0.numel() != 12 * c:
        raise ValueError("icp_refine_torch: pair_src, pair_dst [c] and T0 [c, 3, 4] disagree")
    dev = xyz_q.device
    if out is None:
        out = (torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev))
    elif out[0].shape != (c, 3, 4) or out[1].shape != (c, ICP_STATS.itemsize):
        raise ValueError("icp_refine_torch: out belongs to another c")
    with _on_stream(ctx, dev, ts + tuple(out)) as cx, icp_search(cx, search):
        cx.check(cx.lib.pr_icp_pairs_dev(cx.h, _p(xyz_q), _p(offs_q), offs_q.numel() - 1, _p(xyz_db), _p(offs_db), offs_db.numel() - 1,
                                         _p(pair_src), _p(pair_dst), c, _p(T0), int(max_src_pts), int(max_dst_pts), int(max_iter),
                                         float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), _p(out[0]), _p(out[1])))
    return out


def icp_accept(stats, min_fitness: float, max_rmse: float) -> np.ndarray:
    """accepted = (status is converged or max_iter) and fitness >= min_fitness and rmse <= max_rmse, per pair."""
    ok = (stats["status"] == _lib.ICP_CONVERGED) | (stats["status"] == _lib.ICP_MAX_ITER)
    return ok & (stats["fitness"] >= min_fitness) & (stats["rmse"] <= max_rmse)


def verify_matches(clouds_q, clouds_db, idx, variant, frames_q, frames_db, max_corr: float = 1.0, min_fitness: float = 0.5,
                   max_rmse: float = 0.5, max_iter: int = 30, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3,
                   ctx: Context | None = None, search: str | None = None):
    """Use a match: sc_relative_pose -> icp_refine for every (query q, candidate idx[q, j]).  clouds_q / clouds_db: (xyz, offs) CSR sets;
    idx [m, k] DB rows as match_topk returns them (-1 = none); variant [m, k] the SC structure-channel variants (match_align(...)[0][..., 0]);
    frames_q [m, 16] / frames_db [n, 16] as cloud_frames returns them.  Returns (T [m, k, 3, 4], stats [m, k] of ICP_STATS, accepted bool
    [m, k]); a pair without a candidate or a variant has status ICP_NO_PAIR, T = identity and is not accepted.  SC only: only SC has a
    relative pose.  search: None | "brute" | "grid", the correspondence search of this call (icp_search)."""
    ix = np.ascontiguousarray(idx, np.int32)
    v = np.ascontiguousarray(variant, np.int32)
    if ix.ndim != 2 or v.shape != ix.shape:
        raise ValueError("idx and variant must be [m, k]")
    m, k = ix.shape
    fq = np.ascontiguousarray(frames_q, np.float64).reshape(-1, 16); fd = np.ascontiguousarray(frames_db, np.float64).reshape(-1, 16)
    has = ((ix >= 0) & (v >= 0)).reshape(-1)
    src = np.repeat(np.arange(m, dtype=np.int32), k)
    dst = np.where(has, ix.reshape(-1), -1).astype(np.int32)
    src = np.where(has, src, -1).astype(np.int32)
    T0 = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (m * k, 1, 1))
    if has.any():
        T0[has] = sc_relative_pose(fq[src[has]], fd[dst[has]], v.reshape(-1)[has])
    T, stats = icp_refine(clouds_q[0], clouds_q[1], clouds_db[0], clouds_db[1], src, dst, T0, max_iter, max_corr, tol_rmse, tol_fitness,
                          min_inliers, ctx, search)
    return T.reshape(m, k, 3, 4), stats.reshape(m, k), icp_accept(stats, min_fitness, max_rmse).reshape(m, k)


# ------------------------------------------------------------------------------- pose seeds of every type and the device verify chain (pose.hip)
_POSE_TYPES = {"sc": _lib.POSE_SC, "m2dp": _lib.POSE_M2DP, "delight": _lib.POSE_DELIGHT, _lib.POSE_SC: _lib.POSE_SC, _lib.POSE_M2DP: _lib.POSE_M2DP,
               _lib.POSE_DELIGHT: _lib.POSE_DELIGHT}


def _pose_type(type_) -> int:
    if type_ not in _POSE_TYPES:
        raise ValueError("pose type must be 'sc', 'm2dp' or 'delight'")
    return _POSE_TYPES[type_]


def relative_pose(type_, frames_q, frames_db, variant) -> np.ndarray:
    """sc_relative_pose for every type with variants (pr_relative_pose, host only): type_ 'sc' | 'm2dp' | 'delight', the frames [c, 16] of
    the clouds the descriptors were generated from and the pair's variant [c] (one channel of match_align / Matcher.align) ->
    [R | t] float64 [c, 3, 4] mapping query-camera-frame points into the DB entry's camera frame.  For 'sc': sc_relative_pose's bits."""
    t = _pose_type(type_)
    fq = np.ascontiguousarray(frames_q, np.float64).reshape(-1, 16)
    fd = np.ascontiguousarray(frames_db, np.float64).reshape(-1, 16)
    v = np.ascontiguousarray(variant, np.int32).reshape(-1)
    if fq.shape[0] != v.shape[0] or fd.shape[0] != v.shape[0]:
        raise ValueError("frames_q, frames_db and variant must describe the same pairs")
    T = np.empty((v.shape[0], 3, 4), np.float64)
    lib = _lib.load()
    rc = lib.pr_relative_pose(t, _ptr(fq), _ptr(fd), _ptr(v), v.shape[0], _ptr(T))
    if rc != 0:
        raise PRError(rc, lib.pr_last_error(None).decode())
    return T


def _variant_view(variant, m, k, H):
    """(pointer tensor, stride in ints) of a variant tensor [m, k] or [m, k, >= H] whose channels may be a slice of a wider tensor."""
    import torch
    if variant.dtype != torch.int32 or not variant.is_cuda:
        raise ValueError("variant must be an int32 CUDA tensor")
    if variant.dim() == 2:
        variant = variant.unsqueeze(-1)
    if variant.dim() != 3 or tuple(variant.shape[:2]) != (m, k) or variant.shape[2] < H:
        raise ValueError("variant must be [m, k] or [m, k, >= hypotheses]")
    if m * k == 0:
        return variant, max(H, 1)
    stride = variant.stride(1) if k > 1 or m == 1 else variant.stride(0)
    ok = (variant.shape[2] == 1 or variant.stride(2) == 1) and (k == 1 or variant.stride(1) == stride) and (m == 1 or variant.stride(0) == k * stride)
    if not ok or stride < H:
        variant = variant.contiguous()
        stride = variant.shape[2]
    return variant, int(stride)


def relative_pose_torch(type_, frames_q, frames_db, idx, variant, hypotheses: int = 1, db_row0: int = 0, ctx: Context | None = None):
    """Device form (pr_relative_pose_dev): CUDA tensors frames_q [m, 16] / frames_db [n_local, 16] float64, idx int32 [m, k] GLOBAL DB rows,
    variant int32 [m, k] or [m, k, >= hypotheses] (a channel slice of Matcher.align's tensor is read in place).  Returns device tensors
    (T0 float64 [m, k, H, 3, 4], pair_src int32 [m, k, H], pair_dst int32 [m, k, H]) for icp_refine_torch; slots without a pose are -1 /
    [I | 0].  Nothing synchronises."""
    import torch
    from .eval import _on_stream, _p
    t = _pose_type(type_)
    H = int(hypotheses)
    if any((not x.is_cuda) or x.dtype != w or not x.is_contiguous() for x, w in ((frames_q, torch.float64), (frames_db, torch.float64), (idx, torch.int32))):
        raise ValueError("relative_pose_torch: expected contiguous CUDA tensors frames f64 [*, 16], idx i32 [m, k]")
    m, k = idx.shape
    if frames_q.shape != (m, 16) or frames_db.dim() != 2 or frames_db.shape[1] != 16:
        raise ValueError("relative_pose_torch: frames_q must be [m, 16] and frames_db [n_local, 16]")
    var, stride = _variant_view(variant, m, k, H)
    dev = idx.device
    T0 = torch.empty((m, k, H, 3, 4), dtype=torch.float64, device=dev)
    src = torch.empty((m, k, H), dtype=torch.int32, device=dev)
    dst = torch.empty((m, k, H), dtype=torch.int32, device=dev)
    with _on_stream(ctx, dev, (frames_q, frames_db, idx, var, T0, src, dst)) as cx:
        cx.check(cx.lib.pr_relative_pose_dev(cx.h, t, _p(frames_q), m, _p(frames_db), frames_db.shape[0], int(db_row0), k, _p(idx), _p(var), stride, H,
                                             _p(T0), _p(src), _p(dst)))
    return T0, src, dst


def _verify_out(out, m, k, dev, who):
    """The result tensors (T, stats, accepted, hyp) of a verify call over [m, k] pairs: new ones, or the checked tuple of an earlier call."""
    import torch
    if out is None:
        # (every element is written by the call; torch.empty enqueues nothing on torch's stream that the context's stream could overtake)
        return (torch.empty((m, k, 3, 4), dtype=torch.float64, device=dev), torch.empty((m, k, ICP_STATS.itemsize), dtype=torch.uint8, device=dev),
                torch.empty((m, k), dtype=torch.bool, device=dev), torch.empty((m, k), dtype=torch.int32, device=dev))
    if out[0].shape != (m, k, 3, 4) or out[1].shape != (m, k, ICP_STATS.itemsize) or out[2].shape != (m, k) or out[3].shape != (m, k):
        raise ValueError(f"{who}: out belongs to another [m, k]")
    return out


def verify_pairs_torch(type_, clouds_q, clouds_db, frames_q, frames_db, idx, variant, max_src_pts: int, max_dst_pts: int, hypotheses: int = 1,
                       db_row0: int = 0, max_corr: float = 1.0, min_fitness: float = 0.5, max_rmse: float = 0.5, max_iter: int = 30,
                       tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3, ctx: Context | None = None, out=None,
                       search: str | None = None):
    """The device form of verify (pr_verify_pairs_dev): seed -> ICP over the [m, k, hypotheses] slots -> the better hypothesis, all on the
    context's stream without read-back.  clouds_q / clouds_db: (xyz float64 [*, 3], offs int64 [N + 1]) CUDA tensors, cloud q = query q,
    cloud r = DB row db_row0 + r; frames, idx, variant as relative_pose_torch takes them.  Returns device tensors (T float64 [m, k, 3, 4],
    stats uint8 [m, k, 32] - ICP_STATS on the host -, accepted bool [m, k], hyp int32 [m, k]); out: the tuple an earlier call returned for
    the same [m, k] - written again (fixed addresses: what a captured graph needs).  search: None | "brute" | "grid", the correspondence
    search of this call (icp_search)."""
    import torch
    from .eval import _on_stream, _p
    t = _pose_type(type_)
    H = int(hypotheses)
    xq, oq = clouds_q
    xd, od = clouds_db
    ts = (xq, oq, xd, od, frames_q, frames_db, idx)
    want = (torch.float64, torch.int64, torch.float64, torch.int64, torch.float64, torch.float64, torch.int32)
    if any((not x.is_cuda) or x.dtype != w or not x.is_contiguous() for x, w in zip(ts, want)):
        raise ValueError("verify_pairs_torch: expected contiguous CUDA tensors xyz f64, offs i64, frames f64, idx i32")
    m, k = idx.shape
    if frames_q.shape != (m, 16) or frames_db.dim() != 2 or frames_db.shape[1] != 16:
        raise ValueError("verify_pairs_torch: frames_q must be [m, 16] and frames_db [n_local, 16]")
    var, stride = _variant_view(variant, m, k, H)
    dev = idx.device
    out = _verify_out(out, m, k, dev, "verify_pairs_torch")
    with _on_stream(ctx, dev, ts + (var,) + tuple(out)) as cx, icp_search(cx, search):
        cx.check(cx.lib.pr_verify_pairs_dev(cx.h, t, _p(xq), _p(oq), oq.numel() - 1, _p(xd), _p(od), od.numel() - 1, _p(frames_q), _p(frames_db), m,
                                            frames_db.shape[0], int(db_row0), k, _p(idx), _p(var), stride, H, int(max_src_pts), int(max_dst_pts),
                                            int(max_iter), float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers),
                                            float(min_fitness), float(max_rmse), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3])))
    return out


def run_test(type_, hist1, hist2, gt1=None, gt2=None, loop_diff=None, mask_width=0, ctx: Context | None = None, device_eval: bool = False):
    """run_test.m:1.  Without ground truth: returns (diff_v, diff_idx) of run_test.m:57 (0-based indices).
    With gt1/gt2/loop_diff: returns (AUC, top_recall, lp_detected) through eval.precision_recall; the sweep ranks the QUERIES by their
    best score (run_test.m:58), so every query is then answered from its exact fp64 row unless the caller brings a context of its own
    (pr_set_exact_statistics: scores are the reference's doubles to rounding, two queries whose scores agree to 1e-5 keep their places).
    device_eval: the evaluation runs on the device (eval.precision_recall_gpu) instead of the host loops; the same values."""
    if gt1 is not None and ctx is None and type_ in ("sc", "m2dp", TYPE_SC, TYPE_M2DP):
        with _exact_statistics(default_context()) as c:            # the default context (its device, its arithmetic), exact statistics for this call
            idx, sc = match_topk(type_, hist1, hist2, mask_width, 2.0, 1, c)
    else:
        idx, sc = match_topk(type_, hist1, hist2, mask_width, 2.0, 1, ctx)
    if gt1 is None:
        return sc[:, 0], idx[:, 0]
    from . import eval as _eval
    if device_eval:
        return _eval.precision_recall_gpu(sc[:, 0], idx[:, 0], np.asarray(gt1), np.asarray(gt2), loop_diff, mask_width, ctx)[:3]
    return _eval.precision_recall(sc[:, 0], idx[:, 0], np.asarray(gt1), np.asarray(gt2), loop_diff, mask_width)[:3]


# ------------------------------------------------------------------------------- host-side rows a1 / a2
class CloudWindow:
    """pr_window: the pre-stage one keyframe at a time.  The reference's "nearby" point set stays in HBM; push() appends a keyframe's new
    world points, prunes against its pose and returns its down-sampled cloud (None during the 30 warm-up frames after a reset) - bit for
    bit the cloud the batch pre-stage emits for that pose.  point_capacity: most points alive at once (plus one keyframe's new ones),
    max_new: most new points of a push, max_out: most points of an emitted cloud.  Exceeding a capacity drops the excess and sets
    WINDOW_OVERFLOW in info[3] until the next reset (there is no error: nothing is read back in the device form)."""

    def __init__(self, ctx: Context | None = None, lidar_range: float = 45.0, polar: bool = False, point_capacity: int = 1 << 20,
                 max_new: int = 1 << 16, max_out: int = 1 << 17):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.polar, self.lidar_range = bool(polar), float(lidar_range)
        self.point_capacity, self.max_new, self.max_out = int(point_capacity), int(max_new), int(max_out)
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_window_create(self.ctx.h, self.lidar_range, int(polar) if isinstance(polar, (bool, np.bool_)) else polar,
                                                 self.point_capacity, self.max_new, self.max_out, C.byref(h)))
        self.h = h
        self._oxyz = np.empty((self.max_out, 3), np.float64)
        self._oint = np.empty(self.max_out, np.float32)

    def push(self, pose, xyz, inten):
        """Host form (pr_window_push; synchronises): pose = 3x4 world-to-camera (12 numbers, row-major), xyz [n, 3] world points, inten [n].
        Returns (xyz [n_out, 3] f64 | None, inten [n_out] f32 | None, frame [16] f64, info [4] i32 = emitted, n_out, alive, flags)."""
        w = np.ascontiguousarray(pose, np.float64).reshape(12)
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        it = np.ascontiguousarray(inten, np.float32).reshape(-1)
        if len(it) != len(x):
            raise ValueError("CloudWindow.push: xyz [n, 3] and inten [n] disagree")
        frame = np.empty(16, np.float64); info = np.empty(4, np.int32); n_out = C.c_int32()
        self.ctx.check(self.lib.pr_window_push(self.h, _ptr(w), _ptr(x) if len(x) else None, _ptr(it) if len(x) else None, len(x),
                                               _ptr(self._oxyz), _ptr(self._oint), C.byref(n_out), _ptr(frame), _ptr(info)))
        if not info[0]:
            return None, None, frame, info
        return self._oxyz[:n_out.value].copy(), self._oint[:n_out.value].copy(), frame, info

    def empty_out(self, device=None):
        """The output tensors of push_torch (fixed addresses for a captured graph): dict xyz [max_out, 3] f64, inten [max_out] f32,
        offs [2] i64, frame [16] f64, info [4] i32."""
        import torch
        dev = device if device is not None else torch.device("cuda", self.ctx.device)
        return dict(xyz=torch.zeros((self.max_out, 3), dtype=torch.float64, device=dev), inten=torch.zeros(self.max_out, dtype=torch.float32, device=dev),
                    offs=torch.zeros(2, dtype=torch.int64, device=dev), frame=torch.zeros(16, dtype=torch.float64, device=dev),
                    info=torch.zeros(4, dtype=torch.int32, device=dev))

    def push_torch(self, pose, xyz, inten, n_new, out=None):
        """Device form (pr_window_push_dev): contiguous CUDA tensors pose f64 [12] (or [3, 4]), xyz f64 [max_new', 3], inten f32 [max_new'],
        n_new i32 [1] - the count is read on the device.  Enqueued on the window's context's stream (the caller orders it against the
        producers of the inputs, e.g. a Context made on torch's current stream); nothing synchronises, nothing is allocated when out= (a
        dict of empty_out()) is given, so the call can be captured and the graph replayed for every keyframe.  Returns out."""
        import torch
        ts = (pose, xyz, inten, n_new)
        want = (torch.float64, torch.float64, torch.float32, torch.int32)
        if any((not t.is_cuda) or t.dtype != w or not t.is_contiguous() for t, w in zip(ts, want)):
            raise ValueError("push_torch: expected contiguous CUDA tensors pose f64, xyz f64, inten f32, n_new i32")
        if pose.numel() != 12 or xyz.dim() != 2 or xyz.shape[1] != 3 or inten.numel() != xyz.shape[0] or n_new.numel() != 1:
            raise ValueError("push_torch: pose [12], xyz [n, 3], inten [n], n_new [1]")
        if out is None:
            out = self.empty_out(pose.device)
        elif out["xyz"].shape != (self.max_out, 3) or out["inten"].numel() != self.max_out:
            raise ValueError("push_torch: out belongs to another window")
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_window_push_dev(self.h, p(pose), p(xyz), p(inten), p(n_new), int(xyz.shape[0]), p(out["xyz"]), p(out["inten"]),
                                                   p(out["offs"]), p(out["frame"]), p(out["info"])))
        return out

    def reset(self):
        self.ctx.check(self.lib.pr_window_reset(self.h))

    def count(self) -> int:
        n = C.c_int32()
        self.ctx.check(self.lib.pr_window_count(self.h, C.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_window_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyframeMap:
    """pr_map: the clouds, PCA frames, poses and ids of the keyframes seen so far as one CSR set in HBM that grows on the stream - what
    verify_dev needs as its DB side, at fixed addresses.  The seven buffers are zeroed torch tensors on the context's
    device (or the caller's: buffers = dict of the seven names): .xyz [point_capacity, 3] f64, .inten [point_capacity] f32, .offs
    [keyframe_capacity + 1] i64, .frames [keyframe_capacity, 16] f64, .poses [keyframe_capacity, 12] f64, .ids [keyframe_capacity] i32,
    .state [4] i32 = keyframes, flags, 0, 0; .clouds = (xyz, offs).  A cloud that finds a free row always takes it (the map stays in step
    with a signature database growing beside it); one that does not fit (more than max_cloud_points points, no room left in xyz, beyond
    the call's max_points) leaves an empty cloud and a zero frame there and sets MAP_OVERFLOW | MAP_DROPPED in info[3]; without a free
    row nothing is appended and MAP_OVERFLOW is set.  MAP_OVERFLOW stays until reset().  There is no error: nothing is read back."""

    NAMES = ("xyz", "inten", "offs", "frames", "poses", "ids", "state")

    def __init__(self, ctx: Context | None, keyframe_capacity: int, point_capacity: int, max_cloud_points: int, max_append: int = 1,
                 buffers: dict | None = None):
        import torch
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.keyframe_capacity, self.point_capacity = int(keyframe_capacity), int(point_capacity)
        self.max_cloud_points, self.max_append = int(max_cloud_points), int(max_append)
        self.h = None
        kc, pc = max(self.keyframe_capacity, 0), max(self.point_capacity, 0)
        dev = torch.device("cuda", self.ctx.device)
        shapes = dict(xyz=((pc, 3), torch.float64), inten=((pc,), torch.float32), offs=((kc + 1,), torch.int64), frames=((kc, 16), torch.float64),
                      poses=((kc, 12), torch.float64), ids=((kc,), torch.int32), state=((4,), torch.int32))
        if buffers is None:
            buffers = {n: torch.zeros(s, dtype=dt, device=dev) for n, (s, dt) in shapes.items()}
        for n, (s, dt) in shapes.items():
            t = buffers[n]
            if (not t.is_cuda) or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != tuple(s):
                raise ValueError(f"KeyframeMap: buffer {n} must be a contiguous CUDA tensor {dt} {list(s)}")
            setattr(self, n, t)
        torch.cuda.synchronize(dev)                       # torch's fills (its stream) before the library's stream writes the buffers
        rec = _lib.MapBuffers(*(C.c_void_p(getattr(self, n).data_ptr()) for n in self.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_map_create(self.ctx.h, C.byref(rec), self.keyframe_capacity, self.point_capacity, self.max_cloud_points,
                                              self.max_append, C.byref(h)))
        self.h = h

    @property
    def clouds(self):
        return self.xyz, self.offs

    def append_torch(self, xyz, inten, offs, frames, poses=None, ids=None, emitted=None, max_points=None, info=None):
        """Device form (pr_map_append_dev): contiguous CUDA tensors xyz f64 [n, 3], inten f32 [n], offs i64 [N + 1] (cloud i = points
        offs[i] .. offs[i + 1]; offs[0] need not be 0), frames f64 [N, 16] ([16] for N = 1), poses f64 [N, 12] | None (zeros), ids i32 [N] |
        None (-1), emitted i32 [>= 1] | None - emitted[0] == 0 switches the call off on the device (info of the window push in front).
        max_points: the most points the N clouds hold together (default n).  Enqueued on the map's context's stream; nothing synchronises,
        nothing is allocated when info= (i32 [4]) is given, so a captured append serves every keyframe.  Returns info (device) =
        clouds appended, first row | -1, keyframes after, flags."""
        import torch
        N = offs.numel() - 1
        ts = [(xyz, torch.float64), (inten, torch.float32), (offs, torch.int64), (frames, torch.float64)]
        ts += [(t, w) for t, w in ((poses, torch.float64), (ids, torch.int32), (emitted, torch.int32), (info, torch.int32)) if t is not None]
        if any((not t.is_cuda) or t.dtype != w or not t.is_contiguous() for t, w in ts):
            raise ValueError("append_torch: expected contiguous CUDA tensors xyz f64, inten f32, offs i64, frames f64, poses f64, ids i32, "
                             "emitted i32, info i32")
        if N < 0 or xyz.dim() != 2 or xyz.shape[1] != 3 or inten.numel() != xyz.shape[0] or frames.numel() != 16 * N \
                or (poses is not None and poses.numel() != 12 * N) or (ids is not None and ids.numel() != N) \
                or (emitted is not None and emitted.numel() < 1) or (info is not None and info.numel() != 4):
            raise ValueError("append_torch: xyz [n, 3], inten [n], offs [N + 1], frames [N, 16], poses [N, 12], ids [N], emitted [>= 1], info [4]")
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=xyz.device)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_map_append_dev(self.h, p(xyz), p(inten), p(offs), p(frames), p(poses), p(ids), p(emitted), N,
                                                  int(xyz.shape[0] if max_points is None else max_points), p(info)))
        return info

    def append_push(self, out, pose=None, id=None, info=None):
        """The keyframe a CloudWindow.push_torch left in `out` (its cloud, frame and - as emitted - its info: a warm-up push appends
        nothing), with pose f64 [12] and id i32 [1] device tensors (or None)."""
        return self.append_torch(out["xyz"], out["inten"], out["offs"], out["frame"], poses=pose, ids=id, emitted=out["info"],
                                 max_points=int(out["xyz"].shape[0]), info=info)

    def append(self, xyz, inten, offs, frames, poses=None, ids=None, emitted=None):
        """Host form (pr_map_append; synchronises): numpy arrays of the same meaning.  Returns info int32 [4]."""
        o = np.ascontiguousarray(offs, np.int64).reshape(-1)
        N = len(o) - 1
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        it = np.ascontiguousarray(inten, np.float32).reshape(-1)
        fr = np.ascontiguousarray(frames, np.float64).reshape(-1)
        po = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1)
        ii = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
        em = None if emitted is None else np.ascontiguousarray(emitted, np.int32).reshape(-1)
        if N < 0 or len(it) != len(x) or len(fr) != 16 * N or (po is not None and len(po) != 12 * N) or (ii is not None and len(ii) != N) \
                or (em is not None and len(em) < 1) or (N > 0 and (o.min() < 0 or o.max() > len(x))):
            raise ValueError("KeyframeMap.append: xyz [n, 3], inten [n], offs [N + 1] within n, frames [N, 16], poses [N, 12], ids [N], emitted [>= 1]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_map_append(self.h, _ptr(x), _ptr(it), _ptr(o), _ptr(fr), _ptr(po), _ptr(ii), _ptr(em), N, _ptr(info)))
        return info

    def verify_dev(self, matcher, idx, clouds_q, frames_q, max_src_pts: int, hypotheses: int = 1, seed: str | None = None, max_corr: float = 1.0,
                   min_fitness: float = 0.5, max_rmse: float = 0.5, max_iter: int = 30, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6,
                   min_inliers: int = 3, out=None, search: str | None = None):
        """matcher.verify_dev with this map as the DB side (pr_map_verify_dev): matcher.align(idx), then seed -> ICP -> choice against the
        map's rows idx - stream-ordered, capturable, the keywords and the result of matcher.verify_dev.  A row the map does not hold yet
        (or holds as a dropped cloud) comes back ICP_NO_PAIR / not accepted.  The matcher must run on the map's context."""
        import torch
        from .eval import _p
        if matcher.ctx is not self.ctx:
            raise ValueError("KeyframeMap.verify_dev: the matcher and the map must share one context (one stream)")
        seed, var, idx = matcher._verify_variants(idx, hypotheses, seed, 0)
        H = int(hypotheses)
        xq, oq = clouds_q
        ts = (xq, oq, frames_q, idx)
        if any((not x.is_cuda) or x.dtype != w or not x.is_contiguous() for x, w in zip(ts, (torch.float64, torch.int64, torch.float64, torch.int32))):
            raise ValueError("KeyframeMap.verify_dev: expected contiguous CUDA tensors xyz f64, offs i64, frames f64, idx i32")
        m, k = idx.shape
        if frames_q.shape != (m, 16):
            raise ValueError("KeyframeMap.verify_dev: frames_q must be [m, 16]")
        var, stride = _variant_view(var, m, k, H)
        dev = idx.device
        out = _verify_out(out, m, k, dev, "KeyframeMap.verify_dev")
        matcher._enter()
        with icp_search(self.ctx, search):
            self.ctx.check(self.lib.pr_map_verify_dev(self.h, _pose_type(seed), _p(xq), _p(oq), oq.numel() - 1, _p(frames_q), m, k, _p(idx), _p(var),
                                                      stride, H, int(max_src_pts), int(max_iter), float(max_corr), float(tol_rmse),
                                                      float(tol_fitness), int(min_inliers), float(min_fitness), float(max_rmse), _p(out[0]),
                                                      _p(out[1]), _p(out[2]), _p(out[3])))
        matcher._leave()
        return out

    def verify_variants(self, type_, idx, variant, clouds_q, frames_q, max_src_pts: int, hypotheses: int = 1, max_corr: float = 1.0,
                        min_fitness: float = 0.5, max_rmse: float = 0.5, max_iter: int = 30, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6,
                        min_inliers: int = 3, out=None, search: str | None = None):
        """verify_dev without a matcher (pr_map_verify_dev): the pairs' variants are the caller's - OnlineDatabase.align's, or any int32
        tensor [m, k] / [m, k, >= hypotheses] as relative_pose_torch takes them - and type_ = 'sc' | 'm2dp' | 'delight' names the seed.
        The other arguments, the result and the capturability are verify_dev's.  Enqueued on the map's context's stream."""
        import torch
        from .eval import _p
        H = int(hypotheses)
        if H not in (1, 2) or (H == 2 and type_ == "delight"):
            raise ValueError("KeyframeMap.verify_variants: hypotheses is 1 or 2, and 1 for DELIGHT (one variant per pair)")
        xq, oq = clouds_q
        ts = (xq, oq, frames_q, idx)
        if any((not x.is_cuda) or x.dtype != w or not x.is_contiguous() for x, w in zip(ts, (torch.float64, torch.int64, torch.float64, torch.int32))):
            raise ValueError("KeyframeMap.verify_variants: expected contiguous CUDA tensors xyz f64, offs i64, frames f64, idx i32")
        m, k = idx.shape
        if frames_q.shape != (m, 16):
            raise ValueError("KeyframeMap.verify_variants: frames_q must be [m, 16]")
        var, stride = _variant_view(variant, m, k, H)
        out = _verify_out(out, m, k, idx.device, "KeyframeMap.verify_variants")
        with icp_search(self.ctx, search):
            self.ctx.check(self.lib.pr_map_verify_dev(self.h, _pose_type(type_), _p(xq), _p(oq), oq.numel() - 1, _p(frames_q), m, k, _p(idx), _p(var),
                                                      stride, H, int(max_src_pts), int(max_iter), float(max_corr), float(tol_rmse),
                                                      float(tol_fitness), int(min_inliers), float(min_fitness), float(max_rmse), _p(out[0]),
                                                      _p(out[1]), _p(out[2]), _p(out[3])))
        return out

    def reset(self):
        self.ctx.check(self.lib.pr_map_reset(self.h))

    def count(self):
        """(keyframes, stored points, flags); synchronises (pr_map_count)."""
        k, f, n = C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx.check(self.lib.pr_map_count(self.h, C.byref(k), C.byref(n), C.byref(f)))
        return int(k.value), int(n.value), int(f.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_map_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _OnlineEngine:
    """What OnlineDatabase and OnlineSet share - the two front ends of ONE engine (online.hip): the buffers, made or validated from
    .parts = ((name, rows per entry, row length), ...); the checks of emitted= / out= / rows= / info=; match, append, step, reset, count
    and close.  A subclass names itself (_WHO), its C family (_C), its buffers record (_REC) and the order in which the family's calls
    take the part pointers (_ORDER; None for a part this object does not have), and sets .parts and .channels before _create."""

    def _create(self, ctx, code, capacity, max_k, buffers):
        import torch
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.capacity, self.max_k, self.h = int(capacity), int(max_k), None
        cap, dev = max(self.capacity, 0), torch.device("cuda", self.ctx.device)
        shapes = {**{n: ((cap * r, L), torch.float64) for n, r, L in self.parts}, "state": ((4,), torch.int32)}
        if buffers is None:
            buffers = {n: torch.zeros(s, dtype=dt, device=dev) for n, (s, dt) in shapes.items()}
        for n, (s, dt) in shapes.items():
            t = buffers[n]
            if (not t.is_cuda) or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != tuple(s):
                raise ValueError(f"{self._WHO}: buffer {n} must be a contiguous CUDA tensor {dt} {list(s)}")
            setattr(self, n, t)
        torch.cuda.synchronize(dev)                       # torch's fills (its stream) before the library's stream writes the buffers
        rec = self._REC(*(self._p(getattr(self, n)) if n in shapes else None for n, _ in self._REC._fields_))
        h = C.c_void_p()
        self.ctx.check(self._fn("create")(self.ctx.h, code, C.byref(rec), self.capacity, self.max_k, C.byref(h)))
        self.h = h

    _p = staticmethod(lambda t: None if t is None else C.c_void_p(t.data_ptr()))

    def _fn(self, name):
        return getattr(self.lib, f"{self._C}_{name}")

    def _sigs(self, sigs, who, emitted=None):
        """the call's part tensors, checked (as is emitted=), and their pointers in the C family's order"""
        import torch
        ts = tuple(sigs) if isinstance(sigs, (tuple, list)) else (sigs,)
        if len(ts) != len(self.parts):
            raise ValueError(f"{who}: sigs must hold {len(self.parts)} tensor(s): " + ", ".join(n for n, _, _ in self.parts))
        for t, (n, r, L) in zip(ts, self.parts):
            if (not t.is_cuda) or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != r * L:
                raise ValueError(f"{who}: {n} must be a contiguous CUDA tensor f64 [{r}, {L}]")
        if emitted is not None and ((not emitted.is_cuda) or emitted.dtype != torch.int32 or not emitted.is_contiguous() or emitted.numel() < 1):
            raise ValueError(f"{who}: emitted must be a CUDA tensor i32 [>= 1]")
        ptr = {n: self._p(t) for t, (n, _, _) in zip(ts, self.parts)}
        return ts, tuple(ptr.get(n) for n in self._ORDER)

    def match_torch(self, sigs, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, emitted=None, out=None, rows=None):
        """Device form (<family>_match_dev): the query's part(s) against the rows held NOW (the count is read on the device); the query
        counts as row `count` for the mask.  emitted i32 [>= 1] | None: emitted[0] == 0 switches the call off on the device (idx = -1,
        score = NaN).  Returns (idx int32 [1, k], score float64 [1, k]) - the shape verify takes; out: an earlier call's pair, written
        again.  rows f64 [channels, capacity] | None receives the distances (the first `count` of each row): 'sc' structure, intensity;
        'm2dp' count, intensity; 'fused' those four; 'delight' its one (no p_weight).  Nothing synchronises or, given out=, allocates."""
        import torch
        who = f"{self._WHO}.match_torch"
        ts, parts = self._sigs(sigs, who, emitted)
        k = int(k)
        dev, shape = ts[0].device, (self.channels, self.capacity)
        if rows is not None and ((not rows.is_cuda) or rows.dtype != torch.float64 or not rows.is_contiguous() or tuple(rows.shape) != shape):
            raise ValueError(f"{who}: rows must be a contiguous CUDA tensor f64 [{self.channels}, capacity]")
        if out is None:
            out = (torch.empty((1, max(k, 0)), dtype=torch.int32, device=dev), torch.empty((1, max(k, 0)), dtype=torch.float64, device=dev))
        elif tuple(out[0].shape) != (1, k) or tuple(out[1].shape) != (1, k) or out[0].dtype != torch.int32 or out[1].dtype != torch.float64 \
                or not (out[0].is_cuda and out[1].is_cuda and out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError(f"{who}: out must be (idx i32 [1, k], score f64 [1, k]) CUDA tensors")
        p = self._p
        self.ctx.check(self._fn("match_dev")(self.h, *parts, p(emitted), int(mask_width), float(p_weight), k, p(out[0]), p(out[1]), p(rows)))
        return out

    def append_torch(self, sigs, emitted=None, info=None):
        """Device form (<family>_append_dev, one launch): every part becomes row `count`, then the one count is committed (emitted as in
        match_torch).  Returns info (device i32 [4]) = appended, row | -1, count after, flags."""
        import torch
        who = f"{self._WHO}.append_torch"
        ts, parts = self._sigs(sigs, who, emitted)
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=ts[0].device)
        elif (not info.is_cuda) or info.dtype != torch.int32 or not info.is_contiguous() or info.numel() != 4:
            raise ValueError(f"{who}: info must be a CUDA tensor i32 [4]")
        self.ctx.check(self._fn("append_dev")(self.h, *parts, self._p(emitted), self._p(info)))
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

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self._fn("destroy")(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OnlineDatabase(_OnlineEngine):
    """pr_online: the raw SC or M2DP rows of the keyframes seen so far with a DEVICE-side count, matched exactly in fp64 and grown on the
    stream - the sibling of KeyframeMap for signatures.  type_ 'sc' | 'm2dp'; the two buffers are zeroed torch tensors
    on the context's device (or the caller's: buffers = dict(sig=, state=)): .sig [capacity * rows_per_sig, sig_len] f64 (1 x 2400 /
    4 x 384) and .state [4] i32 = count, flags, 0, 0.  Every call's launch geometry depends on capacity and max_k only and the count is
    read on the device, so ONE captured step_torch serves every keyframe of a drive.  At count == capacity an append stores nothing and
    sets ONLINE_OVERFLOW in info[3] until reset().  There is no error: nothing is read back.  All *_torch calls are enqueued on the
    context's stream (the caller orders it against the producers of the inputs, e.g. a Context made on torch's current stream)."""

    NAMES = ("sig", "state")
    _WHO, _C, _REC, _ORDER = "OnlineDatabase", "pr_online", _lib.OnlineBuffers, ("sig",)

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
        if (not idx.is_cuda) or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.dim() != 2 or idx.shape[0] != 1:
            raise ValueError(f"{who}: idx must be a contiguous CUDA tensor i32 [1, k]")
        k = idx.shape[1]
        ch = slice(0, 2) if self.type == _lib.TYPE_SC else slice(2, 4)
        if out is None:
            var = torch.empty((1, k, 4), dtype=torch.int32, device=idx.device)
            dist = torch.empty((1, k, 4), dtype=torch.float64, device=idx.device)
        else:
            var, dist = out[0]._base, out[1]._base
            if var is None or dist is None or tuple(var.shape) != (1, k, 4) or tuple(dist.shape) != (1, k, 4):
                raise ValueError(f"{who}: out must be the pair an earlier align() of the same k returned")
        p = lambda t: C.c_void_p(t.data_ptr())
        sc = (p(sig), p(self.sig), _lib.F64) if self.type == _lib.TYPE_SC else (None, None, 0)
        m2 = (p(sig), p(self.sig), _lib.F64) if self.type == _lib.TYPE_M2DP else (None, None, 0)
        self.ctx.check(self.lib.pr_align_pairs_dev(self.ctx.h, *sc, *m2, 1, self.capacity, 0, k, p(idx), p(var), p(dist)))
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
    _WHO, _C, _REC, _ORDER = "OnlineSet", "pr_onlineset", _lib.OnlineSetBuffers, ("sc", "m2dp", "delight")

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
        if (not idx.is_cuda) or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.dim() != 2 or idx.shape[0] != 1:
            raise ValueError(f"{who}: idx must be a contiguous CUDA tensor i32 [1, k]")
        k = idx.shape[1]
        C_ = 4 if self.kind == _lib.ONLINESET_FUSED else 2
        if out is None:
            var = torch.empty((1, k, C_), dtype=torch.int32, device=idx.device)
            dist = torch.empty((1, k, C_), dtype=torch.float64, device=idx.device)
        else:
            var, dist = out
            if tuple(var.shape) != (1, k, C_) or tuple(dist.shape) != (1, k, C_) or var.dtype != torch.int32 or dist.dtype != torch.float64 \
                    or not (var.is_cuda and dist.is_cuda and var.is_contiguous() and dist.is_contiguous()):
                raise ValueError(f"{who}: out must be the pair an earlier align() of the same k returned")
        p = lambda t: C.c_void_p(t.data_ptr())
        if self.kind == _lib.ONLINESET_FUSED:
            self.ctx.check(self.lib.pr_align_pairs_dev(self.ctx.h, p(ts[0]), p(self.sc), _lib.F64, p(ts[1]), p(self.m2dp), _lib.F64, 1, self.capacity, 0, k,
                                                       p(idx), p(var), p(dist)))
            return var, dist
        tmp = self._align_tmp.get(k)                      # the library writes [1][k] contiguous: staged, then copied into slot 0
        if tmp is None:
            tmp = self._align_tmp[k] = (torch.empty((1, k), dtype=torch.int32, device=idx.device), torch.empty((1, k), dtype=torch.float64, device=idx.device))
        self.ctx.check(self.lib.pr_delight_align_pairs_dev(self.ctx.h, p(ts[0]), p(self.delight), _lib.F64, 1, self.capacity, 0, k, p(idx), p(tmp[0]), p(tmp[1])))
        var[..., 0].copy_(tmp[0]); var[..., 1].fill_(-1)
        dist[..., 0].copy_(tmp[1]); dist[..., 1].fill_(float("nan"))
        return var, dist


class PoseGraph:
    """pr_posegraph: the accepted closures of a drive over caller-owned buffers with a DEVICE-side count, and a pose-graph relaxation of
    the map's poses over the odometry chain plus those closures.  The four buffers are zeroed torch tensors on the
    context's device (or the caller's: buffers = dict of the four names): .edge_ij [edge_capacity, 2] i32 (DB row i, query row j),
    .edge_Z [edge_capacity, 12] f64, .edge_w [edge_capacity, 2] f64 (w_rot, w_trans) and .state [4] i32 = edges, flags, 0, 0.  Every
    launch's geometry depends on the create sizes (and outer) only and both counts are read on the device, so ONE captured add_torch
    serves every keyframe and ONE captured relax_torch every count.  At edges == edge_capacity an add stores nothing and sets
    POSEGRAPH_OVERFLOW in info[3] until reset().  All *_torch calls are enqueued on the context's stream; nothing is read back."""

    NAMES = ("edge_ij", "edge_Z", "edge_w", "state")

    def __init__(self, ctx: Context | None, node_capacity: int, edge_capacity: int, max_outer: int = 10, max_inner: int = 256,
                 buffers: dict | None = None):
        import torch
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.node_capacity, self.edge_capacity = int(node_capacity), int(edge_capacity)
        self.max_outer, self.max_inner = int(max_outer), int(max_inner)
        self.h = None
        ec = max(self.edge_capacity, 0)
        dev = torch.device("cuda", self.ctx.device)
        shapes = dict(edge_ij=((ec, 2), torch.int32), edge_Z=((ec, 12), torch.float64), edge_w=((ec, 2), torch.float64), state=((4,), torch.int32))
        if buffers is None:
            buffers = {n: torch.zeros(s, dtype=dt, device=dev) for n, (s, dt) in shapes.items()}
        for n, (s, dt) in shapes.items():
            t = buffers[n]
            if (not t.is_cuda) or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != tuple(s):
                raise ValueError(f"PoseGraph: buffer {n} must be a contiguous CUDA tensor {dt} {list(s)}")
            setattr(self, n, t)
        torch.cuda.synchronize(dev)                       # torch's fills (its stream) before the library's stream writes the buffers
        rec = _lib.PoseGraphBuffers(*(C.c_void_p(getattr(self, n).data_ptr()) for n in self.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_posegraph_create(self.ctx.h, C.byref(rec), self.node_capacity, self.edge_capacity, self.max_outer,
                                                    self.max_inner, C.byref(h)))
        self.h = h

    @staticmethod
    def _dev(t, dtype, numel, who, what, exact=True):
        if (not t.is_cuda) or t.dtype != dtype or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise ValueError(f"{who}: {what}")

    def add_torch(self, idx, T, accepted, query_row, w_rot: float = 1.0, w_trans: float = 1.0, info=None):
        """Device form (pr_posegraph_add_dev): a verify's idx i32 [1, k] (or [k]), T f64 [1, k, 3, 4] and accepted bool | u8 [1, k], and query_row
        i32 [>= 1] - the row the query keyframe received: map_info[1:2] of the map append in front (a negative value switches the call
        off on the device).  Every accepted pair with a valid row and a finite T is logged as the edge (idx, query_row) with the weights
        (w_rot, w_trans).  Returns info (device i32 [4]) = edges logged, first row | -1, edges after, flags.  Nothing synchronises,
        nothing is allocated when info= is given."""
        import torch
        who = "PoseGraph.add_torch"
        k = idx.numel()
        self._dev(idx, torch.int32, k, who, "idx must be a contiguous CUDA tensor i32 [k]")
        self._dev(T, torch.float64, 12 * k, who, "T must be a contiguous CUDA tensor f64 [k, 3, 4]")
        self._dev(accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, k, who,
                  "accepted must be a contiguous CUDA tensor bool or u8 [k]")
        self._dev(query_row, torch.int32, 1, who, "query_row must be a CUDA tensor i32 [>= 1]", exact=False)
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=idx.device)
        else:
            self._dev(info, torch.int32, 4, who, "info must be a CUDA tensor i32 [4]")
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_posegraph_add_dev(self.h, p(idx), p(T), p(accepted), p(query_row), k, float(w_rot), float(w_trans), p(info)))
        return info

    def add(self, idx, T, accepted, query_row: int, w_rot: float = 1.0, w_trans: float = 1.0):
        """Host form (pr_posegraph_add; synchronises): numpy arrays of the same meaning, query_row an int.  Returns info int32 [4]."""
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        k = len(i)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        if len(t) != 12 * k or len(a) != k:
            raise ValueError("PoseGraph.add: idx [k], T [k, 3, 4], accepted [k]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraph_add(self.h, _ptr(i), _ptr(t), _ptr(a), int(query_row), k, float(w_rot), float(w_trans), _ptr(info)))
        return info

    def add_weighted_torch(self, idx, T, accepted, query_row, w, info=None):
        """Device form (pr_posegraphw_add_dev): add_torch with per-slot weights w f64 [k, 2] = (w_rot, w_trans) in device memory -
        RegistrationInfo's .w.  A slot is logged under add_torch's conditions and only if both of its weights are finite and >= 0.
        Returns info (device i32 [4]); nothing synchronises, nothing is allocated when info= is given."""
        import torch
        who = "PoseGraph.add_weighted_torch"
        k = idx.numel()
        self._dev(idx, torch.int32, k, who, "idx must be a contiguous CUDA tensor i32 [k]")
        self._dev(T, torch.float64, 12 * k, who, "T must be a contiguous CUDA tensor f64 [k, 3, 4]")
        self._dev(accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, k, who,
                  "accepted must be a contiguous CUDA tensor bool or u8 [k]")
        self._dev(query_row, torch.int32, 1, who, "query_row must be a CUDA tensor i32 [>= 1]", exact=False)
        self._dev(w, torch.float64, 2 * k, who, "w must be a contiguous CUDA tensor f64 [k, 2]")
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=idx.device)
        else:
            self._dev(info, torch.int32, 4, who, "info must be a CUDA tensor i32 [4]")
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_posegraphw_add_dev(self.h, p(idx), p(T), p(accepted), p(query_row), k, p(w), p(info)))
        return info

    def add_weighted(self, idx, T, accepted, query_row: int, w):
        """Host form (pr_posegraphw_add; synchronises): numpy arrays of the same meaning, w [k, 2].  Returns info int32 [4]."""
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        k = len(i)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        ww = np.ascontiguousarray(w, np.float64).reshape(-1)
        if len(t) != 12 * k or len(a) != k or len(ww) != 2 * k:
            raise ValueError("PoseGraph.add_weighted: idx [k], T [k, 3, 4], accepted [k], w [k, 2]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraphw_add(self.h, _ptr(i), _ptr(t), _ptr(a), int(query_row), k, _ptr(ww), _ptr(info)))
        return info

    def add_batch_torch(self, i, j, T, accepted, w=None, w_rot: float = 1.0, w_trans: float = 1.0, info=None):
        """Device form (pr_posegraphb_add_dev): c slots that carry their own rows - i i32 [c] the DB rows, j i32 [c] the query rows (a
        ProximitySearch's pair_dst and pair_src), T f64 [c, 3, 4], accepted bool | u8 [c], w f64 [c, 2] or None (then w_rot, w_trans for
        every slot).  Slot p is logged iff accepted, i >= 0, j >= 0, i != j, T finite and its weights finite and >= 0, in the order of p:
        what c calls of add_weighted_torch with one slot each leave.  Returns info (device i32 [4]); nothing synchronises, nothing is
        allocated when info= is given."""
        import torch
        who = "PoseGraph.add_batch_torch"
        c = i.numel()
        self._dev(i, torch.int32, c, who, "i must be a contiguous CUDA tensor i32 [c]")
        self._dev(j, torch.int32, c, who, "j must be a contiguous CUDA tensor i32 [c]")
        self._dev(T, torch.float64, 12 * c, who, "T must be a contiguous CUDA tensor f64 [c, 3, 4]")
        self._dev(accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, c, who,
                  "accepted must be a contiguous CUDA tensor bool or u8 [c]")
        if w is not None:
            self._dev(w, torch.float64, 2 * c, who, "w must be a contiguous CUDA tensor f64 [c, 2]")
        if info is None:
            info = torch.empty(4, dtype=torch.int32, device=i.device)
        else:
            self._dev(info, torch.int32, 4, who, "info must be a CUDA tensor i32 [4]")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_posegraphb_add_dev(self.h, p(i), p(j), p(T), p(accepted), p(w), float(w_rot), float(w_trans), c, p(info)))
        return info

    def add_batch(self, i, j, T, accepted, w=None, w_rot: float = 1.0, w_trans: float = 1.0):
        """Host form (pr_posegraphb_add; synchronises): numpy arrays of the same meaning.  Returns info int32 [4]."""
        ii = np.ascontiguousarray(i, np.int32).reshape(-1)
        jj = np.ascontiguousarray(j, np.int32).reshape(-1)
        c = len(ii)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        ww = None if w is None else np.ascontiguousarray(w, np.float64).reshape(-1)
        if len(jj) != c or len(t) != 12 * c or len(a) != c or (ww is not None and len(ww) != 2 * c):
            raise ValueError("PoseGraph.add_batch: i [c], j [c], T [c, 3, 4], accepted [c], w [c, 2]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraphb_add(self.h, _ptr(ii), _ptr(jj), _ptr(t), _ptr(a), _ptr(ww), float(w_rot), float(w_trans), c, _ptr(info)))
        return info

    def relax_torch(self, poses, n, outer: int = 5, inner: int = 64, lam: float = 1e-9, w_odo_rot: float = 1.0, w_odo_trans: float = 1.0,
                    out=None, report=None):
        """Device form (pr_posegraph_relax_dev): poses f64 [node_capacity, 12] (world to camera), n i32 [>= 1] whose word 0 is the node
        count - a KeyframeMap's .poses and .state.  `outer` damped Gauss-Newton steps of exactly `inner` preconditioned conjugate gradient
        iterations each over the odometry chain of the input poses (weights w_odo_rot, w_odo_trans) plus the logged edges.  out: f64
        [node_capacity, 12], may be poses itself (rows >= n are not written); report f64 [outer + 2] = the cost before each step, the
        final cost, the edges used.  Returns (out, report).  Nothing synchronises, nothing is allocated when out= and report= are given."""
        import torch
        who = "PoseGraph.relax_torch"
        outer = int(outer)
        self._dev(poses, torch.float64, 12 * self.node_capacity, who, "poses must be a contiguous CUDA tensor f64 [node_capacity, 12]")
        self._dev(n, torch.int32, 1, who, "n must be a CUDA tensor i32 [>= 1]", exact=False)
        if out is None:
            out = torch.zeros((self.node_capacity, 12), dtype=torch.float64, device=poses.device)
        else:
            self._dev(out, torch.float64, 12 * self.node_capacity, who, "out must be a contiguous CUDA tensor f64 [node_capacity, 12]")
        if report is None:
            report = torch.zeros(max(outer, 0) + 2, dtype=torch.float64, device=poses.device)
        else:
            self._dev(report, torch.float64, outer + 2, who, "report must be a CUDA tensor f64 [outer + 2]")
        prm = _lib.PoseGraphParams(outer, int(inner), float(lam), float(w_odo_rot), float(w_odo_trans))
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_posegraph_relax_dev(self.h, p(poses), p(n), C.byref(prm), p(out), p(report)))
        return out, report

    def relax_map(self, km, **kw):
        """relax_torch(km.poses, km.state, ...) for a KeyframeMap: out=km.poses corrects the map in place.  The map must live on this
        handle's context (one stream) and have node_capacity keyframes; anything else is refused before the library is called."""
        if km.ctx is not self.ctx:
            raise ValueError("PoseGraph.relax_map: the pose graph and the map must share one context (one stream)")
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError("PoseGraph.relax_map: node_capacity must equal the map's keyframe_capacity")
        return self.relax_torch(km.poses, km.state, **kw)

    def reset(self):
        self.ctx.check(self.lib.pr_posegraph_reset(self.h))

    def count(self):
        """(edges, flags); synchronises (pr_posegraph_count)."""
        n, f = C.c_int32(), C.c_int32()
        self.ctx.check(self.lib.pr_posegraph_count(self.h, C.byref(n), C.byref(f)))
        return int(n.value), int(f.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_posegraph_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClosureGate:
    """pr_gate: the closure consistency gate in front of the relaxation.  Every ordered pair of closures logged in pg_src
    is compared along the odometry chain of the poses; a closure is kept when at least min_support kept closures within max_gap
    keyframes (|i_a - i_b| + |j_a - j_b|, another query keyframe) agree with it, repeated `rounds` times; the kept closures are copied,
    in log order, into pg_dst's log, which pg_dst.relax_torch / relax_map then relaxes.  The tables are rot_tab[g] = 2 (1 - cos(rad(rot_deg
    + g rot_deg_per_kf))) and trans2_tab[g] = (trans + g trans_per_kf)^2 for g = 0 .. max_gap, or the arrays given (passed through
    unchanged; +Inf switches a test off).  Calls are enqueued on the context's stream, read both counts on the device and allocate no
    device scratch; ONE captured run_torch serves every count.  Close it before either graph."""

    def __init__(self, ctx: Context | None, pg_src, pg_dst, max_gap: int, min_support: int = 2, rounds: int = 8, rot_deg: float = 2.0,
                 rot_deg_per_kf: float = 0.05, trans: float = 0.5, trans_per_kf: float = 0.02, rot_tab=None, trans2_tab=None):
        self.ctx = ctx or default_context()
        self.h = None
        if pg_src is pg_dst:
            raise ValueError("ClosureGate: pg_src and pg_dst must be two graphs")
        if pg_src.ctx is not self.ctx or pg_dst.ctx is not self.ctx:
            raise ValueError("ClosureGate: the gate and both graphs must share one context (one stream)")
        if pg_src.node_capacity != pg_dst.node_capacity:
            raise ValueError("ClosureGate: both graphs must have the same node_capacity")
        if pg_dst.edge_capacity < pg_src.edge_capacity:
            raise ValueError("ClosureGate: pg_dst.edge_capacity must be at least pg_src.edge_capacity")
        self.lib = self.ctx.lib
        self.src, self.dst = pg_src, pg_dst
        self.node_capacity, self.edge_capacity = pg_src.node_capacity, pg_src.edge_capacity
        self.max_gap, self.min_support, self.rounds = int(max_gap), int(min_support), int(rounds)
        g = np.arange(max(self.max_gap, 0) + 1, dtype=np.float64)
        if rot_tab is None:
            rot_tab = 2.0 * (1.0 - np.cos(np.radians(float(rot_deg) + g * float(rot_deg_per_kf))))
        if trans2_tab is None:
            trans2_tab = (float(trans) + g * float(trans_per_kf)) ** 2
        self.rot_tab = np.ascontiguousarray(rot_tab, np.float64).reshape(-1)
        self.trans2_tab = np.ascontiguousarray(trans2_tab, np.float64).reshape(-1)
        if len(self.rot_tab) != len(g) or len(self.trans2_tab) != len(g):
            raise ValueError("ClosureGate: rot_tab and trans2_tab must have max_gap + 1 entries")
        recs = [_lib.PoseGraphBuffers(*(C.c_void_p(getattr(pg, n).data_ptr()) for n in pg.NAMES)) for pg in (pg_src, pg_dst)]
        prm = _lib.GateParams(self.max_gap, self.min_support, self.rounds)
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_gate_create(self.ctx.h, C.byref(recs[0]), C.byref(recs[1]), self.node_capacity, self.edge_capacity,
                                               pg_dst.edge_capacity, C.byref(prm), _ptr(self.rot_tab), _ptr(self.trans2_tab), C.byref(h)))
        self.h = h

    def _t(self, who, name, t, dtype, numel, exact=True):
        dev = self.src.state.device
        if (not t.is_cuda) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} of {'' if exact else 'at least '}{numel} elements on the "
                             "graphs' device")
        return t

    def run_torch(self, poses, n, keep=None, support=None, map=None, info=None):
        """Device form (pr_gate_run_dev): poses f64 [node_capacity, 12] (world to camera), n i32 [>= 1] whose word 0 is the node count - a
        KeyframeMap's .poses and .state.  Returns (keep u8 [edge_capacity], support i32 [edge_capacity] - the kept supporters of the last
        round, -1 for an edge that is not valid -, map i32 [edge_capacity] - the row in pg_dst or -1 -, info i32 [4] = valid, kept, edges
        read, flags GATE_*).  Nothing synchronises, nothing is allocated when all four are given."""
        import torch
        who = "ClosureGate.run_torch"
        ec, dev = self.edge_capacity, self.src.state.device
        self._t(who, "poses", poses, torch.float64, 12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, 1, exact=False)
        keep = torch.empty(ec, dtype=torch.uint8, device=dev) if keep is None else self._t(who, "keep", keep, torch.uint8, ec)
        support = torch.empty(ec, dtype=torch.int32, device=dev) if support is None else self._t(who, "support", support, torch.int32, ec)
        map = torch.empty(ec, dtype=torch.int32, device=dev) if map is None else self._t(who, "map", map, torch.int32, ec)
        info = torch.empty(4, dtype=torch.int32, device=dev) if info is None else self._t(who, "info", info, torch.int32, 4)
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_gate_run_dev(self.h, p(poses), p(n), p(keep), p(support), p(map), p(info)))
        return keep, support, map, info

    def run_map(self, km, **kw):
        """run_torch(km.poses, km.state, ...) for a KeyframeMap, with PoseGraph.relax_map's refusals."""
        if km.ctx is not self.ctx:
            raise ValueError("ClosureGate.run_map: the gate and the map must share one context (one stream)")
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError("ClosureGate.run_map: node_capacity must equal the map's keyframe_capacity")
        return self.run_torch(km.poses, km.state, **kw)

    def run(self, poses, n):
        """Host form (pr_gate_run; synchronises): poses and n as for run_torch (device tensors); returns NumPy (keep u8, support i32,
        map i32, info i32 [4])."""
        import torch
        who = "ClosureGate.run"
        self._t(who, "poses", poses, torch.float64, 12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, 1, exact=False)
        ec = self.edge_capacity
        keep, support, map_, info = np.empty(ec, np.uint8), np.empty(ec, np.int32), np.empty(ec, np.int32), np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_gate_run(self.h, C.c_void_p(poses.data_ptr()), C.c_void_p(n.data_ptr()), _ptr(keep), _ptr(support), _ptr(map_),
                                            _ptr(info)))
        return keep, support, map_, info

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_gate_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrajEval(NamedTuple):
    """What a TrajectoryEval run returns (torch tensors from run_torch / run_map, NumPy arrays from run); the parts a run does not have
    are None.  ate [B, 24] = N, sse, rmse, mean, max, argmax, s, R (9), t (3), flags, sigma (3), var_x; rpe [B, K, 8] = pairs, rmse / mean /
    max of d, rmse / mean / max of theta, mean c_rot; seg [B, L + 1, 4] = segments, mean t_err, mean r_err, mean path ratio (row L: all
    lengths); clo [8] = evaluated, wrong, rmse / max of theta, rmse / max of d, edges read, 0; err [B, cap]; seg_end [B, slots, L] i32;
    edge_err [EC, 2]; centres [B + 1, cap, 3]; prefix [B, 2, cap]."""
    ate: object
    rpe: object
    seg: object
    clo: object
    err: object
    seg_end: object
    edge_err: object
    centres: object
    prefix: object


class AteStats(NamedTuple):
    """The columns of TrajEval.ate by name (TrajectoryEval.ate_stats)."""
    N: object
    sse: object
    rmse: object
    mean: object
    max: object
    argmax: object
    s: object
    R: object
    t: object
    flags: object
    sigma: object
    var_x: object


class TrajectoryEval:
    """pr_trajeval: a trajectory against ground truth on the device - ATE under an alignment ("none", "first", "se3",
    "sim3"), RPE per row delta, KITTI's segment metric per path length and the error of logged closures - for B candidate pose arrays a
    call.  est f64 [B, node_capacity, 12] (or [node_capacity, 12] with B = 1): rows as KeyframeMap.poses (world to camera); gt by gt_kind:
    "w2c" [node_capacity, 12], "c2w" [node_capacity, 12] (KITTI's file rows) or "positions" [node_capacity, 3] (ATE only).  Calls are
    enqueued on the context's stream, read every count on the device and allocate no device scratch; ONE captured run_torch serves every
    count.  The rule is in include/place_recognition.h."""

    ALIGN = dict(none=_lib.TRAJ_ALIGN_NONE, first=_lib.TRAJ_ALIGN_FIRST, se3=_lib.TRAJ_ALIGN_SE3, sim3=_lib.TRAJ_ALIGN_SIM3)
    GT = dict(w2c=_lib.TRAJ_GT_W2C, c2w=_lib.TRAJ_GT_C2W, positions=_lib.TRAJ_GT_POSITIONS)
    NAMES = TrajEval._fields

    def __init__(self, ctx: Context | None, node_capacity: int, B: int = 1, align: str = "sim3", gt_kind: str = "c2w", deltas=(1, 10),
                 lengths=(100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0), step: int = 1, edge_capacity: int = 0,
                 rot_thr: float = float(np.radians(5.0)), trans_thr: float = 2.0):
        self.h = None
        if align not in self.ALIGN:
            raise ValueError(f"TrajectoryEval: align must be one of {sorted(self.ALIGN)}")
        if gt_kind not in self.GT:
            raise ValueError(f"TrajectoryEval: gt_kind must be one of {sorted(self.GT)}")
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.node_capacity, self.B, self.align, self.gt_kind = int(node_capacity), int(B), align, gt_kind
        self.deltas = np.ascontiguousarray(deltas, np.int32).reshape(-1)
        self.lengths = np.ascontiguousarray(lengths, np.float64).reshape(-1)
        self.K, self.L, self.step, self.edge_capacity = len(self.deltas), len(self.lengths), int(step), int(edge_capacity)
        self.gt_cols = 3 if gt_kind == "positions" else 12
        self.slots = -(-self.node_capacity // self.step) if self.step >= 1 and self.node_capacity >= 1 else 0
        self.params = _lib.TrajEvalParams(self.node_capacity, self.B, self.ALIGN[align], self.GT[gt_kind], self.K, self.L, self.step,
                                          self.edge_capacity, float(rot_thr), float(trans_thr))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_trajeval_create(self.ctx.h, C.byref(self.params), _ptr(self.deltas) if self.K else None,
                                                   _ptr(self.lengths) if self.L else None, C.byref(h)))
        self.h = h

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_trajeval_scratch_bytes(C.byref(self.params)))

    def shapes(self, log: bool = True):
        """name -> (shape, NumPy dtype) of every output this handle can write (clo and edge_err only with a closure log)."""
        B, cap, K, L = self.B, self.node_capacity, self.K, self.L
        s = dict(ate=((B, _lib.TRAJ_ATE_STATS), np.float64), err=((B, cap), np.float64), centres=((B + 1, cap, 3), np.float64),
                 prefix=((B, 2, cap), np.float64))
        if K:
            s["rpe"] = ((B, K, _lib.TRAJ_RPE_STATS), np.float64)
        if L:
            s["seg"] = ((B, L + 1, _lib.TRAJ_SEG_STATS), np.float64)
            s["seg_end"] = ((B, self.slots, L), np.int32)
        if log and self.edge_capacity:
            s["clo"] = ((_lib.TRAJ_CLO_STATS,), np.float64)
            s["edge_err"] = ((self.edge_capacity, 2), np.float64)
        return s

    @staticmethod
    def ate_stats(ate) -> AteStats:
        """TrajEval.ate [B, 24] split into its named columns (views)."""
        return AteStats(ate[:, 0], ate[:, 1], ate[:, 2], ate[:, 3], ate[:, 4], ate[:, 5], ate[:, 6], ate[:, 7:16].reshape(-1, 3, 3), ate[:, 16:19],
                        ate[:, 19], ate[:, 20:23], ate[:, 23])

    def _t(self, who, name, t, dtype, numel, exact=True):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if (not t.is_cuda) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} of {'' if exact else 'at least '}{numel} elements on the "
                             "context's device")
        return t

    def _inputs(self, who, est, n, gt, valid, log):
        import torch
        cap = self.node_capacity
        self._t(who, "est", est, torch.float64, 12 * self.B * cap)
        self._t(who, "n", n, torch.int32, 1, exact=False)
        self._t(who, "gt", gt, torch.float64, self.gt_cols * cap)
        if valid is not None:
            self._t(who, "valid", valid, torch.bool if valid.dtype == torch.bool else torch.uint8, cap)
        rec = None
        if log is not None:
            if log.ctx is not self.ctx:
                raise ValueError(f"{who}: the closure log and the evaluation must share one context (one stream)")
            if self.edge_capacity < 1 or self.edge_capacity > log.edge_capacity:        # the rows [0, edge_capacity) of the log must exist
                raise ValueError(f"{who}: edge_capacity must lie between 1 and the log's edge_capacity")
            rec = _lib.PoseGraphBuffers(*(C.c_void_p(getattr(log, nm).data_ptr()) for nm in log.NAMES))
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return p(est), p(n), p(gt), p(valid), rec

    def run_torch(self, est, n, gt, valid=None, log=None, out: dict | None = None, optional=("err", "seg_end", "edge_err")) -> TrajEval:
        """Device form (pr_trajeval_run_dev).  n i32 [>= 1] whose word 0 is the row count (a KeyframeMap's .state); valid bool | u8
        [node_capacity] or None; log a PoseGraph whose logged closures are evaluated, or None.  out: a dict name -> preallocated tensor
        (shapes()); the statistics blocks are allocated when absent, the arrays named in `optional` too ("centres", "prefix" may be
        added), the others stay NULL.  Returns TrajEval.  Nothing synchronises; nothing is allocated when `out` holds every array wanted."""
        import torch
        who = "TrajectoryEval.run_torch"
        pe, pn, pg, pv, rec = self._inputs(who, est, n, gt, valid, log)
        dev = torch.device("cuda", self.ctx.device)
        out = dict(out or {})
        got = {}
        for name, (shape, dt) in self.shapes(log is not None).items():
            tdt = torch.int32 if dt == np.int32 else torch.float64
            if name in out:
                got[name] = self._t(who, name, out[name], tdt, int(np.prod(shape)))
            elif name in ("ate", "rpe", "seg", "clo") or name in optional:
                got[name] = torch.empty(shape, dtype=tdt, device=dev)
        o = _lib.TrajEvalOut(*(C.c_void_p(got[nm].data_ptr()) if nm in got else None for nm in self.NAMES))
        self.ctx.check(self.lib.pr_trajeval_run_dev(self.h, pe, pn, pg, pv, C.byref(rec) if rec is not None else None, C.byref(o)))
        return TrajEval(*(got.get(nm) for nm in self.NAMES))

    def run_map(self, km, gt, poses=None, **kw) -> TrajEval:
        """run_torch for a KeyframeMap: its .state as the count and its .poses - or `poses` [node_capacity, 12], e.g. the out of
        PoseGraph.relax_torch - as the estimate (B = 1).  The map must live on this handle's context."""
        if km.ctx is not self.ctx:
            raise ValueError("TrajectoryEval.run_map: the evaluation and the map must share one context (one stream)")
        if km.keyframe_capacity != self.node_capacity or self.B != 1:
            raise ValueError("TrajectoryEval.run_map: node_capacity must equal the map's keyframe_capacity and B must be 1")
        return self.run_torch(km.poses if poses is None else poses, km.state, gt, **kw)

    def run(self, est, n, gt, valid=None, log=None, optional=("err", "seg_end", "edge_err", "centres", "prefix")) -> TrajEval:
        """Host form (pr_trajeval_run; synchronises): inputs as for run_torch (device tensors); returns TrajEval of NumPy arrays."""
        who = "TrajectoryEval.run"
        pe, pn, pg, pv, rec = self._inputs(who, est, n, gt, valid, log)
        got = {name: np.empty(shape, dt) for name, (shape, dt) in self.shapes(log is not None).items()
               if name in ("ate", "rpe", "seg", "clo") or name in optional}
        o = _lib.TrajEvalOut(*(_ptr(got[nm]) if nm in got else None for nm in self.NAMES))
        self.ctx.check(self.lib.pr_trajeval_run(self.h, pe, pn, pg, pv, C.byref(rec) if rec is not None else None, C.byref(o)))
        return TrajEval(*(got.get(nm) for nm in self.NAMES))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_trajeval_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Proximity(NamedTuple):
    """The outputs of a ProximitySearch search: idx i32, d2 f64 [query_capacity, k]; T0 f64 [query_capacity k, 3, 4]; pair_src, pair_dst
    i32 and known u8 [query_capacity k]; info i32 [4] = rows searched, slots filled, slots known, flags."""
    idx: object
    d2: object
    T0: object
    pair_src: object
    pair_dst: object
    known: object
    info: object


class ProximitySearch:
    """pr_proximity: loop-closure candidates from the poses - for every query row q0 + r the earlier keyframes within
    radius + growth x (path between the rows), capped at radius_max, that look the same way (cos_min), one per bucket of `stride` rows,
    the k nearest - with the seeds and pair lists of verify_map_torch and PoseGraph.add_batch_torch.  Calls are enqueued on the context's
    stream, read n, qrange and the log's count on the device and allocate no device scratch: ONE captured search_torch serves every
    count and every query range.  The rule is in include/place_recognition.h."""

    def __init__(self, ctx: Context | None, node_capacity: int, query_capacity: int, k_max: int):
        self.h = None
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.node_capacity, self.query_capacity, self.k_max = int(node_capacity), int(query_capacity), int(k_max)
        self.last_verify = None
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_proximity_create(self.ctx.h, self.node_capacity, self.query_capacity, self.k_max, C.byref(h)))
        self.h = h

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_proximity_scratch_bytes(self.node_capacity, self.query_capacity, self.k_max))

    @staticmethod
    def tile():
        """(rows, cols) of the search kernel's tile (pr_proximity_tile)."""
        r, c = C.c_int32(), C.c_int32()
        _lib.load().pr_proximity_tile(C.byref(r), C.byref(c))
        return int(r.value), int(c.value)

    def _t(self, who, name, t, dtype, numel, exact=True):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if (not t.is_cuda) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} of {'' if exact else 'at least '}{numel} elements on the "
                             "context's device")
        return t

    def shapes(self, k: int):
        Q = self.query_capacity
        return dict(idx=((Q, k), np.int32), d2=((Q, k), np.float64), T0=((Q * k, 3, 4), np.float64), pair_src=((Q * k,), np.int32),
                    pair_dst=((Q * k,), np.int32), known=((Q * k,), np.uint8), info=((4,), np.int32))

    def _args(self, who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window):
        import torch
        self._t(who, "poses", poses, torch.float64, 12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, 1, exact=False)
        self._t(who, "qrange", qrange, torch.int32, 2)
        k = int(k)
        if k < 1 or k > self.k_max:
            raise ValueError(f"{who}: k must lie in 1 .. k_max")
        rec, ec = None, 0
        if log is not None:
            if log.ctx is not self.ctx:
                raise ValueError(f"{who}: the closure log and the search must share one context (one stream)")
            rec = _lib.PoseGraphBuffers(*(C.c_void_p(getattr(log, nm).data_ptr()) for nm in log.NAMES))
            ec = log.edge_capacity
        prm = _lib.ProximityParams(float(radius), float(growth), float(radius if radius_max is None else radius_max), float(cos_min), int(min_gap),
                                   int(stride), k, int(known_window))
        return k, prm, rec, ec

    def search_torch(self, poses, n, qrange, *, radius, growth=0.0, radius_max=None, cos_min=-1.0, min_gap, stride=1, k=1, log=None,
                     known_window=0, out=None) -> Proximity:
        """Device form (pr_proximity_search_dev): poses f64 [node_capacity, 12] and n i32 [>= 1] - a KeyframeMap's .poses and .state - and
        qrange i32 [2] = (q0, mq): output row r stands for query row q0 + r, r < mq.  radius_max None: radius.  log: a PoseGraph whose
        logged pairs (within known_window rows at both ends) come back known = 1 and switched off.  out: the Proximity an earlier call
        returned for the same k (fixed addresses: what a captured graph needs).  Nothing synchronises; nothing is allocated with out=."""
        import torch
        who = "ProximitySearch.search_torch"
        k, prm, rec, ec = self._args(who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window)
        dev = torch.device("cuda", self.ctx.device)
        got = {}
        for name, (shape, dt) in self.shapes(k).items():
            tdt = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}[dt]
            if out is not None:
                got[name] = self._t(who, name, getattr(out, name), tdt, int(np.prod(shape)))
            else:
                got[name] = torch.empty(shape, dtype=tdt, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_proximity_search_dev(self.h, p(poses), p(n), p(qrange), C.byref(prm), C.byref(rec) if rec is not None else None,
                                                        ec, *(p(got[nm]) for nm in Proximity._fields)))
        return Proximity(*(got[nm] for nm in Proximity._fields))

    def _map(self, who, km):
        if km.ctx is not self.ctx:
            raise ValueError(f"{who}: the search and the map must share one context (one stream)")
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError(f"{who}: node_capacity must equal the map's keyframe_capacity")

    def search_map(self, km, qrange, **kw) -> Proximity:
        """search_torch(km.poses, km.state, qrange, ...) for a KeyframeMap on this handle's context with node_capacity keyframes; anything
        else is refused before the library is called."""
        self._map("ProximitySearch.search_map", km)
        return self.search_torch(km.poses, km.state, qrange, **kw)

    def search(self, poses, n, qrange, *, radius, growth=0.0, radius_max=None, cos_min=-1.0, min_gap, stride=1, k=1, log=None,
               known_window=0) -> Proximity:
        """Host form (pr_proximity_search; synchronises): inputs as for search_torch (device tensors); returns Proximity of NumPy arrays."""
        who = "ProximitySearch.search"
        k, prm, rec, ec = self._args(who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window)
        got = {name: np.empty(shape, dt) for name, (shape, dt) in self.shapes(k).items()}
        p = lambda t: C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_proximity_search(self.h, p(poses), p(n), p(qrange), C.byref(prm), C.byref(rec) if rec is not None else None, ec,
                                                    *(_ptr(got[nm]) for nm in Proximity._fields)))
        return Proximity(*(got[nm] for nm in Proximity._fields))

    def verify_map_torch(self, km, cand: Proximity, max_src_pts: int, *, max_iter: int = 30, max_corr: float = 1.0, min_fitness: float = 0.5,
                         max_rmse: float = 0.5, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3, search=None, out=None):
        """The candidates of a search refined and judged on the stream: pr_icp_pairs_dev with the map's own CSR on BOTH sides (N =
        keyframe_capacity: cloud pair_src onto cloud pair_dst from T0; a slot switched off answers ICP_NO_PAIR), then
        pr_verify_select_dev with one hypothesis - verify's accept rule.  Returns (T f64 [c, 3, 4], stats u8 [c, 32], accepted bool [c]), c =
        query_capacity k: what PoseGraph.add_batch_torch(cand.pair_dst, cand.pair_src, T, accepted) logs.  out: the dict an earlier call
        left in .last_verify for the same c (fixed addresses for a capture)."""
        import torch
        who = "ProximitySearch.verify_map_torch"
        self._map(who, km)
        c = cand.pair_src.numel()
        dev = cand.pair_src.device
        if out is None:
            out = dict(refine=(torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev)),
                       T=torch.empty((c, 3, 4), dtype=torch.float64, device=dev), stats=torch.empty((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev),
                       accepted=torch.empty(c, dtype=torch.bool, device=dev), hyp=torch.empty(c, dtype=torch.int32, device=dev))
            torch.cuda.synchronize(dev)                   # torch's fill (its stream) before the library's stream writes the buffers
        elif out["T"].shape != (c, 3, 4):
            raise ValueError(f"{who}: out belongs to another c")
        p = lambda t: C.c_void_p(t.data_ptr())
        N = km.keyframe_capacity
        with icp_search(self.ctx, search):
            self.ctx.check(self.lib.pr_icp_pairs_dev(self.ctx.h, p(km.xyz), p(km.offs), N, p(km.xyz), p(km.offs), N, p(cand.pair_src), p(cand.pair_dst),
                                                     c, p(cand.T0), int(max_src_pts), int(km.max_cloud_points), int(max_iter), float(max_corr),
                                                     float(tol_rmse), float(tol_fitness), int(min_inliers), p(out["refine"][0]), p(out["refine"][1])))
        self.ctx.check(self.lib.pr_verify_select_dev(self.ctx.h, p(out["refine"][0]), p(out["refine"][1]), c, 1, float(min_fitness), float(max_rmse),
                                                     p(out["T"]), p(out["stats"]), p(out["accepted"]), p(out["hyp"])))
        self.last_verify = out
        return out["T"], out["stats"], out["accepted"]

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_proximity_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Submaps(NamedTuple):
    """The outputs of a SubmapBuilder build: a CSR set of slot_capacity clouds - xyz f64 [point_capacity, 3] (rows at or behind
    offs[c] are not written), offs i64 [slot_capacity + 1] - with rows i32 [slot_capacity, 2] = rows taken, flags and info i32 [4] =
    slots non-empty, points written (low word, high word), flags OR-ed."""
    xyz: object
    offs: object
    rows: object
    info: object


class SubmapBuilder:
    """pr_submap: local submaps - for every slot the clouds of the map rows centre - w .. centre + w gathered into ONE
    cloud in the centre row's camera frame, with the poses the map holds or relaxed ones; a CSR set icp_refine_torch reads as it stands.
    Calls are enqueued on the context's stream, read the map's count on the device and allocate no device scratch: ONE captured
    build_torch serves every count.  keyframe_capacity and max_cloud_points are the map's.  buffers: dict of xyz, offs, rows, info
    (the shapes of Submaps) to build into by default; otherwise allocated here.  The rule is in include/place_recognition.h."""

    NAMES = Submaps._fields

    def __init__(self, ctx: Context | None, slot_capacity: int, w_max: int, point_capacity: int, max_cloud_points: int,
                 keyframe_capacity: int | None = None, buffers: dict | None = None):
        """keyframe_capacity None: the handle is created by the first call that names a map, with that map's keyframe_capacity (an
        eager call in front of a capture, as every capture here has)."""
        self.h = None
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.slot_capacity, self.w_max, self.point_capacity = int(slot_capacity), int(w_max), int(point_capacity)
        self.max_cloud_points, self.keyframe_capacity = int(max_cloud_points), None
        self.last_pair = None
        if keyframe_capacity is not None:
            self._create(int(keyframe_capacity))
        self.out = self.new_out() if buffers is None else self._out("SubmapBuilder", Submaps(*(buffers[n] for n in self.NAMES)))
        import torch
        self.identity = torch.arange(self.slot_capacity, dtype=torch.int32, device=torch.device("cuda", self.ctx.device))
        torch.cuda.synchronize(self.identity.device)      # torch's fills (its stream) before the library's stream reads the buffers

    def _create(self, keyframe_capacity: int):
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_submap_create(self.ctx.h, self.slot_capacity, self.w_max, self.point_capacity, self.max_cloud_points,
                                                 keyframe_capacity, C.byref(h)))
        self.h, self.keyframe_capacity = h, keyframe_capacity

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_submap_scratch_bytes(self.slot_capacity, self.w_max))

    def shapes(self):
        S = self.slot_capacity
        return dict(xyz=((self.point_capacity, 3), np.float64), offs=((S + 1,), np.int64), rows=((S, 2), np.int32), info=((4,), np.int32))

    def new_out(self) -> Submaps:
        """A fresh set of output tensors (zeroed) on the context's device."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        tdt = {np.int32: torch.int32, np.float64: torch.float64, np.int64: torch.int64}
        return Submaps(*(torch.zeros(s, dtype=tdt[dt], device=dev) for s, dt in self.shapes().values()))

    def _t(self, who, name, t, dtype, numel, exact=True):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if (not t.is_cuda) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or (t.numel() != numel if exact else t.numel() < numel):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} of {'' if exact else 'at least '}{numel} elements on the "
                             "context's device")
        return t

    def _out(self, who, out: Submaps) -> Submaps:
        import torch
        tdt = {np.int32: torch.int32, np.float64: torch.float64, np.int64: torch.int64}
        for name, (shape, dt) in self.shapes().items():
            self._t(who, name, getattr(out, name), tdt[dt], int(np.prod(shape)))
        return out

    def _map(self, who, km):
        if km.ctx is not self.ctx:
            raise ValueError(f"{who}: the builder and the map must share one context (one stream)")
        if self.keyframe_capacity is None:
            self._create(int(km.keyframe_capacity))
        if km.keyframe_capacity != self.keyframe_capacity:
            raise ValueError(f"{who}: keyframe_capacity must equal the map's")

    def _params(self, who, c, w, past_only, avoid_gap, max_pts):
        if c < 0 or c > self.slot_capacity:
            raise ValueError(f"{who}: the centre list must hold 0 .. slot_capacity rows")
        w = int(w)
        if w < 0 or w > self.w_max:
            raise ValueError(f"{who}: w must lie in 0 .. w_max")
        return _lib.SubmapParams(w, 1 if past_only else 0, int(avoid_gap),
                                 int(min(self.point_capacity, 2 ** 31 - 1) if max_pts is None else max_pts))

    def build_torch(self, km, centers, avoid=None, poses=None, n=None, *, w: int, past_only: bool = False, avoid_gap: int = 0, max_pts=None,
                    out: Submaps | None = None) -> Submaps:
        """Device form (pr_submap_build_dev): km a KeyframeMap on this builder's context, centers i32 [c] the slots' centre rows (negative:
        the slot is switched off), avoid i32 [c] | None - rows within avoid_gap of avoid[p] stay out of slot p (the other end of the pair),
        poses f64 [>= keyframe_capacity, 12] | None (the map's own; or PoseGraph.relax_torch's out), n i32 [>= 1] | None (the map's state).
        max_pts: the most points of one submap (default point_capacity) - what icp_refine_torch takes as max_src_pts / max_dst_pts.
        out: the Submaps to write (default: the builder's own; fixed addresses are what a captured graph needs).  Nothing synchronises,
        nothing is allocated."""
        import torch
        who = "SubmapBuilder.build_torch"
        self._map(who, km)
        c = centers.numel()
        prm = self._params(who, c, w, past_only, avoid_gap, max_pts)
        self._t(who, "centers", centers, torch.int32, c)
        if avoid is not None:
            self._t(who, "avoid", avoid, torch.int32, c)
        poses = km.poses if poses is None else self._t(who, "poses", poses, torch.float64, 12 * self.keyframe_capacity, exact=False)
        n = km.state if n is None else self._t(who, "n", n, torch.int32, 1, exact=False)
        out = self.out if out is None else self._out(who, out)
        rec = _lib.MapBuffers(*(C.c_void_p(getattr(km, nm).data_ptr()) for nm in km.NAMES))
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_submap_build_dev(self.h, C.byref(rec), p(poses), p(n), p(centers), p(avoid), c, C.byref(prm), p(out.xyz), p(out.offs),
                                                    p(out.rows), p(out.info)))
        return out

    def build(self, km, centers, avoid=None, poses=None, n=None, *, w: int, past_only: bool = False, avoid_gap: int = 0, max_pts=None) -> Submaps:
        """Host form (pr_submap_build; synchronises): centers / avoid are NumPy arrays, the map, poses and n stay device memory.  Returns
        Submaps of NumPy arrays; xyz holds the offs[c] rows that were written."""
        who = "SubmapBuilder.build"
        self._map(who, km)
        cen = np.ascontiguousarray(centers, np.int32).reshape(-1)
        c = len(cen)
        av = None if avoid is None else np.ascontiguousarray(avoid, np.int32).reshape(-1)
        if av is not None and len(av) != c:
            raise ValueError(f"{who}: centers [c] and avoid [c] disagree")
        prm = self._params(who, c, w, past_only, avoid_gap, max_pts)
        got = {name: np.empty(shape, dt) for name, (shape, dt) in self.shapes().items()}
        poses = km.poses if poses is None else poses
        n = km.state if n is None else n
        rec = _lib.MapBuffers(*(C.c_void_p(getattr(km, nm).data_ptr()) for nm in km.NAMES))
        self.ctx.check(self.lib.pr_submap_build(self.h, C.byref(rec), C.c_void_p(poses.data_ptr()), C.c_void_p(n.data_ptr()), _ptr(cen), _ptr(av), c,
                                                C.byref(prm), *(_ptr(got[nm]) for nm in self.NAMES)))
        got["xyz"] = got["xyz"][:int(got["offs"][c])]
        return Submaps(*(got[nm] for nm in self.NAMES))

    def pair_torch(self, km, idx_db, idx_q, poses=None, n=None, *, w: int, avoid_gap: int = 0, max_pts=None, out=None):
        """Both sides of a pair list in two builds: the DB side centred on idx_db avoiding idx_q, the query side centred on idx_q avoiding
        idx_db with past_only (online the query has no future).  idx_db, idx_q i32 [c] - a ProximitySearch's pair_dst and pair_src.  Returns
        (db: Submaps, q: Submaps, pair_src i32 [c], pair_dst i32 [c]) with identity pair lists, so that
        icp_refine_torch(q.xyz, q.offs, db.xyz, db.offs, pair_src, pair_dst, T0, max_pts, max_pts) runs on them unchanged (a slot switched
        off holds two empty clouds: ICP_TOO_FEW).  out: the (db, q) pair an earlier call returned - kept in .last_pair - for a capture."""
        if out is None:
            out = (self.out, self.new_out())
            import torch
            torch.cuda.synchronize(self.identity.device)
        c = idx_db.numel()
        db = self.build_torch(km, idx_db, idx_q, poses, n, w=w, past_only=False, avoid_gap=avoid_gap, max_pts=max_pts, out=out[0])
        q = self.build_torch(km, idx_q, idx_db, poses, n, w=w, past_only=True, avoid_gap=avoid_gap, max_pts=max_pts, out=out[1])
        self.last_pair = (db, q)
        return db, q, self.identity[:c], self.identity[:c]

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_submap_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SequenceFilter:
    """pr_seqmatch: the online form of the sequence matcher - a ring of the last L fused score rows of a drive.  Every
    keyframe, push_torch takes the distance rows an OnlineDatabase / OnlineSet match wrote (rows=) and the database's .state, fuses them
    into one row (the row z-scores weighted, or the one row as it is with normalize=False), stores it and returns the k rows whose
    scores summed along the step table's trajectories over the earlier pushed rows are smallest.  steps: api.seq_steps(L, velocities).
    Calls are enqueued on the context's stream, read the count on the device and allocate nothing; ONE captured push_torch serves every
    keyframe (the weights' values are part of the capture)."""

    def __init__(self, ctx: Context | None, capacity: int, channels: int, steps, max_k: int = 8):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.h = None
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
        if (not rows.is_cuda) or rows.dtype != torch.float64 or not rows.is_contiguous() or rows.numel() != self.channels * self.capacity:
            raise ValueError(f"{who}: rows must be a contiguous CUDA tensor f64 [{self.channels}, {self.capacity}]")
        for name, t in (("state", state), ("emitted", emitted)):
            if t is not None and ((not t.is_cuda) or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < 1):
                raise ValueError(f"{who}: {name} must be a CUDA tensor i32 [>= 1]")
        w = self._weights(weights, who)
        dev = rows.device
        if out is None:
            out = (torch.empty((1, max(k, 0)), dtype=torch.int32, device=dev), torch.empty((1, max(k, 0)), dtype=torch.float64, device=dev),
                   torch.empty((1, max(k, 0)), dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev))
        elif len(out) != 4 or any(tuple(t.shape) != (1, k) or not t.is_cuda or not t.is_contiguous() for t in out[:3]) or out[3].numel() != 4 \
                or [t.dtype for t in out] != [torch.int32, torch.float64, torch.int32, torch.int32] or not out[3].is_cuda:
            raise ValueError(f"{who}: out must be (idx i32 [1, k], score f64 [1, k], vel i32 [1, k], info i32 [4]) CUDA tensors")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_seqmatch_push_dev(self.h, p(rows), p(state), p(emitted), _ptr(w), int(bool(normalize)), int(mask_width), k,
                                                     p(out[0]), p(out[1]), p(out[2]), p(out[3])))
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

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_seqmatch_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WorldMap:
    """pr_worldmap: all clouds of a KeyframeMap fused into ONE world-frame point set, one point per occupied voxel, under any pose array -
    the map's own or the ones PoseGraph.relax_map returns.  The six buffers are zeroed torch tensors on the context's
    device (or the caller's: buffers = dict of the six names): .xyz [out_capacity, 3] f64, .inten [out_capacity] f32, .src [out_capacity]
    i64 (the point's index in the map), .row [out_capacity] i32 (its keyframe row), .count [out_capacity] i32 (the points of its voxel)
    and .state [4] i32 = rows written, flags, 0, 0.  A fuse is a full rebuild by launches whose geometry depends on the create capacities
    only and both counts are read on the device, so ONE captured fuse_torch serves every count; its bytes are a function of its inputs
    alone.  All scratch is allocated here; the world map must be closed before its map."""

    NAMES = ("xyz", "inten", "src", "row", "count", "state")
    KEEP = {"first": 0, "last": 1}

    def __init__(self, ctx: Context | None, km, out_capacity: int, buffers: dict | None = None):
        import torch
        self.ctx = ctx or default_context()
        self.h = None
        if km.ctx is not self.ctx:
            raise ValueError("WorldMap: the world map and the map must share one context (one stream)")
        self.lib = self.ctx.lib
        self.km = km
        self.out_capacity = int(out_capacity)
        oc = max(self.out_capacity, 0)
        dev = torch.device("cuda", self.ctx.device)
        shapes = dict(xyz=((oc, 3), torch.float64), inten=((oc,), torch.float32), src=((oc,), torch.int64), row=((oc,), torch.int32),
                      count=((oc,), torch.int32), state=((4,), torch.int32))
        if buffers is None:
            buffers = {n: torch.zeros(s, dtype=dt, device=dev) for n, (s, dt) in shapes.items()}
        for n, (s, dt) in shapes.items():
            t = buffers[n]
            if (not t.is_cuda) or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != tuple(s):
                raise ValueError(f"WorldMap: buffer {n} must be a contiguous CUDA tensor {dt} {list(s)}")
            setattr(self, n, t)
        torch.cuda.synchronize(dev)                       # torch's fills (its stream) before the library's stream writes the buffers
        rec = _lib.WorldMapBuffers(*(C.c_void_p(getattr(self, n).data_ptr()) for n in self.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_worldmap_create(self.ctx.h, km.h, C.byref(rec), self.out_capacity, C.byref(h)))
        self.h = h

    def _args(self, who, cell, min_count, keep):
        """the checks both forms share, made before the library is called; -> (cell, min_count, keep code)"""
        if keep not in self.KEEP:
            raise ValueError(f"{who}: keep is 'first' or 'last'")
        return float(cell), int(min_count), self.KEEP[keep]

    def fuse_torch(self, poses=None, n=None, cell: float = 0.2, min_count: int = 1, keep: str = "first", info=None):
        """Device form (pr_worldmap_fuse_dev): poses f64 [keyframe_capacity, 12] (world to camera; None = the map's own), n i32 [>= 1] whose
        word 0 is the keyframe count (None = the map's state), both contiguous CUDA tensors on the map's device.  cell: the voxel's edge;
        a voxel of fewer than min_count points is left out; keep = 'first' | 'last' picks a voxel's earliest or latest point.  Returns info
        (device i64 [4]) = rows written, voxels that qualified, valid points, flags (WORLDMAP_*); the rows are .xyz[:rows] ... Enqueued
        on the context's stream; nothing synchronises, nothing is allocated when info= is given."""
        import torch
        who = "WorldMap.fuse_torch"
        cell, min_count, kcode = self._args(who, cell, min_count, keep)
        dev = self.state.device
        if poses is not None and ((not poses.is_cuda) or poses.device != dev or poses.dtype != torch.float64 or not poses.is_contiguous()
                                  or tuple(poses.shape) != (self.km.keyframe_capacity, 12)):
            raise ValueError(f"{who}: poses must be a contiguous CUDA tensor f64 [keyframe_capacity, 12] on the map's device")
        if n is not None and ((not n.is_cuda) or n.device != dev or n.dtype != torch.int32 or not n.is_contiguous() or n.numel() < 1):
            raise ValueError(f"{who}: n must be a CUDA tensor i32 [>= 1] on the map's device")
        if info is None:
            info = torch.empty(4, dtype=torch.int64, device=dev)
        elif (not info.is_cuda) or info.device != dev or info.dtype != torch.int64 or not info.is_contiguous() or info.numel() != 4:
            raise ValueError(f"{who}: info must be a CUDA tensor i64 [4] on the map's device")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self.ctx.check(self.lib.pr_worldmap_fuse_dev(self.h, p(poses), p(n), cell, min_count, kcode, p(info)))
        return info

    def fuse(self, poses=None, n=None, cell: float = 0.2, min_count: int = 1, keep: str = "first"):
        """Host form (pr_worldmap_fuse; synchronises): poses a numpy array [keyframe_capacity, 12] or None, n an int or None.  Returns
        (xyz [rows, 3] f64, inten [rows] f32, src [rows] i64, row [rows] i32, count [rows] i32, info [4] i64) as numpy arrays."""
        who = "WorldMap.fuse"
        cell, min_count, kcode = self._args(who, cell, min_count, keep)
        po = None
        if poses is not None:
            po = np.ascontiguousarray(poses, np.float64)
            if po.shape != (self.km.keyframe_capacity, 12):
                raise ValueError(f"{who}: poses must be [keyframe_capacity, 12]")
        nn = None if n is None else np.array([int(n)], np.int32)
        oc = max(self.out_capacity, 0)
        xyz, inten = np.zeros((oc, 3), np.float64), np.zeros(oc, np.float32)
        src, row, count = np.zeros(oc, np.int64), np.zeros(oc, np.int32), np.zeros(oc, np.int32)
        info = np.zeros(4, np.int64)
        self.ctx.check(self.lib.pr_worldmap_fuse(self.h, _ptr(po), _ptr(nn), cell, min_count, kcode, _ptr(xyz), _ptr(inten), _ptr(src), _ptr(row),
                                                 _ptr(count), _ptr(info)))
        r = int(info[0])
        return xyz[:r], inten[:r], src[:r], row[:r], count[:r], info

    def rows(self):
        """The rows the last fuse wrote, as host arrays (xyz, inten, src, row, count); synchronises."""
        r, _ = self.count_rows()
        return tuple(getattr(self, n)[:r].cpu().numpy() for n in self.NAMES[:5])

    def write_ply(self, path: str, binary: bool = True) -> int:
        """The rows of the last fuse as a PLY file (vertex properties x, y, z double, intensity float, count int; binary little endian
        or ascii).  A debug aid: synchronises and copies to the host.  Returns the number of vertices."""
        xyz, inten, _, _, count = self.rows()
        r = len(inten)
        rec = np.empty(r, np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("intensity", "<f4"), ("count", "<i4")]))
        rec["x"], rec["y"], rec["z"], rec["intensity"], rec["count"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], inten, count
        head = ("ply\nformat %s 1.0\ncomment so_dso_place_recognition_amd world map\nelement vertex %d\nproperty double x\nproperty double y\n"
                "property double z\nproperty float intensity\nproperty int count\nend_header\n"
                % ("binary_little_endian" if binary else "ascii", r))
        with open(path, "wb") as f:
            f.write(head.encode("ascii"))
            if binary:
                f.write(rec.tobytes())
            else:
                for v in rec:
                    f.write(("%r %r %r %r %d\n" % (float(v["x"]), float(v["y"]), float(v["z"]), float(v["intensity"]), int(v["count"]))).encode("ascii"))
        return r

    def count_rows(self):
        """(rows written, flags) of the last fuse; synchronises (pr_worldmap_count)."""
        r, f = C.c_int64(), C.c_int32()
        self.ctx.check(self.lib.pr_worldmap_count(self.h, C.byref(r), C.byref(f)))
        return int(r.value), int(f.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_worldmap_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MapLocalizer:
    """pr_maploc: scan-to-map registration against a WorldMap's rows.  One voxel hash index per fuse, shared by every pair
    of a call; the correspondence search through it is exact within max_corr (which may not exceed cell / (1 + 2^-10)); the ICP update is
    pr_icp_pairs_dev's.  `cell` is fixed here and must be the cell the world map is fused with (a mismatch shows as MAPLOC_DUPLICATE in
    index's info).  Calls are enqueued on the context's stream, read their counts on the device and allocate no device scratch: index_torch
    behind every fuse_torch, then seed_torch / refine_torch or localize_torch; all of them can be captured.  Close it before its world map."""

    def __init__(self, ctx: Context | None, wm, cell: float, pair_capacity: int, max_src_pts: int):
        self.ctx = ctx or default_context()
        self.h = None
        if wm.ctx is not self.ctx:
            raise ValueError("MapLocalizer: the localiser and the world map must share one context (one stream)")
        self.lib = self.ctx.lib
        self.wm = wm
        self.cell, self.pair_capacity, self.max_src_pts = float(cell), int(pair_capacity), int(max_src_pts)
        rec = _lib.WorldMapBuffers(*(C.c_void_p(getattr(wm, n).data_ptr()) for n in wm.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_maploc_create(self.ctx.h, C.byref(rec), wm.out_capacity, self.cell, self.pair_capacity, self.max_src_pts,
                                                 C.byref(h)))
        self.h = h

    # ---- checks made before the library is called
    def _t(self, who, name, t, dtype, shape=None, numel_min=None):
        dev = self.wm.state.device
        if (not t.is_cuda) or t.device != dev or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} on the world map's device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} must be {list(shape)}")
        if numel_min is not None and t.numel() < numel_min:
            raise ValueError(f"{who}: {name} must have at least {numel_min} elements")
        return t

    def _pairs(self, who, xyz_q, offs_q, pair_src, T, excl):
        import torch
        self._t(who, "xyz_q", xyz_q, torch.float64)
        self._t(who, "offs_q", offs_q, torch.int64, numel_min=1)
        self._t(who, "pair_src", pair_src, torch.int32)
        if xyz_q.dim() != 2 or xyz_q.shape[1] != 3 or offs_q.dim() != 1 or pair_src.dim() != 1:
            raise ValueError(f"{who}: xyz_q must be [*, 3], offs_q [Nq + 1] and pair_src [c]")
        c = pair_src.numel()
        if c > self.pair_capacity:
            raise ValueError(f"{who}: c={c} exceeds pair_capacity={self.pair_capacity}")
        self._t(who, "T", T, torch.float64, (c, 3, 4))
        if excl is not None:
            self._t(who, "excl", excl, torch.int32, (c, 2))
        return c

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def index_torch(self, info=None):
        """Device form (pr_maploc_index_dev): rebuilds the index from the world map's rows as they are on the stream; call it behind every
        fuse_torch.  Returns info (device i64 [4]) = rows indexed, rows read, flags (MAPLOC_*), 0."""
        import torch
        who = "MapLocalizer.index_torch"
        if info is None:
            info = torch.empty(4, dtype=torch.int64, device=self.wm.state.device)
        else:
            self._t(who, "info", info, torch.int64, (4,))
        self.ctx.check(self.lib.pr_maploc_index_dev(self.h, self._p(info)))
        return info

    def seed_torch(self, poses, n, idx, accepted=None, T_rel=None, src=None, out=None):
        """Device form (pr_maploc_seed_dev): poses f64 [keyframe_capacity, 12] (world to camera: KeyframeMap.poses or the relaxed ones), n
        i32 [>= 1] (KeyframeMap.state), idx i32 [c] map rows (a verify's idx, flattened, as it is), accepted bool / u8 [c] or None, T_rel
        f64 [c, 3, 4] or None (a verify's T: query camera into row idx's camera), src i32 [c] or None (the pair's query cloud; None: p).
        Returns (T0 f64 [c, 3, 4] mapping the query cloud into the world, pair_src i32 [c]; -1 and the identity where a pair is off)."""
        import torch
        who = "MapLocalizer.seed_torch"
        self._t(who, "poses", poses, torch.float64)
        if poses.dim() != 2 or poses.shape[1] != 12 or poses.shape[0] < 1:
            raise ValueError(f"{who}: poses must be [keyframe_capacity, 12]")
        self._t(who, "n", n, torch.int32, numel_min=1)
        idx = idx.reshape(-1) if idx.is_contiguous() else idx
        self._t(who, "idx", idx, torch.int32)
        c = idx.numel()
        if c > self.pair_capacity:
            raise ValueError(f"{who}: c={c} exceeds pair_capacity={self.pair_capacity}")
        if accepted is not None:
            accepted = accepted.reshape(-1) if accepted.is_contiguous() else accepted
            if accepted.dtype == torch.bool:
                accepted = accepted.view(torch.uint8)
            self._t(who, "accepted", accepted, torch.uint8, (c,))
        if T_rel is not None:
            T_rel = T_rel.reshape(-1, 3, 4) if T_rel.is_contiguous() else T_rel
            self._t(who, "T_rel", T_rel, torch.float64, (c, 3, 4))
        if src is not None:
            self._t(who, "src", src, torch.int32, (c,))
        dev = self.wm.state.device
        if out is None:
            out = (torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.empty(c, dtype=torch.int32, device=dev))
        else:
            self._t(who, "out[0]", out[0], torch.float64, (c, 3, 4))
            self._t(who, "out[1]", out[1], torch.int32, (c,))
        p = self._p
        self.ctx.check(self.lib.pr_maploc_seed_dev(self.h, p(poses), p(n), poses.shape[0], p(idx), p(accepted), p(T_rel), p(src), c, p(out[0]),
                                                   p(out[1])))
        return out

    def nn_torch(self, xyz_q, offs_q, pair_src, T, excl=None, max_corr: float = 0.9, out=None):
        """Device form (pr_maploc_nn_dev): one correspondence pass of the clouds (xyz_q f64 [*, 3], offs_q i64 [Nq + 1]) of pair_src i32 [c]
        under T f64 [c, 3, 4]; excl i32 [c, 2] or None: world rows whose keyframe row lies in [lo, hi] are no candidates.  Returns
        (out_offs i64 [c + 1], nn_idx i32 [c * max(max_src_pts, 1)], nn_d2 f64 [same]): pair p's points are rows out_offs[p] ..
        out_offs[p + 1]; -1 / +Inf where no row lies within max_corr."""
        import torch
        who = "MapLocalizer.nn_torch"
        c = self._pairs(who, xyz_q, offs_q, pair_src, T, excl)
        dev = self.wm.state.device
        rows = c * max(self.max_src_pts, 1)
        if out is None:
            out = (torch.empty(c + 1, dtype=torch.int64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                   torch.empty(rows, dtype=torch.float64, device=dev))
        else:
            self._t(who, "out[0]", out[0], torch.int64, (c + 1,))
            self._t(who, "out[1]", out[1], torch.int32, (rows,))
            self._t(who, "out[2]", out[2], torch.float64, (rows,))
        p = self._p
        self.ctx.check(self.lib.pr_maploc_nn_dev(self.h, p(xyz_q), p(offs_q), offs_q.numel() - 1, p(pair_src), c, p(T), p(excl), float(max_corr),
                                                 p(out[0]), p(out[1]), p(out[2])))
        return out

    def refine_torch(self, xyz_q, offs_q, pair_src, T0, excl=None, max_iter: int = 30, max_corr: float = 0.9, tol_rmse: float = 1e-6,
                     tol_fitness: float = 1e-6, min_inliers: int = 3, out=None):
        """Device form (pr_maploc_refine_dev): point-to-point ICP of every pair from its seed T0 f64 [c, 3, 4] against the world rows.
        Returns (T f64 [c, 3, 4], stats u8 [c, 32] - ICP_STATS on the host); out: the pair an earlier call returned for the same c, written
        again (fixed addresses: what a captured graph needs); out[0] may be T0."""
        import torch
        who = "MapLocalizer.refine_torch"
        c = self._pairs(who, xyz_q, offs_q, pair_src, T0, excl)
        dev = self.wm.state.device
        if out is None:
            out = (torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev))
        else:
            self._t(who, "out[0]", out[0], torch.float64, (c, 3, 4))
            self._t(who, "out[1]", out[1], torch.uint8, (c, ICP_STATS.itemsize))
        p = self._p
        self.ctx.check(self.lib.pr_maploc_refine_dev(self.h, p(xyz_q), p(offs_q), offs_q.numel() - 1, p(pair_src), c, p(T0), p(excl), int(max_iter),
                                                     float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), p(out[0]),
                                                     p(out[1])))
        return out

    def localize_torch(self, xyz_q, offs_q, poses, n, idx, accepted=None, T_rel=None, src=None, excl=None, max_iter: int = 30,
                       max_corr: float = 0.9, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3, min_fitness: float = 0.5,
                       max_rmse: float = 0.5, out=None):
        """seed_torch -> refine_torch -> pr_verify_select_dev with one hypothesis, all on the context's stream without read-back.  Returns
        (T f64 [c, 3, 4] query cloud into the world, stats u8 [c, 32], accepted bool [c] = converged or max_iter, fitness >= min_fitness
        and rmse <= max_rmse).  out: the dict an earlier call left in .last_localize for the same c (fixed addresses for a capture)."""
        import torch
        who = "MapLocalizer.localize_torch"
        c = idx.numel()
        dev = self.wm.state.device
        if out is None:
            out = dict(seed=None, refine=None, T=torch.empty((c, 3, 4), dtype=torch.float64, device=dev),
                       stats=torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev),
                       accepted=torch.zeros(c, dtype=torch.bool, device=dev), hyp=torch.zeros(c, dtype=torch.int32, device=dev))
        elif out["T"].shape != (c, 3, 4):
            raise ValueError(f"{who}: out belongs to another c")
        out["seed"] = self.seed_torch(poses, n, idx, accepted, T_rel, src, out=out["seed"])
        T0, pair_src = out["seed"]
        out["refine"] = self.refine_torch(xyz_q, offs_q, pair_src, T0, excl, max_iter, max_corr, tol_rmse, tol_fitness, min_inliers, out=out["refine"])
        p = self._p
        self.ctx.check(self.lib.pr_verify_select_dev(self.ctx.h, p(out["refine"][0]), p(out["refine"][1]), c, 1, float(min_fitness), float(max_rmse),
                                                     p(out["T"]), p(out["stats"]), p(out["accepted"]), p(out["hyp"])))
        self.last_localize = out
        return out["T"], out["stats"], out["accepted"]

    # ---- host forms (synchronise)
    def index(self):
        """Host form (pr_maploc_index): info i64 [4] as a numpy array."""
        info = np.zeros(4, np.int64)
        self.ctx.check(self.lib.pr_maploc_index(self.h, _ptr(info)))
        return info

    def _host_pairs(self, who, xyz_q, offs_q, pair_src, T, excl):
        xq = np.ascontiguousarray(xyz_q, np.float64).reshape(-1, 3); oq = np.ascontiguousarray(offs_q, np.int64).reshape(-1)
        ps = np.ascontiguousarray(pair_src, np.int32).reshape(-1)
        if len(oq) < 1 or oq[-1] != len(xq):
            raise ValueError(f"{who}: the clouds are a CSR set: xyz [offs[-1], 3] and offs [Nq + 1]")
        c = len(ps)
        T = np.ascontiguousarray(T, np.float64)
        if T.size != 12 * c:
            raise ValueError(f"{who}: T must be [c, 3, 4]")
        ex = None
        if excl is not None:
            ex = np.ascontiguousarray(excl, np.int32)
            if ex.shape != (c, 2):
                raise ValueError(f"{who}: excl must be [c, 2]")
        return xq, oq, ps, c, T.reshape(c, 3, 4), ex

    def nn(self, xyz_q, offs_q, pair_src, T, excl=None, max_corr: float = 0.9):
        """Host form (pr_maploc_nn) over numpy arrays: (out_offs i64 [c + 1], nn_idx i32 [out_offs[-1]], nn_d2 f64 [same])."""
        xq, oq, ps, c, T, ex = self._host_pairs("MapLocalizer.nn", xyz_q, offs_q, pair_src, T, excl)
        Nq = len(oq) - 1
        total = int(sum(min(int(oq[s + 1] - oq[s]), self.max_src_pts) for s in ps if 0 <= s < Nq))
        out_offs = np.zeros(c + 1, np.int64); idx = np.empty(total, np.int32); d2 = np.empty(total, np.float64)
        self.ctx.check(self.lib.pr_maploc_nn(self.h, _ptr(xq), _ptr(oq), Nq, _ptr(ps), c, _ptr(T), _ptr(ex), float(max_corr), _ptr(out_offs),
                                             _ptr(idx), _ptr(d2)))
        return out_offs, idx, d2

    def refine(self, xyz_q, offs_q, pair_src, T0, excl=None, max_iter: int = 30, max_corr: float = 0.9, tol_rmse: float = 1e-6,
               tol_fitness: float = 1e-6, min_inliers: int = 3):
        """Host form (pr_maploc_refine) over numpy arrays: (T f64 [c, 3, 4], stats [c] of dtype ICP_STATS)."""
        xq, oq, ps, c, T0, ex = self._host_pairs("MapLocalizer.refine", xyz_q, offs_q, pair_src, T0, excl)
        T = np.empty((c, 3, 4)); stats = np.zeros(c, ICP_STATS)
        self.ctx.check(self.lib.pr_maploc_refine(self.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(ps), c, _ptr(T0), _ptr(ex), int(max_iter),
                                                 float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), _ptr(T), _ptr(stats)))
        return T, stats

    def count(self):
        """(rows indexed, flags) of the last index; synchronises (pr_maploc_count)."""
        r, f = C.c_int64(), C.c_int32()
        self.ctx.check(self.lib.pr_maploc_count(self.h, C.byref(r), C.byref(f)))
        return int(r.value), int(f.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_maploc_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlaneLocalizer:
    """pr_mapplane: point-to-plane scan-to-map registration over a MapLocalizer.  normals_torch estimates one normal per
    world row through the localiser's voxel index (call it behind index_torch); refine_torch is MapLocalizer.refine_torch with the plane
    metric - the same correspondence search, fitness and rmse, an update from the correspondents whose row has a normal.  It borrows the
    localiser's table and sizes and owns one allocation; every device call is enqueued on the context's stream, reads nothing back and can
    be captured.  Close it before its localiser."""

    def __init__(self, ctx: Context | None, ml):
        self.ctx = ctx or default_context()
        self.h = None
        if ml.ctx is not self.ctx:
            raise ValueError("PlaneLocalizer: the plane localiser and the localiser must share one context (one stream)")
        self.lib = self.ctx.lib
        self.ml = ml
        self.wm = ml.wm
        self.pair_capacity, self.max_src_pts = ml.pair_capacity, ml.max_src_pts
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_mapplane_create(self.ctx.h, ml.h, C.byref(h)))
        self.h = h

    _t = MapLocalizer._t
    _pairs = MapLocalizer._pairs
    _p = staticmethod(MapLocalizer._p)
    _host_pairs = MapLocalizer._host_pairs

    def _normals_args(self, who, normals, ninfo):
        import torch
        oc = self.wm.out_capacity
        self._t(who, "normals", normals, torch.float64, (oc, 3))
        self._t(who, "ninfo", ninfo, torch.int32, (oc,))

    def normals_torch(self, radius: float, min_nbrs: int = 5, max_ratio: float = 0.1, out=None):
        """Device form (pr_mapplane_normals_dev): (normals f64 [out_capacity, 3], ninfo i32 [out_capacity]) of the world rows as they are
        on the stream, through the last index.  ninfo > 0: a valid normal from that many neighbours (the row included) within `radius`;
        < 0: processed and invalid; 0: not an indexed row.  out: the pair an earlier call returned (fixed addresses for a capture)."""
        import torch
        who = "PlaneLocalizer.normals_torch"
        dev, oc = self.wm.state.device, self.wm.out_capacity
        if out is None:
            out = (torch.empty((oc, 3), dtype=torch.float64, device=dev), torch.empty(oc, dtype=torch.int32, device=dev))
        else:
            self._normals_args(who, out[0], out[1])
        p = self._p
        self.ctx.check(self.lib.pr_mapplane_normals_dev(self.h, float(radius), int(min_nbrs), float(max_ratio), p(out[0]), p(out[1])))
        return out

    def refine_torch(self, xyz_q, offs_q, pair_src, T0, normals, ninfo, excl=None, max_iter: int = 30, max_corr: float = 0.9,
                     tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 6, out=None):
        """Device form (pr_mapplane_refine_dev): point-to-plane ICP of every pair from its seed T0 f64 [c, 3, 4] against the world rows
        and their normals (normals_torch's pair).  Returns (T f64 [c, 3, 4], stats u8 [c, 32] - ICP_STATS on the host); out as for
        MapLocalizer.refine_torch; out[0] may be T0."""
        import torch
        who = "PlaneLocalizer.refine_torch"
        c = self._pairs(who, xyz_q, offs_q, pair_src, T0, excl)
        self._normals_args(who, normals, ninfo)
        dev = self.wm.state.device
        if out is None:
            out = (torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev))
        else:
            self._t(who, "out[0]", out[0], torch.float64, (c, 3, 4))
            self._t(who, "out[1]", out[1], torch.uint8, (c, ICP_STATS.itemsize))
        p = self._p
        self.ctx.check(self.lib.pr_mapplane_refine_dev(self.h, p(xyz_q), p(offs_q), offs_q.numel() - 1, p(pair_src), c, p(T0), p(excl),
                                                       int(max_iter), float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers),
                                                       p(normals), p(ninfo), p(out[0]), p(out[1])))
        return out

    def localize_torch(self, xyz_q, offs_q, poses, n, idx, normals, ninfo, accepted=None, T_rel=None, src=None, excl=None, max_iter: int = 30,
                       max_corr: float = 0.9, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 6,
                       min_fitness: float = 0.5, max_rmse: float = 0.5, out=None):
        """MapLocalizer.localize_torch with the plane metric: the localiser's seed_torch -> refine_torch -> pr_verify_select_dev with one
        hypothesis, on the context's stream without read-back.  Returns (T f64 [c, 3, 4], stats u8 [c, 32], accepted bool [c]); out: the
        dict an earlier call left in .last_localize for the same c."""
        import torch
        who = "PlaneLocalizer.localize_torch"
        c = idx.numel()
        dev = self.wm.state.device
        if out is None:
            out = dict(seed=None, refine=None, T=torch.empty((c, 3, 4), dtype=torch.float64, device=dev),
                       stats=torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev),
                       accepted=torch.zeros(c, dtype=torch.bool, device=dev), hyp=torch.zeros(c, dtype=torch.int32, device=dev))
        elif out["T"].shape != (c, 3, 4):
            raise ValueError(f"{who}: out belongs to another c")
        out["seed"] = self.ml.seed_torch(poses, n, idx, accepted, T_rel, src, out=out["seed"])
        T0, pair_src = out["seed"]
        out["refine"] = self.refine_torch(xyz_q, offs_q, pair_src, T0, normals, ninfo, excl, max_iter, max_corr, tol_rmse, tol_fitness,
                                          min_inliers, out=out["refine"])
        p = self._p
        self.ctx.check(self.lib.pr_verify_select_dev(self.ctx.h, p(out["refine"][0]), p(out["refine"][1]), c, 1, float(min_fitness), float(max_rmse),
                                                     p(out["T"]), p(out["stats"]), p(out["accepted"]), p(out["hyp"])))
        self.last_localize = out
        return out["T"], out["stats"], out["accepted"]

    # ---- host forms (synchronise)
    def normals(self, radius: float, min_nbrs: int = 5, max_ratio: float = 0.1):
        """Host form (pr_mapplane_normals): (normals f64 [out_capacity, 3], ninfo i32 [out_capacity]) as numpy arrays."""
        oc = self.wm.out_capacity
        nrm = np.zeros((oc, 3), np.float64); info = np.zeros(oc, np.int32)
        self.ctx.check(self.lib.pr_mapplane_normals(self.h, float(radius), int(min_nbrs), float(max_ratio), _ptr(nrm), _ptr(info)))
        return nrm, info

    def refine(self, xyz_q, offs_q, pair_src, T0, normals, ninfo, excl=None, max_iter: int = 30, max_corr: float = 0.9, tol_rmse: float = 1e-6,
               tol_fitness: float = 1e-6, min_inliers: int = 6):
        """Host form (pr_mapplane_refine) over numpy arrays: (T f64 [c, 3, 4], stats [c] of dtype ICP_STATS)."""
        who = "PlaneLocalizer.refine"
        xq, oq, ps, c, T0, ex = self._host_pairs(who, xyz_q, offs_q, pair_src, T0, excl)
        oc = self.wm.out_capacity
        nrm = np.ascontiguousarray(normals, np.float64); info = np.ascontiguousarray(ninfo, np.int32)
        if nrm.shape != (oc, 3) or info.shape != (oc,):
            raise ValueError(f"{who}: normals must be [out_capacity, 3] and ninfo [out_capacity]")
        T = np.empty((c, 3, 4)); stats = np.zeros(c, ICP_STATS)
        self.ctx.check(self.lib.pr_mapplane_refine(self.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(ps), c, _ptr(T0), _ptr(ex), int(max_iter),
                                                   float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), _ptr(nrm), _ptr(info),
                                                   _ptr(T), _ptr(stats)))
        return T, stats

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_mapplane_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegInfo(NamedTuple):
    """What a RegistrationInfo call returns, row p = slot p: H f64 [c, 6, 6] the normal matrix in the order (w0, w1, w2, v0, v1, v2), cov f64
    [c, 6, 6] its inverse, spec f64 [c, 16] = cr0 <= cr1 <= cr2, ct0 <= ct1 <= ct2 (the marginal covariance spectra), dir_r, dir_t (the
    weakest directions), SSE, s2, 0, 0; w f64 [c, 2] = (w_rot, w_trans), exactly 0 where a flag is set; stat i32 [c, 4] = n_inl, n_used,
    dof, flags (_lib.REGINFO_*); ok bool [c] = no flag."""
    H: object
    cov: object
    spec: object
    w: object
    stat: object
    ok: object


class RegistrationInfo:
    """pr_reginfo: how well the geometry constrains a registered pose.  Behind a correspondence pass at the pose T that is
    to be judged - icp_nn_radius / icp_nn (point metric) or MapLocalizer.nn_torch (plane metric) - it gives the normal matrix, its
    inverse, the marginal spectra of rotation and translation with their weakest directions, the flags (too few, singular, weak rotation,
    weak translation) and a per-slot (w_rot, w_trans) for PoseGraph.add_weighted_torch.  One allocation at create; every *_torch call is
    enqueued on the context's stream, reads nothing back and can be captured (out= keeps the result's addresses fixed).  pairs_torch and
    maploc_torch run the pass themselves into work tensors the first call for a given c allocates - make that call before a capture."""

    def __init__(self, ctx: Context | None, pair_capacity: int, max_src_pts: int):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.pair_capacity, self.max_src_pts = int(pair_capacity), int(max_src_pts)
        self.h = None
        self._work = {}
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_reginfo_create(self.ctx.h, self.pair_capacity, self.max_src_pts, C.byref(h)))
        self.h = h

    # ---- checks made before the library is called
    def _t(self, who, name, t, dtype, shape=None, numel_min=None):
        if (not t.is_cuda) or t.device.index != self.ctx.device or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} on the context's device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {name} must be {list(shape)}")
        if numel_min is not None and t.numel() < numel_min:
            raise ValueError(f"{who}: {name} must have at least {numel_min} elements")
        return t

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _args(self, who, xyz_q, offs_q, pair_src, T, accepted, nn):
        import torch
        self._t(who, "xyz_q", xyz_q, torch.float64)
        self._t(who, "offs_q", offs_q, torch.int64, numel_min=1)
        self._t(who, "pair_src", pair_src, torch.int32)
        if xyz_q.dim() != 2 or xyz_q.shape[1] != 3 or offs_q.dim() != 1 or pair_src.dim() != 1:
            raise ValueError(f"{who}: xyz_q must be [*, 3], offs_q [Nq + 1] and pair_src [c]")
        c = pair_src.numel()
        if c > self.pair_capacity:
            raise ValueError(f"{who}: c={c} exceeds pair_capacity={self.pair_capacity}")
        if T.numel() != 12 * c:
            raise ValueError(f"{who}: T must be [c, 3, 4]")
        self._t(who, "T", T, torch.float64)
        if accepted is not None:
            if accepted.dtype == torch.bool:
                accepted = accepted.view(torch.uint8)
            if accepted.numel() != c:
                raise ValueError(f"{who}: accepted must be [c]")
            self._t(who, "accepted", accepted, torch.uint8)
        if len(nn) != 3:
            raise ValueError(f"{who}: nn must be the triple (out_offs, nn_idx, nn_d2) of a correspondence pass")
        self._t(who, "nn[0]", nn[0], torch.int64, (c + 1,))
        self._t(who, "nn[1]", nn[1], torch.int32)
        self._t(who, "nn[2]", nn[2], torch.float64)
        if nn[1].numel() != nn[2].numel():
            raise ValueError(f"{who}: nn_idx and nn_d2 must have the same length")
        return c, accepted

    def _out(self, who, c, out):
        import torch
        if out is None:
            dev = torch.device("cuda", self.ctx.device)
            return RegInfo(torch.empty((c, 6, 6), dtype=torch.float64, device=dev), torch.empty((c, 6, 6), dtype=torch.float64, device=dev),
                           torch.empty((c, 16), dtype=torch.float64, device=dev), torch.empty((c, 2), dtype=torch.float64, device=dev),
                           torch.empty((c, 4), dtype=torch.int32, device=dev), torch.empty(c, dtype=torch.bool, device=dev))
        want = ((torch.float64, (c, 6, 6)), (torch.float64, (c, 6, 6)), (torch.float64, (c, 16)), (torch.float64, (c, 2)), (torch.int32, (c, 4)),
                (torch.bool, (c,)))
        if len(out) != 6:
            raise ValueError(f"{who}: out must be an earlier result")
        for name, t, (dt, sh) in zip(RegInfo._fields, out, want):
            self._t(who, f"out.{name}", t, dt, sh)
        return RegInfo(*out)

    def point_torch(self, xyz_q, offs_q, pair_src, T, nn, accepted=None, max_corr: float = 1.0, min_inliers: int = 10, min_ratio: float = 1e-4,
                    sigma_min: float = 0.01, w_max: float = 1e6, out=None):
        """Device form (pr_reginfo_point_dev): the clouds (xyz_q f64 [*, 3], offs_q i64 [Nq + 1]) of pair_src i32 [c] under T f64 [c, 3, 4],
        accepted bool / u8 [c] or None, nn = (out_offs i64 [c + 1], nn_idx i32, nn_d2 f64) of the pass at T.  Returns a RegInfo of device
        tensors; out: an earlier result for the same c, written again."""
        who = "RegistrationInfo.point_torch"
        c, accepted = self._args(who, xyz_q, offs_q, pair_src, T, accepted, nn)
        out = self._out(who, c, out)
        p = self._p
        self.ctx.check(self.lib.pr_reginfo_point_dev(self.h, p(xyz_q), p(offs_q), offs_q.numel() - 1, p(pair_src), c, p(T), p(accepted), p(nn[0]),
                                                     p(nn[1]), p(nn[2]), float(max_corr), int(min_inliers), float(min_ratio), float(sigma_min),
                                                     float(w_max), *(p(t) for t in out)))
        return out

    def plane_torch(self, xyz_q, offs_q, pair_src, T, nn, world_xyz, normals, ninfo, accepted=None, max_corr: float = 0.9, min_inliers: int = 10,
                    min_ratio: float = 1e-4, sigma_min: float = 0.01, w_max: float = 1e6, out=None):
        """Device form (pr_reginfo_plane_dev): point_torch's arguments with nn from MapLocalizer.nn_torch at T, plus world_xyz f64
        [out_capacity, 3] (WorldMap.xyz) and PlaneLocalizer.normals_torch's (normals f64 [out_capacity, 3], ninfo i32 [out_capacity])."""
        import torch
        who = "RegistrationInfo.plane_torch"
        c, accepted = self._args(who, xyz_q, offs_q, pair_src, T, accepted, nn)
        self._t(who, "world_xyz", world_xyz, torch.float64)
        if world_xyz.dim() != 2 or world_xyz.shape[1] != 3 or world_xyz.shape[0] < 1:
            raise ValueError(f"{who}: world_xyz must be [out_capacity, 3]")
        oc = world_xyz.shape[0]
        self._t(who, "normals", normals, torch.float64, (oc, 3))
        self._t(who, "ninfo", ninfo, torch.int32, (oc,))
        out = self._out(who, c, out)
        p = self._p
        self.ctx.check(self.lib.pr_reginfo_plane_dev(self.h, p(xyz_q), p(offs_q), offs_q.numel() - 1, p(pair_src), c, p(T), p(accepted), p(nn[0]),
                                                     p(nn[1]), p(nn[2]), p(world_xyz), oc, p(normals), p(ninfo), float(max_corr),
                                                     int(min_inliers), float(min_ratio), float(sigma_min), float(w_max), *(p(t) for t in out)))
        return out

    def pairs_torch(self, clouds_q, clouds_db, idx, T, accepted, max_src_pts: int, max_dst_pts: int, max_corr: float = 1.0, min_inliers: int = 10,
                    min_ratio: float = 1e-4, sigma_min: float = 0.01, w_max: float = 1e6, out=None):
        """The information of a verify's result: clouds_q = (xyz, offs) of the m queries, clouds_db = (xyz, offs) of the DB side or a
        KeyframeMap, idx i32 [m, k], T f64 [m, k, 3, 4] and accepted bool / u8 [m, k] as verify returns them.  pair_dst = where(accepted,
        idx, -1) on the device, then pr_icp_nn_radius_dev at T (the context's search mode), then point_torch with the same accepted;
        slot p = q k + j reads query cloud q.  Returns a RegInfo over c = m k slots; out as for point_torch."""
        import torch
        who = "RegistrationInfo.pairs_torch"
        if hasattr(clouds_db, "clouds"):
            if clouds_db.ctx is not self.ctx:
                raise ValueError(f"{who}: the map must live on this handle's context (one stream)")
            clouds_db = clouds_db.clouds
        xq, oq = clouds_q
        xd, od = clouds_db
        if idx.dim() != 2:
            raise ValueError(f"{who}: idx must be [m, k]")
        m, k = idx.shape
        c = m * k
        if c > self.pair_capacity:
            raise ValueError(f"{who}: c={c} exceeds pair_capacity={self.pair_capacity}")
        if int(max_src_pts) > self.max_src_pts:
            raise ValueError(f"{who}: max_src_pts={max_src_pts} exceeds the handle's {self.max_src_pts}")
        self._t(who, "idx", idx, torch.int32)
        self._t(who, "xyz_db", xd, torch.float64)
        self._t(who, "offs_db", od, torch.int64, numel_min=1)
        if accepted.dtype == torch.bool:
            accepted = accepted.view(torch.uint8)
        self._t(who, "accepted", accepted, torch.uint8, (m, k))
        dev = idx.device
        wk = self._work.get(("pairs", m, k))
        if wk is None:
            rows = c * max(self.max_src_pts, 1)
            wk = dict(src=torch.arange(m, dtype=torch.int32, device=dev).repeat_interleave(k).contiguous(),
                      dst=torch.empty(c, dtype=torch.int32, device=dev), minus1=torch.full((m, k), -1, dtype=torch.int32, device=dev),
                      nn=(torch.zeros(c + 1, dtype=torch.int64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                          torch.empty(rows, dtype=torch.float64, device=dev)))
            self._work[("pairs", m, k)] = wk
        torch.where(accepted != 0, idx, wk["minus1"], out=wk["dst"].view(m, k))
        Tc = T.reshape(c, 3, 4) if T.is_contiguous() else T
        self._t(who, "T", Tc, torch.float64, (c, 3, 4))
        self._t(who, "xyz_q", xq, torch.float64)
        self._t(who, "offs_q", oq, torch.int64, numel_min=1)
        p = self._p
        nn = wk["nn"]
        self.ctx.check(self.lib.pr_icp_nn_radius_dev(self.ctx.h, p(xq), p(oq), oq.numel() - 1, p(xd), p(od), od.numel() - 1, p(wk["src"]), p(wk["dst"]),
                                                     c, p(Tc), int(max_src_pts), int(max_dst_pts), float(max_corr), p(nn[0]), p(nn[1]), p(nn[2])))
        return self.point_torch(xq, oq, wk["src"], Tc, nn, accepted.reshape(c), max_corr, min_inliers, min_ratio, sigma_min, w_max, out=out)

    def maploc_torch(self, plane_localizer, xyz_q, offs_q, pair_src, T, normals, ninfo, accepted=None, excl=None, max_corr: float = 0.9,
                     min_inliers: int = 10, min_ratio: float = 1e-4, sigma_min: float = 0.01, w_max: float = 1e6, out=None):
        """The information of a scan-to-map result: pr_maploc_nn_dev at T through plane_localizer's localiser (its index, excl as there),
        then plane_torch against its world rows.  The localiser must live on this handle's context and have its pair_capacity and
        max_src_pts within this handle's."""
        who = "RegistrationInfo.maploc_torch"
        ml = plane_localizer.ml
        if plane_localizer.ctx is not self.ctx:
            raise ValueError(f"{who}: the plane localiser must live on this handle's context (one stream)")
        if ml.max_src_pts > self.max_src_pts:
            raise ValueError(f"{who}: the localiser's max_src_pts={ml.max_src_pts} exceeds the handle's {self.max_src_pts}")
        c = pair_src.numel()
        wk = self._work.get(("maploc", c))
        wk = ml.nn_torch(xyz_q, offs_q, pair_src, T, excl, max_corr, out=wk)
        self._work[("maploc", c)] = wk
        return self.plane_torch(xyz_q, offs_q, pair_src, T, wk, ml.wm.xyz, normals, ninfo, accepted, max_corr, min_inliers, min_ratio, sigma_min,
                                w_max, out=out)

    # ---- host forms (synchronise)
    def _host(self, who, xyz_q, offs_q, pair_src, T, accepted, nn):
        xq = np.ascontiguousarray(xyz_q, np.float64).reshape(-1, 3); oq = np.ascontiguousarray(offs_q, np.int64).reshape(-1)
        ps = np.ascontiguousarray(pair_src, np.int32).reshape(-1)
        if len(oq) < 1 or oq[-1] != len(xq):
            raise ValueError(f"{who}: the clouds are a CSR set: xyz [offs[-1], 3] and offs [Nq + 1]")
        c = len(ps)
        T = np.ascontiguousarray(T, np.float64)
        if T.size != 12 * c:
            raise ValueError(f"{who}: T must be [c, 3, 4]")
        acc = None
        if accepted is not None:
            acc = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
            if len(acc) != c:
                raise ValueError(f"{who}: accepted must be [c]")
        oo = np.ascontiguousarray(nn[0], np.int64).reshape(-1); ni = np.ascontiguousarray(nn[1], np.int32).reshape(-1)
        nd = np.ascontiguousarray(nn[2], np.float64).reshape(-1)
        if len(oo) != c + 1 or len(ni) != len(nd) or (c > 0 and oo[-1] > len(ni)):
            raise ValueError(f"{who}: nn must be (out_offs [c + 1], nn_idx, nn_d2 [>= out_offs[-1]])")
        out = RegInfo(np.zeros((c, 6, 6)), np.zeros((c, 6, 6)), np.zeros((c, 16)), np.zeros((c, 2)), np.zeros((c, 4), np.int32), np.zeros(c, np.uint8))
        return xq, oq, ps, c, T, acc, oo, ni, nd, out

    def point(self, xyz_q, offs_q, pair_src, T, nn, accepted=None, max_corr: float = 1.0, min_inliers: int = 10, min_ratio: float = 1e-4,
              sigma_min: float = 0.01, w_max: float = 1e6):
        """Host form (pr_reginfo_point) over numpy arrays: a RegInfo of numpy arrays (ok as bool)."""
        xq, oq, ps, c, T, acc, oo, ni, nd, out = self._host("RegistrationInfo.point", xyz_q, offs_q, pair_src, T, accepted, nn)
        self.ctx.check(self.lib.pr_reginfo_point(self.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(ps), c, _ptr(T), _ptr(acc), _ptr(oo), _ptr(ni), _ptr(nd),
                                                 float(max_corr), int(min_inliers), float(min_ratio), float(sigma_min), float(w_max),
                                                 *(_ptr(a) for a in out)))
        return out._replace(ok=out.ok.astype(bool))

    def plane(self, xyz_q, offs_q, pair_src, T, nn, world_xyz, normals, ninfo, accepted=None, max_corr: float = 0.9, min_inliers: int = 10,
              min_ratio: float = 1e-4, sigma_min: float = 0.01, w_max: float = 1e6):
        """Host form (pr_reginfo_plane) over numpy arrays: a RegInfo of numpy arrays (ok as bool)."""
        who = "RegistrationInfo.plane"
        xq, oq, ps, c, T, acc, oo, ni, nd, out = self._host(who, xyz_q, offs_q, pair_src, T, accepted, nn)
        wx = np.ascontiguousarray(world_xyz, np.float64).reshape(-1, 3)
        oc = len(wx)
        nrm = np.ascontiguousarray(normals, np.float64); info = np.ascontiguousarray(ninfo, np.int32)
        if nrm.shape != (oc, 3) or info.shape != (oc,):
            raise ValueError(f"{who}: normals must be [out_capacity, 3] and ninfo [out_capacity]")
        self.ctx.check(self.lib.pr_reginfo_plane(self.h, _ptr(xq), _ptr(oq), len(oq) - 1, _ptr(ps), c, _ptr(T), _ptr(acc), _ptr(oo), _ptr(ni), _ptr(nd),
                                                 _ptr(wx), oc, _ptr(nrm), _ptr(info), float(max_corr), int(min_inliers), float(min_ratio),
                                                 float(sigma_min), float(w_max), *(_ptr(a) for a in out)))
        return out._replace(ok=out.ok.astype(bool))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_reginfo_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MapGrower:
    """pr_mapgrow:the world map, the localiser's voxel index and the world-map normals grown by ONE keyframe a call.
    After a rebuild - WorldMap.fuse_torch(keep='first', min_count=1, cell=the localiser's) -> MapLocalizer.index_torch ->
    PlaneLocalizer.normals_torch -> sync_torch, which rebuild_torch issues in that order - extend_torch(row) takes in map row `row` (word
    1 of KeyframeMap.append's info) and normals_torch recomputes the normals around its new rows; both leave the rebuild's bytes at a cost
    that follows the cloud, not the map.  Rebuild again when the poses change (after a relaxation).  It borrows the world map and the
    localiser and owns one allocation; every device call is enqueued on the context's stream, decides on the device, reads nothing back
    and can be captured.  Close it before them."""

    def __init__(self, ctx: Context | None, wm, ml):
        self.ctx = ctx or default_context()
        self.h = None
        if wm.ctx is not self.ctx or ml.ctx is not self.ctx:
            raise ValueError("MapGrower: the grower, the world map and the localiser must share one context (one stream)")
        if ml.wm is not wm:
            raise ValueError("MapGrower: the localiser must have been created over this world map")
        self.lib = self.ctx.lib
        self.wm, self.ml = wm, ml
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_mapgrow_create(self.ctx.h, wm.h, ml.h, C.byref(h)))
        self.h = h

    _t = MapLocalizer._t
    _p = staticmethod(MapLocalizer._p)

    def sync_torch(self, n=None):
        """Device form (pr_mapgrow_sync_dev): from here on extends follow the fuse + index that lie in front on the stream.  n i32 [>= 1]
        whose word 0 is the keyframe count that fuse took (None = the map's state)."""
        import torch
        if n is not None:
            self._t("MapGrower.sync_torch", "n", n, torch.int32, numel_min=1)
        self.ctx.check(self.lib.pr_mapgrow_sync_dev(self.h, self._p(n)))

    def extend_torch(self, row, poses=None, info=None):
        """Device form (pr_mapgrow_extend_dev): row i32 [>= 1] whose word 0 is the map row to take in or -1 (the call is off) - a view of
        word 1 of an append's info; poses f64 [keyframe_capacity, 12] (None = the map's own).  Returns info (device i64 [4]) = rows
        stored, rows after, valid points of the row, flags: WORLDMAP_* of the call, or MAPGROW_ORDER | STALE | FULL when it was refused
        and nothing changed."""
        import torch
        who = "MapGrower.extend_torch"
        self._t(who, "row", row, torch.int32, numel_min=1)
        if poses is not None:
            self._t(who, "poses", poses, torch.float64, (self.wm.km.keyframe_capacity, 12))
        if info is None:
            info = torch.empty(4, dtype=torch.int64, device=self.wm.state.device)
        else:
            self._t(who, "info", info, torch.int64, (4,))
        p = self._p
        self.ctx.check(self.lib.pr_mapgrow_extend_dev(self.h, p(poses), p(row), p(info)))
        return info

    def normals_torch(self, radius: float, min_nbrs: int, max_ratio: float, normals, ninfo):
        """Device form (pr_mapgrow_normals_dev): recomputes, in place, the entries of normals f64 [out_capacity, 3] / ninfo i32
        [out_capacity] (a PlaneLocalizer.normals_torch pair, kept up to date since the rebuild) around the rows the last extend stored."""
        import torch
        who = "MapGrower.normals_torch"
        oc = self.wm.out_capacity
        self._t(who, "normals", normals, torch.float64, (oc, 3))
        self._t(who, "ninfo", ninfo, torch.int32, (oc,))
        p = self._p
        self.ctx.check(self.lib.pr_mapgrow_normals_dev(self.h, float(radius), int(min_nbrs), float(max_ratio), p(normals), p(ninfo)))
        return normals, ninfo

    def rebuild_torch(self, plane, poses=None, n=None, radius: float = 0.4, min_nbrs: int = 5, max_ratio: float = 0.1, out=None, infos=None):
        """The rebuild, in the one order that is right: fuse(keep='first', min_count=1, the localiser's cell) -> index -> normals -> sync.
        plane: the PlaneLocalizer over the same localiser; out: a (normals, ninfo) pair to write; infos: a (fuse info, index info) pair.
        Returns (normals, ninfo, fuse info, index info)."""
        if plane.ml is not self.ml:
            raise ValueError("MapGrower.rebuild_torch: the plane localiser must lie over this grower's localiser")
        finfo = self.wm.fuse_torch(poses, n, self.ml.cell, 1, "first", info=None if infos is None else infos[0])
        iinfo = self.ml.index_torch(info=None if infos is None else infos[1])
        out = plane.normals_torch(radius, min_nbrs, max_ratio, out=out)
        self.sync_torch(n)
        return out[0], out[1], finfo, iinfo

    # ---- host forms (synchronise)
    def extend(self, row: int, poses=None):
        """Host form (pr_mapgrow_extend): row an int, poses a numpy array [keyframe_capacity, 12] or None.  Returns info [4] i64."""
        po = None
        if poses is not None:
            po = np.ascontiguousarray(poses, np.float64)
            if po.shape != (self.wm.km.keyframe_capacity, 12):
                raise ValueError("MapGrower.extend: poses must be [keyframe_capacity, 12]")
        info = np.zeros(4, np.int64)
        self.ctx.check(self.lib.pr_mapgrow_extend(self.h, _ptr(po), int(row), _ptr(info)))
        return info

    def normals(self, radius: float, min_nbrs: int, max_ratio: float, normals, ninfo):
        """Host form (pr_mapgrow_normals): normals f64 [out_capacity, 3] and ninfo i32 [out_capacity] are contiguous numpy arrays holding
        the earlier normals; the recomputed rows are overwritten in place.  Returns the pair."""
        oc = self.wm.out_capacity
        if not (isinstance(normals, np.ndarray) and normals.dtype == np.float64 and normals.flags.c_contiguous and normals.shape == (oc, 3)
                and isinstance(ninfo, np.ndarray) and ninfo.dtype == np.int32 and ninfo.flags.c_contiguous and ninfo.shape == (oc,)):
            raise ValueError("MapGrower.normals: normals must be a contiguous f64 [out_capacity, 3] and ninfo a contiguous i32 [out_capacity] array")
        self.ctx.check(self.lib.pr_mapgrow_normals(self.h, float(radius), int(min_nbrs), float(max_ratio), _ptr(normals), _ptr(ninfo)))
        return normals, ninfo

    def count(self):
        """(keyframes fused, world rows seen, the last extend's flags); synchronises (pr_mapgrow_count)."""
        f, r, fl = C.c_int32(), C.c_int64(), C.c_int32()
        self.ctx.check(self.lib.pr_mapgrow_count(self.h, C.byref(f), C.byref(r), C.byref(fl)))
        return int(f.value), int(r.value), int(fl.value)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.pr_mapgrow_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_points_by_pose(pose_ids, point_ids) -> np.ndarray:
    """The reference's cursor rule (utils/pts_preprocess.h:196-200) as per-pose pushes: at pose p the cursor takes points while
    id <= pose id, so an out-of-order id makes it wait.  Returns cuts int64 [len(pose_ids) + 1]: pose p is pushed the points
    [cuts[p], cuts[p + 1]) of the file; points behind cuts[-1] are never delivered."""
    pid = np.asarray(pose_ids, np.int64).reshape(-1)
    qid = np.asarray(point_ids, np.int64).reshape(-1)
    # the cursor stops at the first point with id > pose id: position c advances past point j while max(id[.. j]) <= pose id
    run = np.maximum.accumulate(qid) if len(qid) else qid
    cuts = np.zeros(len(pid) + 1, np.int64)
    c = 0
    for p, i in enumerate(pid):
        c = max(c, int(np.searchsorted(run, i, side="right")))
        cuts[p + 1] = c
    return cuts


def read_poses_points(poses_file: str, pts_file: str):
    """The two PosesPts text files as arrays, parsed like the reference's reader for well-formed files:
    (pose_ids i32 [M], w2c f64 [M, 12], point_ids i32 [T], xyz f64 [T, 3], inten f32 [T]).  A missing file is an empty one."""
    def rows(path, ncol):
        try:
            txt = open(path).read().split()
        except OSError:
            txt = []
        n = len(txt) // ncol
        return np.array(txt[:n * ncol], dtype=object).reshape(n, ncol)
    pr_, qr = rows(poses_file, 13), rows(pts_file, 5)
    pid = pr_[:, 0].astype(np.int64).astype(np.int32) if len(pr_) else np.zeros(0, np.int32)
    w = np.array([[float(v) for v in r[1:]] for r in pr_], np.float64).reshape(len(pr_), 12)
    qid = qr[:, 0].astype(np.int64).astype(np.int32) if len(qr) else np.zeros(0, np.int32)
    xyz = np.array([[float(v) for v in r[1:4]] for r in qr], np.float64).reshape(len(qr), 3)
    it = np.array([np.float32(r[4]) for r in qr], np.float32).reshape(len(qr))
    return pid, w, qid, xyz, it


def _pts_preprocess_stream(poses_file, pts_file, incoming_id_file, lidarRange, polar_filter, ctx, capacities=None, return_frames=False):
    """A pair of files replayed through a CloudWindow, keyframe by keyframe."""
    pid, w, qid, xyz, it = read_poses_points(poses_file, pts_file)
    cuts = split_points_by_pose(pid, qid)
    per = np.diff(cuts)
    cap = capacities or (max(int(cuts[-1]), 1), max(int(per.max()) if len(per) else 1, 1), max(int(cuts[-1]), 1))
    win = CloudWindow(ctx, lidarRange, polar_filter, *cap)
    X, I, offs, ids, frames = [], [], [0], [], []
    try:
        for p in range(len(pid)):
            a, b = int(cuts[p]), int(cuts[p + 1])
            ox, oi, fr, info = win.push(w[p], xyz[a:b], it[a:b])
            if info[0]:
                X.append(ox); I.append(oi); offs.append(offs[-1] + len(oi)); ids.append(pid[p]); frames.append(fr)
    finally:
        win.close()
    if incoming_id_file:
        with open(incoming_id_file, "w") as f:
            f.write("".join("%d\n" % i for i in ids))
    res = (np.concatenate(X) if X else np.zeros((0, 3)), np.concatenate(I) if I else np.zeros((0,), np.float32),
           np.array(offs, np.int64), np.array(ids, np.int32))
    return res + (np.array(frames, np.float64).reshape(len(ids), 16),) if return_frames else res


def pts_preprocess(poses_file: str, pts_file: str, incoming_id_file: str | None, lidarRange: float = 45.0,
                   polar_filter: bool = False, verbose: bool = False, gpu=False, ctx: Context | None = None):
    """pts_preprocess(...) of utils/pts_preprocess.h:169-232 -> (xyz [T,3] f64, inten [T] f32, offs [N+1] i64, ids [N] i32).
    gpu=True runs the sliding-window / best-point-per-cell work on the device (same clouds, same point order); gpu="stream" replays the
    files keyframe by keyframe through a CloudWindow (the online form: the same clouds again)."""
    if isinstance(gpu, str):
        if gpu != "stream":
            raise ValueError('pts_preprocess: gpu is False, True or "stream"')
        return _pts_preprocess_stream(poses_file, pts_file, incoming_id_file, lidarRange, polar_filter, ctx or default_context())
    lib = _lib.load()
    h = C.c_void_p()
    args = (poses_file.encode(), pts_file.encode(), incoming_id_file.encode() if incoming_id_file else None,
            float(lidarRange), int(polar_filter), int(verbose), C.byref(h))
    if gpu:
        ctx = ctx or default_context()
        ctx.check(lib.pr_pts_preprocess_gpu(ctx.h, *args))
    else:
        rc = lib.pr_pts_preprocess(*args)
        if rc != 0:
            raise PRError(rc, lib.pr_host_last_error().decode())
    try:
        N = lib.pr_clouds_count(h)
        offs = np.ctypeslib.as_array(lib.pr_clouds_offs(h), (N + 1,)).copy()
        T = int(offs[-1])
        xyz = np.ctypeslib.as_array(lib.pr_clouds_xyz(h), (T, 3)).copy() if T else np.zeros((0, 3))
        it = np.ctypeslib.as_array(lib.pr_clouds_inten(h), (T,)).copy() if T else np.zeros((0,), np.float32)
        ids = np.ctypeslib.as_array(lib.pr_clouds_ids(h), (N,)).copy() if N else np.zeros((0,), np.int32)
        pts_preprocess.last_avg_ms = float(lib.pr_clouds_avg_ms(h))     # "generate_spherical_points average time"
    finally:
        lib.pr_clouds_free(h)
    return xyz, it, offs, ids


def hash_order(keys) -> np.ndarray:
    """Iteration order of a libstdc++ unordered_map<int,...> after inserting these distinct keys in this order."""
    k = np.ascontiguousarray(keys, np.int32)
    out = np.empty(len(k), np.int32)
    rc = _lib.load().pr_hash_order(_ptr(k), len(k), _ptr(out))
    if rc != 0:
        raise PRError(rc, "pr_hash_order")
    return out


def write_signatures(path: str, sig, dtype=np.float64) -> None:
    """`ofstream << Eigen::MatrixXd` text (test_sc.cpp:63-66); a path ending in .bin writes the binary side-car."""
    sig = np.ascontiguousarray(sig, np.float64)
    lib = _lib.load()
    if path.endswith(".bin"):
        rc = lib.pr_write_signatures_bin(path.encode(), _ptr(sig), sig.shape[0], sig.shape[1],
                                         _lib.F32 if dtype == np.float32 else _lib.F64)
    else:
        rc = lib.pr_write_signatures(path.encode(), _ptr(sig), sig.shape[0], sig.shape[1])
    if rc != 0:
        raise PRError(rc, lib.pr_host_last_error().decode())


def read_signatures(path: str) -> np.ndarray:
    lib = _lib.load()
    p = C.c_void_p(); r = C.c_int64(); c = C.c_int64()
    fn = lib.pr_read_signatures_bin if path.endswith(".bin") else lib.pr_read_signatures
    rc = fn(path.encode(), C.byref(p), C.byref(r), C.byref(c))
    if rc != 0:
        raise PRError(rc, lib.pr_host_last_error().decode())
    try:
        out = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (r.value, c.value)).copy()
    finally:
        lib.pr_free(p)
    return out


def write_poses(path: str, ids, w2c) -> None:
    ids = np.ascontiguousarray(ids, np.int32); w2c = np.ascontiguousarray(w2c, np.float64).reshape(len(ids), 12)
    _lib.load().pr_write_poses(path.encode(), _ptr(ids), _ptr(w2c), len(ids))


def write_points(path: str, ids, xyz, inten) -> None:
    ids = np.ascontiguousarray(ids, np.int32); xyz = np.ascontiguousarray(xyz, np.float64)
    inten = np.ascontiguousarray(inten, np.float32)
    _lib.load().pr_write_points(path.encode(), _ptr(ids), _ptr(xyz), _ptr(inten), len(ids))
