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

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _handle, _lib
from ._lib import PRError, TYPE_BOW, TYPE_DELIGHT, TYPE_GIST, TYPE_M2DP, TYPE_SC  # noqa: F401
from ._context import Context, default_context, _torch_default_context  # noqa: F401
from ._handle import _ptr
# The device-handle classes and the registration calls live in modules of their own; api stays the one public namespace.
from .registration import *  # noqa: F401,F403
from .registration import _ICP_SEARCH, _POSE_TYPES, _icp_sets, _pose_type, _variant_view, _verify_out  # noqa: F401
from .mapping import *  # noqa: F401,F403
from .online import *  # noqa: F401,F403
from .online import _OnlineEngine, _check_steps  # noqa: F401
from .graph import *  # noqa: F401,F403


class GISTParams(NamedTuple):
    """cls::GISTParams (GIST/include/gist.h): use_color, width, height, blocks, scale, orients."""
    use_color: bool = False
    width: int = 256
    height: int = 256
    blocks: int = 4
    scale: int = 4
    orients: tuple = (8, 8, 8, 8)

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
    ctx.check(ctx.lib.pr_gist_generate_dev(ctx.h, _handle.ptr(img), dtype, N, H, W, int(nblocks), len(o), _ptr(o), _handle.ptr(out)))
    if lib_stream is not None:
        cur.wait_stream(lib_stream)                # torch's later work sees the rows
        img.record_stream(lib_stream)
        out.record_stream(lib_stream)
    return out


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
    ctx.check(ctx.lib.pr_bow_generate_dev(ctx.h, vocab._handle(), _handle.ptr(desc), F, _handle.ptr(offs), N, int(cols), _handle.ptr(out), _handle.ptr(n_words),
                                          _handle.ptr(feature_words)))
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


def seq_select_torch(d_p, d_i, mom, steps, q_row0: int = 0, db_row0: int = 0, mask_width: int = 0, p_weight: float = 2.0, k: int = 1,
                     dense: bool = False, ctx: Context | None = None, out=None):
    """Device form of the sequence selection (pr_seq_select_dev): d_p, d_i f32 [m, n] and mom f64 [m, 2, 3] as
    pr_distances_dev / pr_row_moments_dev wrote them (d_i = None: one matrix, no normalisation, mom unused), steps a CUDA i32 [V, L]
    tensor.  Returns (idx i32 [m, k] global DB rows, score f64 [m, k], vel i32 [m, k][, S f64 [m, n] with dense=True]); out: an earlier
    call's tuple, written again.  Enqueued on the context's stream; nothing synchronises or, given out=, allocates."""
    import torch
    ctx = ctx or _torch_default_context(d_p.device.index)
    who, dev = "seq_select_torch", d_p.device
    msg = f"{who}: d_p must be a contiguous CUDA tensor f32 [m, n]"
    _handle.check(who, "d_p", d_p, torch.float32, dev, msg=msg)
    if d_p.dim() != 2:
        raise ValueError(msg)
    m, n = d_p.shape
    if d_i is not None:
        _handle.check(who, "d_i", d_i, torch.float32, dev, shape=(m, n), msg=f"{who}: d_i must be a contiguous CUDA tensor f32 [m, n]")
        msg = f"{who}: mom must be a contiguous CUDA tensor f64 [m, 2, 3]"
        if mom is None:
            raise ValueError(msg)
        _handle.check(who, "mom", mom, torch.float64, dev, numel=6 * m, msg=msg)
    msg = f"{who}: steps must be a contiguous CUDA tensor i32 [V, L]"
    _handle.check(who, "steps", steps, torch.int32, dev, msg=msg)
    if steps.dim() != 2:
        raise ValueError(msg)
    V, L = steps.shape
    k = int(k)
    msg = f"{who}: out must be (idx i32 [m, k], score f64 [m, k], vel i32 [m, k][, S f64 [m, n]]) CUDA tensors"
    if out is not None and len(out) != (4 if dense else 3):
        raise ValueError(msg)
    mk = (m, max(k, 0) if out is None else k)
    want = ((torch.int32, mk), (torch.float64, mk), (torch.int32, mk)) + (((torch.float64, (m, n)),) if dense else ())
    out = tuple(_handle.result(who, "out", t, dt, sh, dev, msg=msg) for t, (dt, sh) in zip(out or (None,) * len(want), want))
    if m == 0:
        return out
    ctx.check(ctx.lib.pr_seq_select_dev(ctx.h, _handle.ptr(d_p), _handle.ptr(d_i), m, n, _handle.ptr(mom) if d_i is not None else None, _handle.ptr(steps), V, L, int(q_row0),
                                        int(db_row0), int(mask_width), float(p_weight), k, _handle.ptr(out[0]), _handle.ptr(out[1]), _handle.ptr(out[2]),
                                        _handle.ptr(out[3]) if dense else None))
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
    ctx.check(ctx.lib.pr_cloud_frames_dev(ctx.h, _handle.ptr(x), _handle.ptr(it), _handle.ptr(o), N, _handle.ptr(fr)))
    ctx.sync()
    return fr.cpu().numpy()


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
