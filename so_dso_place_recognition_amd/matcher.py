"""Device-resident matcher: run_test.m:26-57 on signatures that already live in HBM, optionally with the
database row-sharded over the ranks of a torch.distributed group (one process per GPU, RCCL over xGMI).

PyTorch is plumbing here (device buffers, streams, the two small collectives); all arithmetic is in
libpr_amd.so through the C ABI (plain device pointers).  The library context is created ON torch's current
stream (pr_create_on_stream), so the library's kernels, torch's allocations and RCCL's collectives are ordered
by the stream itself: a step has no host synchronisation at all.

Sharding: every rank holds the DB rows [db_row0, db_row0 + n_local) and ALL queries.
  1. local: pack, distances (m x n_local), per-row fp64 moments (count, mean, M2) per channel          [HIP]
  2. all_gather_into_tensor of the moments  (m x 2 x 3 f64 per rank = 48 B per query)                        [RCCL]
     (all-gather + Chan combination in rank order instead of §8-e's all-reduce: same bytes at this size, and the
     result does not depend on the reduction order RCCL happens to pick - every rank computes the same bits)
  3. local: Chan-combine -> global mean/std, fused fp32 score, mask on GLOBAL indices, per-shard top-(k+8)
     (ties -> lower global index)                                                                      [HIP]
  4. all_gather_into_tensor of the per-shard (idx i32, fp32 score) lists, k-way merge on the device by
     (score, idx) (pr_merge_topk_dev) -> the GLOBAL top-(k+8) candidates, the same list an unsharded run
     selects                                                                                           [RCCL + HIP]
  5. local: fp64 re-evaluation, from the raw signatures, of the candidates that lie in this shard
     (pr_rerank_partial_dev; on average (k+8)/G pairs per query: the cost does not grow with G)          [HIP]
  6. all_gather_into_tensor of the shards' evaluations (p5 blocks: score + 4 exact channel distances per candidate, 40 (k+8) B per
     query per rank), every candidate's score taken from its owner, the k best by (score, idx) and the order check
     (pr_rerank_finish_dev)                                                                             [RCCL + HIP]
  7. queries the re-evaluated candidates cannot answer for certain - their order hangs on the fp32 pass's sigmas, or the k + 8 candidates do
     not provably hold the top-k (near-copies of one place) - none, as a rule: the kernels leave at once.  Such a query is answered from
     its EXACT ROW (run_test.m:38-57 are fp64 over the whole row): this shard's fp64 distances to all of its entries and their moments
     (pr_order_exact_moments_dev), all_gather_into_tensor (96 B per query per rank), the shard's k best under the statistics of the whole
     row (pr_order_exact_select_dev), all_gather_into_tensor (64 x 16 k B per rank), merge on every rank (pr_order_exact_merge_dev)
                                                                                                [HIP + RCCL + HIP + RCCL + HIP]
With one rank steps 2, 4, 6 and 7's gathers are skipped (pr_rerank_dev does 5 + the selection, pr_order_resolve_async_dev does 7).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .api import Context


def _dptr(t: torch.Tensor | None):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _torch_dt(t: torch.Tensor) -> int:
    return {torch.float64: _lib.F64, torch.float32: _lib.F32}[t.dtype]


def _raw_rows(d) -> tuple:
    """(queries, DB, dtype) of a descriptor store: the raw rows of its last local_phase1() / its DB shard (the fp64 kernels read them)."""
    assert d._q_sig.dtype == d.db_sig.dtype
    return _dptr(d._q_sig), _dptr(d.db_sig), _torch_dt(d.db_sig)


_NO_ROWS = (None, None, 0)


def _stream_context(device: int, **kw) -> Context:
    """A library context whose kernels run on torch's current stream of that device."""
    return Context(device, stream=int(torch.cuda.current_stream(device).cuda_stream), **kw)


RESOLVE_SLOTS = 64      # flagged queries one pass of the exact-row resolution serves (kernels.hpp)


class _Base:
    """The device-resident protocol, written once over the matcher's descriptor stores `descs`: (self,) for a Matcher, (sc, m2) for a
    FusedMatcher.  Every store holds its raw rows (_q_sig, db_sig), its distance matrices (_bufs) and, after local_select(), its part of
    the moments of all shards (_mom [G, m, 2, 3]); the matcher itself holds _m / n (queries of the last local_phase1(), DB rows of this
    shard) and, in its own _bufs, the call's candidate lists and results."""
    resolved = None       # queries the last single-shard match() of more than 64 queries answered from their exact rows (it reads the count back)
    plain = False         # True for DELIGHT (Matcher): one distance matrix, no z-score fusion
    _raw = None           # the capacity-sized raw DB of reserve_database()
    _twin = None          # the split-f16 twin of the f16 arithmetic (_split_twin)

    def _init_ctx(self, ctx, device):
        if device is None:
            device = ctx.device if ctx is not None else torch.cuda.current_device()
        self.ctx = ctx or _stream_context(device)
        self.dev = torch.device("cuda", self.ctx.device)
        self.lib = self.ctx.lib
        self._lib_stream = None if self.ctx.stream == 0 else torch.cuda.ExternalStream(self.ctx.stream, device=self.dev)
        self._bufs = {}
        self._flat = {}

    def close(self):
        if self._twin is not None:
            self._twin.close()
            self._twin = None

    # The library's kernels run on self.ctx.stream; torch work (casts, zero_(), all_gather_into_tensor, output allocations) runs on torch's
    # CURRENT stream, which may differ from the one the context was created on (`with torch.cuda.stream(s)`, DDP side streams).  The two
    # are compared at every call: the same stream needs nothing, different streams are joined by events (no host wait).
    def _same_stream(self) -> bool:
        return self.ctx.stream == int(torch.cuda.current_stream(self.dev).cuda_stream)

    def _enter(self):      # torch work issued so far must be visible to the library's stream
        if self._same_stream():
            return
        if self._lib_stream is not None:
            self._lib_stream.wait_stream(torch.cuda.current_stream(self.dev))
        else:
            torch.cuda.current_stream(self.dev).synchronize()

    def _leave(self):      # ... and the library's work to torch's
        if self._same_stream():
            return
        if self._lib_stream is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self._lib_stream)
        else:
            self.ctx.sync()

    def _buf(self, name, shape, dtype):
        """The call's working tensors, kept between calls.  A shape that grows a little per call (a DB that gains a row per keyframe: the
        [m, n] distance matrices) is served as a view of flat storage with an eighth of headroom instead of a new allocation per call."""
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            need = 1
            for d in shape:
                need *= int(d)
            flat = self._flat.get(name)
            if flat is None or flat.dtype != dtype or flat.numel() < need:
                flat = torch.empty(need + (need >> 3 if self._raw is not None else 0), dtype=dtype, device=self.dev)
                self._flat[name] = flat
            t = flat[:need].view(shape)
            self._bufs[name] = t
        return t

    # ---- the library's argument slots (the C++ Types::dev): one SC and one M2DP slot, None / (None, None, 0) for a type the matcher lacks
    def _slots(self):
        sc = m2 = None
        for d in self.descs:
            if d.type == _lib.TYPE_SC:
                sc = d
            elif d.type == _lib.TYPE_M2DP:
                m2 = d
        return sc, m2

    def _raw6(self) -> tuple:
        """(q_sc, db_sc, dt_sc, q_m2, db_m2, dt_m2)"""
        sc, m2 = self._slots()
        return (*(_NO_ROWS if sc is None else _raw_rows(sc)), *(_NO_ROWS if m2 is None else _raw_rows(m2)))

    def _moms(self) -> tuple:
        """(mom_sc, mom_m2): the moments of all shards the last local_select() was given."""
        sc, m2 = self._slots()
        return None if sc is None else sc._mom, None if m2 is None else m2._mom

    # ---- PR_SC_ARITH_F16 (single f16 product per term): exact indices need a margin check of the candidate list and, for the
    # queries that fail it, a second pass in split-f16 (include/place_recognition.h)
    @property
    def f16(self) -> bool:
        return self.ctx.sc_arith == "f16"

    def _margin(self, mom_sc, mom_m2, G, p_weight, cand_sc: torch.Tensor, k: int, score: torch.Tensor):
        """pr_f16_margin_dev -> (flags int32 [m], count int32 [1]) device tensors; no host synchronisation."""
        m, kin = cand_sc.shape
        flags = torch.empty((m,), dtype=torch.int32, device=self.dev)
        count = torch.empty((1,), dtype=torch.int32, device=self.dev)
        self._enter()
        self.ctx.check(self.lib.pr_f16_margin_dev(self.ctx.h, _dptr(mom_sc), _dptr(mom_m2), m, G, float(p_weight), kin, _dptr(cand_sc.contiguous()),
                                                  int(k), _dptr(score.contiguous()), _dptr(flags), _dptr(count)))
        self._leave()
        self.f16_flags, self.f16_count = flags, count
        return flags, count

    def _fallback_rows(self, run_rows, idx, score, mask_width, q_row0):
        """Recomputes the flagged queries through `run_rows(rows tensor, q_row0 or None)` (a split-f16 matcher over the same DB) and
        patches idx / score.  Reads the flag count back: one host synchronisation per call, only in the f16 arithmetic."""
        cnt = int(self.f16_count.item())
        self.f16_fallbacks = cnt
        if cnt == 0:
            return idx, score
        rows = torch.nonzero(self.f16_flags, as_tuple=False).flatten()
        idx, score = idx.clone(), score.clone()
        if mask_width <= 0:                       # the mask does not look at the query's row number: one batch
            i2, s2 = run_rows(rows, None)
            idx[rows], score[rows] = i2, s2
        else:
            for r in rows.tolist():
                i2, s2 = run_rows(rows.new_tensor([r]), q_row0 + r)
                idx[r], score[r] = i2[0], s2[0]
        return idx, score

    def _split_twin(self):
        """The same matcher in split-f16 over the same (already resident) raw DB, created and packed on first use."""
        db = self.descs[0].db_sig
        if self._twin is None or self._twin_of is not db:
            if self._twin is not None:
                self._twin.close()
            tw = type(self)(*self._spec, ctx=Context(self.ctx.device, sc_arith="f16x2", stream=self.ctx.stream))
            tw.pack_database(*(d.db_sig for d in self.descs))
            self._twin, self._twin_of = tw, db
        return self._twin

    # ---- the protocol (module docstring): phase 1 is the subclass's, everything after it is written here once
    def local_select(self, mom_all: torch.Tensor, G: int, mask_width, p_weight, k, db_row0, q_row0, with_moments: bool = False):
        """fp32 selection of this shard's k + 8 best with the moments of all shards -> (idx_in i32 [m,kin], score f64 [m,kin]).
        with_moments (one shard, one descriptor type, after local_phase1(moments=False)): mom_all [1, m, 2, 3] is still to be written -
        pr_moments_select_f64_dev forms the moments in the selection's own sweep of the distances."""
        m, n = self._m, self.n
        stores = self.descs
        if with_moments:
            assert G == 1 and len(stores) == 1 and not self.plain and mom_all.is_contiguous()
            stores[0]._mom = mom_all
            lib = self.lib
            select = lambda h, d_p, d_i, m_, n_, mom, G_, *rest: lib.pr_moments_select_f64_dev(h, d_p, d_i, m_, n_, mom, *rest)
        elif len(stores) == 1:        # one descriptor type: its moments [G, m, 2, 3] as they are
            stores[0]._mom = mom_all.contiguous()
            select = self.lib.pr_fuse_select_f64_dev
        else:                         # SC + M2DP: [G, m, 4, 3] split per type
            for d, t in zip(stores, mom_all.reshape(G, m, 4, 3).split(2, dim=2)):
                d._mom = t.contiguous()
            select = self.lib.pr_fuse_select2_f64_dev
        self._args = (G, q_row0, db_row0, int(mask_width), float(p_weight))
        kin = k if self.plain else int(self.lib.pr_rerank_width(self.ctx.h, int(k)))
        idx_in = self._buf("idx_in", (m, kin), torch.int32)
        sc32 = self._buf("sc32", (m, kin), torch.float32)
        sc64 = self._buf("sc64", (m, kin), torch.float64)
        dists = [_dptr(t) for d in stores for t in (d._bufs["d_p"], d._bufs.get("d_i"))]
        self._enter()
        self.ctx.check(select(self.ctx.h, *dists, m, n, *[_dptr(d._mom) for d in stores], G, q_row0, db_row0, int(mask_width), float(p_weight),
                              int(kin), _dptr(idx_in), _dptr(sc32), _dptr(sc64)))
        self._leave()
        return idx_in, sc64

    def local_rerank(self, cand_idx: torch.Tensor, k: int, partial: bool, cand_sc: torch.Tensor = None):
        """fp64 re-evaluation of the candidates [m,kin]: partial=False -> (idx [m,k], score [m,k]) (all candidates are this
        shard's: the one-rank path); partial=True -> scores [m,kin], NaN for candidates outside this shard.  cand_sc: the
        candidates' fp32-pass scores as f64 [m,kin] (ascending) - candidates that cannot reach the top-k are then not evaluated."""
        m, n = self._m, self.n
        G, q_row0, db_row0, mask_width, p_weight = self._args
        kin = cand_idx.shape[1]
        cand_idx = cand_idx.contiguous()
        cand_sc = None if cand_sc is None else cand_sc.contiguous()
        self._last_cand = (cand_idx, cand_sc)
        rows = (*self._raw6(), *map(_dptr, self._moms()))
        self._enter()
        if partial:
            part = self._buf("part", (m, 5, kin), torch.float64)           # the shard's p5 block (include/place_recognition.h)
            self.ctx.check(self.lib.pr_rerank_partial_dev(self.ctx.h, *rows, m, n, G, q_row0, db_row0, mask_width, p_weight, kin, _dptr(cand_idx),
                                                          _dptr(cand_sc), int(k), _dptr(part)))
            self._leave()
            return part
        idx = self._buf("idx", (m, k), torch.int32)
        score = self._buf("score", (m, k), torch.float64)
        self.ctx.check(self.lib.pr_rerank_dev(self.ctx.h, *rows, m, n, G, q_row0, db_row0, mask_width, p_weight, kin, _dptr(cand_idx),
                                              _dptr(cand_sc), int(k), _dptr(idx), _dptr(score)))
        self._leave()
        return idx, score

    def local_phase2(self, mom_all: torch.Tensor, G: int, mask_width, p_weight, k, db_row0, q_row0):
        """Selection + re-evaluation of this shard alone -> its own top-k (what rank g would answer by itself)."""
        idx_in, sc = self.local_select(mom_all, G, mask_width, p_weight, k, db_row0, q_row0)
        if self.plain:
            return idx_in, sc
        return self.local_rerank(idx_in, k, partial=False, cand_sc=sc)

    def merge(self, idx_all: torch.Tensor, sc_all: torch.Tensor, k: int):
        """pr_merge_topk_dev on [G, m, k] device tensors."""
        G, m, kk = idx_all.shape
        assert kk == k
        idx = torch.empty((m, k), dtype=torch.int32, device=idx_all.device)
        score = torch.empty((m, k), dtype=torch.float64, device=idx_all.device)
        self._enter()
        self.ctx.check(self.lib.pr_merge_topk_dev(self.ctx.h, _dptr(idx_all.contiguous()), _dptr(sc_all.contiguous()), G, m, k, _dptr(idx),
                                                  _dptr(score)))
        self._leave()
        return idx, score

    def finish(self, cand_idx: torch.Tensor, cand_sc: torch.Tensor | None, part_all: torch.Tensor, k: int):
        """pr_rerank_finish_dev: candidates [m, kin] (+ their merged pass scores) + the shards' p5 blocks [G, m, 5, kin] -> (idx [m,k], score [m,k]);
        the order and containment checks of the result (under the statistics of the last local_select()) stay in the context:
        pr_f16_margin_dev (PR_SC_ARITH_F16) or exact_moments() / exact_select() / exact_merge() take them."""
        G, m, five, kin = part_all.shape
        assert five == 5
        idx = torch.empty((m, k), dtype=torch.int32, device=cand_idx.device)
        score = torch.empty((m, k), dtype=torch.float64, device=cand_idx.device)
        cand_idx = cand_idx.contiguous()
        cand_sc = None if cand_sc is None else cand_sc.contiguous()
        part_all = part_all.contiguous()
        self._enter()
        self.ctx.check(self.lib.pr_rerank_finish_dev(self.ctx.h, *map(_dptr, self._moms()), int(self._args[0]), _dptr(cand_idx), _dptr(cand_sc),
                                                     _dptr(part_all), G, m, kin, k, float(self._args[4]), _dptr(idx), _dptr(score)))
        self._leave()
        return idx, score

    def exact_moments(self, offset: int = 0, last: bool = True):
        """Step 7, first local part: this shard's exact rows of flagged queries offset .. offset + 63 of the last finish() (kept in the
        context) and their moments -> [m, 4, 3] f64.  last: no pass follows (flagged queries behind it raise WARN_ORDER_UNRESOLVED)."""
        m, n = self._m, self.n
        raw6 = self._raw6()
        exact = torch.empty((m, 4, 3), dtype=torch.float64, device=self.dev)
        self._enter()
        self.ctx.check(self.lib.pr_order_exact_moments_dev(self.ctx.h, *raw6, *map(_dptr, self._moms()), int(self._args[0]), m, n, int(offset),
                                                           int(bool(last)), _dptr(exact)))
        self._leave()
        return exact

    def exact_select(self, exact_all: torch.Tensor, k: int, offset: int = 0):
        """Step 7, second local part: this shard's k best of the flagged queries' exact rows under the statistics of all shards
        -> [64, 2, k] f64 (scores | global indices)."""
        m, n = self._m, self.n
        _, q_row0, db_row0, mask_width, p_weight = self._args
        mom_sc, mom_m2 = self._moms()
        G = exact_all.shape[0]
        exact_all = exact_all.contiguous()
        sel = torch.empty((RESOLVE_SLOTS, 2, k), dtype=torch.float64, device=self.dev)
        self._enter()
        self.ctx.check(self.lib.pr_order_exact_select_dev(self.ctx.h, _dptr(exact_all), G, m, n, int(q_row0), int(db_row0), int(mask_width),
                                                          float(p_weight), int(mom_sc is not None), int(mom_m2 is not None), int(k), int(offset),
                                                          _dptr(sel)))
        self._leave()
        return sel

    def exact_merge(self, sel_all: torch.Tensor, k: int, idx: torch.Tensor, score: torch.Tensor, offset: int = 0):
        G = sel_all.shape[0]
        sel_all = sel_all.contiguous()
        self._enter()
        self.ctx.check(self.lib.pr_order_exact_merge_dev(self.ctx.h, _dptr(sel_all), G, self._m, int(k), int(offset), _dptr(idx), _dptr(score)))
        self._leave()
        return idx, score

    def _exact_passes(self, exact_order=True):
        """Passes of RESOLVE_SLOTS flagged queries step 7 of the sharded protocol needs (the same number on every rank: the flags are a
        function of the gathered evaluations).  Up to RESOLVE_SLOTS queries: one, unconditionally and without synchronisation; exact_order ==
        "async" (a captured graph): ceil(m / 64), every one of them with its two all-gathers, whatever was flagged - empty passes leave at once;
        otherwise the flagged count is read back (one synchronisation) - none flagged, no pass and no all-gather."""
        m = self._m
        if m <= RESOLVE_SLOTS:
            return 1
        if exact_order == "async":
            return (m + RESOLVE_SLOTS - 1) // RESOLVE_SLOTS
        return (self.flagged_count() + RESOLVE_SLOTS - 1) // RESOLVE_SLOTS

    def _resolve_order(self, k, idx, score, exact_order=True):
        """After a single-shard pr_rerank_dev: queries whose re-evaluated order hangs on the fp32 pass's sigmas, or whose candidate list does
        not provably hold the top-k, are answered from their exact fp64 rows; idx / score (and the moments rows) are patched in place.
        One pass takes RESOLVE_SLOTS flagged queries.  Calls of up to that many queries (and exact_order == "async"): pr_order_resolve_async_dev,
        ceil(m / 64) stream-ordered passes without host synchronisation - all flagged queries, empty passes leave at once
        (PR_WARN_ORDER_RESOLVED at ctx.take_warnings() tells whether it happened).  Larger calls: pr_order_resolve_dev - reads the number of
        flagged queries back (ONE synchronisation of the stream per call) and runs as many passes as it takes."""
        m, n = self._m, self.n
        _, q_row0, _, mask_width, p_weight = self._args
        args = (self.ctx.h, *self._raw6(), *map(_dptr, self._moms()), m, n, int(q_row0), int(mask_width), float(p_weight), int(k), _dptr(idx),
                _dptr(score))
        self._enter()
        if m <= RESOLVE_SLOTS or exact_order == "async":
            self.ctx.check(self.lib.pr_order_resolve_async_dev(*args))
        else:
            cnt = C.c_int32(0)
            self.ctx.check(self.lib.pr_order_resolve_dev(*args, C.byref(cnt)))
            self.resolved = int(cnt.value)
        self._leave()

    def _match(self, queries: tuple, mask_width, p_weight, k, db_row0, q_row0, group, force_exchange, f16_fallback, exact_order, mark):
        """match() with the query rows of every store (queries: one tensor per store, in the order of descs)."""
        G = _world(group)
        f16 = self.f16 and not self.plain
        resolve = ((self.exact_moments, self.exact_select, self.exact_merge, lambda: self._exact_passes(exact_order))
                   if (exact_order and not self.plain and not f16) else None)
        post = (lambda cand_sc, idx, score: self._margin(*self._moms(), self._args[0], p_weight, cand_sc, k, score)) if f16 else None
        # one shard of one descriptor type: the moments come out of the selection's sweep (pr_moments_select_f64_dev), phase 1 leaves them out
        one = G == 1 and not force_exchange and not self.plain and len(self.descs) == 1 and self.descs[0] is self
        idx, score = sharded_topk((lambda: self.local_phase1(*queries, moments=False)) if one else (lambda: self.local_phase1(*queries)),
                                  lambda mom_all, G_: self.local_select(mom_all, G_, mask_width, p_weight, k, db_row0, q_row0, with_moments=one),
                                  k, group if (G > 1 or force_exchange) else None, G, merge=self.merge, force_exchange=force_exchange,
                                  rerank=None if self.plain else self.local_rerank, finish=self.finish, post=post, resolve=resolve, mark=mark)
        if f16 and f16_fallback:
            def run_rows(rows, qr0):
                fb = self._split_twin()
                qsel = [q.view(-1, d.rows_per_sig, d.sig_len)[rows].reshape(-1, d.sig_len).contiguous()   # M2DP: 4 rows per query
                        for d, q in zip(self.descs, queries)]
                return fb._match(qsel, mask_width, p_weight, k, db_row0, q_row0 if qr0 is None else qr0, group, force_exchange, True, exact_order,
                                 None)
            idx, score = self._fallback_rows(run_rows, idx, score, mask_width, q_row0)
        elif resolve is not None and G == 1 and not force_exchange:
            self._resolve_order(k, idx, score, exact_order)
            if mark is not None:
                mark("exact rows (one shard)")
        return idx, score

    def align(self, idx: torch.Tensor, db_row0: int = 0):
        """The best-aligning variant of every pair (query of the last match(), DB row idx[q, j]) -> (variant int32 [m,k,2], dist float64
        [m,k,2]) device tensors, per channel (SC: structure, intensity, v = 2 * shift + mirror; M2DP: count, intensity, v = 4 * query row +
        DB row; DELIGHT: [..., 0] the octant permutation, [..., 1] = -1 / NaN), from the raw rows in fp64 (pr_align_pairs_dev /
        pr_delight_align_pairs_dev: the variant arithmetic of the re-evaluation, whatever the matcher's arithmetic; a growing DB included).
        A FusedMatcher returns [m,k,4]: SC structure, SC intensity, M2DP count, M2DP intensity.
        idx: GLOBAL DB rows [m,k] as match() returns them; db_row0: the first global row of this matcher's shard.  Entries outside
        [db_row0, db_row0 + n) come back -1 / NaN, so with the DB row-sharded exactly one shard fills each pair: combine the shards'
        results with torch.maximum on the variants (torch.fmax on the distances).  Stream-ordered, no host synchronisation."""
        assert all(d.db_sig is not None and d._q_sig is not None for d in self.descs), "match() first"
        idx = idx.to(torch.int32).contiguous()
        m, k = idx.shape
        assert m == self._m
        if self.plain:
            raw = _raw_rows(self)
            v1 = torch.empty((m, k), dtype=torch.int32, device=self.dev)
            d1 = torch.empty((m, k), dtype=torch.float64, device=self.dev)
            self._enter()
            self.ctx.check(self.lib.pr_delight_align_pairs_dev(self.ctx.h, *raw, m, self.n, int(db_row0), k, _dptr(idx), _dptr(v1), _dptr(d1)))
            self._leave()
            return (torch.stack([v1, torch.full_like(v1, -1)], -1), torch.stack([d1, torch.full_like(d1, float("nan"))], -1))
        raw6 = self._raw6()
        var = torch.empty((m, k, 4), dtype=torch.int32, device=self.dev)
        dist = torch.empty((m, k, 4), dtype=torch.float64, device=self.dev)
        self._enter()
        self.ctx.check(self.lib.pr_align_pairs_dev(self.ctx.h, *raw6, m, self.n, int(db_row0), k, _dptr(idx), _dptr(var), _dptr(dist)))
        self._leave()
        ch = slice(0 if raw6[0] is not None else 2, 4 if raw6[3] is not None else 2)     # the channels of the matcher's descriptor types
        return var[..., ch], dist[..., ch]

    def evaluate(self, idx: torch.Tensor, score: torch.Tensor, gt1: torch.Tensor, gt2: torch.Tensor, loop_diff: float, mask_width: int = 0,
                 out=None):
        """run_test.m:3-22 + :58-85 of a match()'s (idx, score) (their [m, k] tensors as returned: column 0 is read in place) on this
        matcher's context and stream, without read-back: eval.precision_recall_torch's dict of device tensors."""
        from . import eval as _eval
        self._enter()
        res = _eval.precision_recall_torch(score, idx, gt1, gt2, loop_diff, mask_width, ctx=self.ctx, out=out)
        self._leave()
        return res

    def verify(self, idx: torch.Tensor, clouds_q, clouds_db, frames_q, frames_db, max_src_pts: int, max_dst_pts: int, max_corr: float = 1.0,
               min_fitness: float = 0.5, max_rmse: float = 0.5, max_iter: int = 30, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6,
               min_inliers: int = 3, db_row0: int = 0, search: str | None = None):
        """Use a match (api.verify_matches on this matcher's context and stream): align(idx) -> pr_sc_relative_pose -> pr_icp_pairs_dev for
        every (query q of the last match(), DB row idx[q, j]).  clouds_q / clouds_db: (xyz float64 [*, 3], offs int64 [N + 1]) device
        tensors, cloud q of clouds_q = query q, cloud r of clouds_db = DB row db_row0 + r; frames_q [m, 16] / frames_db [n, 16] their PCA
        frames (device tensors or arrays); max_src_pts / max_dst_pts: the largest query / DB cloud.  Returns device tensors (T float64
        [m, k, 3, 4], stats uint8 [m, k, 32] - api.ICP_STATS on the host -, accepted bool [m, k]).  The seed is host code
        (pr_sc_relative_pose): the variants are read back once; the refinement itself is stream-ordered.  SC only: only SC has a pose.
        search: None | "brute" | "grid", the ICP correspondence search of this call (api.icp_search)."""
        from . import api
        assert getattr(self, "type", None) == _lib.TYPE_SC, "verify() needs an SC matcher: only SC has a relative pose"
        var, _ = self.align(idx, db_row0)
        m, k = idx.shape
        v = var[..., 0].reshape(-1).cpu().numpy()
        ix = idx.reshape(-1).cpu().numpy().astype(np.int64) - int(db_row0)
        has = (v >= 0) & (ix >= 0)
        fq = frames_q.cpu().numpy() if torch.is_tensor(frames_q) else np.asarray(frames_q)
        fd = frames_db.cpu().numpy() if torch.is_tensor(frames_db) else np.asarray(frames_db)
        src = np.where(has, np.repeat(np.arange(m), k), -1).astype(np.int32)
        dst = np.where(has, ix, -1).astype(np.int32)
        T0 = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (m * k, 1, 1))
        if has.any():
            T0[has] = api.sc_relative_pose(fq[src[has]], fd[dst[has]], v[has])
        dT0, dsrc, ddst = (torch.from_numpy(a).to(self.dev) for a in (T0, src, dst))
        self._enter()
        T, stats = api.icp_refine_torch(clouds_q[0], clouds_q[1], clouds_db[0], clouds_db[1], dsrc, ddst, dT0, max_src_pts, max_dst_pts, max_iter,
                                        max_corr, tol_rmse, tol_fitness, min_inliers, ctx=self.ctx, search=search)
        self._leave()
        f64 = stats.view(torch.float64)                    # [c, 4]: fitness, rmse, (n_inl, iters), (status, pad)
        status = stats.view(torch.int32)[:, 6]
        accepted = ((status == _lib.ICP_CONVERGED) | (status == _lib.ICP_MAX_ITER)) & (f64[:, 0] >= min_fitness) & (f64[:, 1] <= max_rmse)
        return T.view(m, k, 3, 4), stats.view(m, k, -1), accepted.view(m, k)

    def verify_dev(self, idx: torch.Tensor, clouds_q, clouds_db, frames_q: torch.Tensor, frames_db: torch.Tensor, max_src_pts: int,
                   max_dst_pts: int, hypotheses: int = 1, seed: str | None = None, max_corr: float = 1.0, min_fitness: float = 0.5,
                   max_rmse: float = 0.5, max_iter: int = 30, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3,
                   db_row0: int = 0, out=None, search: str | None = None):
        """verify() without leaving the stream, for every type with variants: align(idx) -> pr_verify_pairs_dev (seed, ICP, choice of the
        hypothesis) with the device tensors as they are - no read-back, no host arithmetic, capturable once an eager call has covered the
        shapes.  clouds_q / clouds_db, max_src_pts / max_dst_pts, the ICP parameters and the thresholds as verify() takes them; frames_q
        [m, 16] / frames_db [n, 16] float64 device tensors: the PCA frames of the clouds this matcher's descriptors were generated from.
        hypotheses = 2 also refines the second channel's variant where it differs from the first's (SC: intensity, M2DP: intensity) and
        keeps the better result; DELIGHT has one variant per pair.  A FusedMatcher chooses the seeding descriptor with seed = "sc" | "m2dp".
        Returns device tensors (T float64 [m, k, 3, 4], stats uint8 [m, k, 32], accepted bool [m, k], hyp int32 [m, k]: the kept
        hypothesis); out: an earlier call's tuple, written again.  search: None | "brute" | "grid", the ICP correspondence search of this
        call (api.icp_search); the context's mode is what it was afterwards.
        clouds_db may be an api.KeyframeMap (with frames_db = None and max_dst_pts = None): the call is then KeyframeMap.verify_dev - the
        map's clouds and frames at their fixed addresses, idx = rows of the map."""
        from . import api
        if isinstance(clouds_db, api.KeyframeMap):
            if frames_db is not None or max_dst_pts is not None or db_row0 != 0:
                raise ValueError("verify_dev: a KeyframeMap brings its frames and bounds: frames_db=None, max_dst_pts=None, db_row0=0")
            return clouds_db.verify_dev(self, idx, clouds_q, frames_q, max_src_pts, hypotheses=hypotheses, seed=seed, max_corr=max_corr,
                                        min_fitness=min_fitness, max_rmse=max_rmse, max_iter=max_iter, tol_rmse=tol_rmse, tol_fitness=tol_fitness,
                                        min_inliers=min_inliers, out=out, search=search)
        seed, var, idx = self._verify_variants(idx, hypotheses, seed, db_row0)
        self._enter()
        res = api.verify_pairs_torch(seed, clouds_q, clouds_db, frames_q, frames_db, idx, var, max_src_pts, max_dst_pts, hypotheses, db_row0,
                                     max_corr, min_fitness, max_rmse, max_iter, tol_rmse, tol_fitness, min_inliers, ctx=self.ctx, out=out,
                                     search=search)
        self._leave()
        return res

    def _verify_variants(self, idx: torch.Tensor, hypotheses: int, seed: str | None, db_row0: int):
        """What verify_dev hands to the verify chain: (the seeding descriptor's name, align(idx)'s variants of that descriptor, idx as
        contiguous int32)."""
        names = {_lib.TYPE_SC: "sc", _lib.TYPE_M2DP: "m2dp", _lib.TYPE_DELIGHT: "delight"}
        have = [names[d.type] for d in self.descs if d.type in names]
        if seed is None and len(have) == 1:
            seed = have[0]
        if seed not in have:
            raise ValueError(f"verify_dev: seed must name one of this matcher's descriptor types {have} (a FusedMatcher needs it), not {seed!r}")
        if hypotheses not in (1, 2) or (hypotheses == 2 and seed == "delight"):
            raise ValueError("verify_dev: hypotheses is 1 or 2, and 1 for DELIGHT (one variant per pair)")
        var, _ = self.align(idx, db_row0)
        if var.shape[-1] == 4 and seed == "m2dp":
            var = var[..., 2:]
        return seed, var, idx.to(torch.int32).contiguous()

    def flagged_count(self) -> int:
        """Queries the last match(..., exact_order=False) of ONE rank left flagged by the order / containment checks (the ones the default
        match() answers from their exact rows).  Synchronises (pr_order_flagged_count); 0 once a resolving call has taken the flags."""
        cnt = C.c_int32(0)
        self._enter()
        self.ctx.check(self.lib.pr_order_flagged_count(self.ctx.h, int(self._m), C.byref(cnt)))
        self._leave()
        return int(cnt.value)

    def take_warnings(self) -> int:
        """PR_WARN_* bits of the context since the last call (synchronises its stream): WARN_ORDER_RESOLVED after a match() whose order
        needed fp64 row statistics (WARN_ORDER_UNRESOLVED: only when exact_moments(.., last=True) was called with flagged queries left)."""
        return self.ctx.take_warnings()


class Matcher(_Base):
    def __init__(self, type_: str, max_queries: int, max_db: int, ctx: Context | None = None, device: int | None = None):
        self.type = {"sc": _lib.TYPE_SC, "m2dp": _lib.TYPE_M2DP, "delight": _lib.TYPE_DELIGHT}[type_]
        self.rows_per_sig, self.sig_len = {_lib.TYPE_SC: (1, 2400), _lib.TYPE_M2DP: (4, 384), _lib.TYPE_DELIGHT: (16, 256)}[self.type]
        self.plain = self.type == _lib.TYPE_DELIGHT      # one distance matrix, no z-score fusion (run_test.m:26-36)
        self._init_ctx(ctx, device)
        self._spec = (type_, max_queries, max_db)
        self.q = C.c_void_p()
        self.db = C.c_void_p()
        self.ctx.check(self.lib.pr_sigset_create(self.ctx.h, self.type, _lib.ROLE_QUERY, max_queries, C.byref(self.q)))
        self.ctx.check(self.lib.pr_sigset_create(self.ctx.h, self.type, _lib.ROLE_DB, max_db, C.byref(self.db)))
        self.max_queries, self.max_db = max_queries, max_db
        self.n = 0
        self.db_sig = None             # the raw DB shard (the fp64 re-evaluation reads it)
        self._q_sig = None             # the raw queries of the last local_phase1()
        self.pre_distances = None      # optional callables (e.g. HIP event records) around the distance launch
        self.post_distances = None

    @property
    def descs(self):                   # (a property: an attribute holding self would make every matcher a reference cycle)
        return (self,)

    def close(self):
        super().close()
        if self.q:
            self.lib.pr_sigset_destroy(self.ctx.h, self.q)
            self.lib.pr_sigset_destroy(self.ctx.h, self.db)
            self.q = self.db = None

    def _pack(self, handle, sig: torch.Tensor):
        assert sig.is_cuda and sig.is_contiguous() and sig.dim() == 2 and sig.shape[1] == self.sig_len
        assert sig.shape[0] % self.rows_per_sig == 0
        n = sig.shape[0] // self.rows_per_sig
        self.ctx.check(self.lib.pr_sigset_pack(self.ctx.h, handle, _dptr(sig), _torch_dt(sig), _lib.DEVICE, n))
        return n

    def pack_database(self, sig: torch.Tensor):
        """processSC.m:18-20 (normalise hist2) + operand layout; sig: device [n(*4), sig_len] f64/f32 (kept: the
        re-evaluation of the selected pairs reads the raw rows)."""
        self._enter()
        self.n = self._pack(self.db, sig)
        self.db_sig = sig
        self._raw = None

    def reserve_database(self, sig: torch.Tensor | None = None):
        """A DB that grows (SC/test_sc.cpp:40-56: one signature per keyframe): the operand image is laid out for the matcher's CAPACITY
        (pr_sigset_reserve) and the raw rows live in a capacity-sized buffer of the matcher, so append_database() adds rows in place - no
        re-pack, no re-upload.  sig (optional): the rows to start with, device [n(*4), sig_len] f64."""
        assert self.type in (_lib.TYPE_SC, _lib.TYPE_M2DP)
        self._enter()
        self.ctx.check(self.lib.pr_sigset_reserve(self.ctx.h, self.db))
        self._raw = torch.empty((self.max_db * self.rows_per_sig, self.sig_len), dtype=torch.float64, device=self.dev)
        self.n = 0
        if sig is not None and sig.shape[0]:
            assert sig.dtype == torch.float64
            r = sig.shape[0]
            self._raw[:r].copy_(sig)
            self._enter()
            self.n = self._pack(self.db, self._raw[:r])
        self.db_sig = self._raw[:self.n * self.rows_per_sig]       # (a view: the same storage as the rows appended later)

    def append_database(self, sig: torch.Tensor):
        """Rows [n, n + n_new) of the growing DB: the raw rows into the matcher's buffer, their operand rows into the image
        (pr_sigset_append: one kernel, bit for bit what a pack of all rows would write there)."""
        assert self._raw is not None, "reserve_database() first"
        assert sig.is_cuda and sig.dim() == 2 and sig.shape[1] == self.sig_len and sig.dtype == torch.float64 and sig.shape[0] % self.rows_per_sig == 0
        k, r0 = sig.shape[0] // self.rows_per_sig, self.n * self.rows_per_sig
        assert self.n + k <= self.max_db
        dst = self._raw[r0:r0 + sig.shape[0]]
        dst.copy_(sig)
        self._enter()                                              # (the copy above is torch's: ordered in front of the library's kernel)
        self.ctx.check(self.lib.pr_sigset_append(self.ctx.h, self.db, _dptr(dst), 0, _lib.DEVICE, k))
        self.n += k
        self.db_sig = self._raw[:self.n * self.rows_per_sig]       # (a new view object: a split-f16 twin of the f16 arithmetic is re-packed when next needed)

    def local_phase1(self, queries: torch.Tensor, moments: bool = True):
        """pack(q) + distances + row moments of this shard -> moments [m, 2, 3] f64 (zeros for DELIGHT).
        moments=False: the returned buffer is left for local_select(with_moments=True) to fill."""
        self._enter()
        m = self._pack(self.q, queries)
        n = self.n
        self._q_sig, self._m = queries, m
        d_p = self._buf("d_p", (m, n), torch.float32)
        d_i = None if self.plain else self._buf("d_i", (m, n), torch.float32)
        mom = self._buf("mom", (m, 2, 3), torch.float64)
        lib, h = self.lib, self.ctx.h
        if self.pre_distances:
            self.pre_distances()
        self.ctx.check(lib.pr_distances_dev(h, self.q, self.db, _dptr(d_p), _dptr(d_i)))
        if self.post_distances:
            self.post_distances()
        if self.plain:
            self._leave()
            mom.zero_()
        else:
            if moments:
                self.ctx.check(lib.pr_row_moments_dev(h, _dptr(d_p), _dptr(d_i), m, n, _dptr(mom)))
            self._leave()
        return mom

    def match(self, queries: torch.Tensor, mask_width: int = 0, p_weight: float = 2.0, k: int = 1,
              db_row0: int = 0, q_row0: int = 0, group=None, force_exchange: bool = False, f16_fallback: bool = True,
              exact_order: bool = True, mark=None):
        """Returns (idx int32 [m,k] GLOBAL DB row indices, score float64 [m,k]) as device tensors.
        force_exchange: run the all-gathers and the merge even with one rank (measures the protocol's overhead).
        exact_order (default): queries whose re-evaluated order is not certain under the fp32 pass's row sigmas, or whose k + 8 candidates
        do not provably hold the top-k of the whole row, are answered from their exact fp64 rows, sharded or not (run_test.m:38-57 are fp64
        over the whole row), 64 flagged queries per pass: a call of up to 64 queries runs one pass of stream-ordered kernels that leave at
        once when nothing is flagged (no host synchronisation: such a call can be captured in a hipGraph); a larger call reads the
        number of flagged queries back (one synchronisation) and runs the passes it takes.  "async": ceil(m / 64) such passes chained on the
        stream whatever was flagged (no read-back: what a captured graph of a large call uses; empty passes leave at once);
        False skips the resolution (the answer of the re-evaluated candidate list; the flags are simply dropped)."""
        return self._match((queries,), mask_width, p_weight, k, db_row0, q_row0, group, force_exchange, f16_fallback, exact_order, mark)

    def match_sequence(self, queries: torch.Tensor, steps, mask_width: int = 0, p_weight: float = 2.0, k: int = 1, db_row0: int = 0,
                       q_row0: int = 0, dense: bool = False):
        """Sequence matching (pr_seq_select_dev): `queries` are consecutive keyframes of a drive; local_phase1() and then
        the trajectory-summed selection over this matcher's own distance matrices.  steps: api.seq_steps(L, velocities), a NumPy table
        or a CUDA i32 [V, L] tensor (uploaded once per call otherwise).  Returns (idx i32 [m, k] GLOBAL DB rows, score f64 [m, k],
        vel i32 [m, k][, S f64 [m, n] with dense=True]) device tensors; evaluate() takes idx and score as they are.  One shard only:
        the lags do not cross query shards and there is no sharded form."""
        from . import api
        if not (torch.is_tensor(steps) and steps.is_cuda):
            steps = torch.from_numpy(api._check_steps(steps, "Matcher.match_sequence")).to(self.dev)
        mom = self.local_phase1(queries)
        d_p, d_i = self.distances()
        self._enter()
        out = api.seq_select_torch(d_p, d_i, None if self.plain else mom, steps, q_row0, db_row0, mask_width, p_weight, k, dense=dense, ctx=self.ctx)
        self._leave()
        return out

    def distances(self):
        """The last distance matrices (device, float32 [m, n_local])."""
        return self._bufs["d_p"], self._bufs.get("d_i")

    @classmethod
    def on_new_stream(cls, type_: str, max_queries: int, max_db: int, device: int | None = None):
        """A matcher whose library context lives on a stream of its own (`.stream`): what hipGraph capture needs (the null
        stream cannot be captured).  Use it under `with torch.cuda.stream(mt.stream):`."""
        return _on_new_stream(cls, device, type_, max_queries, max_db)

    def capture(self, queries: torch.Tensor, mask_width: int = 0, p_weight: float = 2.0, k: int = 1):
        """Captures one single-rank match() of the STATIC tensor `queries` against the resident, packed DB into a hipGraph
        (online use: one keyframe per call - the ~10 kernel launches of a call replay as one graph launch).  Returns a
        CapturedMatch: `.run(new_queries)` copies them into the static input and replays ON THE MATCHER'S STREAM (a replay
        on another stream would not be ordered with the copy), `.idx` / `.score` are the static outputs.  The matcher must
        come from on_new_stream().  A graph cannot read a count back: calls above 64 queries are captured with exact_order="async" (ceil(m / 64)
        chained passes: every flagged query of every replay is resolved)."""
        st = self.stream
        eo = True if queries.shape[0] // self.rows_per_sig <= RESOLVE_SLOTS else "async"
        with torch.cuda.stream(st):
            assert self.ctx.stream == int(st.cuda_stream)
            self.match(queries, mask_width, p_weight, k, exact_order=eo)            # warm-up: allocates every buffer the call uses
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                idx, score = self.match(queries, mask_width, p_weight, k, exact_order=eo)
        return CapturedMatch(g, st, queries, idx, score)


class CapturedMatch:
    """A match() call as a hipGraph (Matcher.capture)."""

    def __init__(self, graph, stream, queries, idx, score):
        self.graph, self.stream, self.queries, self.idx, self.score = graph, stream, queries, idx, score

    check = None          # optional callable run before a replay (BowMatcher.capture: raises once the graph is stale)

    def run(self, new_queries: torch.Tensor | None = None, sync: bool = True):
        if self.check is not None:
            self.check()
        if new_queries is not None:
            self.stream.wait_stream(torch.cuda.current_stream(new_queries.device))   # whoever produced new_queries did it there
            new_queries.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            if new_queries is not None:
                self.queries.copy_(new_queries, non_blocking=True)
            self.graph.replay()
        if sync:
            self.stream.synchronize()
        return self.idx, self.score


class FusedMatcher(_Base):
    """BASELINE.json config 5 ("fused SC + M2DP scoring", build-defined: DESIGN.md §7): an SC and an M2DP matcher over the
    same places; the four row z-scores are added (weights p, 1, p, 1) in ONE top-k pass (pr_fuse_select2_dev).  Shards like
    Matcher: the moments of both descriptor types travel in the same all_gather ([m, 4, 3] f64 per rank)."""

    def __init__(self, max_queries: int, max_db: int, ctx: Context | None = None, device: int | None = None):
        self._init_ctx(ctx, device)
        self._spec = (max_queries, max_db)
        self.sc = Matcher("sc", max_queries, max_db, self.ctx)
        self.m2 = Matcher("m2dp", max_queries, max_db, self.ctx)
        self.descs = (self.sc, self.m2)

    def close(self):
        super().close()
        self.sc.close(); self.m2.close()

    def pack_database(self, sc_sig: torch.Tensor, m2dp_sig: torch.Tensor):
        self.sc.pack_database(sc_sig); self.m2.pack_database(m2dp_sig)
        assert self.sc.n == self.m2.n, "the two databases must describe the same places"
        self.n = self.sc.n

    def local_phase1(self, sc_queries, m2dp_queries):
        a = self.sc.local_phase1(sc_queries)
        b = self.m2.local_phase1(m2dp_queries)
        assert self.sc._m == self.m2._m
        self._m = self.sc._m
        return torch.cat([a, b], dim=1)                                    # [m, 4, 3]

    def match(self, sc_queries: torch.Tensor, m2dp_queries: torch.Tensor, mask_width: int = 0, p_weight: float = 2.0, k: int = 1,
              db_row0: int = 0, q_row0: int = 0, group=None, f16_fallback: bool = True, exact_order: bool = True):
        return self._match((sc_queries, m2dp_queries), mask_width, p_weight, k, db_row0, q_row0, group, False, f16_fallback, exact_order, None)


def _on_new_stream(cls, device, *args, **kw):
    """cls(*args, **kw) with a library context on a stream of its own (`.stream`): what hipGraph capture needs (the null stream cannot
    be captured)."""
    device = torch.cuda.current_device() if device is None else device
    st = torch.cuda.Stream(device)
    with torch.cuda.stream(st):
        mt = cls(*args, ctx=_stream_context(device), **kw)
    mt.stream = st
    return mt


class _ResidentMatcher(_Base):
    """What the matchers over a device-resident exact database (pr_<_kind>_db: BoW, GIST, DELIGHT) share: the DB grows in place and shards
    like Matcher's plain path - every rank holds rows [db_row0, db_row0 + n) and all queries, returns its own top-k by GLOBAL row, the
    lists are merged by pr_merge_topk_dev.  A subclass gives _kind (the C prefix), _name (its name in messages), _rows() (the shape rule
    of its row tensors -> signatures) and an __init__ that creates self.db and ends with _start()."""
    plain = True
    _kind = _name = None

    def _fn(self, name: str):
        return getattr(self.lib, f"pr_{self._kind}_{name}")

    def _start(self):
        self.n = 0
        self._q_sig = None
        self.generation = 0            # counts set / append calls: a captured match is valid for the generation it was captured at

    @property
    def descs(self):
        return (self,)

    def close(self):
        super().close()
        if self.db:
            self._fn("db_destroy")(self.ctx.h, self.db)
            self.db = None

    def _load(self, fn: str, rows: torch.Tensor):
        n = self._rows(rows)
        self._enter()
        self.generation += 1
        self.ctx.check(self._fn(fn)(self.ctx.h, self.db, _dptr(rows), _lib.DEVICE, n))
        self.n = int(self._fn("db_count")(self.db))

    def pack_database(self, rows: torch.Tensor):
        """Replaces the DB with `rows` (pr_<kind>_db_set: synchronises; BoW builds its index and raises PRError naming the first
        non-conforming row)."""
        self._load("db_set", rows)

    def reserve_database(self, rows: torch.Tensor | None = None):
        """A DB that grows: the capacity is there from construction, so this only starts it (empty, or with `rows`)."""
        if rows is None:
            rows = torch.empty((0, self.cols), dtype=torch.float64, device=self.dev)
        self.pack_database(rows)

    def append_database(self, rows: torch.Tensor):
        """Rows [n, n + n_new) (pr_<kind>_db_append; synchronises.  BoW: the tail's lists, or a fold of a full tail)."""
        self._load("db_append", rows)

    def local_phase1(self, queries: torch.Tensor):
        """The plain path has no row statistics: zero moments [m, 2, 3]."""
        m = self._rows(queries)
        assert m <= self.max_queries
        self._q_sig, self._m = queries, m
        return torch.zeros((m, 2, 3), dtype=torch.float64, device=self.dev)

    def local_select(self, mom_all, G, mask_width, p_weight, k, db_row0, q_row0):
        """This shard's top-k (idx int32 [m, k] global rows, score float64 [m, k]) - pr_<kind>_match_topk_dev."""
        m = self._m
        idx = torch.empty((m, k), dtype=torch.int32, device=self.dev)
        score = torch.empty((m, k), dtype=torch.float64, device=self.dev)
        self._enter()
        self.ctx.check(self._fn("match_topk_dev")(self.ctx.h, self.db, _dptr(self._q_sig), m, int(q_row0), int(db_row0), int(mask_width),
                                                  int(k), _dptr(idx), _dptr(score)))
        self._leave()
        return idx, score

    def match(self, queries: torch.Tensor, mask_width: int = 0, k: int = 1, db_row0: int = 0, q_row0: int = 0, group=None,
              force_exchange: bool = False, mark=None):
        """(idx int32 [m,k] GLOBAL DB rows, score float64 [m,k]) device tensors; no host synchronisation.  BoW: a non-conforming query
        row gets -1 / NaN and raises _lib.WARN_BOW_ROWS (take_warnings)."""
        G = _world(group)
        return sharded_topk(lambda: self.local_phase1(queries),
                            lambda mom_all, G_: self.local_select(mom_all, G_, mask_width, 0.0, k, db_row0, q_row0),
                            k, group if (G > 1 or force_exchange) else None, G, merge=self.merge, force_exchange=force_exchange, mark=mark)

    def capture(self, queries: torch.Tensor, mask_width: int = 0, k: int = 1, db_row0: int = 0, q_row0: int = 0):
        """One single-rank match() of the STATIC tensor `queries` as a hipGraph (CapturedMatch; the matcher must come from on_new_stream).
        The graph holds the DB's row count (BoW: and index buffers) as they were at capture; pack_database / append_database change them
        (a BoW append rebuilds the tail lists with rows the graph does not know, a fold swaps the main buffers), so after either the graph
        must be captured again: its run() raises RuntimeError instead of replaying it."""
        st = self.stream
        with torch.cuda.stream(st):
            assert self.ctx.stream == int(st.cuda_stream)
            self.match(queries, mask_width, k, db_row0, q_row0)
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                idx, score = self.match(queries, mask_width, k, db_row0, q_row0)
        cap = CapturedMatch(g, st, queries, idx, score)
        gen, mt, name = self.generation, weakref.ref(self), self._name

        def valid():
            m_ = mt()
            if m_ is None or m_.db is None or m_.generation != gen:
                raise RuntimeError(f"{name}.capture: the database changed (or was closed) since this graph was captured; capture again")
        cap.check = valid
        return cap


class _TwoStageMatcher(_ResidentMatcher):
    """GIST and DELIGHT: a coarse pass lists candidates, their distances are re-evaluated in fp64, and a query whose list is not provably
    complete is answered from its exact row (csrc/resident_match.hpp)."""

    @property
    def device_bytes(self) -> int:
        """Device memory the database holds, scratch included (all of it allocated at construction)."""
        return int(self._fn("db_bytes")(self.db))

    def set_exact(self, on: bool):
        self._fn("db_set_exact")(self.db, 1 if on else 0)

    def flagged_count(self) -> int:
        """Queries of the last match() that were answered from their exact row (synchronises)."""
        c = C.c_int32(0)
        self._enter()
        self.ctx.check(self._fn("flagged_count")(self.ctx.h, int(self._m), C.byref(c)))
        return int(c.value)


class BowMatcher(_ResidentMatcher):
    """BoW (processBoW.m + run_test.m:47-57) against a device-resident inverted file (pr_bow_db): scores are the reference's fp64 values
    bit for bit and the order is its double-precision order, for conforming rows (include/place_recognition.h).  The DB grows in place
    (append_database: a tail segment folded into the main lists when full) and shards like Matcher's plain path: every rank holds rows
    [db_row0, db_row0 + n) and all queries, returns its own top-k by GLOBAL row, the lists are merged by pr_merge_topk_dev.
    Rows: float64 device tensors [2 n, cols] (ids | weights per image, as bow_generate_torch writes them; taken without a copy).
    max_postings: words over all DB rows the index can hold (default max_db * (cols - 1), every row full)."""
    _kind, _name = "bow", "BowMatcher"

    def __init__(self, max_queries: int, max_db: int, cols: int, n_words: int, ctx: Context | None = None, device: int | None = None,
                 max_postings: int | None = None):
        self._init_ctx(ctx, device)
        self._spec = (max_queries, max_db, cols, n_words)
        self.max_queries, self.max_db, self.cols, self.n_words = max_queries, max_db, cols, n_words
        self.rows_per_sig, self.sig_len = 2, cols
        self.db = C.c_void_p()
        mp = max_db * max(cols - 1, 0) if max_postings is None else int(max_postings)
        self.ctx.check(self.lib.pr_bow_db_create(self.ctx.h, int(max_db), int(cols), int(n_words), int(mp), C.byref(self.db)))
        self._start()

    def _rows(self, rows: torch.Tensor) -> int:
        if not (rows.is_cuda and rows.dtype == torch.float64 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == self.cols
                and rows.shape[0] % 2 == 0):
            raise ValueError(f"BoW rows must be a contiguous float64 CUDA tensor [2 n, {self.cols}]")
        return rows.shape[0] // 2

    @classmethod
    def on_new_stream(cls, max_queries: int, max_db: int, cols: int, n_words: int, device: int | None = None, **kw):
        """A matcher whose library context lives on a stream of its own (`.stream`), as capture() needs."""
        return _on_new_stream(cls, device, max_queries, max_db, cols, n_words, **kw)


class GistMatcher(_TwoStageMatcher):
    """GIST (processGIST.m + run_test.m:47-57) against a device-resident database (pr_gist_db): indices and fp64 score bits are the
    reference's double-precision answer for every input.  A coarse pass on the f16 matrix cores lists candidates, their distances are
    re-evaluated in fp64, and a query whose list is not provably complete is answered from its exact row.  The DB grows
    in place and shards like BowMatcher: every rank holds rows [db_row0, db_row0 + n) and all queries, the lists are merged by
    pr_merge_topk_dev.  Rows: float64 device tensors [n, cols], as gist_generate_torch writes them (taken without a copy).
    exact=True (or PR_GIST_EXACT=1): every query takes the exact-row path."""
    _kind, _name = "gist", "GistMatcher"

    def __init__(self, max_queries: int, max_db: int, cols: int, ctx: Context | None = None, device: int | None = None, exact: bool = False):
        if min(int(max_queries), int(max_db), int(cols)) < 1:
            raise ValueError("GistMatcher: max_queries, max_db and cols must be >= 1")
        self._init_ctx(ctx, device)
        self._spec = (max_queries, max_db, cols)
        self.max_queries, self.max_db, self.cols = max_queries, max_db, cols
        self.rows_per_sig, self.sig_len = 1, cols
        self.db = C.c_void_p()
        self.ctx.check(self.lib.pr_gist_db_create(self.ctx.h, int(max_db), int(cols), C.byref(self.db)))
        if exact:
            self.set_exact(True)
        self._start()

    def _rows(self, rows: torch.Tensor) -> int:
        if not (rows.is_cuda and rows.dtype == torch.float64 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == self.cols):
            raise ValueError(f"GIST rows must be a contiguous float64 CUDA tensor [n, {self.cols}]")
        return rows.shape[0]

    @classmethod
    def on_new_stream(cls, max_queries: int, max_db: int, cols: int, device: int | None = None, **kw):
        """A matcher whose library context lives on a stream of its own (`.stream`), as capture() needs."""
        return _on_new_stream(cls, device, max_queries, max_db, cols, **kw)


class DelightMatcher(_TwoStageMatcher):
    """DELIGHT (processDELIGHT.m + run_test.m:47-57) against a device-resident database (pr_delight_db): indices and fp64 score bits are
    the reference's double-precision answer for every input.  A coarse fp32 pass lists candidates without an m x n matrix, their
    distances are re-evaluated in fp64, and a query whose list is not provably complete is answered from its exact row.
    The DB grows in place and shards like GistMatcher: every rank holds signatures [db_row0, db_row0 + n) and all queries, the lists are
    merged by pr_merge_topk_dev.  Rows: float64 device tensors [16 n, 256], as delight_generate_torch writes them (taken without a copy).
    exact=True (or PR_DELIGHT_EXACT=1): every query takes the exact-row path."""
    _kind, _name = "delight", "DelightMatcher"

    def __init__(self, max_queries: int, max_db: int, ctx: Context | None = None, device: int | None = None, exact: bool = False):
        if min(int(max_queries), int(max_db)) < 1:
            raise ValueError("DelightMatcher: max_queries and max_db must be >= 1")
        self._init_ctx(ctx, device)
        self._spec = (max_queries, max_db)
        self.max_queries, self.max_db, self.cols = max_queries, max_db, 256
        self.rows_per_sig, self.sig_len = 16, 256
        self.db = C.c_void_p()
        self.ctx.check(self.lib.pr_delight_db_create(self.ctx.h, int(max_db), C.byref(self.db)))
        if exact:
            self.set_exact(True)
        self._start()

    def _rows(self, rows: torch.Tensor) -> int:
        if not (rows.is_cuda and rows.dtype == torch.float64 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == 256
                and rows.shape[0] % 16 == 0):
            raise ValueError("DELIGHT rows must be a contiguous float64 CUDA tensor [16 n, 256]")
        return rows.shape[0] // 16

    @classmethod
    def on_new_stream(cls, max_queries: int, max_db: int, device: int | None = None, **kw):
        """A matcher whose library context lives on a stream of its own (`.stream`), as capture() needs."""
        return _on_new_stream(cls, device, max_queries, max_db, **kw)



def _world(group) -> int:
    import torch.distributed as dist
    return dist.get_world_size(group) if (group is not None or (dist.is_available() and dist.is_initialized())) else 1


def sharded_topk(local_moments, local_select, k: int, group, G: int, merge=None, force_exchange: bool = False, rerank=None, finish=None,
                 post=None, resolve=None, mark=None):
    """The exchange protocol of SURVEY.md §8-e around two local callables (HIP in production; a numpy stand-in in
    the gloo CPU tests): moments -> all_gather -> select with the moments of all shards -> all_gather -> merge.
    resolve (optional, step 7): (moments(offset, last), select(exact_all, k, offset), merge(sel_all, k, idx, score, offset), passes()).
    mark (optional): called with a phase name after every phase of the protocol has been ENQUEUED (bench.py records an event on the
    stream there: the per-rank phase times of a step)."""
    import torch.distributed as dist
    mark = mark or (lambda name: None)
    mom = local_moments()
    mark("pack+distances+moments")
    if G == 1 and not force_exchange:
        idx_in, sc = local_select(mom.unsqueeze(0) if mom.dim() == 3 else mom, 1)
        mark("select")
        if rerank is None:
            return idx_in, sc
        idx, score = rerank(idx_in, k, False, sc)
        mark("rerank")
        if post is not None:                             # PR_SC_ARITH_F16: margin flags of the candidate list (no synchronisation)
            post(sc, idx, score)
        return idx, score
    stage_on_host = dist.get_backend(group) == "gloo"   # gloo has no device all_gather: used by the single-GPU tests

    def gather(t):   # output = the ranks' tensors concatenated along dim 0, viewed as [G, ...]
        src = t.contiguous()
        if stage_on_host and src.is_cuda:
            src = src.cpu()
        out = torch.empty((G * src.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        dist.all_gather_into_tensor(out, src, group=group)   # nccl: RCCL, on the stream the library's kernels run on
        return out.view((G,) + tuple(src.shape)).to(t.device)

    mom_all = gather(mom)
    mark("all_gather A (moments)")
    idx_in, sc = local_select(mom_all, G)
    mark("select")
    kin = idx_in.shape[1]
    idx_all, sc_all = gather(idx_in), gather(sc)
    mark("all_gather B (candidates)")
    do_merge = merge if (merge is not None and idx_all.is_cuda) else merge_topk
    if rerank is None:                                   # nothing to re-evaluate (numpy stand-ins of the gloo tests, DELIGHT)
        return do_merge(idx_all, sc_all, k)
    cand_idx, cand_sc = do_merge(idx_all, sc_all, kin)   # the global top-(k+8) of the fp32 pass, identical on every rank
    part = rerank(cand_idx, k, True, cand_sc)
    mark("merge+rerank")
    part_all = gather(part)
    mark("all_gather C (evaluations)")
    idx, score = finish(cand_idx, cand_sc, part_all, k)
    mark("finish+checks")
    if resolve is not None:                              # step 7: the flagged queries from their exact rows (moments, per-shard k best, merge),
        exact_moments, exact_select, exact_merge, passes = resolve
        n_pass = passes()                                # 64 per pass; the same number of passes on every rank
        mark("flagged count")                            # (calls above 64 queries: one read-back of the count; none flagged - no pass)
        for p in range(n_pass):
            off = p * RESOLVE_SLOTS
            ex = exact_moments(off, p == n_pass - 1)
            mark("exact rows")
            exact_all = gather(ex)
            mark("all_gather D (exact moments)")
            sel = exact_select(exact_all, k, off)
            mark("exact select")
            sel_all = gather(sel)
            mark("all_gather E (exact lists)")
            idx, score = exact_merge(sel_all, k, idx, score, off)
            mark("exact merge")
    if post is not None:
        post(cand_sc, idx, score)
    return idx, score


def merge_topk(idx_all: torch.Tensor, sc_all: torch.Tensor, k: int):
    """k-way merge of per-shard top-k lists [G, m, k] by (score, index) ascending; -1 / NaN entries sort last.
    (torch restatement of pr_merge_topk_dev for host tensors: the gloo tests)"""
    G, m, kk = idx_all.shape
    idx = idx_all.permute(1, 0, 2).reshape(m, G * kk).to(torch.int64)
    sc = sc_all.permute(1, 0, 2).reshape(m, G * kk).to(torch.float64)
    bad = (idx < 0) | torch.isnan(sc)
    sc = torch.where(bad, torch.full_like(sc, float("inf")), sc)
    idx_key = torch.where(bad, torch.full_like(idx, 2 ** 62), idx)
    o1 = torch.argsort(idx_key, dim=1, stable=True)
    sc1 = torch.gather(sc, 1, o1)
    bad1 = torch.gather(bad, 1, o1)
    # bad entries after every good one, also after good +Inf scores
    key2 = torch.where(bad1, torch.full_like(sc1, float("inf")), sc1)
    o2 = torch.argsort(key2 + 0.0, dim=1, stable=True)
    o2b = torch.argsort(torch.gather(bad1, 1, o2).to(torch.int8), dim=1, stable=True)
    order = torch.gather(o1, 1, torch.gather(o2, 1, o2b))[:, :k]
    out_idx = torch.gather(idx, 1, order)
    out_sc = torch.gather(sc_all.permute(1, 0, 2).reshape(m, G * kk), 1, order)
    out_bad = torch.gather(bad, 1, order)
    out_idx = torch.where(out_bad, torch.full_like(out_idx, -1), out_idx)
    return out_idx.to(torch.int32), out_sc


def combine_moments(mom_all: np.ndarray):
    """Host restatement of the rank-order Chan combination done inside fuse_select (for tests): [G,m,2,3] -> mean,std."""
    G = mom_all.shape[0]
    cn = np.zeros(mom_all.shape[1:3]); mean = np.zeros_like(cn); m2 = np.zeros_like(cn)
    for g in range(G):
        nb, mb, m2b = mom_all[g, ..., 0], mom_all[g, ..., 1], mom_all[g, ..., 2]
        tot = cn + nb
        delta = mb - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + m2b + delta * delta * (cn * nb / tot)
        cn = tot
    return mean, np.sqrt(m2 / (cn - 1.0))
