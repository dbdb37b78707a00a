"""Registration of matched cloud pairs: pose seeds from the descriptors' variants, ICP refinement and
verification over host arrays and on the stream, and the registration information of a refined pose.  `api` re-exports every name."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._context import Context, default_context
from ._handle import Handle, _ptr, check_each, ptr, result
from ._lib import PRError

__all__ = ["ICP_STATS", "RegInfo", "RegistrationInfo", "icp_accept", "icp_nn", "icp_nn_radius", "icp_refine", "icp_refine_torch", "icp_search",
           "icp_tile_rows", "relative_pose", "relative_pose_torch", "sc_relative_pose", "verify_matches", "verify_pairs_torch"]

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
    from .eval import _on_stream
    ts = (xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0)
    want = (torch.float64, torch.int64, torch.float64, torch.int64, torch.int32, torch.int32, torch.float64)
    dev = xyz_q.device
    check_each("icp_refine_torch: expected contiguous CUDA tensors xyz f64, offs i64, pairs i32, T0 f64", dev, ts, want)
    c = pair_src.numel()
    if pair_dst.numel() != c or T0.numel() != 12 * c:
        raise ValueError("icp_refine_torch: pair_src, pair_dst [c] and T0 [c, 3, 4] disagree")
    o, msg = out or (None, None), "icp_refine_torch: out belongs to another c"
    out = (result(None, None, o[0], torch.float64, (c, 3, 4), dev, msg=msg),
           result(None, None, o[1], torch.uint8, (c, ICP_STATS.itemsize), dev, zeros=True, msg=msg))
    with _on_stream(ctx, dev, ts + tuple(out)) as cx, icp_search(cx, search):
        cx.check(cx.lib.pr_icp_pairs_dev(cx.h, ptr(xyz_q), ptr(offs_q), offs_q.numel() - 1, ptr(xyz_db), ptr(offs_db), offs_db.numel() - 1,
                                         ptr(pair_src), ptr(pair_dst), c, ptr(T0), int(max_src_pts), int(max_dst_pts), int(max_iter),
                                         float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers), ptr(out[0]), ptr(out[1])))
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
    from .eval import _on_stream
    t = _pose_type(type_)
    H = int(hypotheses)
    dev = idx.device
    check_each("relative_pose_torch: expected contiguous CUDA tensors frames f64 [*, 16], idx i32 [m, k]", dev, (frames_q, frames_db, idx),
               (torch.float64, torch.float64, torch.int32))
    m, k = idx.shape
    if frames_q.shape != (m, 16) or frames_db.dim() != 2 or frames_db.shape[1] != 16:
        raise ValueError("relative_pose_torch: frames_q must be [m, 16] and frames_db [n_local, 16]")
    var, stride = _variant_view(variant, m, k, H)
    T0 = torch.empty((m, k, H, 3, 4), dtype=torch.float64, device=dev)
    src = torch.empty((m, k, H), dtype=torch.int32, device=dev)
    dst = torch.empty((m, k, H), dtype=torch.int32, device=dev)
    with _on_stream(ctx, dev, (frames_q, frames_db, idx, var, T0, src, dst)) as cx:
        cx.check(cx.lib.pr_relative_pose_dev(cx.h, t, ptr(frames_q), m, ptr(frames_db), frames_db.shape[0], int(db_row0), k, ptr(idx), ptr(var), stride, H,
                                             ptr(T0), ptr(src), ptr(dst)))
    return T0, src, dst


def _verify_out(out, m, k, dev, who):
    """The result tensors (T, stats, accepted, hyp) of a verify call over [m, k] pairs: new ones, or the checked tuple of an earlier call."""
    import torch
    # (every element is written by the call; torch.empty enqueues nothing on torch's stream that the context's stream could overtake)
    want = ((torch.float64, (m, k, 3, 4)), (torch.uint8, (m, k, ICP_STATS.itemsize)), (torch.bool, (m, k)), (torch.int32, (m, k)))
    return tuple(result(None, None, t, dt, sh, dev, msg=f"{who}: out belongs to another [m, k]") for t, (dt, sh) in zip(out or (None,) * 4, want))


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
    from .eval import _on_stream
    t = _pose_type(type_)
    H = int(hypotheses)
    xq, oq = clouds_q
    xd, od = clouds_db
    ts = (xq, oq, xd, od, frames_q, frames_db, idx)
    want = (torch.float64, torch.int64, torch.float64, torch.int64, torch.float64, torch.float64, torch.int32)
    dev = idx.device
    check_each("verify_pairs_torch: expected contiguous CUDA tensors xyz f64, offs i64, frames f64, idx i32", dev, ts, want)
    m, k = idx.shape
    if frames_q.shape != (m, 16) or frames_db.dim() != 2 or frames_db.shape[1] != 16:
        raise ValueError("verify_pairs_torch: frames_q must be [m, 16] and frames_db [n_local, 16]")
    var, stride = _variant_view(variant, m, k, H)
    out = _verify_out(out, m, k, dev, "verify_pairs_torch")
    with _on_stream(ctx, dev, ts + (var,) + tuple(out)) as cx, icp_search(cx, search):
        cx.check(cx.lib.pr_verify_pairs_dev(cx.h, t, ptr(xq), ptr(oq), oq.numel() - 1, ptr(xd), ptr(od), od.numel() - 1, ptr(frames_q), ptr(frames_db), m,
                                            frames_db.shape[0], int(db_row0), k, ptr(idx), ptr(var), stride, H, int(max_src_pts), int(max_dst_pts),
                                            int(max_iter), float(max_corr), float(tol_rmse), float(tol_fitness), int(min_inliers),
                                            float(min_fitness), float(max_rmse), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])))
    return out


def _host_pairs(who, xyz_q, offs_q, pair_src, T, excl=None):
    """The host form of a pair list over a CSR set of query clouds, checked: (xyz f64 [*, 3], offs i64 [Nq + 1], pair_src i32 [c], c,
    T f64 [c, 3, 4], excl i32 [c, 2] | None) - what the host calls of MapLocalizer, PlaneLocalizer and RegistrationInfo take."""
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


class RegistrationInfo(Handle):
    """pr_reginfo: how well the geometry constrains a registered pose.  Behind a correspondence pass at the pose T that is
    to be judged - icp_nn_radius / icp_nn (point metric) or MapLocalizer.nn_torch (plane metric) - it gives the normal matrix, its
    inverse, the marginal spectra of rotation and translation with their weakest directions, the flags (too few, singular, weak rotation,
    weak translation) and a per-slot (w_rot, w_trans) for PoseGraph.add_weighted_torch.  One allocation at create; every *_torch call is
    enqueued on the context's stream, reads nothing back and can be captured (out= keeps the result's addresses fixed).  pairs_torch and
    maploc_torch run the pass themselves into work tensors the first call for a given c allocates - make that call before a capture."""

    _DESTROY = "pr_reginfo_destroy"

    def __init__(self, ctx: Context | None, pair_capacity: int, max_src_pts: int):
        self._attach(ctx)
        self.pair_capacity, self.max_src_pts = int(pair_capacity), int(max_src_pts)
        self._work = {}
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_reginfo_create(self.ctx.h, self.pair_capacity, self.max_src_pts, C.byref(h)))
        self.h = h

    # ---- checks made before the library is called
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
        want = ((torch.float64, (c, 6, 6)), (torch.float64, (c, 6, 6)), (torch.float64, (c, 16)), (torch.float64, (c, 2)), (torch.int32, (c, 4)),
                (torch.bool, (c,)))
        if out is not None and len(out) != 6:
            raise ValueError(f"{who}: out must be an earlier result")
        return RegInfo(*(self._result(who, f"out.{name}", t, dt, sh) for name, t, (dt, sh) in zip(RegInfo._fields, out or (None,) * 6, want)))

    def point_torch(self, xyz_q, offs_q, pair_src, T, nn, accepted=None, max_corr: float = 1.0, min_inliers: int = 10, min_ratio: float = 1e-4,
                    sigma_min: float = 0.01, w_max: float = 1e6, out=None):
        """Device form (pr_reginfo_point_dev): the clouds (xyz_q f64 [*, 3], offs_q i64 [Nq + 1]) of pair_src i32 [c] under T f64 [c, 3, 4],
        accepted bool / u8 [c] or None, nn = (out_offs i64 [c + 1], nn_idx i32, nn_d2 f64) of the pass at T.  Returns a RegInfo of device
        tensors; out: an earlier result for the same c, written again."""
        who = "RegistrationInfo.point_torch"
        c, accepted = self._args(who, xyz_q, offs_q, pair_src, T, accepted, nn)
        out = self._out(who, c, out)
        self.ctx.check(self.lib.pr_reginfo_point_dev(self.h, ptr(xyz_q), ptr(offs_q), offs_q.numel() - 1, ptr(pair_src), c, ptr(T), ptr(accepted), ptr(nn[0]),
                                                     ptr(nn[1]), ptr(nn[2]), float(max_corr), int(min_inliers), float(min_ratio), float(sigma_min),
                                                     float(w_max), *(ptr(t) for t in out)))
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
        self.ctx.check(self.lib.pr_reginfo_plane_dev(self.h, ptr(xyz_q), ptr(offs_q), offs_q.numel() - 1, ptr(pair_src), c, ptr(T), ptr(accepted), ptr(nn[0]),
                                                     ptr(nn[1]), ptr(nn[2]), ptr(world_xyz), oc, ptr(normals), ptr(ninfo), float(max_corr),
                                                     int(min_inliers), float(min_ratio), float(sigma_min), float(w_max), *(ptr(t) for t in out)))
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
        nn = wk["nn"]
        self.ctx.check(self.lib.pr_icp_nn_radius_dev(self.ctx.h, ptr(xq), ptr(oq), oq.numel() - 1, ptr(xd), ptr(od), od.numel() - 1, ptr(wk["src"]), ptr(wk["dst"]),
                                                     c, ptr(Tc), int(max_src_pts), int(max_dst_pts), float(max_corr), ptr(nn[0]), ptr(nn[1]), ptr(nn[2])))
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
        xq, oq, ps, c, T, _ = _host_pairs(who, xyz_q, offs_q, pair_src, T)
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
