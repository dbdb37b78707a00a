"""Evaluation harness of match_signatures/run_test.m: ground-truth loop pairs (:3-22) and the
precision/recall sweep, top recall at 100 % precision and AUC (:58-85).  Host numpy, O(m n) and O(m log m); the `_torch` / `_gpu`
functions run the same arithmetic on the device (csrc/eval.hip)."""
from __future__ import annotations

import numpy as np

from ._handle import ptr


def ground_truth_pairs(gt1, gt2, loop_diff: float, mask_width: int) -> np.ndarray:
    """run_test.m:3-22: for every i the closest j with |i-j| >= mask_width (first minimum), kept when closer than
    loop_diff.  Returns an [L, 2] int array of 0-based (i, j)."""
    gt1 = np.asarray(gt1, np.float64)
    gt2 = np.asarray(gt2, np.float64)
    out = []
    jdx = np.arange(gt2.shape[0])
    for i in range(gt1.shape[0]):
        d = ((gt1[i][None, :] - gt2) ** 2).sum(1)
        d = np.where(np.abs(i - jdx) < mask_width, np.inf, d)
        if d.size == 0:
            continue
        j = int(np.argmin(d))                          # first minimum == strict `min_diff > diff` update
        if d[j] < loop_diff * loop_diff:
            out.append((i, j))
    return np.array(out, np.int64).reshape(-1, 2)


def precision_recall(diff_v, diff_idx, gt1, gt2, loop_diff: float, mask_width: int):
    """run_test.m:57-85 given the per-query best score / index (0-based).  Returns (AUC, top_recall, lp_detected,
    precision, recall); lp_detected is [top_count, 2] 0-based (query, match)."""
    gt1 = np.asarray(gt1, np.float64)
    gt2 = np.asarray(gt2, np.float64)
    diff_v = np.asarray(diff_v, np.float64)
    diff_idx = np.asarray(diff_idx, np.int64)
    # index -1 = no finite candidate (zero-norm signature: every distance NaN; or everything masked): MATLAB's min over an all-NaN /
    # all-Inf row returns index 1 (run_test.m:57) and the sweep pairs the query with gt2(1,:)
    diff_idx = np.where(diff_idx < 0, 0, diff_idx)
    lp_gt = ground_truth_pairs(gt1, gt2, loop_diff, mask_width)
    L = lp_gt.shape[0]
    total_lp = 0 if L == 0 else max(L, 2)              # MATLAB length() of an L x 2 matrix (run_test.m:22)
    rank = np.argsort(diff_v, kind="stable")           # [~, diff_rank] = sort(diff_v)
    m = gt1.shape[0]
    precision = np.zeros(m)
    recall = np.zeros(m)
    tp = fp = 0
    top_recall = 0.0
    top_count = 0
    for i in range(m):
        a = rank[i]
        b = diff_idx[a]
        d = ((gt1[a] - gt2[b]) ** 2).sum()
        if d < loop_diff * loop_diff:
            tp += 1
        else:
            fp += 1
        precision[i] = tp / (tp + fp)
        recall[i] = tp / total_lp if total_lp else (np.inf if tp else np.nan)   # :77 as MATLAB divides (x/0 = Inf, 0/0 = NaN)
        if precision[i] == 1:
            top_count = i + 1
            top_recall = recall[i]
    auc = 0.0                                          # trapz(recall, precision) (:84), summed in sweep order like pr_precision_recall
    with np.errstate(invalid="ignore"):                # (recall is NaN / Inf without ground-truth pairs)
        for i in range(m - 1):
            auc += (recall[i + 1] - recall[i]) * (precision[i] + precision[i + 1]) / 2.0
    lp_detected = np.stack([rank[:top_count], diff_idx[rank[:top_count]]], 1)
    return auc, float(top_recall), lp_detected, precision, recall


# ------------------------------------------------------------------ the same on the device (csrc/eval.hip)
def gt2_tile_rows() -> int:
    """gt2 rows a workgroup of the ground-truth kernel stages at a time (pr_eval_tile_rows)."""
    from . import _lib
    return int(_lib.load().pr_eval_tile_rows())


def _positions(gt1, gt2):
    import torch
    if not (gt1.is_cuda and gt2.is_cuda) or gt1.dim() != 2 or gt2.dim() != 2 or gt1.shape[1] != gt2.shape[1]:
        raise ValueError("expected CUDA position tensors [m, cols] and [n, cols]")
    return gt1.to(torch.float64).contiguous(), gt2.to(torch.float64).contiguous()


class _on_stream:
    """ctx given: its stream is the caller's to order.  ctx None: the per-device default context, joined to torch's current stream by
    stream waits on both sides (no host wait), the tensors marked as used there for torch's caching allocator."""

    def __init__(self, ctx, device, tensors):
        self.ctx, self.lib_stream, self.cur, self.tensors = ctx, None, None, tensors
        if ctx is None:
            import torch
            from . import api
            self.ctx, self.lib_stream = api._torch_default_context(device.index or 0)
            self.cur = torch.cuda.current_stream(device)

    def __enter__(self):
        if self.lib_stream is not None:
            self.lib_stream.wait_stream(self.cur)
        return self.ctx

    def __exit__(self, *exc):
        if self.lib_stream is not None:
            self.cur.wait_stream(self.lib_stream)
            for t in self.tensors:
                t.record_stream(self.lib_stream)


def ground_truth_pairs_torch(gt1, gt2, loop_diff: float, mask_width: int, ctx=None):
    """run_test.m:3-22 on the device (pr_ground_truth_pairs_dev): gt1 [m, cols], gt2 [n, cols] CUDA tensors ->
    (lp_gt int32 [m, 2], n_gt int32 [1], min_j int32 [m], min_d float64 [m]), all on the device; the first n_gt rows of lp_gt are the
    pairs (i, j) in ascending i.  Nothing synchronises: `lp_gt[:int(n_gt)]` is the caller's read."""
    import torch
    g1, g2 = _positions(gt1, gt2)
    m, n, cols = g1.shape[0], g2.shape[0], g1.shape[1]
    dev = g1.device
    lp = torch.empty((m, 2), dtype=torch.int32, device=dev)
    n_gt = torch.empty(1, dtype=torch.int32, device=dev)
    min_j = torch.empty(m, dtype=torch.int32, device=dev)
    min_d = torch.empty(m, dtype=torch.float64, device=dev)
    with _on_stream(ctx, dev, (g1, g2, lp, n_gt, min_j, min_d)) as c:
        c.check(c.lib.pr_ground_truth_pairs_dev(c.h, ptr(g1), m, ptr(g2), n, cols, float(loop_diff), int(mask_width), ptr(min_j), ptr(min_d),
                                                ptr(lp), ptr(n_gt)))
    return lp, n_gt, min_j, min_d


def precision_recall_torch(score, idx, gt1, gt2, loop_diff: float, mask_width: int, ctx=None, out=None):
    """run_test.m:3-22 + :58-85 on the device (pr_precision_recall_dev).  score (float64) / idx (int32): CUDA tensors [m] or the [m, k]
    pair a matcher returned (column 0 is read in place).  Returns a dict of device tensors: auc, top_recall (float64 [1] views of one
    record), n_gt, n_detected (int32 [1]), lp_gt, lp_detected (int32 [m, 2]; the first n_gt / n_detected rows are written), precision,
    recall (float64 [m]).  Nothing synchronises until the caller reads them.  out: a dict this call returned for the same m - its tensors
    are written again (fixed addresses: what a captured graph needs)."""
    import torch
    g1, g2 = _positions(gt1, gt2)
    m, n, cols = g1.shape[0], g2.shape[0], g1.shape[1]
    if not (score.is_cuda and idx.is_cuda) or score.dtype != torch.float64 or idx.dtype != torch.int32 or score.shape != idx.shape \
            or score.dim() not in (1, 2) or score.shape[0] != m or not (score.is_contiguous() and idx.is_contiguous()):
        raise ValueError("precision_recall_torch: score (float64) / idx (int32) must be contiguous CUDA tensors [m] or [m, k]")
    ld = 1 if score.dim() == 1 else int(score.shape[1])
    dev = g1.device
    if out is None:
        rec = torch.empty(3, dtype=torch.float64, device=dev)     # {f64 auc, f64 top_recall, i32 n_gt, i32 n_detected}
        cnt = rec[2:].view(torch.int32)
        out = dict(_record=rec, auc=rec[0:1], top_recall=rec[1:2], n_gt=cnt[0:1], n_detected=cnt[1:2],
                   lp_gt=torch.empty((m, 2), dtype=torch.int32, device=dev), lp_detected=torch.empty((m, 2), dtype=torch.int32, device=dev),
                   precision=torch.empty(m, dtype=torch.float64, device=dev), recall=torch.empty(m, dtype=torch.float64, device=dev))
    elif out["precision"].shape[0] != m:
        raise ValueError("precision_recall_torch: out belongs to another m")
    with _on_stream(ctx, dev, (score, idx, g1, g2, out["_record"], out["lp_gt"], out["lp_detected"], out["precision"], out["recall"])) as c:
        c.check(c.lib.pr_precision_recall_dev(c.h, ptr(score), ptr(idx), ld, m, ptr(g1), ptr(g2), n, cols, float(loop_diff), int(mask_width),
                                              ptr(out["_record"]), ptr(out["lp_gt"]), ptr(out["lp_detected"]), ptr(out["precision"]),
                                              ptr(out["recall"])))
    return out


def precision_recall_gpu(diff_v, diff_idx, gt1, gt2, loop_diff: float, mask_width: int, ctx=None):
    """precision_recall() through the device evaluation, host arrays in and out (pr_precision_recall_gpu): the same tuple
    (AUC, top_recall, lp_detected, precision, recall)."""
    import ctypes as C
    from . import api
    ctx = ctx or api.default_context()
    gt1 = np.ascontiguousarray(gt1, np.float64); gt2 = np.ascontiguousarray(gt2, np.float64)
    v = np.ascontiguousarray(diff_v, np.float64); bi = np.ascontiguousarray(diff_idx, np.int32)
    m, n, cols = gt1.shape[0], gt2.shape[0], gt1.shape[1]
    auc, tr, nd = C.c_double(), C.c_double(), C.c_int32()
    lp = np.zeros((max(m, 1), 2), np.int32); prec = np.zeros(max(m, 1)); rec = np.zeros(max(m, 1))
    ctx.check(ctx.lib.pr_precision_recall_gpu(ctx.h, api._ptr(v), api._ptr(bi), m, api._ptr(gt1), api._ptr(gt2), n, cols, float(loop_diff),
                                              int(mask_width), C.byref(auc), C.byref(tr), None, None, api._ptr(lp), C.byref(nd),
                                              api._ptr(prec), api._ptr(rec)))
    return auc.value, tr.value, lp[:nd.value].astype(np.int64), prec[:m], rec[:m]


# ------------------------------------------------------------------ the drivers: test_kitti.m, test_robotcar.m
KITTI_SEQS = ("seq00", "seq02", "seq05", "seq06", "seq07")                                  # test_kitti.m:5
ROBOTCAR_DATES = ("2014-07-14-14-49-50", "2014-11-28-12-07-13", "2014-12-12-10-45-15", "2015-02-10-11-58-05",
                  "2015-05-19-14-06-38", "2015-05-22-11-14-30", "2015-08-13-16-02-58", "2015-10-30-13-52-14")   # test_robotcar.m:4-6
ROBOTCAR_PAIRS = ((5, 6), (5, 7), (5, 8), (5, 4), (7, 1), (7, 8), (7, 4), (8, 2), (8, 4), (4, 3))              # :9, 1-based
TYPES = ("delight", "m2dp", "sc", "bow", "gist")                                            # :8


def _load(path):
    """MATLAB `load` of a numeric text file (optionally gzip-compressed, as the test fixtures are)."""
    import gzip
    import os
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        path += ".gz"
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return np.loadtxt(f, ndmin=2)


def load_kitti_ground_truth(seq_dir: str) -> np.ndarray:
    """test_kitti.m:23-25: positions of the poses that became clouds - gt.txt rows `incoming_id + 1` (0-based ids in the
    file), columns 4, 8, 12 of the row-major 3 x 4 pose."""
    import os
    ids = _load(os.path.join(seq_dir, "incoming_id_file.txt")).astype(np.int64).ravel()
    return _load(os.path.join(seq_dir, "gt.txt"))[ids][:, [3, 7, 11]]


def load_robotcar_ground_truth(run_dir: str) -> np.ndarray:
    """test_robotcar.m:31-36: gps.txt rows of the poses that became clouds (all three columns)."""
    import os
    ids = _load(os.path.join(run_dir, "incoming_id_file.txt")).astype(np.int64).ravel()
    return _load(os.path.join(run_dir, "gps.txt"))[ids]


def load_pose_history(seq_dir: str):
    """poses_history_file.txt of a sequence: (ids int64 [m], poses float64 [m, 12]).  Column 0 is the frame id, columns 1 .. 12 a
    world-to-camera [R | t], row-major - the rows api.TrajectoryEval takes as the estimate."""
    import os
    a = _load(os.path.join(seq_dir, "poses_history_file.txt"))
    return a[:, 0].astype(np.int64), np.ascontiguousarray(a[:, 1:13])


def load_kitti_gt_poses(seq_dir: str, ids=None) -> np.ndarray:
    """KITTI's gt.txt rows (camera to world, row-major 3 x 4: api.TrajectoryEval's gt_kind "c2w") of the poses that became clouds - rows
    `incoming_id` as in load_kitti_ground_truth - or of the frame ids given.  Rows are matched by index, never by time."""
    import os
    if ids is None:
        ids = _load(os.path.join(seq_dir, "incoming_id_file.txt")).astype(np.int64).ravel()
    return np.ascontiguousarray(_load(os.path.join(seq_dir, "gt.txt"))[np.asarray(ids, np.int64)])


def run_kitti(seq_dir: str, type_: str, hist=None, ctx=None):
    """run_kitti of test_kitti.m:17-29: a sequence against itself, mask_width 100, loop_diff 10 m.  `hist` defaults to
    `<seq_dir>/history_<type>.txt` (or .bin).  Returns (AUC, top_recall, lp_detected)."""
    from . import api
    gt = load_kitti_ground_truth(seq_dir)
    h = _history(seq_dir, type_) if hist is None else hist
    return api.run_test(type_, h, h, gt, gt, 10.0, 100, ctx)


def run_robotcar(run1_dir: str, run2_dir: str, type_: str, hist1=None, hist2=None, ctx=None):
    """run_robotcar of test_robotcar.m:26-41: run 1 against run 2, no mask, loop_diff 25 m."""
    from . import api
    gt1, gt2 = load_robotcar_ground_truth(run1_dir), load_robotcar_ground_truth(run2_dir)
    h1 = _history(run1_dir, type_) if hist1 is None else hist1
    h2 = _history(run2_dir, type_) if hist2 is None else hist2
    return api.run_test(type_, h1, h2, gt1, gt2, 25.0, 0, ctx)


def _history(d: str, type_: str):
    import os
    from . import api
    for ext in (".bin", ".txt"):
        p = os.path.join(d, "history_" + type_ + ext)
        if os.path.exists(p):
            return api.read_signatures(p)
    raise FileNotFoundError(os.path.join(d, "history_" + type_ + ".txt"))


def test_kitti(results_dir: str, types=TYPES, seqs=KITTI_SEQS, ctx=None):
    """test_kitti.m:1-15: (AUCs, TRs), each [len(types), len(seqs)]."""
    import os
    auc = np.zeros((len(types), len(seqs))); tr = np.zeros_like(auc)
    for ti, t in enumerate(types):
        for si, s in enumerate(seqs):
            auc[ti, si], tr[ti, si] = run_kitti(os.path.join(results_dir, "KITTI", s), t, ctx=ctx)[:2]
    return auc, tr


def test_robotcar(results_dir: str, types=TYPES, pairs=ROBOTCAR_PAIRS, ctx=None):
    """test_robotcar.m:1-24: (AUCs, TRs), each [len(types), len(pairs)]; pairs are 1-based indices into ROBOTCAR_DATES."""
    import os
    auc = np.zeros((len(types), len(pairs))); tr = np.zeros_like(auc)
    for ti, t in enumerate(types):
        for si, (a, b) in enumerate(pairs):
            auc[ti, si], tr[ti, si] = run_robotcar(os.path.join(results_dir, "RobotCar", ROBOTCAR_DATES[a - 1]),
                                                   os.path.join(results_dir, "RobotCar", ROBOTCAR_DATES[b - 1]), t, ctx=ctx)[:2]
    return auc, tr


test_kitti.__test__ = False       # (names of the reference's scripts, not pytest tests)
test_robotcar.__test__ = False
