"""The evaluation half of run_test.m on the device (csrc/eval.hip: pr_ground_truth_pairs_dev, pr_precision_recall_dev and their Python
forms) against oracle/pr_ref.cpp's line-for-line pr_ref_precision_recall: lp_gt, lp_detected and the counts EQUAL, precision, recall,
top_recall and AUC equal bit for bit (NaN compared as NaN).  No tolerance anywhere: where a bit differs the arithmetic was not followed.

The oracle indexes gt2 with whatever diff_idx holds (MATLAB would raise); the library's rule for an index >= n is "false positive".  So the
oracle is always handed gt2 as the first n rows of a buffer whose further rows are NaN: its read of such a row is defined and gives a NaN
distance, which is a false positive there too."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from resident_fuzz_cases import bits_equal
from so_dso_place_recognition_amd import api, synth
from so_dso_place_recognition_amd import eval as ev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")
REF = os.path.join(ROOT, "tests", "golden", "ref_sequences")
PATHS = ((0, 0), (1, 1), (1, 4), (2, 1), (2, 4))      # pr_set_eval_path: by shape | every workgroup scans all of gt2 | partials + combine, x 1 | 4 queries per lane


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def oracle(v, idx, gt1, gt2, loop_diff, mask):
    gt2 = np.ascontiguousarray(gt2, np.float64)
    n, cols = gt2.shape
    idx = np.asarray(idx)
    pad = max(1, int(idx.max()) + 1 - n) if idx.size else 1
    buf = np.full((n + pad, cols), np.nan)
    buf[:n] = gt2
    return oracle_lib.precision_recall(v, np.asarray(idx, np.int32), np.asarray(gt1, np.float64).reshape(-1, cols), buf[:n], loop_diff, mask)


def to_host(res):
    torch.cuda.synchronize()
    ng, nd = int(res["n_gt"].item()), int(res["n_detected"].item())
    return dict(auc=float(res["auc"].item()), top_recall=float(res["top_recall"].item()), n_gt=ng, n_detected=nd,
                lp_gt=res["lp_gt"][:ng].cpu().numpy().astype(np.int64), lp_detected=res["lp_detected"][:nd].cpu().numpy().astype(np.int64),
                precision=res["precision"].cpu().numpy(), recall=res["recall"].cpu().numpy())


def device(ctx, v, idx, gt1, gt2, loop_diff, mask, path=(0, 0)):
    ctx.check(ctx.lib.pr_set_eval_path(ctx.h, *path))
    torch.cuda.synchronize()
    try:
        return to_host(ev.precision_recall_torch(dev(v), dev(idx, np.int32), dev(gt1), dev(gt2), loop_diff, mask, ctx=ctx))
    finally:
        ctx.check(ctx.lib.pr_set_eval_path(ctx.h, 0, 0))


def equal(got, want):
    assert got["n_gt"] == len(want["lp_gt"]) and np.array_equal(got["lp_gt"], want["lp_gt"])
    assert got["n_detected"] == len(want["lp_detected"]) and np.array_equal(got["lp_detected"], want["lp_detected"])
    assert bits_equal(got["precision"], want["precision"]) and bits_equal(got["recall"], want["recall"])
    assert bits_equal(got["top_recall"], want["top_recall"]) and bits_equal(got["auc"], want["auc"])


def check_all_paths(ctx, v, idx, gt1, gt2, loop_diff, mask):
    """Every launch geometry gives the oracle's answer (and therefore the same one)."""
    want = oracle(v, idx, gt1, gt2, loop_diff, mask)
    for path in PATHS:
        equal(device(ctx, v, idx, gt1, gt2, loop_diff, mask, path), want)
    return want


def first_minima(gt1, gt2, mask):
    """run_test.m:4-16: (min_j, min_diff) per query - the rounding order of the loop ((0 + t0^2) + t1^2) + ..., the strict update from
    +Inf / -1 (a NaN or +Inf diff never wins) as the first index of the smallest admissible value."""
    m, n = len(gt1), len(gt2)
    out_j, out_d = np.full(m, -1, np.int32), np.full(m, np.inf)
    jj = np.arange(n)
    for i in range(m):
        s = np.zeros(n)
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(gt1.shape[1]):
                t = gt1[i, c] - gt2[:, c]
                s = s + t * t
        s = np.where(np.isnan(s) | (np.abs(i - jj) < mask), np.inf, s)
        if n and s.min() < np.inf:
            out_j[i] = int(np.argmin(s)); out_d[i] = s[out_j[i]]
    return out_j, out_d


def device_minima(ctx, gt1, gt2, loop_diff, mask, path=(0, 0)):
    ctx.check(ctx.lib.pr_set_eval_path(ctx.h, *path))
    torch.cuda.synchronize()
    try:
        lp, ng, mj, md = ev.ground_truth_pairs_torch(dev(gt1), dev(gt2), loop_diff, mask, ctx=ctx)
        torch.cuda.synchronize()
        return lp[:int(ng.item())].cpu().numpy().astype(np.int64), mj.cpu().numpy(), md.cpu().numpy()
    finally:
        ctx.check(ctx.lib.pr_set_eval_path(ctx.h, 0, 0))


def positions(rng, m, n, cols):
    """A drive and a second pass near its first half: loop closures exist at a loop_diff of a few units."""
    gt1 = np.cumsum(rng.normal(0, 3, (m, cols)), 0)
    hn = min(m, n // 2)
    gt2 = np.concatenate([gt1[:hn] + rng.normal(0, 1, (hn, cols)), rng.normal(0, 100, (n - hn, cols))]) if n else np.zeros((0, cols))
    return gt1, gt2


def scores(rng, m, n, special=True):
    """Per-query best score / index with everything the sweep must order: ties, +Inf, NaN, both zeros, index -1."""
    v = np.round(rng.random(m), 2)                       # two decimals: many exact ties, stability decides
    idx = rng.integers(0, max(n, 1), m).astype(np.int32)
    h = min(m, n) // 2
    idx[:h] = np.arange(h)
    v[:h] *= 0.25
    if special and m >= 8:
        v[m - 1] = np.nan; idx[m - 1] = -1
        v[m - 2] = np.inf; idx[m - 2] = 0
        v[m - 3] = -0.0; v[m - 4] = 0.0; v[1] = -0.0; v[m - 5] = np.nan; v[m - 6] = -np.inf
        idx[3] = -1
    return v, idx


SIZES = (0, 1, 2, 3, 63, 64, 65, 257)


@pytest.mark.parametrize("m", SIZES)
def test_sizes(ctx, m):
    rng = np.random.default_rng(100 + m)
    for n in SIZES:
        gt1, gt2 = positions(rng, m, n, 3)
        v, idx = scores(rng, m, n)
        check_all_paths(ctx, v, idx, gt1, gt2, 4.0, 1)


def test_rectangular_1000_by_1300(ctx):
    rng = np.random.default_rng(5)
    gt1, gt2 = positions(rng, 1000, 1300, 3)
    v, idx = scores(rng, 1000, 1300)
    want = check_all_paths(ctx, v, idx, gt1, gt2, 4.0, 5)
    assert 10 < len(want["lp_gt"]) < 1000 and np.isfinite(want["auc"])


def test_one_row_past_a_tile(ctx):
    tile = ev.gt2_tile_rows()
    assert tile == api._lib.load().pr_eval_tile_rows() and tile >= 64
    rng = np.random.default_rng(6)
    m, n = 70, tile + 1
    gt1, gt2 = positions(rng, m, n, 3)
    gt1[:] = gt2[n - 1] + rng.normal(0, 5, (m, 3))        # the nearest row of most queries is the one row of the second tile
    v, idx = scores(rng, m, n)
    want = check_all_paths(ctx, v, idx, gt1, gt2, 10.0, 0)
    assert len(want["lp_gt"]) > 10
    lp, mj, md = device_minima(ctx, gt1, gt2, 10.0, 0)
    wj, wd = first_minima(gt1, gt2, 0)
    assert np.array_equal(mj, wj) and bits_equal(md, wd) and (mj == n - 1).sum() > 10


@pytest.mark.parametrize("cols", [1, 2, 3, 5])
def test_cols_and_masks(ctx, cols):
    rng = np.random.default_rng(20 + cols)
    m, n = 130, 300
    gt1, gt2 = positions(rng, m, n, cols)
    v, idx = scores(rng, m, n)
    for mask in (0, 1, 5, n + 3):
        want = check_all_paths(ctx, v, idx, gt1, gt2, 8.0, mask)
        if mask == n + 3:                                 # everything masked: no pair, recall 0/0 (x/0 = Inf behind a tp), AUC NaN
            assert len(want["lp_gt"]) == 0 and not np.isfinite(want["recall"]).any() and np.isnan(want["recall"][0]) and np.isnan(want["auc"])
            lp, mj, md = device_minima(ctx, gt1, gt2, 8.0, mask)
            assert len(lp) == 0 and (mj == -1).all() and np.isposinf(md).all()
        else:
            assert len(want["lp_gt"]) > 0


def test_sweep_sizes(ctx):
    rng = np.random.default_rng(31)
    for m in (0, 1, 2, 65, 1000):
        n = max(m, 3) + 7
        gt1, gt2 = positions(rng, m, n, 3)
        for special in (False, True):
            v, idx = scores(rng, m, n, special)
            want = oracle(v, idx, gt1, gt2, 4.0, 0)
            equal(device(ctx, v, idx, gt1, gt2, 4.0, 0), want)


def test_first_minimum_on_an_integer_grid(ctx):
    """Distances tie exactly; one gt2 row sits at j = 0, 63, 64, 255, 256 and n - 1, and the mask hides the nearest copies of some
    queries: the answer is the smallest unmasked j under every partition of the scan."""
    rng = np.random.default_rng(8)
    n = m = 2 * ev.gt2_tile_rows() + 9
    gt2 = rng.integers(-6, 7, (n, 3)).astype(np.float64)
    dup = [0, 63, 64, 255, 256, n - 1]
    gt2[dup] = [2.0, -3.0, 1.0]
    gt1 = rng.integers(-6, 7, (m, 3)).astype(np.float64)
    gt1[[0, 3, 60, 64, 70, 250, 256, 300, m - 1]] = [2.0, -3.0, 1.0]       # distance 0 to every copy
    for mask in (0, 8, 70, 200):
        wj, wd = first_minima(gt1, gt2, mask)
        for path in PATHS:
            lp, mj, md = device_minima(ctx, gt1, gt2, 1.5, mask, path)
            assert np.array_equal(mj, wj) and bits_equal(md, wd), (mask, path)
        v, idx = scores(rng, m, n)
        check_all_paths(ctx, v, idx, gt1, gt2, 1.5, mask)
    wj, _ = first_minima(gt1, gt2, 70)
    assert wj[0] == 255 and wj[64] == 255 and wj[300] == 0 and wj[m - 1] == 0      # (copies 0, 63, 64 masked for the first two)


def test_non_finite_coordinates(ctx):
    rng = np.random.default_rng(9)
    m, n = 90, 140
    gt1, gt2 = positions(rng, m, n, 3)
    gt1[7] = np.nan; gt1[8, 1] = np.inf; gt1[9] = -np.inf
    gt2[11] = np.nan; gt2[12, 2] = np.inf; gt2[0, 0] = np.nan
    v, idx = scores(rng, m, n)
    idx[20] = 11; idx[21] = 12; idx[7] = 7; idx[8] = 8
    check_all_paths(ctx, v, idx, gt1, gt2, 4.0, 2)
    lp, mj, md = device_minima(ctx, gt1, gt2, 4.0, 2)
    wj, wd = first_minima(gt1, gt2, 2)
    assert np.array_equal(mj, wj) and bits_equal(md, wd)
    assert mj[7] == -1 and mj[8] == -1 and np.isposinf(md[7]) and 7 not in lp[:, 0]     # every candidate NaN / +Inf: no pair
    all_nan = np.full((5, 3), np.nan)
    lp, mj, md = device_minima(ctx, gt1[:20], all_nan, 4.0, 0)
    assert len(lp) == 0 and (mj == -1).all()
    check_all_paths(ctx, v[:20], np.zeros(20, np.int32), gt1[:20], all_nan, 4.0, 0)


def test_threshold_is_strict_and_single_pair(ctx):
    one = np.zeros((6, 3)); one[:, 0] = np.arange(6) * 100.0
    two = one + 1e4
    two[3] = one[3] + [3.0, 4.0, 0.0]                     # distance exactly 5 = loop_diff: not a loop
    v = np.array([.5, .4, .3, .1, .2, .6]); idx = np.array([1, 2, 0, 3, 3, 3], np.int32)
    want = check_all_paths(ctx, v, idx, one, two, 5.0, 0)
    assert len(want["lp_gt"]) == 0 and len(want["lp_detected"]) == 0 and np.isnan(want["auc"])
    want = check_all_paths(ctx, v, idx, one, two, np.nextafter(5.0, 6.0), 0)
    assert len(want["lp_gt"]) == 1 and want["recall"][0] == 0.5                      # L = 1: total_lp = length() of a 1 x 2 matrix = 2
    assert np.array_equal(want["lp_detected"], [[3, 3]]) and want["top_recall"] == 0.5


def test_sweep_inputs(ctx):
    rng = np.random.default_rng(12)
    m, n = 200, 230
    gt1, gt2 = positions(rng, m, n, 3)
    lp = oracle(np.zeros(m), np.zeros(m, np.int32), gt1, gt2, 4.0, 3)["lp_gt"]
    assert len(lp) > 20
    v, idx = scores(rng, m, n)
    v[:] = np.repeat(rng.random(m // 8), 8)               # runs of eight equal scores
    want = check_all_paths(ctx, v, idx, gt1, gt2, 4.0, 3)
    idx2 = idx.copy(); idx2[10:40] = n + rng.integers(0, 50, 30); idx2[50:60] = -1       # matches beyond gt2 and "no candidate"
    equal(device(ctx, v, idx2, gt1, gt2, 4.0, 3), oracle(v, idx2, gt1, gt2, 4.0, 3))
    va = rng.random(m); ia = np.zeros(m, np.int32)        # all ranks tp: every query paired with a row of gt2 next to it
    g2 = np.concatenate([gt1 + 0.1, gt2[: n - m]])
    ia[:] = np.arange(m)
    want = oracle(va, ia, gt1, g2, 4.0, 3)
    assert len(want["lp_detected"]) == m and (want["precision"] == 1).all()
    equal(device(ctx, va, ia, gt1, g2, 4.0, 3), want)
    vb = va.copy(); ib = ia.copy()
    worst = int(np.argmin(vb)); ib[worst] = n - 1          # first rank fp: top_count = 0
    want = oracle(vb, ib, gt1, g2, 4.0, 3)
    assert len(want["lp_detected"]) == 0 and want["top_recall"] == 0.0
    equal(device(ctx, vb, ib, gt1, g2, 4.0, 3), want)
    vz = np.array([0.0, -0.0, np.nan, np.inf, -0.0, 0.0, -np.inf, np.nan, 1.0, np.inf])  # the comparator's classes, in input order
    equal(device(ctx, vz, ia[:10], gt1[:10], g2, 4.0, 3), oracle(vz, ia[:10], gt1[:10], g2, 4.0, 3))


def _perturbed(rng, gt1, gt2, loop_diff, mask):
    lp = ev.ground_truth_pairs(gt1, gt2, loop_diff, mask)
    m, n = len(gt1), len(gt2)
    v = rng.random(m); idx = rng.integers(0, n, m).astype(np.int32)
    keep = lp[rng.random(len(lp)) < 0.7]
    idx[keep[:, 0]] = np.clip(keep[:, 1] + rng.integers(-2, 3, len(keep)), 0, n - 1)
    v[keep[:, 0]] *= 0.4
    return lp, v, idx


@pytest.mark.parametrize("name", ["kitti_seq06", "kitti_seq07"])
def test_kitti_reference_positions(ctx, name):
    gt = ev.load_kitti_ground_truth(os.path.join(REF, name))
    lp, v, idx = _perturbed(np.random.default_rng(3), gt, gt, 10.0, 100)
    want = oracle(v, idx, gt, gt, 10.0, 100)
    got = device(ctx, v, idx, gt, gt, 10.0, 100)
    equal(got, want)
    assert np.array_equal(got["lp_gt"], lp)


def test_robotcar_reference_positions(ctx):
    g1 = ev.load_robotcar_ground_truth(os.path.join(REF, "robotcar_2015-05-19-14-06-38"))
    g2 = ev.load_robotcar_ground_truth(os.path.join(REF, "robotcar_2015-05-22-11-14-30"))
    lp, v, idx = _perturbed(np.random.default_rng(4), g1, g2, 25.0, 0)
    got = device(ctx, v, idx, g1, g2, 25.0, 0)
    equal(got, oracle(v, idx, g1, g2, 25.0, 0))
    assert np.array_equal(got["lp_gt"], lp) and len(lp) > 0


def test_matchers_chain_into_evaluate():
    """GistMatcher and Matcher('m2dp') at n = 300: evaluate() on the device tensors match() returned (k = 1 and k = 5: ld = 5) equals
    eval.precision_recall on the copied-back top-1."""
    from so_dso_place_recognition_amd.matcher import GistMatcher, Matcher
    n = 300
    rng = np.random.default_rng(14)
    gt = np.cumsum(rng.normal(0, 2, (n, 3)), 0)
    gt[150:] = gt[:150] + rng.normal(0, 0.5, (150, 3))     # the second half revisits the first
    gist = synth.gist_signatures(3, n, 96)
    gist[150:] = gist[:150] + 1e-3 * rng.normal(0, 1, (150, 96))
    m2 = synth.m2dp_database(43, n)
    m2[4 * 150:] = synth.m2dp_queries(44, m2[:4 * 150], 150)[0]
    g = torch.from_numpy(gt).cuda()
    mg = GistMatcher(n, n, 96)
    mg.pack_database(torch.from_numpy(gist).cuda())
    mm = Matcher("m2dp", n, n)
    mm.pack_database(torch.from_numpy(m2).cuda())
    for k in (1, 5):
        for mt, res in ((mg, mg.match(torch.from_numpy(gist).cuda(), 20, k)), (mm, mm.match(torch.from_numpy(m2).cuda(), 20, 2.0, k))):
            idx, sc = res
            assert idx.shape == (n, k) and sc.dtype == torch.float64
            got = to_host(mt.evaluate(idx, sc, g, g, 3.0, 20))
            auc, tr, det, prec, rec = ev.precision_recall(sc[:, 0].cpu().numpy(), idx[:, 0].cpu().numpy(), gt, gt, 3.0, 20)
            assert bits_equal(got["auc"], auc) and bits_equal(got["top_recall"], tr) and np.array_equal(got["lp_detected"], det)
            assert bits_equal(got["precision"], prec) and bits_equal(got["recall"], rec)
            assert np.array_equal(got["lp_gt"], ev.ground_truth_pairs(gt, gt, 3.0, 20)) and got["n_gt"] > 50
    mg.close(); mm.close()


def test_graph_capture_and_replay():
    from so_dso_place_recognition_amd.matcher import _stream_context
    rng = np.random.default_rng(15)
    m, n = 300, 340
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = _stream_context(0)
        gt1, gt2 = positions(rng, m, n, 3)
        v, idx = scores(rng, m, n)
        tv, ti, t1, t2 = dev(v), dev(idx, np.int32), dev(gt1), dev(gt2)
        out = ev.precision_recall_torch(tv, ti, t1, t2, 4.0, 2, ctx=c)          # the scratch grows here, not under capture
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            ev.precision_recall_torch(tv, ti, t1, t2, 4.0, 2, ctx=c, out=out)
        equal(to_host(out), oracle(v, idx, gt1, gt2, 4.0, 2))
        gt1b, gt2b = positions(rng, m, n, 3)
        vb, idxb = scores(rng, m, n)
        tv.copy_(dev(vb)); ti.copy_(dev(idxb, np.int32)); t1.copy_(dev(gt1b)); t2.copy_(dev(gt2b))
        for t in out.values():
            t.zero_()
        g.replay()
        st.synchronize()
        want = oracle(vb, idxb, gt1b, gt2b, 4.0, 2)
        assert len(want["lp_gt"]) > 5
        equal(to_host(out), want)
    del g
    c.close()


def test_run_test_device_eval():
    n = 200
    rng = np.random.default_rng(16)
    gt = np.cumsum(rng.normal(0, 2, (n, 3)), 0)
    gt[100:] = gt[:100] + rng.normal(0, 0.5, (100, 3))
    gist = synth.gist_signatures(5, n, 96)
    gist[100:] = gist[:100] + 1e-3 * rng.normal(0, 1, (100, 96))
    m2 = synth.m2dp_database(45, n)
    m2[400:], planted = synth.m2dp_queries(46, m2[:400], 100)
    gtm = gt.copy()
    gtm[100:] = gt[np.asarray(planted)] + rng.normal(0, 0.5, (100, 3))      # (these revisit random places of the first half)
    for type_, h, g in (("gist", gist, gt), ("m2dp", m2, gtm)):
        a = api.run_test(type_, h, h, g, g, 3.0, 20)
        b = api.run_test(type_, h, h, g, g, 3.0, 20, device_eval=True)
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and len(a[2]) > 0


def test_match_signatures_eval_device(tmp_path):
    """`--eval_device 1` prints the report lines of the host evaluation (the drive of test_cli.py's ground-truth test)."""
    n = 260
    sig = synth.sc_database(45, n)
    sig[130:] = synth.sc_queries(46, sig[:130], 130)[0]
    f = str(tmp_path / "history_sc.txt"); api.write_signatures(f, sig)
    gt = np.cumsum(np.random.default_rng(4).normal(0, 4, (n, 3)), 0)
    g = str(tmp_path / "gt.txt"); np.savetxt(g, gt)
    reports = []
    for extra in ([], ["--eval_device", "1"]):
        res = str(tmp_path / f"m{len(extra)}.txt")
        r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", "sc", "--hist1", f, "--hist2", f, "--mask_width", "20",
                            "--out", res, "--gt1", g, "--gt2", g, "--loop_diff", "15"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        reports.append([ln for ln in r.stdout.splitlines() if ln.startswith(("AUC = ", "top_recall = ", "lp_detected = "))])
    assert len(reports[0]) == 3 and reports[0] == reports[1]
