"""The alignment layer on the MI355X: which variant of the query lines up best with each matched DB entry (pr_align_pairs_dev,
pr_delight_align_pairs_dev, their host forms, Matcher.align / FusedMatcher.align, match_signatures --align_out) and the SC relative pose
built on it.  References: the planted shifts of the samplers, a numpy fp64 restatement of processSC.m:22-33 / processM2DP.m:12-22 /
processDELIGHT.m:7-37 that keeps the argmin, and the re-evaluation's own p5 distances."""
import os
import subprocess

import numpy as np
import pytest
import torch

from so_dso_place_recognition_amd import api, synth
from so_dso_place_recognition_amd.matcher import FusedMatcher, Matcher
from test_align import _frame, _rot_err_deg, _scene, _yaw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")
MUT = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [5, 4, 7, 6, 1, 0, 3, 2, 13, 12, 15, 14, 9, 8, 11, 10],
                [6, 7, 4, 5, 2, 3, 0, 1, 14, 15, 12, 13, 10, 11, 8, 9], [3, 2, 1, 0, 7, 6, 5, 4, 11, 10, 9, 8, 15, 14, 13, 12]])


# ------------------------------------------------------------------------------------------ numpy fp64 restatement (all variants)
def np_sc_variants(q, d):
    """[2 channels][120 variants] distances of processSC.m:15-30 for one pair, variant v = 2 s + r."""
    out = np.empty((2, 120))
    c = np.arange(60)
    for ch in range(2):
        with np.errstate(invalid="ignore", divide="ignore"):
            a = q[ch * 1200:(ch + 1) * 1200] / np.linalg.norm(q[ch * 1200:(ch + 1) * 1200])
            b = d[ch * 1200:(ch + 1) * 1200] / np.linalg.norm(d[ch * 1200:(ch + 1) * 1200])
        img, dim = a.reshape(60, 20), b.reshape(60, 20)
        for s in range(60):
            out[ch, 2 * s] = (1 - (img[(s + c) % 60] * dim).sum()) / 2
            out[ch, 2 * s + 1] = (1 - (img[(s - c) % 60] * dim).sum()) / 2
    return out


def np_m2dp_variants(q, d):
    """q, d [4][384] -> [2][16], v = 4 a + b (processM2DP.m:14-18)."""
    return np.stack([((1 - q[:, ch * 192:(ch + 1) * 192] @ d[:, ch * 192:(ch + 1) * 192].T) / 2).reshape(16) for ch in range(2)])


def np_delight_variants(q, d):
    """q, d [16][256] -> [4] means of processDELIGHT.m:16-31 (NaN without an occupied bin)."""
    out = np.empty(4)
    for k in range(4):
        a, b = q, d[MUT[k]]
        s = a + b
        occ = s > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            out[k] = (2 * (a[occ] - b[occ]) ** 2 / s[occ]).sum() / occ.sum()
    return out


def check_against_numpy(var, dist, allv):
    """var / dist: one channel's result, allv: numpy's distances of every variant.  dist within 1e-12; variant = numpy's argmin wherever
    the runner-up is more than 1e-12 away."""
    if np.all(np.isnan(allv)):
        assert var == -1 and np.isnan(dist)
        return
    order = np.argsort(np.where(np.isnan(allv), np.inf, allv), kind="stable")
    best = allv[order[0]]
    assert abs(dist - best) <= 1e-12, (dist, best)
    if allv[order[1]] - best > 1e-12:
        assert var == order[0], (var, order[0])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int64) if t.dtype == torch.float64 else t.cpu().numpy()


def _sc_matcher(db, m):
    mt = Matcher("sc", m, db.shape[0])
    mt.pack_database(_cuda(db))
    return mt


# ------------------------------------------------------------------------------------------ 1. planted SC shifts
def test_sc_planted_shift_and_mirror():
    n, m = 20000, 512
    db = synth.sc_database(11, n)
    q, et = synth.sc_queries(12, db, m)
    u = synth.uniform(12, np.arange(m, dtype=np.uint64), 3 + 3600)
    shift = np.minimum((u[:, 1] * 60).astype(np.int64), 59)
    mirror = (u[:, 2] < 0.5).astype(np.int64)
    mt = _sc_matcher(db, m)
    idx, _ = mt.match(_cuda(q), 0, 2.0, 1)
    var, dist = mt.align(idx)
    torch.cuda.synchronize()
    idx, var, dist = idx.cpu().numpy(), var.cpu().numpy(), dist.cpu().numpy()
    assert var.shape == (m, 1, 2) and dist.shape == (m, 1, 2)
    assert np.array_equal(idx[:, 0], et)
    assert np.array_equal(var[:, 0, 0], 2 * shift + mirror)
    assert np.all(np.isfinite(dist))
    mt.close()


# ------------------------------------------------------------------------------------------ 2. + 3. numpy fp64 and the rerank's own distances
def test_sc_k5_numpy_and_rerank_bits():
    n, m, k = 3000, 48, 5
    db = synth.sc_database(21, n)
    q, _ = synth.sc_queries(22, db, m)
    mt = _sc_matcher(db, m)
    idx, _ = mt.match(_cuda(q), 0, 2.0, k)
    var, dist = mt.align(idx)
    part = mt.local_rerank(idx, k, partial=True)                        # p5 block of the same pairs, every one evaluated
    torch.cuda.synchronize()
    ix, v, d = idx.cpu().numpy(), var.cpu().numpy(), dist.cpu().numpy()
    for i in range(m):
        for j in range(k):
            allv = np_sc_variants(q[i], db[ix[i, j]])
            for ch in range(2):
                check_against_numpy(v[i, j, ch], d[i, j, ch], allv[ch])
    p5 = part.cpu().numpy()
    for ch in range(2):
        assert np.array_equal(d[:, :, ch].view(np.int64), p5[:, 1 + ch, :].view(np.int64))
    mt.close()


def test_m2dp_k5_numpy_dominant_pair_and_rerank_bits():
    n, m, k = 2000, 40, 5
    db = synth.m2dp_database(31, n)
    rng = np.random.default_rng(32)
    et = rng.integers(0, n, m)
    a0, b0 = rng.integers(0, 4, m), rng.integers(0, 4, m)
    other = synth.m2dp_database(33, m).reshape(m, 4, 384)               # unrelated rows ...
    q = other.copy()
    for i in range(m):                                                  # ... but query row a0 is the entry's row b0, slightly perturbed
        r = db.reshape(n, 4, 384)[et[i], b0[i]] + 0.01 * (rng.random(384) - 0.5)
        r[:64] /= np.linalg.norm(r[:64]); r[64:192] /= np.linalg.norm(r[64:192])
        r[192:256] /= np.linalg.norm(r[192:256]); r[256:] /= np.linalg.norm(r[256:])
        q[i, a0[i]] = r
    q = q.reshape(4 * m, 384)
    mt = Matcher("m2dp", m, n)
    mt.pack_database(_cuda(db))
    idx, _ = mt.match(_cuda(q), 0, 2.0, k)
    var, dist = mt.align(idx)
    part = mt.local_rerank(idx, k, partial=True)
    torch.cuda.synchronize()
    ix, v, d = idx.cpu().numpy(), var.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(ix[:, 0], et)
    assert np.array_equal(v[:, 0, 0], 4 * a0 + b0) and np.array_equal(v[:, 0, 1], 4 * a0 + b0)
    for i in range(m):
        for j in range(k):
            allv = np_m2dp_variants(q.reshape(m, 4, 384)[i], db.reshape(n, 4, 384)[ix[i, j]])
            for ch in range(2):
                check_against_numpy(v[i, j, ch], d[i, j, ch], allv[ch])
    p5 = part.cpu().numpy()
    for ch in range(2):
        assert np.array_equal(d[:, :, ch].view(np.int64), p5[:, 3 + ch, :].view(np.int64))
    mt.close()


def test_delight_k5_numpy_planted_permutation():
    n, m, k = 300, 24, 5
    db = synth.delight_database(41, n)
    q, et = synth.delight_queries(42, db, m)
    u = synth.uniform(42, np.arange(m, dtype=np.uint64), 2 + 2 * 4096)
    perm = np.minimum((u[:, 1] * 4).astype(np.int64), 3)
    mt = Matcher("delight", m, n)
    mt.pack_database(_cuda(db))
    idx, _ = mt.match(_cuda(q), 0, 2.0, k)
    var, dist = mt.align(idx)
    torch.cuda.synchronize()
    ix, v, d = idx.cpu().numpy(), var.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(ix[:, 0], et)
    # query row r is its entry's row Mut(perm, r): exactly the rows variant perm pairs it with (processDELIGHT.m:14-15)
    assert np.array_equal(v[:, 0, 0], perm)
    assert np.all(v[:, :, 1] == -1) and np.all(np.isnan(d[:, :, 1]))
    for i in range(m):
        for j in range(k):
            check_against_numpy(v[i, j, 0], d[i, j, 0], np_delight_variants(q.reshape(m, 16, 256)[i], db.reshape(n, 16, 256)[ix[i, j]]))
    hv, hd = api.match_align("delight", q, db, ix)
    assert np.array_equal(hv, v) and np.array_equal(hd.view(np.int64), d.view(np.int64))
    # an empty pair (no occupied bin in either signature): -1 / +Inf, the reference's untouched min_dist = Inf
    z = np.zeros((16, 256))
    hv, hd = api.match_align("delight", z, np.concatenate([z, db[:16]]), np.array([[0, 1]], np.int32))
    assert hv[0, 0, 0] == -1 and np.isposinf(hd[0, 0, 0]) and hv[0, 1, 0] >= 0
    mt.close()


# ------------------------------------------------------------------------------------------ 4. host vs device, missing pairs, zero norm
def test_host_equals_device_and_missing_pairs():
    n, m, k = 1000, 32, 3
    db = synth.sc_database(51, n)
    q, _ = synth.sc_queries(52, db, m)
    q[5, :1200] = 0.0                                                   # a zero-norm structure channel (processSC.m:16: NaN)
    mt = _sc_matcher(db, m)
    idx, _ = mt.match(_cuda(q), 0, 2.0, k)
    torch.cuda.synchronize()
    ix = idx.cpu().numpy().copy()
    ix[5] = [int(np.argmax(np.linalg.norm(db[:, :1200], axis=1))), 7, 9]   # query 5 (whose channel-0 distances are all NaN) gets pairs of its own
    ix[0, 1] = -1
    var, dist = mt.align(_cuda(ix))
    hv, hd = api.match_align("sc", q, db, ix)
    torch.cuda.synchronize()
    v, d = var.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(hv, v) and np.array_equal(hd.view(np.int64), d.view(np.int64))
    assert np.all(v[0, 1] == -1) and np.all(np.isnan(d[0, 1]))
    assert np.all(v[5, :, 0] == -1) and np.all(np.isnan(d[5, :, 0]))
    assert np.all(v[5, :, 1] >= 0) and np.all(np.isfinite(d[5, :, 1]))
    # out of this shard: db_row0 moves the window [db_row0, db_row0 + n) past some of the indices
    var2, dist2 = mt.align(_cuda(ix), db_row0=500)
    v2, d2 = var2.cpu().numpy(), dist2.cpu().numpy()
    out = (ix < 500)
    assert np.all(v2[out] == -1) and np.all(np.isnan(d2[out]))
    # the fused host form: slots 0-1 the SC host form, 2-3 -1 / NaN only where the pair is missing
    m2 = synth.m2dp_database(53, n)
    m2q = synth.m2dp_database(54, m)
    fv, fd = api.match_align_fused(q, m2q, db, m2, ix)
    assert np.array_equal(fv[..., :2], hv) and np.array_equal(fd[..., :2].view(np.int64), hd.view(np.int64))
    mv, md = api.match_align("m2dp", m2q, m2, ix)
    assert np.array_equal(fv[..., 2:], mv) and np.array_equal(fd[..., 2:].view(np.int64), md.view(np.int64))
    with pytest.raises(api.PRError):
        api.match_align("sc", q, db, np.full((m, 1), n, np.int32))     # not a row of hist2
    with pytest.raises(ValueError):
        api.match_align("gist", q, db, ix)
    mt.close()


# ------------------------------------------------------------------------------------------ 5. two shards
def test_two_shards_combine_to_the_one_shard_result():
    n, m, k = 4000, 64, 5
    db = synth.sc_database(61, n)
    q, _ = synth.sc_queries(62, db, m)
    one = _sc_matcher(db, m)
    idx, _ = one.match(_cuda(q), 0, 2.0, k)
    v1, d1 = one.align(idx)
    halves = [(0, _sc_matcher(db[: n // 2], m)), (n // 2, _sc_matcher(db[n // 2:], m))]
    vs, ds = [], []
    for row0, mt in halves:
        mt.match(_cuda(q), 0, 2.0, k, db_row0=row0)
        v, d = mt.align(idx, db_row0=row0)
        vs.append(v); ds.append(d)
    v2, d2 = torch.maximum(vs[0], vs[1]), torch.fmax(ds[0], ds[1])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(v1), _bits(v2)) and np.array_equal(_bits(d1), _bits(d2))
    ix = idx.cpu().numpy()
    assert np.all((vs[0].cpu().numpy()[..., 0] >= 0) == (ix < n // 2))   # exactly one shard filled each pair
    for _, mt in halves:
        mt.close()
    one.close()


# ------------------------------------------------------------------------------------------ 6. growing DB
def test_growing_database_aligns_like_the_bulk_pack():
    n, m, k = 1500, 16, 3
    db = synth.sc_database(71, n)
    q, _ = synth.sc_queries(72, db, m)
    bulk = _sc_matcher(db, m)
    idx, _ = bulk.match(_cuda(q), 0, 2.0, k)
    vb, db_ = bulk.align(idx)
    grow = Matcher("sc", m, n)
    grow.reserve_database(_cuda(db[:100]))
    for s in range(100, n, 350):
        grow.append_database(_cuda(db[s:s + 350]))
    grow.match(_cuda(q), 0, 2.0, k)
    vg, dg = grow.align(idx)
    torch.cuda.synchronize()
    assert grow.n == n
    assert np.array_equal(_bits(vb), _bits(vg)) and np.array_equal(_bits(db_), _bits(dg))
    bulk.close(); grow.close()


def test_f16_arithmetic_matcher_aligns_from_the_raw_rows():
    """The single-f16 matcher arithmetic keeps the raw fp64 rows: its alignment is the default matcher's, bit for bit."""
    n, m, k = 1500, 24, 3
    db = synth.sc_database(75, n)
    q, _ = synth.sc_queries(76, db, m)
    ref = _sc_matcher(db, m)
    idx, _ = ref.match(_cuda(q), 0, 2.0, k)
    vr, dr = ref.align(idx)
    f16 = Matcher("sc", m, n, ctx=api.Context(0, sc_arith="f16", stream=int(torch.cuda.current_stream().cuda_stream)))
    f16.pack_database(_cuda(db))
    f16.match(_cuda(q), 0, 2.0, k)
    vf, df = f16.align(idx)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(vr), _bits(vf)) and np.array_equal(_bits(dr), _bits(df))
    ref.close(); f16.close()


# ------------------------------------------------------------------------------------------ 7. fused
def test_fused_matcher_slots_equal_the_single_type_matchers():
    n, m, k = 1500, 32, 3
    sc_db = synth.sc_database(81, n)
    sc_q, et = synth.sc_queries(82, sc_db, m)
    m2_db = synth.m2dp_database(83, n)
    m2_q = m2_db.reshape(n, 4, 384)[et].reshape(4 * m, 384) + 0.0   # the same places
    fm = FusedMatcher(m, n)
    fm.pack_database(_cuda(sc_db), _cuda(m2_db))
    idx, _ = fm.match(_cuda(sc_q), _cuda(m2_q), 0, 2.0, k)
    fv, fd = fm.align(idx)
    ms = _sc_matcher(sc_db, m)
    ms.match(_cuda(sc_q), 0, 2.0, k)
    sv, sd = ms.align(idx)
    mm = Matcher("m2dp", m, n)
    mm.pack_database(_cuda(m2_db))
    mm.match(_cuda(m2_q), 0, 2.0, k)
    mv, md = mm.align(idx)
    part = fm.local_rerank(idx, k, partial=True)
    torch.cuda.synchronize()
    assert fv.shape == (m, k, 4)
    assert np.array_equal(_bits(fv[..., :2]), _bits(sv)) and np.array_equal(_bits(fd[..., :2]), _bits(sd))
    assert np.array_equal(_bits(fv[..., 2:]), _bits(mv)) and np.array_equal(_bits(fd[..., 2:]), _bits(md))
    p5 = part.cpu().numpy()
    assert np.array_equal(fd.cpu().numpy().transpose(0, 2, 1).view(np.int64), p5[:, 1:, :].view(np.int64))
    hv, hd = api.match_align_fused(sc_q, m2_q, sc_db, m2_db, idx.cpu().numpy())
    assert np.array_equal(hv, fv.cpu().numpy()) and np.array_equal(hd.view(np.int64), _bits(fd))
    for x in (fm, ms, mm):
        x.close()


# ------------------------------------------------------------------------------------------ 8. hipGraph capture
def test_align_captured_in_a_graph_replays_the_same_bits():
    n, m, k = 2000, 16, 5
    db = synth.sc_database(91, n)
    q, _ = synth.sc_queries(92, db, m)
    mt = Matcher.on_new_stream("sc", m, n)
    with torch.cuda.stream(mt.stream):
        mt.pack_database(_cuda(db))
        queries = _cuda(q)
        idx, _ = mt.match(queries, 0, 2.0, k)
        idx_static = idx.clone()
        ve, de = mt.align(idx_static)                                   # eager (also the warm-up)
        idx2 = torch.roll(idx_static, 1, dims=0)
        ve2, de2 = mt.align(idx2)
        ve, de, ve2, de2 = ve.clone(), de.clone(), ve2.clone(), de2.clone()
        mt.stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=mt.stream):
            vg, dg = mt.align(idx_static)
        g.replay()
        mt.stream.synchronize()
        assert np.array_equal(_bits(ve), _bits(vg)) and np.array_equal(_bits(de), _bits(dg))
        idx_static.copy_(idx2)
        g.replay()
        mt.stream.synchronize()
        assert np.array_equal(_bits(ve2), _bits(vg)) and np.array_equal(_bits(de2), _bits(dg))
    mt.close()


# ------------------------------------------------------------------------------------------ 9. end to end: clouds -> match -> align -> pose
def test_end_to_end_relative_pose_from_device_frames():
    rng = np.random.default_rng(101)
    c = 12
    yaws = rng.random(c) * 2 * np.pi
    qs, ds, Rs, ts = [], [], [], []
    for i in range(c):
        base = _scene(rng)
        R, t = _yaw(yaws[i]), np.array([rng.normal(0, 3), rng.normal(0, 0.2), rng.normal(0, 3)])
        qs.append(base + rng.normal(0, 0.02, base.shape))
        ds.append(base @ R.T + t + rng.normal(0, 0.02, base.shape))
        Rs.append(R); ts.append(t)
    P = qs[0].shape[0]
    offs = np.arange(c + 1, dtype=np.int64) * P
    inten = rng.random(c * P).astype(np.float32)                        # the same intensity per physical point in both clouds
    xq, xd = np.concatenate(qs), np.concatenate(ds)
    sig_q, sig_d = api.sc_generate(xq, inten, offs), api.sc_generate(xd, inten, offs)
    fq, fd = api.cloud_frames(xq, inten, offs), api.cloud_frames(xd, inten, offs)
    assert fq.shape == (c, 16) and np.all(fq[:, 13] == P) and np.all(fq[:, 15] == 1.0)
    for i in range(c):                                                  # the oracle's frame up to the eigenvectors' signs
        ref = _frame(qs[i])
        assert np.allclose(fq[i, :3], ref[:3], atol=1e-9)
        assert np.allclose(np.abs(fq[i, 3:6] @ ref[3:6]), 1.0, atol=1e-6)
    mt = _sc_matcher(sig_d, c)
    idx, _ = mt.match(_cuda(sig_q), 0, 2.0, 1)
    var, _ = mt.align(idx)
    torch.cuda.synchronize()
    ix, v = idx.cpu().numpy()[:, 0], var.cpu().numpy()[:, 0, 0]
    assert np.array_equal(ix, np.arange(c))
    T = api.sc_relative_pose(fq, fd[ix], v)
    err = np.array([_rot_err_deg(T[i, :, :3], Rs[i]) for i in range(c)])
    terr = np.array([np.linalg.norm(T[i, :, 3] - ts[i]) for i in range(c)])
    assert err.max() <= 4.0, err
    assert terr.max() <= 0.5, terr
    mt.close()


# ------------------------------------------------------------------------------------------ 10. CLI
@pytest.mark.parametrize("type_", ["sc", "m2dp", "delight"])
def test_cli_align_out_equals_match_align(tmp_path, type_):
    n, m, k = 120, 20, 2
    if type_ == "sc":
        db = synth.sc_database(111, n); q, _ = synth.sc_queries(112, db, m)
    elif type_ == "m2dp":
        db = synth.m2dp_database(113, n); q, _ = synth.m2dp_queries(114, db, m)
    else:
        db = synth.delight_database(115, n); q, _ = synth.delight_queries(116, db, m)
    h1, h2 = str(tmp_path / "h1.bin"), str(tmp_path / "h2.bin")
    api.write_signatures(h1, q); api.write_signatures(h2, db)
    out, al = str(tmp_path / "out.txt"), str(tmp_path / "align.txt")
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", type_, "--hist1", h1, "--hist2", h2, "--topk", str(k), "--out", out,
                        "--align_out", al], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    res = np.loadtxt(out).reshape(m, k, 2)
    ix = res[..., 0].astype(np.int32)
    got = np.loadtxt(al, dtype=np.int64).reshape(m, k, 2)
    want, _ = api.match_align(type_, q, db, ix)
    assert np.array_equal(got, want)
    assert np.all(got[:, 0, 0] >= 0)
    # the online form: indices are rows of hist1
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", type_, "--hist1", h2, "--hist2", h2, "--topk", str(k), "--out", out,
                        "--align_out", al, "--online", "1", "--mask_width", "3"], capture_output=True, text=True, timeout=300)
    if type_ == "delight":
        assert r.returncode == 1                                        # --online needs sc | m2dp
        return
    assert r.returncode == 0, r.stderr
    res = np.loadtxt(out).reshape(n, k, 2)
    ix = np.where(np.isnan(res[..., 1]), -1, res[..., 0]).astype(np.int32)
    got = np.loadtxt(al, dtype=np.int64).reshape(n, k, 2)
    want, _ = api.match_align(type_, db, db, ix)
    assert np.array_equal(got, want)
