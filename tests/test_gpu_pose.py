"""The pose seeds and the stream-ordered verify chain on the device (csrc/pose.hip: pr_relative_pose_dev, pr_verify_select_dev,
pr_verify_pairs_dev and their Python forms) against the host form pr_relative_pose, the restatement pose_np.py, the composition of the
separate calls and the host-seeded Matcher.verify.

Seed kernel against the host form: pair_src / pair_dst equal; R within 1e-12, t within 1e-12 x (1 + |mu_q| + |mu_db|) - unit-scale fp64
products and three-term sums differ by a few 1e-16 at most (both sides are built without contraction, so they are expected to agree
bit for bit; the margin is four orders above that and far below anything ICP can see)."""
import ctypes as C

import numpy as np
import pytest

import icp_cases
import pose_np
from resident_fuzz_cases import bits_equal
from test_pose_cpu import SELECT_CASES, TYPES, random_frames, stats_rec
from so_dso_place_recognition_amd import _lib, api

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-10            # what the order of the update's sums may move T and rmse


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def icp_out(c):
    """Result tensors of icp_refine_torch that no fill kernel on torch's stream touches (the matcher's context runs on a stream of its own)."""
    return (torch.empty((c, 3, 4), dtype=torch.float64, device="cuda"), torch.empty((c, 32), dtype=torch.uint8, device="cuda"))


def stats_host(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), api.ICP_STATS)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------ 1. the seed kernel against pr_relative_pose
@pytest.mark.parametrize("name,t", TYPES)
def test_seed_kernel_equals_the_host_form(ctx, name, t):
    rng = np.random.default_rng(100 + t)
    nv, db_row0, n_local = pose_np.VARIANTS[t], 5, 40
    H = 1 if name == "delight" else 2
    fd = random_frames(rng, n_local)
    fd[7, 13] = 2                                   # a frame of two points
    fd[11, 4] = np.nan                              # a frame with a NaN
    worst_R = worst_t = 0.0
    covered = set()
    for m in (0, 1, 63, 64, 65, 257):
        fq = random_frames(rng, m)
        if m > 20:
            fq[3, 13] = 2; fq[9, 0] = np.inf
        for k in (1, 3):
            width = 4 if (name != "delight" and k == 3) else H         # the [m, k, 4] tensor of align, or a tight one
            idx = rng.integers(0, db_row0 + n_local + 5, (m, k)).astype(np.int32)     # rows below, inside and above the shard
            var = np.zeros((m, k, width), np.int32)
            var[..., 0] = (np.arange(m * k).reshape(m, k) * 7 + m) % nv
            if H == 2:
                var[..., 1] = (var[..., 0] + rng.integers(0, 3, (m, k))) % nv         # a third of the second hypotheses repeat the first
            if m > 20:
                idx[0, 0] = -1; idx[1, 0] = db_row0 + 7; idx[2, 0] = db_row0 + 11; idx[4, 0] = db_row0 - 1; idx[5, 0] = db_row0 + n_local
                var[6, 0, 0] = -1; var[7, 0, 0] = nv; var[8, 0, H - 1] = nv + 3; var[10, 0, H - 1] = -1
            T0, src, dst = api.relative_pose_torch(name, dev(fq.reshape(m, 16)), dev(fd), dev(idx, np.int32), dev(var, np.int32)[..., :H] if width == 4
                                                   else dev(var, np.int32), H, db_row0, ctx=ctx)
            ctx.sync()
            T0, src, dst = T0.cpu().numpy(), src.cpu().numpy(), dst.cpu().numpy()
            assert T0.shape == (m, k, H, 3, 4)
            wT, wsrc, wdst = pose_np.seed_slots(t, fq.reshape(m, 16), fd, db_row0, idx, var, H)
            assert np.array_equal(src, wsrc) and np.array_equal(dst, wdst), (m, k)
            has = wsrc >= 0
            assert np.array_equal(T0[~has], np.tile(pose_np.IDENT, (int((~has).sum()), 1, 1)))
            if has.any():
                qq, ll = wsrc[has], wdst[has]
                vv = np.broadcast_to(var[..., :H], (m, k, H))[has]
                host = api.relative_pose(name, fq[qq], fd[ll], vv)
                got = T0[has]
                scale = 1 + np.linalg.norm(fq[qq, :3], axis=1) + np.linalg.norm(fd[ll, :3], axis=1)
                worst_R = max(worst_R, float(np.abs(got[:, :, :3] - host[:, :, :3]).max()))
                worst_t = max(worst_t, float((np.abs(got[:, :, 3] - host[:, :, 3]).max(1) / scale).max()))
                covered |= set(vv.tolist())
            if m > 20:
                assert not has[0, 0].any() and not has[1, 0].any() and not has[2, 0].any() and not has[4, 0].any() and not has[5, 0].any()
                assert not has[3].any() and not has[9].any() and not has[6, 0, 0] and not has[7, 0, 0]
    print("   %s: device seed against the host form: max |dR| %.2e, max |dt| / (1 + |mu_q| + |mu_db|) %.2e" % (name, worst_R, worst_t))
    assert covered == set(range(nv))
    assert worst_R <= 1e-12 and worst_t <= 1e-12


def test_select_kernel_on_hand_made_statistics(ctx):
    for H in (1, 2):
        cases = [c for c in SELECT_CASES if len(c[0]) == H]
        for mf, mr in sorted({(c[1], c[2]) for c in cases}):
            grp = [c for c in cases if (c[1], c[2]) == (mf, mr)]
            c = len(grp)
            st = np.concatenate([stats_rec(g[0]) for g in grp])
            Th = np.arange(c * H * 12, dtype=np.float64).reshape(c, H, 3, 4)
            dT = torch.zeros((c, 3, 4), dtype=torch.float64, device="cuda")
            dst_ = torch.zeros((c, 32), dtype=torch.uint8, device="cuda")
            acc = torch.zeros(c, dtype=torch.uint8, device="cuda"); hyp = torch.full((c,), -7, dtype=torch.int32, device="cuda")
            dTh = dev(Th); dsh = torch.from_numpy(np.frombuffer(st.tobytes(), np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
            ctx.check(ctx.lib.pr_verify_select_dev(ctx.h, p(dTh), p(dsh), c, H, mf, mr, p(dT), p(dst_), p(acc), p(hyp)))
            ctx.sync()
            got = stats_host(dst_)
            for i, g in enumerate(grp):
                assert (int(hyp[i]), bool(acc[i])) == g[3] == pose_np.select(st[i * H:(i + 1) * H], mf, mr), g
                assert np.array_equal(dT[i].cpu().numpy(), Th[i, g[3][0]]) and got[i].tobytes() == st[i * H + g[3][0]].tobytes()


# ------------------------------------------------------------------------------------------ 2. the chain against its parts and the host-seeded verify
@pytest.fixture(scope="module")
def sc_world():
    """The six committed ICP cases as one query set (the P clouds) and one DB (the Q clouds) behind an SC matcher."""
    from so_dso_place_recognition_amd.matcher import Matcher
    names = list(icp_cases.CASES)
    cs = [icp_cases.case(n) for n in names]
    rng = np.random.default_rng(5)
    xq, oq = icp_cases.csr([c["P"] for c in cs]); xd, od = icp_cases.csr([c["Q"] for c in cs])
    iq, idn = rng.random(len(xq)).astype(np.float32), rng.random(len(xd)).astype(np.float32)
    sig_q, sig_d = api.sc_generate(xq, iq, oq), api.sc_generate(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    mt = Matcher("sc", len(cs), len(cs), ctx=api.Context(0, exact_statistics=True))
    mt.pack_database(dev(sig_d))
    mt.match(dev(sig_q), 0, 2.0, 1)
    w = dict(mt=mt, cs=cs, cq=(dev(xq), dev(oq, np.int64)), cd=(dev(xd), dev(od, np.int64)), fq=fq, fd=fd, dfq=dev(fq), dfd=dev(fd),
             ms=max(len(c["P"]) for c in cs), md=max(len(c["Q"]) for c in cs))
    yield w
    mt.close()


def test_verify_dev_equals_its_parts_and_the_host_seeded_verify(sc_world):
    w = sc_world; mt = w["mt"]; n = len(w["cs"])
    idx = dev(np.stack([np.arange(n), (np.arange(n) + 1) % n], 1), np.int32)          # the true entry and another place
    idx[2, 1] = -1
    kw = dict(max_corr=1.0, min_fitness=0.6, max_rmse=0.3, **{k: v for k, v in icp_cases.PARAMS.items() if k != "max_corr"})
    T, st, acc, hyp = mt.verify_dev(idx, w["cq"], w["cd"], w["dfq"], w["dfd"], w["ms"], w["md"], **kw)
    var, _ = mt.align(idx)
    T0, src, dst = api.relative_pose_torch("sc", w["dfq"], w["dfd"], idx, var, 1, ctx=mt.ctx)
    T2, st2 = api.icp_refine_torch(*w["cq"], *w["cd"], src.reshape(-1), dst.reshape(-1), T0.reshape(-1, 3, 4), w["ms"], w["md"], ctx=mt.ctx,
                                   out=icp_out(src.numel()), **icp_cases.PARAMS)
    hT, hst, hacc = mt.verify(idx, w["cq"], w["cd"], w["fq"], w["fd"], w["ms"], w["md"], **kw)
    torch.cuda.synchronize()
    assert bits_equal(T.cpu().numpy().reshape(-1, 3, 4), T2.cpu().numpy()) and bytes(st.cpu().numpy()) == bytes(st2.cpu().numpy())
    assert not hyp.any()
    s, hs = stats_host(st), stats_host(hst)
    for f in ("status", "iters", "n_inl", "fitness"):
        assert np.array_equal(s[f], hs[f]), f
    assert np.array_equal(acc.cpu().numpy(), hacc.cpu().numpy())
    dT, dr = np.abs(T.cpu().numpy() - hT.cpu().numpy()).max(), np.abs(s["rmse"] - hs["rmse"]).max()
    print("   verify_dev against the host-seeded verify: max |dT| %.2e, max |d rmse| %.2e" % (dT, dr))
    assert dT <= TOL and dr <= TOL
    assert s["status"].reshape(n, 2)[2, 1] == _lib.ICP_NO_PAIR and not acc[2, 1]
    # no queries: a valid call that launches nothing
    e = api.verify_pairs_torch("sc", w["cq"], w["cd"], w["dfq"][:0], w["dfd"], idx[:0], var[:0], w["ms"], w["md"], 1, ctx=mt.ctx, **icp_cases.PARAMS)
    assert e[0].shape == (0, 2, 3, 4) and e[1].shape == (0, 2, 32) and e[2].shape == (0, 2) and e[3].shape == (0, 2)
    for H in (1, 2):
        e = api.verify_pairs_torch("sc", w["cq"], w["cd"], w["dfq"], w["dfd"], idx[:, :0], var[:, :0], w["ms"], w["md"], H, ctx=mt.ctx)    # k = 0
        assert e[0].shape == (n, 0, 3, 4)
    torch.cuda.synchronize()
    print("   accepted:", acc.cpu().numpy().astype(int).tolist())


# ------------------------------------------------------------------------------------------ 3. two hypotheses
def test_two_hypotheses_keep_the_better_one(sc_world):
    w = sc_world; mt = w["mt"]; n = len(w["cs"])
    idx = dev(np.arange(n)[:, None], np.int32)
    v = mt.align(idx)[0][..., 0].cpu().numpy().reshape(n)                             # the structure channel's variants
    off = (v + 60) % 120                                                              # 30 sectors away: the scene seen backwards
    var = np.stack([off, v], 1).reshape(n, 1, 2)
    var[1, 0] = (v[1], v[1])                                                          # both channels agree
    var[2, 0] = (-1, -1)                                                              # no pose at all
    var[3, 0] = (v[3], off[3])                                                        # the right one first
    dv = dev(var, np.int32)
    T, st, acc, hyp = api.verify_pairs_torch("sc", w["cq"], w["cd"], w["dfq"], w["dfd"], idx, dv, w["ms"], w["md"], 2, ctx=mt.ctx,
                                             **icp_cases.PARAMS)
    T0, src, dst = api.relative_pose_torch("sc", w["dfq"], w["dfd"], idx, dv, 2, ctx=mt.ctx)
    Th, sth = api.icp_refine_torch(*w["cq"], *w["cd"], src.reshape(-1), dst.reshape(-1), T0.reshape(-1, 3, 4), w["ms"], w["md"], ctx=mt.ctx,
                                   out=icp_out(src.numel()), **icp_cases.PARAMS)
    torch.cuda.synchronize()
    Th = Th.cpu().numpy().reshape(n, 2, 3, 4); sh = stats_host(sth).reshape(n, 2)
    T = T.cpu().numpy().reshape(n, 3, 4); s = stats_host(st); acc = acc.cpu().numpy().reshape(n); hyp = hyp.cpu().numpy().reshape(n)
    for i in range(n):
        wh, wa = pose_np.select(sh[i], 0.5, 0.5)
        print("  pair", i, "hyp", hyp[i], "accepted", acc[i], "fitness", sh[i]["fitness"], "rmse", sh[i]["rmse"], "status", sh[i]["status"])
        assert (hyp[i], bool(acc[i])) == (wh, wa)
        assert bits_equal(T[i], Th[i, wh]) and s[i].tobytes() == sh[i, wh].tobytes()
    assert hyp[0] == 1 and acc[0] and hyp[4] == 1 and acc[4] and hyp[5] == 1 and acc[5]
    assert hyp[1] == 0 and sh[1, 1]["status"] == _lib.ICP_NO_PAIR and acc[1]
    assert hyp[2] == 0 and not acc[2] and (sh[2]["status"] == _lib.ICP_NO_PAIR).all()
    assert hyp[3] == 0 and acc[3]


# ------------------------------------------------------------------------------------------ 4. M2DP and DELIGHT end to end
@pytest.mark.parametrize("name,H", (("m2dp", 1), ("m2dp", 2), ("delight", 1)))
def test_m2dp_and_delight_match_verify_dev_on_a_generated_drive(name, H):
    """match -> verify_dev for an M2DP and a DELIGHT matcher, with the acceptance and pose-error thresholds of test_gpu_icp.py's SC drive
    (accepted at min_fitness 0.6 / max_rmse 0.3, under 0.2 degrees and 0.05 m; the second candidate - another place - not accepted).
    The drive is pose_drive.drive(): 6 places of the box scene (synth.scene_cloud, seed 411, 2000 points), each seen twice as 90 %
    subsets with 2 cm jitter, the DB view moved by a random yaw, a tilt of up to 2 degrees and a few metres.  It was chosen on the CPU
    with the restatements alone (the oracle's signatures and PCA frames, pose_np's argmin and seed, icp_np): every true revisit's seed
    is within 1.4 degrees and 0.55 m for both types (M2DP variants 0, 15, 5, 14, 1, 4; DELIGHT 0, 0, 0, 2, 2, 2), converges in 5 - 8
    iterations to at most 0.014 degrees and 5.3 mm with fitness 0.959 - 0.973 and rmse 0.163 - 0.171; seed 412 does as well.  All twelve
    frames are right-handed there; the handedness of the device's frames is printed, since a mirrored pair is outside either
    descriptor's variant set."""
    import pose_drive
    from so_dso_place_recognition_amd.matcher import Matcher
    qs, ds, iq, idn, Rs, ts = pose_drive.drive()
    c = len(qs)
    xq, oq = icp_cases.csr(qs); xd, od = icp_cases.csr(ds)
    gen = {"m2dp": api.m2dp_generate, "delight": api.delight_generate}[name]
    sig_q, sig_d = gen(xq, iq, oq), gen(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    mt = Matcher(name, c, c, ctx=api.Context(0, exact_statistics=True))
    mt.pack_database(dev(sig_d))
    idx, _ = mt.match(dev(sig_q), 0, 2.0, 2)
    T, stats, acc, hyp = mt.verify_dev(idx, (dev(xq), dev(oq, np.int64)), (dev(xd), dev(od, np.int64)), dev(fq), dev(fd), max(len(q) for q in qs),
                                       max(len(d) for d in ds), hypotheses=H, max_corr=1.0, min_fitness=0.6, max_rmse=0.3)
    torch.cuda.synchronize()
    ix = idx.cpu().numpy(); T = T.cpu().numpy(); acc = acc.cpu().numpy(); st = stats_host(stats).reshape(c, 2)
    handed = [(np.sign(np.linalg.det(pose_np.E_of(a))), np.sign(np.linalg.det(pose_np.E_of(b)))) for a, b in zip(fq, fd)]
    print("   handedness of the frames (query, DB):", handed)
    assert np.array_equal(ix[:, 0], np.arange(c))
    for i in range(c):
        er, et = icp_cases.pose_error(T[i, 0], Rs[i], ts[i])
        print("  place", i, "status", st[i, 0]["status"], "iters", st[i, 0]["iters"], "fitness %.3f rmse %.3f" % (st[i, 0]["fitness"], st[i, 0]["rmse"]),
              "err %.3f deg %.3f m" % (er, et), "hyp", int(hyp[i, 0]), "| second candidate accepted:", bool(acc[i, 1]))
        assert acc[i, 0] and er < 0.2 and et < 0.05
        assert not acc[i, 1]                                                    # another place does not verify
    mt.close()


# ------------------------------------------------------------------------------------------ 5. capture
@pytest.mark.parametrize("name,H", (("sc", 2), ("m2dp", 2), ("delight", 1)))
def test_verify_dev_is_capturable_and_replays_bit_equal(name, H):
    from so_dso_place_recognition_amd import synth
    from so_dso_place_recognition_amd.matcher import Matcher
    N, P = 5, 1500
    xyz, it, offs = synth.scene_clouds(61, N, P)
    rng = np.random.default_rng(62)
    xq = xyz + rng.normal(0, 0.02, xyz.shape)                                         # the same places seen again
    gen = {"sc": api.sc_generate, "m2dp": api.m2dp_generate, "delight": api.delight_generate}[name]
    sig_q, sig_d = gen(xq, it, offs), gen(xyz, it, offs)
    fq, fd = api.cloud_frames(xq, it, offs), api.cloud_frames(xyz, it, offs)
    st_ = torch.cuda.Stream()
    with torch.cuda.stream(st_):
        mt = Matcher(name, N, N, ctx=api.Context(0, stream=int(st_.cuda_stream)))
        mt.pack_database(dev(sig_d))
        mt.match(dev(sig_q), 0, 2.0, 2)
        cq, cd = (dev(xq), dev(offs, np.int64)), (dev(xyz), dev(offs, np.int64))
        dfq, dfd = dev(fq), dev(fd)
        idx_a = np.stack([np.arange(N), (np.arange(N) + 2) % N], 1)
        idx_b = np.stack([(np.arange(N) + 1) % N, np.arange(N)], 1); idx_b[0, 0] = -1
        idx = dev(idx_a, np.int32)
        args = (idx, cq, cd, dfq, dfd, P, P)
        kw = dict(hypotheses=H, max_iter=8)
        out = mt.verify_dev(*args, **kw)                                              # eager: also the covering warm-up
        st_.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st_):
            mt.verify_dev(*args, out=out, **kw)
        idx.copy_(dev(idx_b, np.int32))
        for o in out:
            o.zero_()
        g.replay()
        st_.synchronize()
        got = [o.cpu().numpy().copy() for o in out]
        want = mt.verify_dev(*args, **kw)                                             # eager, on the changed idx
        st_.synchronize()
        want = [o.cpu().numpy() for o in want]
        assert bits_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        s = stats_host(torch.from_numpy(got[1])).reshape(N, 2)
        assert s["status"][0, 0] == _lib.ICP_NO_PAIR and (s["status"][1:] != _lib.ICP_NO_PAIR).all()
        print("  ", name, "accepted", got[2].astype(int).tolist(), "hyp", got[3].tolist())
        mt.close()
