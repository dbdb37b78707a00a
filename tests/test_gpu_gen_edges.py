"""The SC / M2DP / DELIGHT generators at bin edges and under translation, against the oracle.

Fixed frames (gen_edge_cases.py): pr_*_generate_frames_dev on hand-made frames, so the aligned coordinates are known bit for bit and the
oracle's *_aligned entry points give the expected signature of exactly those points.  The probes sit on and next to every sector edge and a
spread of ring edges, inside and outside every accept margin of the fp32 classifiers (fast_bins.hpp), at the first / last / tail-loop /
padding-lane indices of the kernels' loops; test_gen_edge_cases_cpu.py shows that ONE probe binned on the wrong side changes the expected
signature.  Equality is exact wherever the values are integers or differences of identical doubles.

PCA frames: clouds translated by up to a UTM northing (the moments are accumulated about the cloud's first point, frames.hpp) and degenerate
clouds.  Measured on an MI355X for synth.scene_cloud(42, 1, 20011) translated by (s, -s/2, s/3): largest || v_gpu x v_oracle || over the three
eigenvectors with raw moments (sum p p^T - n mean mean^T, the form before the pivot) -> with moments about the first point:
    s = 0: 4.4e-16 -> 4.5e-16    s = 1e3: 2.1e-13 -> 7.2e-16    s = 1e5: 6.6e-10 -> 4.4e-16    s = 5.7e6: 1.3e-5 -> 5.6e-16 rad
(the 1500-point cloud: 5.1e-16 -> 5.8e-16, 1.1e-13 -> 4.9e-16, 3.3e-10 -> 5.8e-16, 6.7e-6 -> 1.3e-16), and the SC structure channel of the
raw form was 2.9e-8 (s = 1e5) and 5.3e-4 m (s = 5.7e6) off the oracle's: with raw moments the tests below fail from s = 1e5 on (at s = 1e3
the raw form is still inside the 1e-12 rad bound, so those parametrisations do not tell the two forms apart).
"""
import functools

import numpy as np
import pytest

import gen_edge_cases as G
import oracle_lib
from so_dso_place_recognition_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from so_dso_place_recognition_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    """a context of this module's own: the sticky warning bits of degenerate clouds stay out of the default context other modules assert on"""
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return G.all_cases()


@functools.lru_cache(maxsize=None)
def _expected(kind):
    out = {}
    for c in G.all_cases()[kind]:
        if kind == "sc":
            out[c.name] = oracle_lib.sc_signature_aligned(c.aligned, c.inten, c.max_rho)
        elif kind == "m2dp":
            out[c.name] = oracle_lib.m2dp_signature_aligned(c.aligned, c.inten, c.max_rho)
        else:
            out[c.name] = oracle_lib.delight_signature_aligned(c.aligned, c.inten)
    return out


def _generate(ctx, kind, batch, have_ave=1):
    """pr_<kind>_generate_frames_dev over the clouds of `batch` with their hand-made frames -> [len(batch), rows, cols]"""
    import torch
    xyz = np.concatenate([c.xyz for c in batch])
    inten = np.concatenate([c.inten for c in batch])
    offs = np.concatenate([[0], np.cumsum([len(c.xyz) for c in batch])]).astype(np.int64)
    frames = np.stack([c.frame for c in batch]).copy()
    if not have_ave:
        frames[:, 14:] = 0.0                               # the call computes the averages itself
    dx, di, do, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xyz, inten, offs, frames))
    N = len(batch)
    rows, cols = {"sc": (1, 2400), "m2dp": (4, 384), "delight": (16, 256)}[kind]
    out = torch.full((N * rows, cols), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = ctx.lib
    if kind == "sc":
        ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, dx.data_ptr(), di.data_ptr(), do.data_ptr(), N, batch[0].max_rho, df.data_ptr(), have_ave, out.data_ptr()))
    elif kind == "m2dp":
        ctx.check(lib.pr_m2dp_generate_frames_dev(ctx.h, dx.data_ptr(), di.data_ptr(), do.data_ptr(), N, batch[0].max_rho, df.data_ptr(), have_ave, out.data_ptr()))
    else:
        ctx.check(lib.pr_delight_generate_frames_dev(ctx.h, dx.data_ptr(), di.data_ptr(), do.data_ptr(), N, df.data_ptr(), out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy().reshape(N, rows, cols)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ fixed frames: SC
@pytest.mark.parametrize("have_ave", [1, 0])
def test_sc_edges_on_fixed_frames(ctx, cases, have_ave):
    want = _expected("sc")
    got = _generate(ctx, "sc", cases["sc"], have_ave)[:, 0]
    for c, g in zip(cases["sc"], got):
        o = want[c.name]
        bad = np.nonzero(_bits(g) != _bits(o))[0]
        # occupancy and binarised intensity equal, structure = max - min of identical doubles: the bits of the oracle
        assert np.array_equal(g[1200:], o[1200:]), (c.name, bad[:8], g[bad[:8]], o[bad[:8]])
        assert np.array_equal(g[:1200], o[:1200]), (c.name, bad[:8], g[bad[:8]], o[bad[:8]])


# ------------------------------------------------------------------------------------------------ fixed frames: DELIGHT
def test_delight_edges_on_fixed_frames(ctx, cases):
    want = _expected("delight")
    got = _generate(ctx, "delight", cases["delight"])
    for c, g in zip(cases["delight"], got):
        o = want[c.name]
        bad = np.argwhere(g != o)
        assert np.array_equal(g, o), (c.name, bad[:8], [(g[tuple(b)], o[tuple(b)]) for b in bad[:8]])


# ------------------------------------------------------------------------------------------------ fixed frames: M2DP
@pytest.mark.parametrize("have_ave", [1, 0])
def test_m2dp_edges_on_fixed_frames_both_templates(api, ctx, cases, have_ave):
    """batches of 3 clouds take the 4-plane template (nc * 16 < 768), the same cases tiled to 48 clouds the 16-plane one: the oracle's rows
    within 1e-9, no row named by pr_m2dp_svd_rows, and the two templates give the same bits"""
    want = _expected("m2dp")
    cs = cases["m2dp"]
    assert len(cs) == 6
    ctx.take_warnings()                                 # (start from clean warning bits whatever ran before on this context)
    small = np.concatenate([_generate(ctx, "m2dp", cs[0:3], have_ave), _generate(ctx, "m2dp", cs[3:6], have_ave)])
    assert len(api.m2dp_svd_rows(ctx)) == 0
    for c, g in zip(cs, small):
        err = np.abs(g - want[c.name]).max()
        print(f"{c.name}: |g - o| = {err:.2e}")
        assert err < 1e-9, (c.name, err)
    tiled = _generate(ctx, "m2dp", cs * 8, have_ave)
    assert len(api.m2dp_svd_rows(ctx)) == 0 and not (ctx.take_warnings() & 2)
    for t in range(8):
        assert np.array_equal(_bits(tiled[6 * t:6 * t + 6]), _bits(small)), t


# ------------------------------------------------------------------------------------------------ a case alone and inside a batch
@pytest.mark.parametrize("kind,name", [("sc", "sc_sector0_rot"), ("m2dp", "m2dp_257_rot"), ("delight", "delight_1537")])
def test_case_in_the_middle_of_a_batch_gives_the_bits_it_gives_alone(ctx, cases, kind, name):
    cs = cases[kind]
    k = [c.name for c in cs].index(name)
    assert 0 < k < len(cs) - 1
    alone = _generate(ctx, kind, [cs[k]])[0]
    batch = _generate(ctx, kind, cs)[k]
    assert np.array_equal(_bits(alone), _bits(batch))


# ------------------------------------------------------------------------------------------------ PCA frames of shifted clouds
SHIFTS = (0.0, 1e3, 1e5, 5.7e6)                 # the last: a UTM northing
CLOUDS = {"20011": (42, 1, 20011), "1500": (42, 1, 1500)}


@functools.lru_cache(maxsize=None)
def _shifted(cloud, s):
    xyz, it = synth.scene_cloud(*CLOUDS[cloud])
    return xyz + np.array([s, -s / 2, s / 3]), it, np.array([0, len(xyz)], np.int64)


@functools.lru_cache(maxsize=None)
def _oracle_frame(cloud, s):
    xyz, _, _ = _shifted(cloud, s)
    al, ev = oracle_lib.align_pca(xyz)
    return al, ev.T                                  # rows v0, v1, v2 as in a frame


def _max_angle(R, E):
    return max(np.linalg.norm(np.cross(R[j], E[j])) for j in range(3))


def _check_rotation(R, tol=1e-12):
    assert np.isfinite(R).all()
    assert np.abs(R @ R.T - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1) <= tol


@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("cloud", list(CLOUDS))
def test_frames_of_shifted_clouds(api, ctx, cloud, s):
    """eigenvectors within 1e-12 rad of the oracle's (which centres first) whatever the translation; the mean within 4 ulp of the coordinate
    it is the mean of (per component, ulp at |t_k|; for s = 0 at max_rho = 45, the largest coordinate of an untranslated scene cloud)"""
    xyz, it, offs = _shifted(cloud, s)
    f = api.cloud_frames(xyz, it, offs, ctx=ctx)[0]
    R = f[3:12].reshape(3, 3)
    _, E = _oracle_frame(cloud, s)
    ang = _max_angle(R, E)
    mean = xyz.astype(np.longdouble).mean(0)
    t = np.array([s, -s / 2, s / 3])
    tol = 4 * np.spacing(np.maximum(np.abs(t), 45.0))
    dm = np.abs(f[:3].astype(np.longdouble) - mean).astype(np.float64)
    print(f"cloud {cloud} s = {s:g}: angle {ang:.2e} rad, mean off by {dm.max():.2e} (tolerance {tol.min():.2e})")
    assert f[13] == len(xyz)
    assert ang <= 1e-12, ang
    assert (dm <= tol).all(), (dm, tol)
    _check_rotation(R)


@functools.lru_cache(maxsize=None)
def _oracle_sigs(cloud, s):
    xyz, it, offs = _shifted(cloud, s)
    al, _ = _oracle_frame(cloud, s)
    # pre-condition, in longdouble on the oracle's aligned coordinates: nothing within 1e-6 bins (metres) of an edge, so that frames that
    # agree to 1e-12 rad cannot put a point into another bin.  M2DP on the 20011-point cloud is the exception: 5e6 projections (64 planes x
    # 4 variants) cannot all keep 1e-6 bins away for any seed - the closest is 4.2e-9 ... 6.3e-9 bins over the four translations - so its
    # guard is 1e-9 bins: 1e-12 rad of frame error is 3e-12 sector bins and, at 45 m, 8e-12 ring bins.
    assert G.sc_guard(al).min() > G.GUARD_BINS and G.delight_guard(al).min() > G.GUARD_M
    assert G.m2dp_guard(al).min() > (G.GUARD_BINS if cloud == "1500" else 1e-9)
    sig = dict(sc=oracle_lib.sc_generate(xyz, it, offs), delight=oracle_lib.delight_generate(xyz, it, offs),
               m2dp=oracle_lib.m2dp_generate(xyz, it, offs))
    return sig


@pytest.mark.parametrize("path", ["default", "batched", "cluster"])
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("cloud", list(CLOUDS))
def test_signatures_of_shifted_clouds(api, ctx, monkeypatch, cloud, s, path):
    xyz, it, offs = _shifted(cloud, s)
    want = _oracle_sigs(cloud, s)
    if path != "default":
        monkeypatch.setenv("PR_SC_GEN", path)
    g = api.sc_generate(xyz, it, offs, ctx=ctx)
    o = want["sc"]
    assert np.array_equal(g[:, 1200:], o[:, 1200:]) and np.array_equal(g[:, :1200] != 0, o[:, :1200] != 0)
    assert np.abs(g[:, :1200] - o[:, :1200]).max() <= 1e-10 + 16 * np.spacing(s)
    if path != "default":
        return                                        # PR_SC_GEN selects among SC paths only
    assert np.array_equal(api.delight_generate(xyz, it, offs, ctx=ctx), want["delight"])
    gm = api.m2dp_generate(xyz, it, offs, ctx=ctx)
    assert np.abs(gm - want["m2dp"]).max() < 1e-9 and len(api.m2dp_svd_rows(ctx)) == 0


# ------------------------------------------------------------------------------------------------ degenerate clouds
def _degenerate_clouds():
    rng = np.random.default_rng(2024)
    t = np.array([12.5, -3.25, 40.0])
    d = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
    n = np.array([0.3, 0.9, -0.2]) / np.linalg.norm([0.3, 0.9, -0.2])
    u = np.cross(n, [1.0, 0, 0]); u /= np.linalg.norm(u)
    w = np.cross(n, u)
    ax = np.array([0.6, 0.0, 0.8])
    b1 = np.cross(ax, [0, 1.0, 0]); b1 /= np.linalg.norm(b1)
    b2 = np.cross(ax, b1)
    ph = np.arange(500) * (2 * np.pi / 500)
    cl = {
        "one": rng.normal(0, 5, (1, 3)) + t,
        "two": rng.normal(0, 5, (2, 3)) + t,
        "three": rng.normal(0, 5, (3, 3)) + t,
        "line": t + np.linspace(-20, 20, 500)[:, None] * d,
        "plane": t + rng.uniform(-20, 20, (500, 1)) * u + rng.uniform(-6, 6, (500, 1)) * w,
        "cylinder": t + 3.0 * (np.cos(ph)[:, None] * b1 + np.sin(ph)[:, None] * b2) + np.tile(np.linspace(-9, 9, 20), 25)[:, None] * ax,
        "same": np.tile(t, (64, 1)),
    }
    return cl, dict(line=("axis", d), plane=("normal", n), cylinder=("axis", ax))


@pytest.mark.parametrize("name", ["one", "two", "three", "line", "plane", "cylinder", "same"])
def test_frames_and_signatures_of_degenerate_clouds(api, ctx, name):
    """ill-conditioned eigenvectors are not compared: mean, count, a finite proper rotation, the direction that IS defined (the line's axis =
    the largest eigenvector, the plane's normal = the smallest, the cylinder's axis = the largest: two equal eigenvalues across it) within
    1e-9 of the oracle's, finite signatures, DELIGHT's total = the number of points with an intensity in [0, 256)"""
    clouds, defined = _degenerate_clouds()
    xyz = np.ascontiguousarray(clouds[name])
    P = len(xyz)
    it = (np.arange(P) * 37 % 300 - 20).astype(np.float32)          # some below 0, some from 256 up
    offs = np.array([0, P], np.int64)
    f = api.cloud_frames(xyz, it, offs, ctx=ctx)[0]
    assert np.isfinite(f).all() and f[13] == P
    assert np.abs(f[:3] - xyz.astype(np.longdouble).mean(0).astype(np.float64)).max() <= 4 * np.spacing(np.abs(xyz).max())
    R = f[3:12].reshape(3, 3)
    _check_rotation(R)
    if name in defined:
        which, direction = defined[name]
        _, ev = oracle_lib.align_pca(xyz)
        j = 0 if which == "normal" else 2
        assert np.linalg.norm(np.cross(R[j], ev[:, j])) <= 1e-9 and np.linalg.norm(np.cross(R[j], direction)) <= 1e-9
    assert np.isfinite(api.sc_generate(xyz, it, offs, ctx=ctx)).all()
    assert np.isfinite(api.m2dp_generate(xyz, it, offs, ctx=ctx)).all()
    ctx.take_warnings()                                 # (a degenerate cloud's leading singular pair may be named: not this test's subject)
    dl = api.delight_generate(xyz, it, offs, ctx=ctx)
    assert np.isfinite(dl).all() and dl.sum() == ((it >= 0) & (it < 256)).sum()
