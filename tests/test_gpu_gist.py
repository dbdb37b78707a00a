"""GIST generation on the GPU (pr_gist_generate / pr_gist_generate_dev, gist_gen.hip) against the fp64 restatement of
libgist's bw_gist_scaletab (tests/gist_np.py), its exactness properties, its errors, and the drop-in bin/test_gist."""
import os
import subprocess

import numpy as np
import pytest

import gist_np
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")

pytestmark = pytest.mark.gpu


def _smooth(rng, shape, sigma):
    """Gaussian-smoothed noise (periodic), rescaled to [0, 1]."""
    h, w = shape
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.fftfreq(w)[None, :]
    x = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * np.exp(-2 * (np.pi * sigma) ** 2 * (fx ** 2 + fy ** 2))))
    return (x - x.min()) / (x.max() - x.min() + 1e-12)


def _texture(rng, shape=(256, 256)):
    j, i = np.indices(shape, dtype=np.float64)
    x = 0.5 * _smooth(rng, shape, rng.uniform(1.5, 6.0))
    for _ in range(4):
        th, f, ph = rng.uniform(0, np.pi), rng.uniform(0.02, 0.3), rng.uniform(0, 2 * np.pi)
        x += rng.uniform(0.05, 0.2) * np.sin(2 * np.pi * f * (i * np.cos(th) + j * np.sin(th)) + ph)
    x = (x - x.min()) / (x.max() - x.min())
    return np.clip(np.round(255 * x), 0, 255).astype(np.uint8)


def parity_images(seed, n=36):
    """Textures, gradients, checkerboards, noise and a 0 / 255 step."""
    rng = np.random.default_rng(seed)
    j, i = np.indices((256, 256), dtype=np.float64)
    out = []
    for q in range(n):
        kind = q % 6
        if kind in (0, 1):
            im = _texture(rng)
        elif kind == 2:
            th = rng.uniform(0, 2 * np.pi)
            g = i * np.cos(th) + j * np.sin(th)
            im = np.round(255 * (g - g.min()) / (g.max() - g.min())).astype(np.uint8)
        elif kind == 3:
            s = int(rng.integers(3, 40))
            im = (((i // s + j // s) % 2) * rng.integers(100, 256)).astype(np.uint8)
        elif kind == 4:
            im = rng.integers(0, 256, (256, 256)).astype(np.uint8)
        else:
            c = int(rng.integers(1, 255))
            im = np.where((i if q % 2 else j) < c, 0, 255).astype(np.uint8)
        out.append(im)
    return np.array(out)


def _parity(g, g64):
    tol = 1e-6 + 1e-5 * np.abs(g64).max(axis=1, keepdims=True)
    err = np.abs(g.astype(np.float64) - g64)
    assert np.all(err <= tol), (err / tol).max()
    return (err / np.abs(g64).max(axis=1, keepdims=True)).max()


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- parity
def test_parity_default_parameters(ctx):
    imgs = parity_images(11)
    g = api.gist_generate(imgs, ctx=ctx)
    assert g.shape == (len(imgs), 512) and g.dtype == np.float32
    rel = _parity(g, gist_np.gist_batch(imgs))
    print(f"max |g - g64| / max|row| = {rel:.2e}")


def test_parity_uneven_blocks_mixed_orientations(ctx):
    imgs = parity_images(12, 32)
    g = api.gist_generate(imgs, nblocks=5, orients=(4, 6, 8), ctx=ctx)
    assert g.shape == (32, 25 * 18)
    _parity(g, gist_np.gist_batch(imgs, 5, (4, 6, 8)))


def test_class_mirrors_cls_gist(ctx):
    imgs = parity_images(13, 2)
    G = api.GIST(api.GISTParams(False, 256, 256, 4, 4, (8, 8, 8, 8)), ctx=ctx)
    assert G.getSignatureSize() == 512
    assert np.array_equal(G.extract(imgs[1]), api.gist_generate(imgs, ctx=ctx)[1])


# ---------------------------------------------------------------------------------------------------------------- exactness
def test_zero_image_gives_exact_zeros(ctx):
    g = api.gist_generate(np.zeros((3, 256, 256), np.uint8), ctx=ctx)
    assert not np.any(g)


def test_u8_and_f32_inputs_are_bit_identical(ctx):
    imgs = parity_images(14, 8)
    assert np.array_equal(api.gist_generate(imgs, ctx=ctx), api.gist_generate(imgs.astype(np.float32), ctx=ctx))


def test_row_independent_of_batch_position_and_chunks(ctx):
    rng = np.random.default_rng(15)
    imgs = rng.integers(0, 256, (512, 256, 256)).astype(np.uint8)
    imgs[300] = _texture(rng)
    imgs[331] = _texture(rng)
    full = api.gist_generate(imgs, ctx=ctx)
    alone = api.gist_generate(imgs[300], ctx=ctx)[0]
    assert np.array_equal(full[300], alone)
    part = api.gist_generate(imgs[300 - 31:300 + 9], ctx=ctx)        # rows 31 / 32 of this call straddle the first chunk boundary
    assert np.array_equal(part[31], alone)
    assert np.array_equal(part[32], full[301])
    assert np.array_equal(api.gist_generate(imgs[331], ctx=ctx)[0], full[331])


def test_device_form_equals_host_form_and_replays_in_a_graph():
    import torch
    imgs = parity_images(16, 40)
    c = api.Context(0)
    host = api.gist_generate(imgs, ctx=c)
    c.close()
    s = torch.cuda.Stream()
    dc = api.Context(0, stream=int(s.cuda_stream))
    with torch.cuda.stream(s):
        t = torch.from_numpy(imgs).cuda()
        out = torch.empty((40, 512), dtype=torch.float32, device="cuda")
        api.gist_generate_torch(t, ctx=dc, out=out)                 # first call: tables and scratch
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        api.gist_generate_torch(t, ctx=dc, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    # default context on torch's current stream, f32 input
    assert np.array_equal(api.gist_generate_torch(t.float()).cpu().numpy(), host)
    del g
    dc.close()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors(ctx):
    for shape in ((2, 256, 200), (2, 128, 128), (1, 512, 512)):
        with pytest.raises(_lib.PRError) as e:
            api.gist_generate(np.zeros(shape, np.uint8), ctx=ctx)
        assert e.value.code == _lib.PR_EINVAL and "resize" in str(e.value)
    assert api.gist_generate(np.zeros((0, 256, 256), np.uint8), ctx=ctx).shape == (0, 512)
    bad = parity_images(17, 3).astype(np.float32)
    bad[1, 10, 20] = np.nan
    with pytest.raises(_lib.PRError) as e:
        api.gist_generate(bad, ctx=ctx)
    assert e.value.code == _lib.PR_ENAN
    with pytest.raises(ValueError):
        api.gist_generate(bad[0], nblocks=17, ctx=ctx)


def test_device_form_leaves_a_non_finite_row_as_nan():
    import torch
    imgs = parity_images(17, 3).astype(np.float32)
    good = api.gist_generate(imgs)
    imgs[1, 10, 20] = np.nan
    g = api.gist_generate_torch(torch.from_numpy(imgs).cuda()).cpu().numpy()
    assert np.all(np.isnan(g[1]))
    assert np.array_equal(g[[0, 2]], good[[0, 2]])
    imgs[1, 10, 20] = np.inf
    g = api.gist_generate_torch(torch.from_numpy(imgs).cuda()).cpu().numpy()
    assert np.all(np.isnan(g[1])) and np.array_equal(g[[0, 2]], good[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------- end to end
def synthetic_drive(seed, n=220):
    """Frames of 6 scenes (shifted 256 x 256 crops of a 384 x 384 texture, 20 frames each) and, from frame 120 on, a second pass
    over scenes 0..4 with a 2-pixel offset and sensor noise: the revisits."""
    rng = np.random.default_rng(seed)
    scenes = [_texture(rng, (384, 384)).astype(np.float64) for _ in range(6)]
    frames = []
    for f in range(n):
        if f < 120:
            sc, k, off, noise = f // 20, f % 20, 0, 2.0
        else:
            sc, k, off, noise = ((f - 120) // 20) % 5, (f - 120) % 20, 2, 6.0
        y0, x0 = 40 + (k % 3) + off, 6 * k + off
        im = scenes[sc][y0:y0 + 256, x0:x0 + 256] + rng.normal(0, noise, (256, 256))
        frames.append(np.clip(np.round(im), 0, 255).astype(np.uint8))
    return np.array(frames)


def _top1_with_margin(sig, mask_width):
    d = ((sig[:, None, :] - sig[None, :, :]) ** 2).sum(-1)
    i, j = np.indices(d.shape)
    d = np.where(np.abs(i - j) < mask_width, np.inf, d)
    o = np.argsort(d, axis=1)
    return o[:, 0], d, o


def test_end_to_end_drive_through_api_and_executables(ctx, tmp_path):
    frames = synthetic_drive(18)
    ids = [f for f in range(len(frames)) if f % 11 != 5]          # a selection as the incoming ids make it
    sel = frames[ids]
    mask = 25
    g = api.gist_generate(sel, ctx=ctx)
    g64 = gist_np.gist_batch(sel)
    _parity(g, g64)
    idx, _ = api.match_topk("gist", g, g, mask_width=mask, ctx=ctx)
    best, d64, order = _top1_with_margin(g64, mask)
    eps = 1e-6 + 1e-5 * np.abs(g64).max(axis=1)                     # the parity bound per row
    D = g64.shape[1]

    def bound(q, j):                                               # |d_gpu - d64| for rows within the parity bound
        e = eps[q] + eps[j]
        return 2 * np.abs(g64[q] - g64[j]).sum() * e + D * e * e

    rows = np.arange(len(sel))
    decided = [q for q in rows if np.isfinite(d64[q, order[q, 1]]) and
               d64[q, order[q, 1]] - d64[q, order[q, 0]] > bound(q, order[q, 0]) + bound(q, order[q, 1])]
    assert len(decided) >= 0.75 * len(sel)
    assert np.array_equal(idx[decided, 0], best[decided])
    revisits = [q for q in decided if ids[q] >= 120]
    assert np.mean([ids[best[q]] < 120 for q in revisits]) > 0.9      # the revisits find the first pass

    # the same through bin/test_gist and bin/match_signatures
    lst = tmp_path / "images.txt"
    names = []
    for f, im in enumerate(frames):
        name = f"frame_{f:04d}.pgm"
        with open(tmp_path / name, "wb") as fh:
            fh.write(b"P5\n# synthetic drive\n256 256\n255\n" + im.tobytes())
        names.append(name)
    lst.write_text("\n".join(names) + "\n")
    idf = tmp_path / "incoming_id_file.txt"
    idf.write_text("".join(f"{i}\n" for i in ids))
    out = tmp_path / "history_gist.txt"
    r = subprocess.run([os.path.join(BIN, "test_gist"), f"_incoming_id_file:={idf}", f"_images:={lst}", f"_gist_file:={out}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "GIST average time: " in r.stdout and r.stdout.rstrip().endswith("ms")
    text = out.read_text().split("\n")
    assert len(text) == len(sel) + 1 and text[-1] == "" and all(line.endswith(" ") for line in text[:-1])
    parsed = np.loadtxt(out, dtype=np.float64)
    want = np.array([[float("%g" % v) for v in row] for row in g])   # default ostream precision: 6 significant digits
    assert np.array_equal(parsed, want)
    res = tmp_path / "gist.out"
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", "gist", "--hist1", str(out), "--hist2", str(out),
                        "--mask_width", str(mask), "--out", str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = np.loadtxt(res)
    assert np.array_equal(m[decided, 0].astype(np.int64), best[decided])
