"""BoW generation on the GPU (pr_bow_generate / pr_bow_generate_dev, bow_gen.hip) against the numpy restatement of DBoW2's transform
(tests/bow_np.py): bit-equal ids and values for every weighting and normalisation class on several trees, edge-sized images, batch
independence, overflow handling, the device form and graph replay, and a synthetic drive through bin/test_bow and bin/match_signatures."""
import os
import subprocess

import numpy as np
import pytest

import bow_np
from so_dso_place_recognition_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")

pytestmark = pytest.mark.gpu

CLASSES = [(w, s) for w in range(4) for s in (bow_np.L1_NORM, bow_np.L2_NORM, bow_np.DOT_PRODUCT)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def uneven_tree(seed, n=3000):
    """Random tree: parents drawn among earlier nodes (uneven depths, families of 1 to ~40 children), duplicated sibling descriptors,
    leaf-flagged inner nodes, childless nodes that are not words (word id 0 with their own weight) and stopped words."""
    rng = np.random.default_rng(seed)
    parent = np.full(n, -1, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    desc[0] = rng.integers(0, 256, 32)
    for i in range(1, n):
        parent[i] = int(rng.integers(0, i)) if rng.random() < 0.6 else int(rng.integers(max(0, i - 30), i))
        if i > 1 and parent[i - 1] == parent[i] and rng.random() < 0.1:
            desc[i] = desc[i - 1]                                     # duplicate sibling: the first one wins
        else:
            desc[i] = synth._flip_bits(rng, desc[parent[i]][None], 0.15)[0]
    childless = np.bincount(parent[1:], minlength=n) == 0
    is_leaf = (childless & (rng.random(n) < 0.85)) | (~childless & (rng.random(n) < 0.05))
    is_leaf[0] = False
    weight = rng.uniform(0.1, 4.0, n)
    weight[rng.random(n) < 0.1] = 0.0
    return parent, is_leaf.astype(np.uint8), desc, weight


def images_near(seed, desc_pool, sizes, flips=0.05):
    rng = np.random.default_rng(seed)
    return [synth._flip_bits(rng, desc_pool[rng.integers(0, len(desc_pool), s)], flips) if s else np.zeros((0, 32), np.uint8)
            for s in sizes]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check(arrays, weighting, scoring, images, ctx, cols=None):
    v_np = bow_np.Vocab(10, 6, scoring, weighting, *arrays)
    voc = api.ORBVocabulary.from_arrays(10, 6, scoring, weighting, *arrays)
    cols = cols or max([len(d) for d in images] + [1])
    out, nw = api.bow_generate(images, voc, cols=cols, ctx=ctx, return_counts=True)
    want = bow_np.rows(v_np, images, cols)
    assert np.array_equal(_bits(out), _bits(want))
    assert np.array_equal(nw, [len(bow_np.transform(v_np, d)[0]) for d in images])
    return out, nw


K10L4 = synth.bow_vocabulary(7, k=10, L=4, stop_frac=0.1)
UNEVEN = uneven_tree(8)


@pytest.mark.parametrize("weighting,scoring", CLASSES)
def test_bit_equal_k10_l4(ctx, weighting, scoring):
    imgs = images_near(10 + weighting, K10L4[2][K10L4[1] > 0], [300, 1, 0, 777, 64, 1500])
    out, nw = check(K10L4, weighting, scoring, imgs, ctx)
    assert nw[0] > 100


@pytest.mark.parametrize("weighting,scoring", CLASSES)
def test_bit_equal_uneven_tree(ctx, weighting, scoring):
    p, leaf, d, w = UNEVEN
    imgs = images_near(20 + scoring, d, [500, 3, 0, 1200]) + images_near(21, d[:1], [50], flips=0.5)
    check(UNEVEN, weighting, scoring, imgs, ctx)


def test_duplicate_siblings_stopped_words_and_empty_vocabulary(ctx):
    Z, O = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    p = [-1, 0, 0, 0, 1, 1, 3]
    leaf = [0, 0, 0, 0, 1, 1, 1]
    d = np.array([Z, Z, O, Z, Z, np.full(32, 15, np.uint8), Z])
    imgs = [np.array([Z, O, np.full(32, 15, np.uint8), Z]), np.array([O, O]), np.array([Z])]
    for w in ([0, 0, 0.5, 0, 1.0, 2.0, 7.0], [0, 0, 0.5, 0, 0.0, 2.0, 7.0]):
        for weighting, scoring in CLASSES:
            out, nw = check((p, leaf, d, np.array(w)), weighting, scoring, imgs, ctx, cols=4)
    assert list(out[0, :2]) == [0, 1]                                # node 6 (word 2) is behind a tied sibling: never reached
    empty = (np.array([-1, 0, 1]), np.zeros(3, np.uint8), np.array([Z, Z, O]), np.ones(3))
    out, nw = check(empty, 0, 0, imgs, ctx, cols=5)
    assert np.all(out == -1) and not nw.any()
    voc = api.ORBVocabulary.from_arrays(10, 6, 0, 0, *empty)
    import torch
    fw = torch.zeros(7, dtype=torch.int32, device="cuda")
    api.bow_generate_torch(torch.from_numpy(np.concatenate(imgs)).cuda(), torch.tensor([0, 4, 6, 7], device="cuda"), voc, cols=5,
                           feature_words=fw)
    assert np.all(fw.cpu().numpy() == -1)


def test_image_sizes_0_1_8000_and_beyond_the_lds_sort(ctx):
    leaves = K10L4[2][K10L4[1] > 0]
    imgs = images_near(30, leaves, [0, 1, 8000, 8192, 8193, 20000], flips=0.2)
    for weighting, scoring in ((0, 0), (1, 1), (2, 5)):
        out, nw = check(K10L4, weighting, scoring, imgs, ctx)
        assert nw[0] == 0 and nw[1] == 1 and nw[5] > 5000


def test_rows_do_not_depend_on_batch_position(ctx):
    voc = api.ORBVocabulary.from_arrays(10, 4, 0, 0, *K10L4)
    imgs = images_near(40, K10L4[2], [int(s) for s in np.random.default_rng(4).integers(0, 900, 70)])
    full = api.bow_generate(imgs, voc, cols=1000, ctx=ctx)
    for i in (0, 33, 69):
        assert np.array_equal(_bits(api.bow_generate([imgs[i]], voc, cols=1000, ctx=ctx)), _bits(full[2 * i:2 * i + 2]))
    part = api.bow_generate(imgs[20:41], voc, cols=1000, ctx=ctx)
    assert np.array_equal(_bits(part), _bits(full[40:82]))


def test_overflow_host_error_and_device_truncation(ctx):
    import torch
    voc = api.ORBVocabulary.from_arrays(10, 4, 0, 0, *K10L4)
    imgs = images_near(50, K10L4[2][K10L4[1] > 0], [40, 900, 60], flips=0.2)
    full, nw = api.bow_generate(imgs, voc, cols=900, ctx=ctx, return_counts=True)
    cols = int(nw[1]) - 7
    assert nw[0] < cols and nw[2] < cols
    with pytest.raises(_lib.PRError) as e:
        api.bow_generate(imgs, voc, cols=cols, ctx=ctx)
    assert e.value.code == _lib.PR_EINVAL and "image 1" in str(e.value)
    assert (ctx.take_warnings() & _lib.WARN_BOW_TRUNCATED) == 0          # the host form reports an error, not a warning
    dc = api.Context(0)
    desc = torch.from_numpy(np.concatenate(imgs)).cuda()
    offs = torch.tensor([0, 40, 940, 1000], device="cuda")
    n_words = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                         # dc runs on a stream of its own
    out = api.bow_generate_torch(desc, offs, voc, cols=cols, ctx=dc, n_words=n_words)
    dc.sync()
    o = out.cpu().numpy()
    assert np.array_equal(_bits(o[2:4]), _bits(full[2:4, :cols]))     # the first cols words of the true vector
    assert np.array_equal(_bits(o[[0, 1, 4, 5]]), _bits(full[[0, 1, 4, 5], :cols]))
    assert np.array_equal(n_words.cpu().numpy(), nw)
    assert dc.take_warnings() & _lib.WARN_BOW_TRUNCATED
    assert dc.take_warnings() == 0
    dc.close()


def test_device_form_equals_host_form_and_replays_in_a_graph():
    import torch
    voc = api.ORBVocabulary.from_arrays(10, 4, 1, 0, *K10L4)
    imgs = images_near(60, K10L4[2][K10L4[1] > 0], [300, 0, 9000, 5, 700])
    c = api.Context(0)
    host, nw = api.bow_generate(imgs, voc, cols=9000, ctx=c, return_counts=True)
    c.close()
    v_np = bow_np.Vocab(10, 4, 1, 0, *K10L4)
    allf = np.concatenate(imgs)
    offs_np = np.concatenate([[0], np.cumsum([len(d) for d in imgs])]).astype(np.int64)
    s = torch.cuda.Stream()
    dc = api.Context(0, stream=int(s.cuda_stream))
    with torch.cuda.stream(s):
        desc = torch.from_numpy(allf).cuda()
        offs = torch.from_numpy(offs_np).cuda()
        out = torch.empty((10, 9000), dtype=torch.float64, device="cuda")
        n_words = torch.empty(5, dtype=torch.int32, device="cuda")
        fw = torch.empty(len(allf), dtype=torch.int32, device="cuda")
        api.bow_generate_torch(desc, offs, voc, cols=9000, ctx=dc, out=out, n_words=n_words, feature_words=fw)   # uploads, scratch
    s.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(host)) and np.array_equal(n_words.cpu().numpy(), nw)
    assert np.array_equal(fw.cpu().numpy(), v_np.word[bow_np.descend(v_np, allf)])
    out.zero_()
    n_words.zero_()
    fw.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        api.bow_generate_torch(desc, offs, voc, cols=9000, ctx=dc, out=out, n_words=n_words, feature_words=fw)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(host)) and np.array_equal(n_words.cpu().numpy(), nw)
    assert np.array_equal(fw.cpu().numpy(), v_np.word[bow_np.descend(v_np, allf)])
    # default context joined to torch's current stream
    assert np.array_equal(_bits(api.bow_generate_torch(desc, offs, voc, cols=9000).cpu().numpy()), _bits(host))
    del g
    dc.close()


def test_transform_mirrors_orbvocabulary(ctx):
    voc = api.ORBVocabulary.from_arrays(10, 4, 0, 0, *K10L4)
    d = images_near(70, K10L4[2], [400])[0]
    ids, vals = voc.transform(d, ctx=ctx)
    want = bow_np.transform(bow_np.Vocab(10, 4, 0, 0, *K10L4), d)
    assert ids.tolist() == want[0] and np.array_equal(_bits(vals), _bits(want[1]))


def test_end_to_end_drive_through_test_bow_and_match_signatures(tmp_path):
    p, leaf, d, w = K10L4
    n_first, revisits = 60, list(range(0, 60, 2))
    desc, offs, planted = synth.bow_drive(80, d[leaf > 0], n_first, revisits, per_image=400)
    frames = [desc[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    v_np = bow_np.Vocab(10, 4, 0, 0, p, leaf, d, w)
    (tmp_path / "voc.txt").write_text(bow_np.to_text(v_np))
    names = []
    for f, fd in enumerate(frames):
        names.append(f"frame_{f:04d}.orb")
        (tmp_path / names[-1]).write_bytes(fd.tobytes())
    (tmp_path / "desc.txt").write_text("\n".join(names) + "\n")
    ids = [f for f in range(len(frames)) if f % 13 != 7]                 # a selection as the incoming ids make it
    (tmp_path / "incoming_id_file.txt").write_text("".join(f"{i}\n" for i in ids))
    out = tmp_path / "history_bow.txt"
    r = subprocess.run([os.path.join(BIN, "test_bow"), f"_voc_file:={tmp_path / 'voc.txt'}",
                        f"_incoming_id_file:={tmp_path / 'incoming_id_file.txt'}", f"_descriptors:={tmp_path / 'desc.txt'}",
                        f"_output_file:={out}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "BoW vector transform time: " in r.stdout and f"Saved to {out}" in r.stdout
    want = bow_np.write_history([bow_np.transform(v_np, frames[f]) for f in ids])
    assert out.read_text() == want
    res = tmp_path / "bow.out"
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", "bow", "--hist1", str(out), "--hist2", str(out),
                        "--mask_width", "10", "--out", str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    top1 = np.loadtxt(res)[:, 0].astype(np.int64)
    pos = {f: q for q, f in enumerate(ids)}
    checked = 0
    for q, f in enumerate(ids):
        if planted[f] >= 0 and planted[f] in pos:
            assert top1[q] == pos[planted[f]], (f, planted[f], ids[top1[q]])
            checked += 1
    assert checked >= 20
    r = subprocess.run([os.path.join(BIN, "test_bow"), f"_voc_file:={tmp_path / 'voc.txt'}"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Fail to get params, exit." in r.stdout
