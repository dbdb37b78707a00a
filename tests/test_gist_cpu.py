"""CPU checks of the GIST generator's pieces: the fp64 restatement (tests/gist_np.py) against hand-computed small cases, the
separable whitening low-pass against the literal FFT form, and the C ABI entry points."""
import ctypes as C

import numpy as np

import gist_np
from so_dso_place_recognition_amd import _lib, api


def test_symmetric_padding_repeats_the_edge_pixel():
    img = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float64)
    want = np.array([[5, 4, 4, 5, 6, 6, 5],
                     [2, 1, 1, 2, 3, 3, 2],
                     [2, 1, 1, 2, 3, 3, 2],
                     [5, 4, 4, 5, 6, 6, 5],
                     [8, 7, 7, 8, 9, 9, 8],
                     [8, 7, 7, 8, 9, 9, 8],
                     [5, 4, 4, 5, 6, 6, 5]], np.float64)
    assert np.array_equal(gist_np.pad_symmetric(img, 2), want)


def test_fftshift_swaps_quadrants():
    a = np.arange(16.0).reshape(4, 4)
    want = np.array([[10, 11, 8, 9], [14, 15, 12, 13], [2, 3, 0, 1], [6, 7, 4, 5]], np.float64)
    assert np.array_equal(gist_np.fftshift(a), want)
    assert np.array_equal(gist_np.fftshift(a), np.fft.fftshift(a))


def test_down_n_uneven_blocks_are_column_major():
    img = np.arange(25.0).reshape(5, 5)          # bounds 0, 2, 5 on both axes (i W / N, integer division)
    res = gist_np.down_n(img, 2)
    # res[k N + l]: k = x (column) block, l = y (row) block
    want = [img[0:2, 0:2].mean(), img[2:5, 0:2].mean(), img[0:2, 2:5].mean(), img[2:5, 2:5].mean()]
    assert np.allclose(res, want)
    assert res[1] == (10 + 11 + 15 + 16 + 20 + 21) / 6


def test_separable_prefilter_equals_fft_form():
    rng = np.random.default_rng(3)
    for img in (rng.integers(0, 256, (256, 256)).astype(np.uint8), np.tile(np.arange(256, dtype=np.uint8), (256, 1))):
        a, b = gist_np.prefilt(img), gist_np.prefilt_separable(img)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_gabor_bank_shape_and_dc():
    G = gist_np.gabor((4, 6, 8))
    assert G.shape == (18, 256, 256)
    assert np.isclose(G[0, 0, 0], np.exp(-3.5))   # DC bin: fr = 0, angle 0 -> exp(-10 p0) for the first orientation
    assert np.all((G >= 0) & (G <= 1))


def test_gist_entry_points_are_exported_and_declared():
    lib = _lib.load()
    for name in ("pr_gist_signature_size", "pr_gist_generate", "pr_gist_generate_dev"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.U8 == 2
    o = np.array([8, 8, 8, 8], np.int32)
    assert lib.pr_gist_signature_size(4, 4, o.ctypes.data_as(C.c_void_p)) == 512
    assert api.gist_signature_size(5, (4, 6, 8)) == 450
    assert api.GIST().getSignatureSize() == 512
    assert lib.pr_gist_signature_size(17, 4, o.ctypes.data_as(C.c_void_p)) == _lib.PR_EINVAL
    assert lib.pr_gist_signature_size(4, 0, o.ctypes.data_as(C.c_void_p)) == _lib.PR_EINVAL
    # arguments are checked before any device work: a NULL context is PR_EINVAL, not a crash
    rc = lib.pr_gist_generate(None, None, _lib.U8, 0, 256, 256, 4, 4, o.ctypes.data_as(C.c_void_p), None)
    assert rc == _lib.PR_EINVAL
