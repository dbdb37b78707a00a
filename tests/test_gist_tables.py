"""CPU check of the tables the GIST kernels are fed (so_dso_place_recognition_amd/csrc/gist_tables.hpp, compiled on the host by
tests/native/gist_tables_dump.cpp): the whitening circulant and the Gabor bank against the fp64 restatement (tests/gist_np.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gist_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("gist_tables")
    exe = str(d / "gist_tables_dump")
    r = subprocess.run([gxx, "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "gist_tables_dump.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(orients):
        c, g = str(d / "circ.f32"), str(d / "gabor.f32")
        r = subprocess.run([exe, c, g] + [str(o) for o in orients], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return np.fromfile(c, np.float32).reshape(266, 266), np.fromfile(g, np.float32).reshape(sum(orients), 256, 256)
    return run


def test_shipped_circulant_is_the_whitening_low_pass(dump):
    C, _ = dump((8,))
    C64 = gist_np.circulant(266)
    assert np.abs(C.astype(np.float64) - C64).max() <= 1e-7 * np.abs(C64).max()
    assert np.array_equal(C, C.T)
    # C X C equals prefilt's FFT-form low-pass ifft2(fft2(X) gfc) on a padded image, to fp32 table rounding
    rng = np.random.default_rng(4)
    x = gist_np.pad_symmetric(np.log(rng.integers(0, 256, (256, 256)) + 1.0), 5)
    lp = np.real(np.fft.ifft2(np.fft.fft2(x) * gist_np.whitening(266)))
    Cd = C.astype(np.float64)
    assert np.abs(Cd @ x @ Cd - lp).max() <= 1e-6 * np.abs(lp).max()


def test_shipped_gabor_bank_matches_the_restatement(dump):
    for orients in ((8, 8, 8, 8), (4, 6, 8)):
        _, G = dump(orients)
        G64 = gist_np.gabor(orients)
        assert np.abs(G.astype(np.float64) - G64).max() <= 1e-5    # the reference's float arithmetic vs fp64 (values in [0, 1])
