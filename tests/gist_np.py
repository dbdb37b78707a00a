"""fp64 numpy restatement of the reference's GIST descriptor: GIST::extract (GIST/src/gist.cpp:54-94) ->
bw_gist_scaletab (GIST/src/libgist.cpp:914-951) for grayscale 256 x 256 images, written from the algorithm as the
reference's libgist variant states it.  It is the tests' oracle for pr_gist_generate (tests/test_gpu_gist.py).

Steps, with the libgist lines they restate:
  prefilt (:276-409, fc = 4)   log(x + 1); 5 px symmetric padding (:32-65); whitening gfc = exp(-(fx^2 + fy^2) / s1^2),
                               s1 = fc / sqrt(log 2), fftshifted (:314-331); x -= Re ifft2(fft2(x) gfc) / (w h) (:334-347);
                               x /= 0.2 + sqrt(|ifft2(fft2(x^2) gfc)| / (w h)) (:350-395); padding removed (:397)
  create_gabor (:190-272)      at the UNPADDED 256 x 256 size: param = {0.35, 0.3 / 1.85^(s-1), 16 or^2 / 32^2, pi / or (o-1)},
                               angle wrapped to [-pi, pi], exp(-10 p0 (fr/H/p1 - 1)(fr/W/p1 - 1) - 2 p2 pi t^2), fftshifted
  gist_gabor (:685-759)        F = fft2(prefiltered); per filter k (scale-major): |ifft2(F G_k)| / (W H), then down_N
  down_N (:600-629)            block bounds i W / N (integer division); res[k N + l] = mean of x block k, y block l
"""
from __future__ import annotations

import numpy as np

SIDE = 256


def pad_symmetric(img: np.ndarray, p: int = 5) -> np.ndarray:
    """image_add_padding (:32-65): rows then columns mirrored with the edge pixel repeated."""
    h, w = img.shape
    out = np.zeros((h + 2 * p, w + 2 * p), img.dtype)
    out[p:p + h, p:p + w] = img
    for j in range(p):
        out[j, p:p + w] = img[p - j - 1]
        out[j + p + h, p:p + w] = img[h - j - 1]
    for i in range(p):
        out[:, i] = out[:, 2 * p - i - 1]
        out[:, i + p + w] = out[:, out.shape[1] - p - i - 1]
    return out


def fftshift(a: np.ndarray) -> np.ndarray:
    """fftshift (:158-186) for even sizes: element (j, i) moves to ((j + h/2) % h, (i + w/2) % w)."""
    h, w = a.shape[-2:]
    return np.roll(a, (h // 2, w // 2), axis=(-2, -1))


def whitening(n: int, fc: float = 4.0) -> np.ndarray:
    """gfc of prefilt (:314-331) for an n x n padded image (n even), fftshifted into FFT order."""
    s1 = fc / np.sqrt(np.log(2.0))
    f = np.arange(n) - n / 2.0
    fx, fy = np.meshgrid(f, f)
    return fftshift(np.exp(-(fx ** 2 + fy ** 2) / s1 ** 2))


def prefilt(img: np.ndarray, fc: float = 4.0) -> np.ndarray:
    """The literal FFT form of prefilt (:276-409)."""
    x = pad_symmetric(np.log(np.asarray(img, np.float64) + 1.0), 5)
    n = x.shape[0]
    g = whitening(n, fc)
    # numpy's ifft2 divides by w h, FFTW's backward transform does not and the reference divides explicitly: same value
    x = x - np.real(np.fft.ifft2(np.fft.fft2(x) * g))
    x = x / (0.2 + np.sqrt(np.abs(np.fft.ifft2(np.fft.fft2(x * x) * g))))
    return x[5:-5, 5:-5]


def circulant(n: int, fc: float = 4.0) -> np.ndarray:
    """The 1-D factor of the separable whitening low-pass: C[i][j] = c[(i - j) mod n], c = ifft(g) with g(f) = exp(-f^2 / s1^2)
    in FFT order (even, so c is real and C symmetric): ifft2(fft2(X) gfc) = C X C^T."""
    s1 = fc / np.sqrt(np.log(2.0))
    f = np.fft.fftfreq(n, 1.0 / n)
    if n % 2 == 0:
        f[n // 2] = -n // 2          # fftshift puts -n/2 at position n/2 (same value of g)
    c = np.real(np.fft.ifft(np.exp(-f ** 2 / s1 ** 2)))
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    return c[idx]


def prefilt_separable(img: np.ndarray, fc: float = 4.0) -> np.ndarray:
    """prefilt with each low-pass as C X C^T (the form the GPU kernels use)."""
    x = pad_symmetric(np.log(np.asarray(img, np.float64) + 1.0), 5)
    C = circulant(x.shape[0], fc)
    x = x - C @ x @ C.T
    x = x / (0.2 + np.sqrt(np.abs(C @ (x * x) @ C.T)))
    return x[5:-5, 5:-5]


def gabor(orients, n: int = SIDE) -> np.ndarray:
    """create_gabor (:190-272) at n x n: [sum(orients), n, n], scale-major."""
    f = np.arange(n) - n / 2.0
    fx, fy = np.meshgrid(f, f)
    fr = fftshift(np.sqrt(fx ** 2 + fy ** 2))
    th = fftshift(np.arctan2(fy, fx))
    out = []
    for s, nor in enumerate(orients, start=1):
        for o in range(1, nor + 1):
            p0, p1, p2, p3 = 0.35, 0.3 / 1.85 ** (s - 1), 16.0 * nor ** 2 / 32.0 ** 2, np.pi / nor * (o - 1)
            t = th + p3
            t = np.where(t < -np.pi, t + 2 * np.pi, np.where(t > np.pi, t - 2 * np.pi, t))
            out.append(np.exp(-10.0 * p0 * (fr / n / p1 - 1) * (fr / n / p1 - 1) - 2.0 * p2 * np.pi * t * t))
    return np.array(out)


def down_n(img: np.ndarray, N: int) -> np.ndarray:
    """down_N (:600-629): res[k N + l] = mean over x block k (columns) and y block l (rows), bounds i W / N."""
    h, w = img.shape[-2:]
    nx = [i * w // N for i in range(N + 1)]
    ny = [i * h // N for i in range(N + 1)]
    res = np.empty(img.shape[:-2] + (N * N,))
    for l in range(N):
        for k in range(N):
            res[..., k * N + l] = img[..., ny[l]:ny[l + 1], nx[k]:nx[k + 1]].mean(axis=(-2, -1))
    return res


_bank = {}


def gist(img: np.ndarray, nblocks: int = 4, orients=(8, 8, 8, 8)) -> np.ndarray:
    """bw_gist_scaletab (:914-951) of one 256 x 256 image -> fp64 [nblocks^2 sum(orients)]."""
    key = tuple(orients)
    if key not in _bank:
        _bank[key] = gabor(orients)
    G = _bank[key]
    F = np.fft.fft2(prefilt(img))
    y = np.abs(np.fft.ifft2(F[None] * G))        # numpy's ifft2 includes the 1 / (W H) of :745
    return down_n(y, nblocks).reshape(-1)


def gist_batch(images, nblocks: int = 4, orients=(8, 8, 8, 8)) -> np.ndarray:
    return np.array([gist(im, nblocks, orients) for im in images])
