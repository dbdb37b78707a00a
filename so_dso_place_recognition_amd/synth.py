"""Deterministic synthetic inputs for tests and bench.

libm-free: only +, -, *, compares and IEEE sqrt are used, so any re-implementation
(C++/numpy) produces identical bits.  RNG: counter-based splitmix64,
    base(seed, stream) = splitmix64(seed ^ splitmix64(stream))
    U(seed, stream, i) = (splitmix64(base + i) >> 11) * 2**-53        in [0, 1)
There is no reference counterpart: the reference ships no synthetic generator and its real
point files are missing blobs (.MISSING_LARGE_BLOBS:2-14).
"""
from __future__ import annotations

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _base(seed: int, stream) -> np.ndarray:
    return splitmix64(np.uint64(seed) ^ splitmix64(np.asarray(stream, dtype=np.uint64)))


def uniform(seed: int, stream, count: int, offset: int = 0) -> np.ndarray:
    """U[0,1) doubles.  `stream` scalar -> shape (count,); array of S streams -> shape (S, count)."""
    ctr = np.arange(offset, offset + count, dtype=np.uint64)
    b = _base(seed, stream)
    with np.errstate(over="ignore"):
        h = splitmix64(b[..., None] + ctr) if np.ndim(b) else splitmix64(b + ctr)
    return (h >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


# ----------------------------------------------------------------------------- point clouds
def scene_cloud(seed: int, cloud: int, P: int, max_rho: float = 45.0):
    """Scene sampler of §8-d config 2: 32 boxes + 30 % ground plane, exactly P accepted points with
    ||p|| < max_rho.  Returns (xyz float64 [P,3] camera frame, intensity float32 [P])."""
    bx = uniform(seed, cloud * 4 + 0, 32 * 7).reshape(32, 7)
    centre = np.stack([-38 + 76 * bx[:, 0], -4 + 5 * bx[:, 1], -24 + 48 * bx[:, 2]], 1)
    half = np.stack([0.5 + 3.5 * bx[:, 3], 0.5 + 2.5 * bx[:, 4], 0.5 + 3.5 * bx[:, 5]], 1)
    base_i = 20 + 215 * bx[:, 6]
    out_xyz = np.empty((0, 3)); out_i = np.empty((0,))
    off = 0
    while out_xyz.shape[0] < P:
        n = int((P - out_xyz.shape[0]) * 1.3) + 64
        u = uniform(seed, cloud * 4 + 1, n * 6, off * 6).reshape(n, 6)
        off += n
        ground = u[:, 0] < 0.3
        box = np.minimum((u[:, 1] * 32).astype(np.int64), 31)
        pg = np.stack([-42 + 84 * u[:, 2], 1.6 + (-0.05 + 0.1 * u[:, 3]), -28 + 56 * u[:, 4]], 1)
        pb = centre[box] + half[box] * (2 * u[:, 2:5] - 1)
        p = np.where(ground[:, None], pg, pb)
        it = np.where(ground, 60.0, base_i[box]) + (-20 + 40 * u[:, 5])
        ok = (p * p).sum(1) < max_rho * max_rho
        out_xyz = np.concatenate([out_xyz, p[ok]]); out_i = np.concatenate([out_i, it[ok]])
    return np.ascontiguousarray(out_xyz[:P]), out_i[:P].astype(np.float32)


def scene_clouds(seed: int, N: int, P: int, max_rho: float = 45.0, first: int = 0):
    """N clouds in CSR layout: (xyz [N*P,3] f64, inten [N*P] f32, offs [N+1] i64)."""
    xyz = np.empty((N * P, 3)); it = np.empty((N * P,), np.float32)
    for c in range(N):
        xyz[c * P:(c + 1) * P], it[c * P:(c + 1) * P] = scene_cloud(seed, first + c, P, max_rho)
    return xyz, it, np.arange(N + 1, dtype=np.int64) * P


# ----------------------------------------------------------------------------- SC signatures
def sc_database(seed: int, n: int, first: int = 0, chunk: int = 4096) -> np.ndarray:
    """SC signature sampler (§8-d metric config): [n, 2400] float64, row = [structure 1200 | intensity 1200],
    bin = sector*20 + ring.  Structure bin occupied w.p. 0.6 with height U[0,8]; intensity bit
    Bernoulli(0.45) on occupied bins."""
    out = np.empty((n, 2400))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        u = uniform(seed, np.arange(first + s, first + e, dtype=np.uint64), 3600).reshape(e - s, 3, 1200)
        occ = u[:, 0] < 0.6
        out[s:e, :1200] = np.where(occ, 8.0 * u[:, 1], 0.0)
        out[s:e, 1200:] = np.where(occ & (u[:, 2] < 0.45), 1.0, 0.0)
    return out


def sc_queries(seed: int, db: np.ndarray, m: int, db_first: int = 0, n_global: int | None = None,
               db_seed: int | None = None):
    """Queries planted on DB entries: query t copies entry e_t = floor(U*n), rotated by floor(U*60) sectors,
    mirrored w.p. 1/2, 3 % of bins re-drawn.  Returns (queries [m,2400], planted index [m] int64).
    `db` may be a shard starting at global row db_first of an n_global-row DB; only queries whose planted
    entry lies inside the shard are copied from it (the others are re-drawn from sc_database(db_seed), default
    db_seed = seed - 1)."""
    db_seed = seed - 1 if db_seed is None else db_seed
    n = db.shape[0] if n_global is None else n_global
    u = uniform(seed, np.arange(m, dtype=np.uint64), 3 + 3600)
    et = np.minimum((u[:, 0] * n).astype(np.int64), n - 1)
    shift = np.minimum((u[:, 1] * 60).astype(np.int64), 59)
    mirror = u[:, 2] < 0.5
    q = np.empty((m, 2400))
    for t in range(m):
        g = et[t] - db_first
        src = db[g] if 0 <= g < db.shape[0] else sc_database(db_seed, 1, first=int(et[t]))[0]
        for ch in range(2):
            img = src[ch * 1200:(ch + 1) * 1200].reshape(60, 20)
            if mirror[t]:
                img = img[(-np.arange(60)) % 60]
            q[t, ch * 1200:(ch + 1) * 1200] = np.roll(img, shift[t], axis=0).reshape(-1)
        r = u[t, 3:].reshape(3, 1200)
        redo = r[0] < 0.03
        occ = r[1] < 0.6
        q[t, :1200] = np.where(redo, np.where(occ, 8.0 * r[2], 0.0), q[t, :1200])
        q[t, 1200:] = np.where(redo, np.where(occ & (r[2] < 0.45), 1.0, 0.0), q[t, 1200:])
    return q, et


# ----------------------------------------------------------------------------- M2DP signatures
def m2dp_database(seed: int, n: int, first: int = 0, chunk: int = 4096) -> np.ndarray:
    """M2DP signature sampler (§8-d config 3): [4n, 384] float64; per entry/variant/channel
    w = 0.3 + U(entry) + 0.15*(U(variant)-0.5); row = [u|v | u|v] with u = w[:64]/||.||, v = w[64:]/||.||."""
    out = np.empty((4 * n, 384))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        u = uniform(seed, np.arange(first + s, first + e, dtype=np.uint64), 384 * 5).reshape(e - s, 5, 2, 192)
        w = 0.3 + u[:, :1] + 0.15 * (u[:, 1:] - 0.5)                      # [e, 4 variants, 2 ch, 192]
        uu = w[..., :64] / np.sqrt((w[..., :64] ** 2).sum(-1, keepdims=True))
        vv = w[..., 64:] / np.sqrt((w[..., 64:] ** 2).sum(-1, keepdims=True))
        out[4 * s:4 * e] = np.concatenate([uu, vv], -1).reshape(4 * (e - s), 384)
    return out


def m2dp_queries(seed: int, db: np.ndarray, m: int):
    """Query t copies DB entry e_t (all 4 variant rows), adds 0.05*(U-0.5) per element, renormalises u and v."""
    n = db.shape[0] // 4
    u = uniform(seed, np.arange(m, dtype=np.uint64), 1 + 4 * 384)
    et = np.minimum((u[:, 0] * n).astype(np.int64), n - 1)
    rows = db.reshape(n, 4, 2, 192)[et] + 0.05 * (u[:, 1:].reshape(m, 4, 2, 192) - 0.5)
    uu = rows[..., :64] / np.sqrt((rows[..., :64] ** 2).sum(-1, keepdims=True))
    vv = rows[..., 64:] / np.sqrt((rows[..., 64:] ** 2).sum(-1, keepdims=True))
    return np.concatenate([uu, vv], -1).reshape(4 * m, 384), et


# ----------------------------------------------------------------------------- DELIGHT histograms
def delight_database(seed: int, n: int, first: int = 0) -> np.ndarray:
    """[16n, 256] float64 histograms: per entry 16 x 256 Poisson-like integer counts around a smooth profile."""
    u = uniform(seed, np.arange(first, first + n, dtype=np.uint64), 4096 + 16).reshape(n, 4096 + 16)
    scale = 4.0 + 28.0 * u[:, 4096:]                                          # per-histogram level
    cnt = np.floor(u[:, :4096].reshape(n, 16, 256) * scale[:, :, None] * (u[:, :4096].reshape(n, 16, 256) < 0.5))
    return cnt.reshape(16 * n, 256)


def delight_queries(seed: int, db: np.ndarray, m: int):
    """Query t copies entry e_t, applies one of the 4 octant permutations of processDELIGHT.m and perturbs 2 % of the bins."""
    from numpy import array
    mut = array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [5, 4, 7, 6, 1, 0, 3, 2, 13, 12, 15, 14, 9, 8, 11, 10],
                 [6, 7, 4, 5, 2, 3, 0, 1, 14, 15, 12, 13, 10, 11, 8, 9], [3, 2, 1, 0, 7, 6, 5, 4, 11, 10, 9, 8, 15, 14, 13, 12]])
    n = db.shape[0] // 16
    u = uniform(seed, np.arange(m, dtype=np.uint64), 2 + 2 * 4096)
    et = np.minimum((u[:, 0] * n).astype(np.int64), n - 1)
    k = np.minimum((u[:, 1] * 4).astype(np.int64), 3)
    q = np.empty((m, 16, 256))
    for t in range(m):
        src = db.reshape(n, 16, 256)[et[t]][mut[k[t]]]
        r = u[t, 2:].reshape(2, 16, 256)
        q[t] = np.where(r[0] < 0.02, np.floor(r[1] * 8), src)
    return q.reshape(16 * m, 256), et


def bow_signatures(seed: int, n: int, cols: int = 120, vocab: int = 400, fill=(20, 90)):
    """[2 n][cols] BoW rows as test_bow.cpp:147-162 writes them: sorted word ids / L1-normalised weights, both padded with -1."""
    rng = np.random.default_rng(seed)
    out = -np.ones((2 * n, cols))
    for i in range(n):
        k = int(rng.integers(fill[0], min(fill[1], cols) + 1))
        ids = np.sort(rng.choice(vocab, size=k, replace=False))
        w = rng.random(k) + 0.05
        out[2 * i, :k] = ids
        out[2 * i + 1, :k] = w / w.sum()
    return out


def bow_signatures_torch(seed: int, n: int, cols: int = 120, vocab: int = 400, fill=(20, 90), zipf: float | None = None, device="cuda",
                         chunk: int = 8192):
    """bow_signatures' layout drawn on the device (torch generator, not the numpy stream): [2 n][cols] float64, per image a row of
    distinct word ids in ascending order and a row of L1-normalised weights, both padded with -1.  A row's word count is uniform in
    `fill` (at most cols; words past column cols - 2 are never read, as in the reference).  zipf = s: word ranks drawn with probability
    ~ rank^-s, ranks mapped to ids by a random permutation (near-stop words whose lists hold a large share of the rows); None: uniform.
    Duplicate draws are dropped, so with a steep zipf a row may get fewer words than drawn."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    hi = max(0, min(int(fill[1]), cols, vocab))
    lo = min(int(fill[0]), hi)
    S = max(2 * hi + 8, 1)
    if zipf is not None:
        cdf = torch.cumsum(torch.arange(1, vocab + 1, dtype=torch.float64, device=device) ** (-float(zipf)), 0)
        cdf /= cdf[-1].clone()
        perm = torch.randperm(vocab, generator=g, device=device)
    out = torch.full((2 * n, cols), -1.0, dtype=torch.float64, device=device)
    for s0 in range(0, n, chunk):
        r = min(n, s0 + chunk) - s0
        if zipf is not None:
            u = torch.rand((r, S), generator=g, device=device, dtype=torch.float64)
            w = perm[torch.searchsorted(cdf, u).clamp_(max=vocab - 1)]
        else:
            w = torch.randint(0, vocab, (r, S), generator=g, device=device)
        w, _ = torch.sort(w, dim=1)
        dup = torch.zeros_like(w, dtype=torch.bool)
        dup[:, 1:] = w[:, 1:] == w[:, :-1]
        key = torch.where(dup, torch.full_like(w, 2, dtype=torch.float64), torch.rand((r, S), generator=g, device=device, dtype=torch.float64))
        ks, ki = torch.sort(key, dim=1)                      # the distinct words in random order
        k = torch.randint(lo, hi + 1, (r,), generator=g, device=device)
        valid = (torch.arange(hi, device=device)[None, :] < k[:, None]) & (ks[:, :hi] < 2)
        sel, _ = torch.sort(torch.where(valid, torch.gather(w, 1, ki[:, :hi]), torch.full_like(w[:, :hi], vocab)), dim=1)
        keep = sel < vocab
        wt = torch.where(keep, torch.rand((r, hi), generator=g, device=device, dtype=torch.float64) + 0.05, torch.zeros((), dtype=torch.float64,
                                                                                                                      device=device))
        wt = wt / wt.sum(1, keepdim=True).clamp_min(1e-300)
        out[2 * s0:2 * (s0 + r):2, :hi] = torch.where(keep, sel.to(torch.float64), torch.full_like(wt, -1.0))
        out[2 * s0 + 1:2 * (s0 + r):2, :hi] = torch.where(keep, wt, torch.full_like(wt, -1.0))
    return out


def gist_signatures(seed: int, n: int, cols: int = 96):
    rng = np.random.default_rng(seed)
    return np.abs(rng.normal(0.1, 0.05, size=(n, cols)))


def gist_signatures_torch(seed: int, n: int, cols: int = 512, device="cuda", clusters: int = 0, cluster_size: int = 40, eps: float = 1e-6,
                          chunk: int = 16384):
    """gist_signatures' distribution (|N(0.1, 0.05)| entries) drawn on the device from a torch generator of its own (not the numpy
    stream): float64 [n, cols].  clusters > 0 plants that many runs of `cluster_size` consecutive near-copies `base + eps * noise`
    (noise standard normal; eps = 0: exact duplicates) at evenly spaced rows - a vehicle standing still."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    out = torch.empty((n, cols), dtype=torch.float64, device=device)
    for s0 in range(0, n, chunk):
        r = min(n, s0 + chunk) - s0
        out[s0:s0 + r] = (torch.randn((r, cols), generator=g, device=device, dtype=torch.float64) * 0.05 + 0.1).abs_()
    cs = min(int(cluster_size), n)
    for c in range(int(clusters)):
        r0 = min(n - cs, (n // (clusters + 1)) * (c + 1))
        base = out[r0].clone()
        out[r0:r0 + cs] = base[None, :] + float(eps) * torch.randn((cs, cols), generator=g, device=device, dtype=torch.float64)
    return out


DELIGHT_CLUSTER_LEVEL = 2200          # a cluster member's own bin holds about this many counts (delight_signatures_torch)


def delight_cluster_bins(cluster_size: int):
    """(flat bins [cs] of the 16 x 256 histogram, counts [cs]) of a planted DELIGHT cluster: member t owns bin 37 t + 11, where every
    member holds 2200 + 3 pi(t) - pi a permutation of 0 .. cs - 1 that is not the identity - and member t one more."""
    cs = int(cluster_size)
    a = next(x for x in range(max(2, (cs * 5) // 8), 2 * cs + 3) if np.gcd(x, cs) == 1)
    t = np.arange(cs)
    return (37 * t + 11) % 4096, DELIGHT_CLUSTER_LEVEL + 3 * ((a * t + 1) % cs)


def delight_signatures_torch(seed: int, n: int, device="cuda", clusters: int = 0, cluster_size: int = 40, chunk: int = 4096):
    """delight_database's distribution (per histogram a level 4 .. 32, half of the bins empty, integer counts) drawn on the device from
    a torch generator of its own (not the numpy stream): float64 [16 n, 256].  clusters > 0 plants that many runs of `cluster_size`
    consecutive near-copies at evenly spaced entries - a vehicle standing still: all members are one base entry whose bins
    delight_cluster_bins() hold ~2200 counts, and member t holds one count more in its own bin.  Against a query that differs from the
    base in some other bin by a large amount, the members' distances differ by ~1e-10 relative: below fp32, far above fp64."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    out = torch.empty((n, 16, 256), dtype=torch.float64, device=device)
    for s0 in range(0, n, chunk):
        r = min(n, s0 + chunk) - s0
        u = torch.rand((r, 16, 256), generator=g, device=device, dtype=torch.float64)
        scale = 4.0 + 28.0 * torch.rand((r, 16, 1), generator=g, device=device, dtype=torch.float64)
        out[s0:s0 + r] = torch.floor(u * scale * (u < 0.5))
    cs = min(int(cluster_size), n)
    if clusters > 0 and cs > 0:
        bins, level = delight_cluster_bins(cs)
        bins_t = torch.as_tensor(bins, device=device)
        flat = out.view(n, 4096)
        for c in range(int(clusters)):
            r0 = min(n - cs, (n // (clusters + 1)) * (c + 1))
            base = flat[r0].clone()
            base[bins_t] = torch.as_tensor(level, dtype=torch.float64, device=device)
            flat[r0:r0 + cs] = base[None, :]
            flat[r0 + torch.arange(cs, device=device), bins_t] += 1.0
    return out.view(16 * n, 256)


# ----------------------------------------------------------------------------- the same samplers on a torch device
# Bit-identical to the numpy versions above (uint64 arithmetic carried in int64 two's complement: add / multiply wrap,
# logical shifts by masking), so that full-size inputs (10^5 - 10^6 signatures, 5000 x 50 000 points) are drawn in HBM in
# a fraction of a second instead of minutes of host time.  tests/test_synth_torch.py pins them against the numpy versions.
def _s64(x: int) -> int:
    x &= 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >= (1 << 63) else x


def _t_lsr(z, s: int):
    return (z >> s) & ((1 << (64 - s)) - 1)


def _t_splitmix64(x):
    z = x + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _t_lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _t_lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _t_lsr(z, 31)


def uniform_torch(seed: int, streams, count: int, offset: int = 0):
    """streams: int64 tensor [S] (on the target device) -> U[0,1) float64 [S, count], == uniform(seed, streams, count, offset)."""
    import torch
    b = _t_splitmix64(_t_splitmix64(streams) ^ _s64(seed))
    ctr = torch.arange(offset, offset + count, dtype=torch.int64, device=streams.device)
    h = _t_splitmix64(b[:, None] + ctr[None, :])
    return _t_lsr(h, 11).to(torch.float64) * (2.0 ** -53)


def sc_database_torch(seed: int, n: int, first: int = 0, device="cuda", chunk: int = 8192):
    """== sc_database(seed, n, first) as a float64 tensor on `device`."""
    import torch
    out = torch.empty((n, 2400), dtype=torch.float64, device=device)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        u = uniform_torch(seed, torch.arange(first + s, first + e, dtype=torch.int64, device=device), 3600).reshape(e - s, 3, 1200)
        occ = u[:, 0] < 0.6
        out[s:e, :1200] = torch.where(occ, 8.0 * u[:, 1], torch.zeros_like(u[:, 1]))
        out[s:e, 1200:] = (occ & (u[:, 2] < 0.45)).to(torch.float64)
    return out


def m2dp_database_torch(seed: int, n: int, first: int = 0, device="cuda", chunk: int = 8192):
    """== m2dp_database(seed, n, first) up to the last ulp of the row norms (torch reduces the 64 / 128 squares in another
    order than numpy); float64 [4n, 384] on `device`."""
    import torch
    out = torch.empty((4 * n, 384), dtype=torch.float64, device=device)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        u = uniform_torch(seed, torch.arange(first + s, first + e, dtype=torch.int64, device=device), 384 * 5).reshape(e - s, 5, 2, 192)
        w = 0.3 + u[:, :1] + 0.15 * (u[:, 1:] - 0.5)
        uu = w[..., :64] / torch.sqrt((w[..., :64] ** 2).sum(-1, keepdim=True))
        vv = w[..., 64:] / torch.sqrt((w[..., 64:] ** 2).sum(-1, keepdim=True))
        out[4 * s:4 * e] = torch.cat([uu, vv], -1).reshape(4 * (e - s), 384)
    return out


def scene_clouds_torch(seed: int, N: int, P: int, max_rho: float = 45.0, first: int = 0, device="cuda", chunk: int = 64):
    """== scene_clouds(seed, N, P, max_rho, first) as device tensors (xyz f64 [N*P,3], inten f32 [N*P], offs i64 [N+1]):
    the first P accepted points of the first int(1.3 P) + 64 draws of every cloud (clouds whose first round accepts fewer
    than P points - none with the §8-d scene parameters - are drawn by the numpy sampler)."""
    import torch
    n = int(P * 1.3) + 64
    xyz = torch.empty((N * P, 3), dtype=torch.float64, device=device)
    it = torch.empty((N * P,), dtype=torch.float32, device=device)
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        C_ = c1 - c0
        cl = torch.arange(first + c0, first + c1, dtype=torch.int64, device=device)
        bx = uniform_torch(seed, cl * 4 + 0, 32 * 7).reshape(C_, 32, 7)
        centre = torch.stack([-38 + 76 * bx[..., 0], -4 + 5 * bx[..., 1], -24 + 48 * bx[..., 2]], -1)
        half = torch.stack([0.5 + 3.5 * bx[..., 3], 0.5 + 2.5 * bx[..., 4], 0.5 + 3.5 * bx[..., 5]], -1)
        base_i = 20 + 215 * bx[..., 6]
        u = uniform_torch(seed, cl * 4 + 1, n * 6).reshape(C_, n, 6)
        ground = u[..., 0] < 0.3
        box = torch.clamp((u[..., 1] * 32).to(torch.int64), max=31)
        pg = torch.stack([-42 + 84 * u[..., 2], 1.6 + (-0.05 + 0.1 * u[..., 3]), -28 + 56 * u[..., 4]], -1)
        gi = box[..., None].expand(-1, -1, 3)
        pb = torch.gather(centre, 1, gi) + torch.gather(half, 1, gi) * (2 * u[..., 2:5] - 1)
        p = torch.where(ground[..., None], pg, pb)
        inten = torch.where(ground, torch.full_like(u[..., 5], 60.0), torch.gather(base_i, 1, box)) + (-20 + 40 * u[..., 5])
        ok = ((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]) < max_rho * max_rho
        rank = torch.cumsum(ok.to(torch.int64), 1) - 1
        have = rank[:, -1] + 1
        take = ok & (rank < P)
        ci, pi = torch.nonzero(take, as_tuple=True)
        dst = (c0 + ci) * P + rank[ci, pi]
        full = have[ci] >= P
        xyz[dst[full]] = p[ci[full], pi[full]]
        it[dst[full]] = inten[ci[full], pi[full]].to(torch.float32)
        for c in torch.nonzero(have < P).flatten().tolist():          # not seen with the §8-d parameters
            a, b = scene_cloud(seed, first + c0 + c, P, max_rho)
            xyz[(c0 + c) * P:(c0 + c + 1) * P] = torch.from_numpy(a).to(device)
            it[(c0 + c) * P:(c0 + c + 1) * P] = torch.from_numpy(b).to(device)
    return xyz, it, torch.arange(N + 1, dtype=torch.int64, device=device) * P


def drive_clouds_torch(frames=2000, per_cloud=6000, seed=5, stops=(), device="cuda", positions=False):
    """Two laps of a closed circuit through a static world: consecutive clouds overlap almost completely, frame i and
    frame i + frames/2 see the same place from slightly different poses.  Returns CSR clouds in the camera frame
    (x right, y down, z forward) and the lap length.  stops: (first frame, frames) stretches where the vehicle stands still - the pose
    of `first frame` is kept for that many frames (the frame-dependent subsample still differs: near-copies, the clusters the matcher's
    containment check exists for); the laps are then measured in MOVING frames.  positions: also return the sensor positions [frames, 3]
    (the ground truth of run_test.m:62-85).  (tests/test_gpu_configs.py::test_drive_2000_frames_mask_100 and bench.py's
    extra.kitti_shape share this sampler.)"""
    import torch
    g = torch.Generator(device=device); g.manual_seed(seed)
    R0 = 160.0                                                        # circuit radius [m]
    # world: ground strip + boxes along the circuit (y down: ground at y = +1.6)
    nb = 900
    ang = torch.rand(nb, generator=g, device=device, dtype=torch.float64) * 2 * np.pi
    rad = R0 + (torch.rand(nb, generator=g, device=device, dtype=torch.float64) - 0.5) * 70
    cx, cz = rad * torch.cos(ang), rad * torch.sin(ang)
    half = 0.5 + 3.5 * torch.rand((nb, 3), generator=g, device=device, dtype=torch.float64)
    base_i = 20 + 215 * torch.rand(nb, generator=g, device=device, dtype=torch.float64)
    ppb = 700
    u = torch.rand((nb, ppb, 3), generator=g, device=device, dtype=torch.float64) * 2 - 1
    bx = torch.stack([cx[:, None] + half[:, None, 0] * u[..., 0], (1.6 - half[:, None, 1]) + half[:, None, 1] * u[..., 1] * 0.999,
                      cz[:, None] + half[:, None, 2] * u[..., 2]], -1).reshape(-1, 3)
    bi = (base_i[:, None] + 40 * (torch.rand((nb, ppb), generator=g, device=device, dtype=torch.float64) - 0.5)).reshape(-1)
    ng = 500_000
    ga = torch.rand(ng, generator=g, device=device, dtype=torch.float64) * 2 * np.pi
    gr = R0 + (torch.rand(ng, generator=g, device=device, dtype=torch.float64) - 0.5) * 100
    gx = torch.stack([gr * torch.cos(ga), 1.6 + 0.1 * (torch.rand(ng, generator=g, device=device, dtype=torch.float64) - 0.5), gr * torch.sin(ga)], -1)
    gi_ = 60 + 40 * (torch.rand(ng, generator=g, device=device, dtype=torch.float64) - 0.5)
    W = torch.cat([bx, gx]); WI = torch.cat([bi, gi_])
    still = np.zeros(frames, bool)
    for f0, cnt in stops:
        still[f0 + 1: f0 + cnt] = True                                                # frames that repeat their predecessor's pose
    step = np.cumsum(~still) - 1                                                      # the pose index of every frame (frame 0 moves)
    moving = int((~still).sum())
    lap = moving // 2
    xyz, inten, offs, poss = [], [], [0], []
    for f in range(frames):
        s = int(step[f])
        th = 2 * np.pi * (s % lap) / lap + (0.002 if s >= lap else 0.0)              # second lap: 0.3 m along-track offset
        r = R0 + (0.4 if s >= lap else 0.0)                                           # ... and 0.4 m lateral
        pos = torch.tensor([r * np.cos(th), 0.0, r * np.sin(th)], dtype=torch.float64, device=device)
        fwd = torch.tensor([-np.sin(th), 0.0, np.cos(th)], dtype=torch.float64, device=device)
        right = torch.tensor([np.cos(th), 0.0, np.sin(th)], dtype=torch.float64, device=device)
        poss.append([r * np.cos(th), 0.0, r * np.sin(th)])
        rel = W - pos
        a, b = rel @ right, rel @ fwd
        near = (a / 26.0) ** 2 + (b / 44.0) ** 2 < 1.0                               # a road corridor: keeps the three PCA eigenvalues apart (N3)
        it = WI[near]
        cam = torch.stack([a[near], rel[near, 1], b[near]], 1)
        if cam.shape[0] > per_cloud:                                                  # frame-dependent subsample (a moving sensor never
            sel = torch.randperm(cam.shape[0], generator=g, device=device)[:per_cloud]   # sees the same points twice)
            cam, it = cam[sel], it[sel]
        xyz.append(cam); inten.append(it.to(torch.float32)); offs.append(offs[-1] + cam.shape[0])
    res = (torch.cat(xyz).cpu().numpy(), torch.cat(inten).cpu().numpy(), np.array(offs, np.int64), lap)
    return res + (np.array(poss),) if positions else res


# ----------------------------------------------------------------------------- BoW vocabularies and ORB descriptor sets
def _flip_bits(rng, desc, p):
    """desc uint8 [n, 32] with each of its 256 bits flipped with probability p."""
    out = np.empty_like(desc)
    for c0 in range(0, desc.shape[0], 1 << 16):
        d = desc[c0:c0 + (1 << 16)]
        flips = rng.random((d.shape[0], 256)) < p
        out[c0:c0 + d.shape[0]] = d ^ np.packbits(flips, axis=1)
    return out


def bow_vocabulary(seed: int, k: int = 10, L: int = 6, stop_frac: float = 0.0):
    """A complete k-ary DBoW2 tree of depth L as node arrays (parent, is_leaf, desc, weight) for api.ORBVocabulary.from_arrays: node 0 is
    the root, nodes in level order (sum of k^l nodes, 1 111 111 for k = 10, L = 6).  A child's descriptor is its parent's with each bit
    flipped with probability 0.5^l at level l (random at level 1), so a descriptor near a leaf descends to that leaf.  Leaves are the
    words, weights (idf-like) uniform in [0.5, 5), a `stop_frac` share of them 0 (stopped words); inner nodes weigh 0."""
    rng = np.random.default_rng(seed)
    sizes = [k ** l for l in range(L + 1)]
    n = sum(sizes)
    parent = np.full(n, -1, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    desc[0] = rng.integers(0, 256, 32, dtype=np.uint8)
    start = 0
    for l in range(1, L + 1):
        p0, c0 = start, start + sizes[l - 1]
        idx = np.arange(sizes[l])
        parent[c0:c0 + sizes[l]] = p0 + idx // k
        desc[c0:c0 + sizes[l]] = _flip_bits(rng, desc[p0 + idx // k], 0.5 ** l)
        start = c0
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[start:] = 1
    weight = np.zeros(n, np.float64)
    weight[start:] = rng.uniform(0.5, 5.0, sizes[L])
    weight[start:][rng.random(sizes[L]) < stop_frac] = 0.0
    return parent, is_leaf, desc, weight


def bow_drive(seed: int, anchors, n_first: int, revisits, per_image: int = 300, share: float = 0.8, flips: float = 0.01):
    """ORB descriptor sets of a drive: frames 0 .. n_first-1 see distinct places, then frame n_first + j revisits the place of frame
    revisits[j].  A place holds per_image descriptors near random rows of `anchors` (uint8 [A, 32], e.g. a vocabulary's leaves); a frame
    shows each with bit-flip probability `flips`, and a revisit keeps `share` of them (a random subset) and adds fresh ones.
    Returns (desc uint8 [F, 32], offs int64 [N + 1], planted int64 [N]: the first visit of a revisit frame, -1 for the others)."""
    rng = np.random.default_rng(seed)
    anchors = np.asarray(anchors, np.uint8)
    pools = [_flip_bits(rng, anchors[rng.integers(0, len(anchors), per_image)], 0.02) for _ in range(n_first)]
    frames, planted = [], []
    for f in range(n_first):
        frames.append(_flip_bits(rng, pools[f], flips))
        planted.append(-1)
    for r in revisits:
        keep = rng.permutation(per_image)[:int(round(share * per_image))]
        fresh = _flip_bits(rng, anchors[rng.integers(0, len(anchors), per_image - len(keep))], 0.02)
        d = np.concatenate([_flip_bits(rng, pools[r][keep], flips), fresh])
        frames.append(d[rng.permutation(len(d))])
        planted.append(int(r))
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in frames])
    return np.concatenate(frames), offs, np.array(planted, np.int64)
