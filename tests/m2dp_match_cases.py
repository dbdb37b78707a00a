"""Inputs on which the M2DP all-pairs matchers (csrc/m2dp_match_h.hip, csrc/m2dp_match.hip) are determined bit for bit, and integer-exact
models of what each arithmetic must return.  Pure numpy.

A signature is 4 variant rows x 384 values, [ch0: 192 | ch1: 192]; per channel the matcher forms the dot products S of the rows scaled by 2^8
(m2dp_pack_h_kernel), keeps the maximum Smax over the 4 x 4 variant pairs and stores float32(0.5 - Smax 2^-17) (processM2DP.m:15,19).

The grid.  Every entry is x = (h + b 2^-12) / 256 with h in {+-2, +-3}, b in {-3 .. 3}, and b = 0 or sign(b) = sign(h) where |h| = 2
(2 - 3 2^-12 lies in the binade below 2, where f16 resolves 2^-10: hi would no longer be h).  Then
  hi = f16(256 x) = h                  (|b| 2^-12 < 2^-10 = half an f16 ulp at 2 .. 4),
  lo = f16(256 x - hi) = b 2^-12       (a normal f16),
every product hi hi', hi lo', lo hi' is a multiple of 2^-12 and the sum of the absolute values of all 576 of a row pair is below 2^12
(192 x (9 + 2 x 9 x 2^-12)): every partial sum, in any order and any grouping, is a multiple of 2^-12 below 2^12 - exact in fp32.  So is the
sum in float64 (numpy's matrix product), which is the model.  The kernels never form lo lo'.
  split-f16 ("f16x2"):  S = hi.hi' + hi.lo' + lo.hi'
  single f16 ("f16")  :  S = hi.hi'
  fp32 ("f32")        :  the same grid with b = 0 (grid32): products and sums of h / 256 are exact in fp32, S = hi.hi'
and the output has ONE rounding, float32(0.5 - Smax 2^-17) of an exact double - the kernels' fmaf (0.5f - 0.5f * max in the fp32 kernel,
whose product is exact).

Variants 1 .. 3 of a signature are variant 0 with the sign of the first 64 and / or the last 128 entries of each channel flipped (M2DP's
+-axis variants; the constraint on b follows the sign), then a tenth of the entries of each is redrawn, so the 16 variant pairs of a
signature pair differ.  Every second query copies a DB signature with its four variant rows permuted and five columns negated: large |S|,
where the lo terms weigh most.  One seeded draw of N_DB signatures and N_Q queries; every shape a test uses is a prefix of it.

The unit family (8 DB signatures, 8 queries): rows with x = +-1 at one place of the first 64 and one of the last 128 entries of a channel
(256 x = +-256 is an f16), whose variants are either the four sign patterns or four equal rows, and an all-zero signature on each side.
S is 0, +-65536 or +-131072, the distance 0.5, 0, 1, -0.5 or 1.5, and 0.5 in the zero signature's row and column.
"""
import numpy as np

SEED = 20261
N_DB, N_Q = 1031, 97
LO_UNIT = 2.0 ** -12
ARITHS = ("f16x2", "f16", "f32")
FLIPS = ((1, 1), (-1, 1), (1, -1), (-1, -1))        # sign of the (first 64, last 128) entries of a channel in variants 0 .. 3


def _draw(rng, shape):
    """(h, b) of the grid."""
    h = rng.choice(np.array([-3, -2, 2, 3]), size=shape)
    b = rng.integers(-3, 4, size=shape)
    b = np.where(np.abs(h) == 2, np.sign(h) * np.abs(b), b)
    return h, b


def _value(h, b):
    return (h + b * LO_UNIT) / 256.0


def _signature_set(rng, count):
    """[count, 4, 2, 192] float64."""
    h, b = _draw(rng, (count, 1, 2, 192))
    x = np.repeat(_value(h, b), 4, axis=1)
    for v, (su, sv) in enumerate(FLIPS):
        x[:, v, :, :64] *= su
        x[:, v, :, 64:] *= sv
    for v in (1, 2, 3):
        again = rng.random((count, 2, 192)) < 0.10
        h, b = _draw(rng, (count, 2, 192))
        x[:, v] = np.where(again, _value(h, b), x[:, v])
    return x


def _build():
    rng = np.random.default_rng(SEED)
    db = _signature_set(rng, N_DB)
    q = _signature_set(rng, N_Q)
    for t in range(0, N_Q, 2):            # a copy of a DB signature; the sources lie low so that small DB prefixes hold some of them
        src = int(rng.integers(0, (7, 60, N_DB)[(t // 2) % 3]))
        rows = db[src][rng.permutation(4)].reshape(4, 384).copy()
        rows[:, rng.choice(384, size=5, replace=False)] *= -1.0
        q[t] = rows.reshape(4, 2, 192)
    return q.reshape(4 * N_Q, 384), db.reshape(4 * N_DB, 384)


_GRID = None


def grid():
    """(queries [4 N_Q, 384], DB [4 N_DB, 384]) float64, read-only."""
    global _GRID
    if _GRID is None:
        q, db = _build()
        q.setflags(write=False)
        db.setflags(write=False)
        _GRID = (q, db)
    return _GRID


def split(x):
    """(hi, lo) of m2dp_pack_h_kernel as float64: hi = f16(256 x), lo = f16(256 x - hi)."""
    v = np.asarray(x, np.float64) * 256.0
    hi = v.astype(np.float16).astype(np.float64)
    lo = (v - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def grid32():
    """The grid with b = 0 (x = h / 256): the case set of the fp32 kernel."""
    return tuple(split(a)[0] / 256.0 for a in grid())


def cases(arith):
    return grid32() if arith == "f32" else grid()


def model_s(q, db, arith, drop=None):
    """S [2, 4m, 4n] float64 of the scaled rows as the arithmetic forms it.  drop = "hl" / "lh" leaves hi.lo' / lo.hi' out (a model of a
    kernel that loses that product, for the sensitivity checks)."""
    out = []
    for ch in (0, 1):
        c = slice(192 * ch, 192 * ch + 192)
        qh, ql = split(q[:, c])
        dh, dl = split(db[:, c])
        s = qh @ dh.T
        if arith == "f16x2":
            if drop != "hl":
                s = s + qh @ dl.T
            if drop != "lh":
                s = s + ql @ dh.T
        elif arith == "f32":
            s = (np.asarray(q[:, c], np.float64) * 256.0) @ (np.asarray(db[:, c], np.float64) * 256.0).T
        else:
            assert arith == "f16"
        out.append(s)
    return np.stack(out)


def block_max(s):
    """[2, 4m, 4n] -> the maximum over the 4 x 4 variant pairs [2, m, n]."""
    c, m4, n4 = s.shape
    return s.reshape(c, m4 // 4, 4, n4 // 4, 4).max(axis=(2, 4))


def expected(q, db, arith, drop=None):
    """The two distance matrices [2, m, n] float32 the arithmetic must return, one rounding each."""
    return (0.5 - block_max(model_s(q, db, arith, drop)) * 2.0 ** -17).astype(np.float32)


def bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def first_difference(got, want):
    """None, or a message naming the first differing (channel, query, entry) of two [2, m, n] float32 stacks compared as uint32."""
    got, want = bits(np.stack(got)), bits(np.stack(want))
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    ch, i, j = (int(v) for v in bad[0])
    return (f"{len(bad)} of {got.size} distances differ, first at (channel {ch}, query {i}, entry {j}): "
            f"{got[ch, i, j]:#010x} ({float(got.view(np.float32)[ch, i, j])!r}) against the model's {want[ch, i, j]:#010x} "
            f"({float(want.view(np.float32)[ch, i, j])!r})")


# ---------------------------------------------------------------------------------------------------------------------- the unit family
# (kind, place in the first 64, place in the last 128, sign of the first, sign of the second); "flip": variants = the four sign
# patterns of that row, "same": four equal rows, "zero": the all-zero signature
UNIT_DB = (("flip", 3, 70, 1, 1), ("flip", 3, 100, 1, 1), ("flip", 40, 191, 1, 1), ("same", 0, 64, 1, 1), ("same", 0, 64, -1, -1),
           ("same", 0, 64, 1, -1), ("zero", 0, 64, 0, 0), ("same", 63, 191, 1, 1))
UNIT_Q = (("flip", 3, 70, 1, 1), ("same", 0, 64, 1, 1), ("same", 0, 100, 1, 1), ("zero", 0, 64, 0, 0), ("same", 63, 191, -1, -1),
          ("flip", 40, 191, 1, 1), ("same", 3, 64, 1, 1), ("same", 0, 64, -1, 1))
UNIT_VALUES = (0.5, 0.0, -0.5, 1.0, 1.5)
UNIT_ZERO_DB, UNIT_ZERO_Q = 6, 3


def _unit_set(specs):
    x = np.zeros((len(specs), 4, 2, 192))
    for s, (kind, pu, pv, su, sv) in enumerate(specs):
        for v in range(4):
            fu, fv = FLIPS[v] if kind == "flip" else (1, 1)
            x[s, v, 0, pu], x[s, v, 0, pv] = su * fu, sv * fv
            x[s, v, 1, 63 - pu], x[s, v, 1, 255 - pv] = su * fu, sv * fv          # channel 1: the same rows at mirrored places
    return x.reshape(4 * len(specs), 384)


def unit_family():
    """(queries [32, 384], DB [32, 384]) float64 at unit scale."""
    return _unit_set(UNIT_Q), _unit_set(UNIT_DB)
