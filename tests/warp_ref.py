"""The numpy restatement of include/aefft.h "aefft_image_warp_affine, aefft_image_remap": int64 arithmetic throughout, every border rule, both
interpolations, the affine's (tx, ty) with its wrap and clamp, aefft_affine_make's rounding and ranges.  The tests compare the library with this
module byte for byte; the product never imports it (tests/test_warp_abi.py asserts that).  A plain module -- pytest collects nothing from it."""
from fractions import Fraction

import numpy as np

INTERP = {"nearest": 0, "linear": 1}
BORDER = {"constant": 0, "replicate": 1, "reflect": 2}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
LIN_LIMIT, OFF_LIMIT = 2 ** 29, 2 ** 39                                          # |a[0,1,3,4]| and |a[2,5]| at most


def affine_make(m):
    """a[k] = m[k] * 2^24 rounded to nearest, ties to even, as six Python ints; None for what aefft_affine_make refuses"""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(6)]
    if not all(np.isfinite(m)):
        return None
    a = [round(Fraction(v) * 2 ** 24) for v in m]                                # (round on a Fraction: exact, ties to even)
    if any(abs(a[k]) > LIN_LIMIT for k in (0, 1, 3, 4)) or any(abs(a[k]) > OFF_LIMIT for k in (2, 5)):
        return None
    return a


def _wrap64(v):
    """Python ints (an object array) modulo 2^64, as signed"""
    return ((v + 2 ** 63) % 2 ** 64) - 2 ** 63


def affine_txty(a, Wd, Hd):
    """(tx, ty) int64 [Hd][Wd] of six Q24 coefficients (any 64-bit patterns): wrapping 64-bit U and V, (U + 2^12) >> 13, clamped to int32"""
    a = [int(v) for v in a]
    exact = max(abs(v) for v in a) < 2 ** 45                                     # then |U| < 2^60: int64 holds it and nothing wraps; Python ints otherwise
    y, x = np.meshgrid(np.arange(Hd, dtype=np.int64 if exact else object), np.arange(Wd, dtype=np.int64 if exact else object), indexing="ij")
    out = []
    for k in (0, 3):
        U = a[k] * x + a[k + 1] * y + a[k + 2]
        if exact:
            out.append(np.clip((U + 4096) >> 13, I32_MIN, I32_MAX))
            continue
        U = _wrap64(U)
        t = _wrap64(U + 4096) >> 13                                              # (Python's >> on ints is arithmetic)
        out.append(np.clip(t, I32_MIN, I32_MAX).astype(np.int64))
    return out[0], out[1]


def border_index(s, S, border):
    """the index a tap at s reads on an axis of S, and whether it is live (False: CONSTANT outside the image)"""
    s = np.asarray(s, np.int64)
    inside = (s >= 0) & (s < S)
    if border == "reflect":
        if S == 1:
            return np.zeros_like(s), np.ones(s.shape, bool)
        P = 2 * (S - 1)
        m = np.mod(s, P)                                                         # (numpy's mod takes the divisor's sign: non-negative)
        return np.where(m < S, m, P - m), np.ones(s.shape, bool)
    return np.clip(s, 0, S - 1), inside if border == "constant" else np.ones(s.shape, bool)


def sample(src, tx, ty, interp="linear", border="constant", value=0):
    """src uint8 [Hs][Ws][D], tx, ty integers [Hd][Wd] (the source position times 2048) -> uint8 [Hd][Wd][D]"""
    Hs, Ws, D = src.shape
    tx, ty = np.asarray(tx, np.int64), np.asarray(ty, np.int64)
    const = np.array([(int(value) >> (8 * d)) & 255 for d in range(D)], np.int64)
    s = src.astype(np.int64)

    def tap(sy, sx):
        iy, ly = border_index(sy, Hs, border)
        ix, lx = border_index(sx, Ws, border)
        return np.where((ly & lx)[..., None], s[iy, ix], const)

    if interp == "nearest":
        return tap((ty + 1024) >> 11, (tx + 1024) >> 11).astype(np.uint8)
    sx, sy, wx, wy = tx >> 11, ty >> 11, (tx & 2047)[..., None], (ty & 2047)[..., None]
    v = (2048 - wy) * ((2048 - wx) * tap(sy, sx) + wx * tap(sy, sx + 1)) + wy * ((2048 - wx) * tap(sy + 1, sx) + wx * tap(sy + 1, sx + 1))
    assert v.max(initial=0) < 2 ** 30
    return ((v + 2 ** 21) >> 22).astype(np.uint8)


def border_word(value, D):
    """border_value of per-channel bytes"""
    return sum((int(v) & 255) << (8 * d) for d, v in enumerate(list(value)[:D]))


def warp_affine(src, a, size, interp="linear", border="constant", value=0):
    """src uint8 [B][Hs][Ws][D]; a: six Q24 integers, or B rows of six -> uint8 [B][Hd][Wd][D]"""
    Wd, Hd = size
    rows = [a] * len(src) if np.ndim(a[0]) == 0 else list(a)
    assert len(rows) == len(src)
    return np.stack([sample(img, *affine_txty(r, Wd, Hd), interp, border, value) for img, r in zip(src, rows)])


def remap(src, table, interp="linear", border="constant", value=0):
    """src uint8 [B][Hs][Ws][D], table int32 [Hd][Wd][2] (x first) -> uint8 [B][Hd][Wd][D]"""
    return np.stack([sample(img, table[..., 0], table[..., 1], interp, border, value) for img in src])
