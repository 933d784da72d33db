"""The numpy restatement of aefft_frames_degrade (include/aefft.h, steps 1 to 6): Philox4x32-10 in uint64 arithmetic, everything else in int64.
A test helper only: the product never imports it."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SIGMA_T = math.sqrt(32767.5)          # the standard deviation of T: six bytes of variance (256^2 - 1) / 12 each


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit words -> the four output words as uint64 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]                 # (< 2^64: both factors are below 2^32)
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def px_u8(v):
    """SpinToImage_C's rule on float32 values: NaN -> 0, clamp to 0..255, halves away from zero; floor(t + 0.5) in float64 is exact for |t| < 2^24"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = np.minimum(np.floor(v.astype(np.float64) + 0.5), 255.0)
        return np.where(v > 0, r, 0.0).astype(np.uint8)


def weights(r):
    return np.array([math.comb(2 * r, k) for k in range(2 * r + 1)], dtype=np.int64)


def quantise(sigma, impulse):
    """the host's two quantisations: (m, t).  sigma and impulse reach the library as float32"""
    s, p = float(np.float32(sigma)), float(np.float32(impulse))
    return int(math.floor((s * 65536.0) / SIGMA_T + 0.5)), int(math.floor(p * 65536.0 + 0.5))


def sigma_eff(sigma):
    return quantise(sigma, 0.0)[0] * SIGMA_T / 65536.0


def blur_q16(p, r):
    """step 2 on pixels p [..][Nx][Ny] (any integer type): u in Q16, int64"""
    p = np.asarray(p).astype(np.int64)
    Nx, Ny = p.shape[-2:]
    w = weights(r)
    h = np.zeros_like(p)
    for k in range(2 * r + 1):
        h += w[k] * p[..., np.clip(np.arange(Nx) + k - r, 0, Nx - 1), :]
    v = np.zeros_like(p)
    for l in range(2 * r + 1):
        v += w[l] * h[..., :, np.clip(np.arange(Ny) + l - r, 0, Ny - 1)]
    assert v.max(initial=0) <= 255 * 16 ** r < 2 ** 24
    return v << (16 - 4 * r)


def random_words(shape, seed, first_frame):
    """step 3 for frames [B][D][Nx][Ny]: (a, c) as uint64 arrays of that shape"""
    B, D, Nx, Ny = shape
    n = np.arange(D * Nx * Ny, dtype=np.uint64)
    a = np.empty((B, D * Nx * Ny), dtype=np.uint64)
    c = np.empty_like(a)
    odd = (n & np.uint64(1)) == 1
    for b in range(B):
        g = (int(first_frame) + b) & 0xFFFFFFFFFFFFFFFF
        x = philox4x32((n >> np.uint64(1), 0, g & 0xFFFFFFFF, g >> 32), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        a[b] = np.where(odd, x[2], x[0])
        c[b] = np.where(odd, x[3], x[1])
    return a.reshape(shape), c.reshape(shape)


def irwin_hall(a, c):
    a, c = a.astype(np.int64), c.astype(np.int64)
    return (a & 255) + ((a >> 8) & 255) + ((a >> 16) & 255) + ((a >> 24) & 255) + (c & 255) + ((c >> 8) & 255) - 765


def degrade_q16(src, blur=0, sigma=0.0, impulse=0.0, seed=0, first_frame=0):
    """steps 1 to 5: src uint8 or float32 [B][D][Nx][Ny] -> u, int64 (|u| < 2^27)"""
    src = np.asarray(src)
    assert src.ndim == 4 and src.dtype in (np.uint8, np.float32)
    p = px_u8(src) if src.dtype == np.float32 else src                           # 1.
    u = blur_q16(p, blur)                                                        # 2.
    m, t = quantise(sigma, impulse)
    a, c = random_words(src.shape, seed, first_frame)                            # 3.
    u = u + irwin_hall(a, c) * m                                                 # 4.
    hit = (c >> np.uint64(16)).astype(np.int64) < t                              # 5.
    u = np.where(hit, np.where((a & np.uint64(1)) == 1, 255 << 16, 0), u)
    assert np.abs(u).max(initial=0) < 2 ** 27
    return u.astype(np.int64)


def degrade(src, blur=0, sigma=0.0, impulse=0.0, seed=0, first_frame=0, dtype=None):
    """the whole definition: the result as uint8 or float32 (`dtype`, the source's by default)"""
    src = np.asarray(src)
    dtype = np.dtype(src.dtype if dtype is None else dtype)
    u = degrade_q16(src, blur, sigma, impulse, seed, first_frame)
    if dtype == np.uint8:                                                        # 6.
        return np.clip((u + 32768) >> 16, 0, 255).astype(np.uint8)
    assert dtype == np.float32
    return u.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -16)
