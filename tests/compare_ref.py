"""aefft_image_compare_map restated (include/aefft.h): numpy for the sums, Python integers for the factors, IEEE doubles for the stated handful
of floating operations.  For the tests only -- the product never imports it.  np.cumsum(...)[-1] adds in order, as the definition does; np.sum
adds pairwise and does not."""
import numpy as np

K1, K2 = 65025, 585225            # 10000 C1, 10000 C2 at a data range of 255


def edges(W, M):
    """the first column of every cell of M on an axis of W, and W: ceil(I W / M) for I = 0..M"""
    return [-(-I * W // M) for I in range(M + 1)]


def check(W, H, D, Mx, My):
    if not (1 <= W <= 8192 and 1 <= H <= 8192 and 1 <= D <= 4 and 1 <= Mx <= min(W, 1024) and 1 <= My <= min(H, 1024)):
        raise ValueError("size out of range")
    if -(-W // Mx) > 64 or -(-H // My) > 64:
        raise ValueError("a cell side above 64")


def ssim_factors(n, Sx, Sr, Sxx, Srr, Sxr):
    """(A1, A2, B1, B2) of one channel of one cell, Python integers"""
    n, Sx, Sr, Sxx, Srr, Sxr = (int(v) for v in (n, Sx, Sr, Sxx, Srr, Sxr))
    return (20000 * Sx * Sr + K1 * n * n, 20000 * (n * Sxr - Sx * Sr) + K2 * n * n,
            10000 * (Sx * Sx + Sr * Sr) + K1 * n * n, 10000 * (n * Sxx - Sx * Sx + n * Srr - Sr * Sr) + K2 * n * n)


def ssim_channel(x, r):
    """the SSIM of one channel of one cell from its bytes: the integer form, one double"""
    x, r = x.astype(np.int64).ravel(), r.astype(np.int64).ravel()
    A1, A2, B1, B2 = ssim_factors(x.size, x.sum(), r.sum(), (x * x).sum(), (r * r).sum(), (x * r).sum())
    assert B1 > 0 and B2 > 0 and max(abs(A1), abs(A2), B1, B2) < 2 ** 63
    return (np.float64(A1) * np.float64(A2)) / (np.float64(B1) * np.float64(B2))


def ssim_textbook(x, r):
    """the float64 formula the integer form was cleared from"""
    x, r = x.astype(np.float64).ravel(), r.astype(np.float64).ravel()
    C1, C2 = 6.5025, 58.5225
    mx, mr = x.mean(), r.mean()
    vx, vr, cov = (x * x).mean() - mx * mx, (r * r).mean() - mr * mr, (x * r).mean() - mx * mr
    return ((2 * mx * mr + C1) * (2 * cov + C2)) / ((mx * mx + mr * mr + C1) * (vx + vr + C2))


def cell(x, r, metric):
    """one map entry from the cell's bytes x, r of shape [ny][nx][D]: a float32"""
    D = x.shape[-1]
    n = x.shape[0] * x.shape[1]
    if metric == "mse":
        d = x.astype(np.int64) - r.astype(np.int64)
        return np.float32(np.float64(int((d * d).sum())) / np.float64(D * n))
    s = ssim_channel(x[..., 0], r[..., 0])
    for d in range(1, D):
        s = s + ssim_channel(x[..., d], r[..., d])
    return np.float32(s / np.float64(D))


def compare_map(a, b, cells, metric="mse"):
    """a, b: uint8 [B][H][W][D]; returns map float32 [B][Mx][My]"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 4 and metric in ("mse", "ssim")
    B, H, W, D = a.shape
    Mx, My = cells
    check(W, H, D, Mx, My)
    ex, ey = edges(W, Mx), edges(H, My)
    if B * Mx * My <= 64:                                   # few cells: each from its bytes, the factors as Python integers
        out = np.empty((B, Mx, My), np.float32)
        for k in range(B):
            for I in range(Mx):
                for J in range(My):
                    out[k, I, J] = cell(a[k, ey[J]:ey[J + 1], ex[I]:ex[I + 1]], b[k, ey[J]:ey[J + 1], ex[I]:ex[I + 1]], metric)
        return out
    # many cells: the same integers in int64 (exact: every factor is below 2^63, and _cells asserts it), all cells at once
    x, r = a.astype(np.int64), b.astype(np.int64)
    n = np.outer(np.diff(ex), np.diff(ey)).astype(np.int64)[None, :, :, None]                  # [1][Mx][My][1]
    if metric == "mse":
        e = _cells((x - r) ** 2, ex, ey).sum(axis=3)
        return (e.astype(np.float64) / (D * n[..., 0]).astype(np.float64)).astype(np.float32)
    Sx, Sr, Sxx, Srr, Sxr = (_cells(v, ex, ey) for v in (x, r, x * x, r * r, x * r))
    bound = 20000.0 * Sx.astype(np.float64) * Sr.astype(np.float64) + 2.0 * K2 * n.astype(np.float64) ** 2 + 20000.0 * n * (Sxx + Srr).astype(np.float64)
    assert bound.max() < 2.0 ** 62
    A1, A2 = 20000 * Sx * Sr + K1 * n * n, 20000 * (n * Sxr - Sx * Sr) + K2 * n * n
    B1, B2 = 10000 * (Sx * Sx + Sr * Sr) + K1 * n * n, 10000 * (n * Sxx - Sx * Sx + n * Srr - Sr * Sr) + K2 * n * n
    q = (A1.astype(np.float64) * A2.astype(np.float64)) / (B1.astype(np.float64) * B2.astype(np.float64))
    s = q[..., 0]
    for d in range(1, D):
        s = s + q[..., d]
    return (s / np.float64(D)).astype(np.float32)


def _cells(v, ex, ey):
    """the sums of int64 [B][H][W][D] over every cell: [B][Mx][My][D]"""
    return np.add.reduceat(np.add.reduceat(v, ey[:-1], axis=1), ex[:-1], axis=2).transpose(0, 2, 1, 3)


def score(m, W, H):
    """the pixel-weighted mean of a map AS STORED (float32 [B][Mx][My]): float32 [B]"""
    m = np.asarray(m)
    assert m.dtype == np.float32 and m.ndim == 3
    B, Mx, My = m.shape
    nx, ny = np.diff(edges(W, Mx)), np.diff(edges(H, My))
    out = np.empty(B, np.float32)
    for k in range(B):
        r = [np.cumsum(m[k, I].astype(np.float64) * (nx[I] * ny).astype(np.float64))[-1] for I in range(Mx)]
        out[k] = np.float32(np.cumsum(np.array(r, np.float64))[-1] / np.float64(W * H))
    return out


def compare(a, b, cells, metric="mse"):
    m = compare_map(a, b, cells, metric)
    return m, score(m, a.shape[2], a.shape[1])
