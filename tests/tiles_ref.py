"""The numpy restatement of tiled inference as include/aefft.h defines it (aefft_tile_plan_make, aefft_image_tiles_to_frames,
aefft_frames_tiles_to_image): the plan per axis, the iterated reflection, the per-axis weights exactly as the header's four cases state them, the
gather and the blend as the sum over EVERY tile in 64-bit integers.  It shares nothing with the library; the product never imports it."""
import numpy as np


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def legal(W, N, V, M):
    return 1 <= W <= 8192 and 2 <= N <= 2048 and 0 <= 2 * V <= N and 0 <= 2 * M <= V


def axis(W, N, V, M):
    """one axis of the plan: dict(n, S, R, o0, den, W, N, V, M); ValueError for values out of range"""
    if not legal(W, N, V, M):
        raise ValueError((W, N, V, M))
    S, R = N - V, V - 2 * M
    n = max(1, -((-(W - N + 2 * M)) // S) + 1)                   # ceil as the negated floor: integers only
    E = (n - 1) * S + N - 2 * M - W
    assert E >= 0
    return dict(n=n, S=S, R=R, o0=-M - E // 2, den=2 * R if R > 0 else 1, W=W, N=N, V=V, M=M)


def plan(W, H, Nx, Ny, overlap, rim=0):
    """(ntx, nty, ox0, oy0, step_x, step_y, ramp_x, ramp_y)"""
    (vx, vy), (mx, my) = _pair(overlap), _pair(rim)
    x, y = axis(W, Nx, vx, mx), axis(H, Ny, vy, my)
    return x["n"], y["n"], x["o0"], y["o0"], x["S"], y["S"], x["R"], y["R"]


def reflect(x, W):
    """reflection without repeating the edge pixel, iterated"""
    x = np.asarray(x, np.int64)
    if W == 1:
        return np.zeros_like(x)
    P = 2 * (W - 1)
    m = np.mod(x, P)                                             # (numpy's mod is non-negative for a positive P)
    return np.where(m < W, m, P - m)


def weights(a):
    """[n][W] int64: the weight of tile t of axis `a` at image coordinate x, the header's four cases in their order (np.select takes the first
    condition that holds)"""
    N, M, R = a["N"], a["M"], a["R"]
    t = np.arange(a["n"], dtype=np.int64)[:, None]
    k = np.arange(a["W"], dtype=np.int64)[None, :] - (a["o0"] + t * a["S"])
    return np.select([(k < M) | (k >= N - M), (t > 0) & (k < M + R), (t < a["n"] - 1) & (k >= N - M - R)],
                     [0, 2 * (k - M) + 1, 2 * (N - M - 1 - k) + 1], a["den"]).astype(np.int64)


def px_u8(v):
    """SpinToImage_C's rule: NaN -> 0, clamp to 0..255, halves away from zero"""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(np.floor(v + 0.5), 255.0), 0.0).astype(np.uint8)


def gather(image, Nx, Ny, overlap, rim=0, dtype=np.uint8):
    """image uint8 [B][H][W][D] -> frames [B * ntx * nty][D][Nx][Ny]: frames[f][d][i][j] = image[b][ry(oy + j)][rx(ox + i)][d]"""
    B, H, W, D = image.shape
    (vx, vy), (mx, my) = _pair(overlap), _pair(rim)
    ax, ay = axis(W, Nx, vx, mx), axis(H, Ny, vy, my)
    out = np.empty((B, ay["n"], ax["n"], D, Nx, Ny), dtype)
    for ty in range(ay["n"]):
        ys = reflect(ay["o0"] + ty * ay["S"] + np.arange(Ny), H)
        for tx in range(ax["n"]):
            xs = reflect(ax["o0"] + tx * ax["S"] + np.arange(Nx), W)
            out[:, ty, tx] = image[:, ys][:, :, xs].transpose(0, 3, 2, 1)          # [B][Ny][Nx][D] -> [B][D][Nx][Ny]
    return out.reshape(B * ay["n"] * ax["n"], D, Nx, Ny)


def blend(frames, W, H, overlap, rim=0):
    """frames uint8 or float32 [T][D][Nx][Ny] -> image uint8 [B][H][W][D]: floor((2 sum wx wy p + denx deny) / (2 denx deny)) over every tile"""
    T, D, Nx, Ny = frames.shape
    (vx, vy), (mx, my) = _pair(overlap), _pair(rim)
    ax, ay = axis(W, Nx, vx, mx), axis(H, Ny, vy, my)
    per = ax["n"] * ay["n"]
    assert T % per == 0
    B = T // per
    p = (frames if frames.dtype == np.uint8 else px_u8(frames)).astype(np.int64).reshape(B, ay["n"], ax["n"], D, Nx, Ny)
    wx, wy = weights(ax), weights(ay)
    acc = np.zeros((B, H, W, D), np.int64)
    for ty in range(ay["n"]):
        oy = ay["o0"] + ty * ay["S"]
        y0, y1 = max(0, oy), min(H, oy + Ny)
        for tx in range(ax["n"]):
            ox = ax["o0"] + tx * ax["S"]
            x0, x1 = max(0, ox), min(W, ox + Nx)
            if y0 >= y1 or x0 >= x1:
                continue
            tile = p[:, ty, tx, :, x0 - ox:x1 - ox, y0 - oy:y1 - oy].transpose(0, 3, 2, 1)      # [B][y][x][D]
            acc[:, y0:y1, x0:x1] += wy[ty, y0:y1, None, None] * wx[tx, None, x0:x1, None] * tile
    dd = ax["den"] * ay["den"]
    out = (2 * acc + dd) // (2 * dd)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
