"""aefft_image_tiles_to_frames / aefft_frames_tiles_to_image measurements, one process on one GPU; prints one JSON line.

8 images of 1920 x 1080 x 3 to 512^2 tiles with overlap 64 and rim 8 (120 frames), and 32 images of 640 x 480 x 3 to 256^2 tiles with overlap 32 and
rim 4; 8-bit frames; per case and direction microseconds per call of
  a   the torch route on the same GPU: F.pad(mode="reflect") + unfold + permute().contiguous() for the gather (reflect padding does not take
      bytes, so the image goes through float), a weighted F.fold, the division and the rounding for the blend
  b   the library's call
  c   for scale: aefft_image_to_frames / aefft_frames_to_image at the same number of frame bytes (T images of the tile's size)
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also its bytes (image + frames, what `image` accounts) over the median as a share of the achievable rate (6.3 TB/s), and whether a's result equals
b's.  With --net also Net.infer_tiled on the 1080p case (a 3 -> 8 -> 3 net, 5 x 5 kernels, scale 2, batch 8) beside its parts.

    python tools/tiles_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant b] [--net]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
aefft = importlib.import_module("autoencoder-fft_amd")
from tools.image_bench import alternate, stats  # noqa: E402

SHAPES = {"8x1920x1080->512x512": (8, 1920, 1080, 512, 64, 8), "32x640x480->256x256": (32, 640, 480, 256, 32, 4)}      # B, W, H, N, overlap, rim
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
D = 3


def axis_weights(W, N, V, M, n, o0):
    """[n][N] weights of each tile's own samples (include/aefft.h), zero where the sample lies outside the image"""
    S, R = N - V, V - 2 * M
    den = 2 * R if R > 0 else 1
    k = np.arange(N)[None, :]
    t = np.arange(n)[:, None]
    w = np.select([(k < M) | (k >= N - M), (t > 0) & (k < M + R), (t < n - 1) & (k >= N - M - R)], [0, 2 * (k - M) + 1, 2 * (N - M - 1 - k) + 1], den)
    x = o0 + t * S + k
    return np.where((x >= 0) & (x < W), w, 0).astype(np.float32), den


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, W, H, N, V, M = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    img = t.as_tensor(np.random.default_rng(len(name)).integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    _, p = aefft.tile_plan(W, H, N, N, V, M)
    T = B * p.ntx * p.nty
    pad = (-p.ox0, (p.ntx - 1) * p.step_x + N + p.ox0 - W, -p.oy0, (p.nty - 1) * p.step_y + N + p.oy0 - H)
    wx, denx = axis_weights(W, N, V, M, p.ntx, p.ox0)
    wy, deny = axis_weights(H, N, V, M, p.nty, p.oy0)
    # weight of sample [i][j] of tile (ty, tx), as fold takes its columns: [1][D * Ny * Nx][nty * ntx]
    wt = t.as_tensor(wy[:, None, :, None] * wx[None, :, None, :], device=dev).reshape(p.nty * p.ntx, 1, N * N).expand(-1, D, -1)
    wt = wt.reshape(p.nty * p.ntx, D * N * N).T.unsqueeze(0).contiguous()
    size = (H + pad[2] + pad[3], W + pad[0] + pad[1])

    def torch_gather():
        x = F.pad(img.permute(0, 3, 1, 2).float(), pad, mode="reflect")
        x = x.unfold(2, N, p.step_y).unfold(3, N, p.step_x)                     # [B][D][nty][ntx][Ny][Nx]
        return x.permute(0, 2, 3, 1, 5, 4).contiguous().to(t.uint8).view(T, D, N, N)

    tiles = ctx.image_tiles_to_frames(img, (N, N), V, M)

    def torch_blend():
        x = tiles.view(B, p.nty * p.ntx, D, N, N).permute(0, 2, 4, 3, 1).float().reshape(B, D * N * N, p.nty * p.ntx)      # columns: [d][j][i]
        acc = F.fold(x * wt, size, (N, N), stride=(p.step_y, p.step_x))[:, :, pad[2]:pad[2] + H, pad[0]:pad[0] + W]
        return ((2 * acc + denx * deny) / (2 * denx * deny)).floor().to(t.uint8).permute(0, 2, 3, 1).contiguous()

    plain = t.as_tensor(np.random.default_rng(1).integers(0, 256, (T, N, N, D), dtype=np.uint8), device=dev)
    pf = ctx.image_to_frames(plain)
    o_t, o_i, o_p = t.empty_like(tiles), t.empty_like(img), t.empty_like(plain)
    out = {"tiles": T, "torch_gather_equals": bool(t.equal(torch_gather(), tiles)),
           "torch_blend_equals": bool(t.equal(torch_blend(), ctx.frames_tiles_to_image(tiles, (W, H), V, M)))}
    cases = {"gather": {"a": torch_gather, "b": lambda: ctx.image_tiles_to_frames(img, (N, N), V, M, out=o_t), "c": lambda: ctx.image_to_frames(plain, out=pf)},
             "blend": {"a": torch_blend, "b": lambda: ctx.frames_tiles_to_image(tiles, (W, H), V, M, out=o_i), "c": lambda: ctx.frames_to_image(pf, out=o_p)}}
    nbytes = B * W * H * D + T * D * N * N
    for case, fns in cases.items():
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            rate = nbytes / (r["b"]["us_median"] * 1e-6)
            r["b"].update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
            if "a" in r:
                r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
                r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
            if "c" in r:
                r["b_over_c"] = r["b"]["us_median"] / r["c"]["us_median"]
        out[case] = r
    return out


def bench_net(ctx, calls, warmup, rounds):
    t = ctx.torch
    B, W, H, N, V, M = SHAPES["8x1920x1080->512x512"]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2)
    img = t.as_tensor(rng.integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    net = aefft.Net(ctx, D, N, N, [8], 5, 2, batch=8)
    net.set_pair(0, 0.05 * rng.uniform(-1, 1, (8, D, 5, 5)), rng.uniform(-1, 1, 8), 0.05 * rng.uniform(-1, 1, (D, 8, 5, 5)), rng.uniform(-1, 1, D))
    tiles = ctx.image_tiles_to_frames(img, (N, N), V, M)
    recon, out = t.empty_like(tiles), t.empty_like(img)

    def infer_all():
        for k in range(0, tiles.shape[0], 8):
            net.infer(tiles[k:k + 8], recon[k:k + 8])

    fns = {"infer_tiled": lambda: net.infer_tiled(img, V, M, out=out), "gather": lambda: ctx.image_tiles_to_frames(img, (N, N), V, M, out=tiles),
           "infer_chunks": infer_all, "blend": lambda: ctx.frames_tiles_to_image(recon, (W, H), V, M, out=out)}
    r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
    r["sum_of_parts_us"] = r["gather"]["us_median"] + r["infer_chunks"]["us_median"] + r["blend"]["us_median"]
    net.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b or c alone")
    ap.add_argument("--net", action="store_true", help="also Net.infer_tiled on the 1080p case beside its parts")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        out[name] = bench(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    if a.net:
        out["infer_tiled 8x1920x1080"] = bench_net(ctx, max(1, a.calls // 8), max(1, a.warmup // 5), a.rounds)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
