"""aefft_image_compare_map measurements, one process on one GPU; prints one JSON line.

8 images of 1920 x 1080 x 3 on 120 x 68 cells and 32 images of 640 x 480 x 3 on 40 x 30 cells (cells of about 16 pixels); both metrics, with and
without the score; per case microseconds per call of
  a   the torch route on the same GPU: float copies of both images, the squared difference or the five moment products, an avg_pool2d
      reduction (ceil_mode: these cells are 16 pixels but for the last row of the 1080p grid), the formula, the mean
  b   the library's call, on the same two buffers every time (99.5 / 59 MB: they fit the 256 MiB last-level cache)
  b_cold   the call on a ring of image pairs of more than twice that cache, so that every call reads from memory
  d   for scale: aefft_frames_tiles_to_image on the same image (512^2 tiles, overlap 64, rim 8; 256^2, 32, 4), which the call follows in
      Net.score_tiled
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also c, the floor: its accounted bytes (2 B W H D + 4 B Mx My) over the achievable rate (6.3 TB/s), and b as a multiple of it; and how far a's
map lies from b's.  With --net also Net.score_tiled beside Net.infer_tiled on the 1080p case (a 3 -> 8 -> 3 net, 5 x 5 kernels, scale 2, batch 8).

    python tools/compare_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant b] [--net]
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

SHAPES = {"8x1920x1080 on 120x68": (8, 1920, 1080, 512, 64, 8), "32x640x480 on 40x30": (32, 640, 480, 256, 32, 4)}      # B, W, H, then d's tile, overlap, rim
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
CACHE_BYTES = 256 << 20                                                         # the last-level (Infinity) cache
D, TILE = 3, 16


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, W, H, N, V, M = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name))
    a8 = rng.integers(0, 256, (B, H, W, D), dtype=np.uint8)
    b8 = (a8.astype(np.int64) + rng.integers(-30, 31, a8.shape)).clip(0, 255).astype(np.uint8)
    a, b = t.as_tensor(a8, device=dev), t.as_tensor(b8, device=dev)
    Mx, My = aefft.cells_for_tile(W, H, TILE)
    pool = lambda v: F.avg_pool2d(v, TILE, ceil_mode=True)                       # [B][D][H][W] -> [B][D][My][Mx], the short last cells by their own count

    def torch_mse(score):
        x, r = a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()
        m = pool((x - r) ** 2).mean(dim=1).transpose(1, 2).contiguous()
        return (m, m.mean(dim=(1, 2))) if score else (m, None)                   # (the plain mean of the map, as for SSIM: the cells are all but equal)

    def torch_ssim(score):
        x, r = a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()
        mx, mr, mxx, mrr, mxr = pool(x), pool(r), pool(x * x), pool(r * r), pool(x * r)
        s = ((2 * mx * mr + 6.5025) * (2 * (mxr - mx * mr) + 58.5225)) / ((mx * mx + mr * mr + 6.5025) * (mxx - mx * mx + mrr - mr * mr + 58.5225))
        m = s.mean(dim=1).transpose(1, 2).contiguous()
        return (m, m.mean(dim=(1, 2))) if score else (m, None)                   # (the plain mean: the cells are all but equal)

    _, p = aefft.tile_plan(W, H, N, N, V, M)
    tiles = ctx.image_tiles_to_frames(a, (N, N), V, M)
    o_i, o_m, o_s = t.empty_like(a), ctx.empty(B, Mx, My), ctx.empty(B)
    nbytes = 2 * B * W * H * D + 4 * B * Mx * My
    out = {"cells": [Mx, My], "bytes": nbytes, "floor_us": 1e6 * nbytes / HBM_ACHIEVABLE}
    # b_cold: the call on a ring of image pairs larger than the 256 MiB last-level cache twice over, so that no call finds its bytes there
    ring = [(a.clone(), b.clone()) for _ in range(-(-2 * CACHE_BYTES // (2 * a.numel())) + 1)]
    turn = [0]

    def cold(metric, score):
        x, r = ring[turn[0] % len(ring)]
        turn[0] += 1
        return ctx.image_compare_map(x, r, (Mx, My), metric, map=o_m, score=o_s if score else False)

    for metric, route in (("mse", torch_mse), ("ssim", torch_ssim)):
        got = ctx.image_compare_map(a, b, (Mx, My), metric)[0]
        if W % TILE == 0 and H % TILE == 0:                                      # (otherwise avg_pool2d's cells are not the call's: 16 x 67 + 8 rows against 15s and 16s)
            out[f"{metric}_torch_max_abs_difference"] = float((route(False)[0] - got).abs().max())
        for score in (True, False):
            fns = {"a": lambda: route(score), "b": lambda: ctx.image_compare_map(a, b, (Mx, My), metric, map=o_m, score=o_s if score else False),
                   "b_cold": lambda: cold(metric, score), "d": lambda: ctx.frames_tiles_to_image(tiles, (W, H), V, M, out=o_i)}
            fns = {k: v for k, v in fns.items() if not variant or k == variant}
            r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
            if "b_cold" in r:
                r["b_cold_over_floor_rounds"] = [u / out["floor_us"] for u in r["b_cold"]["us_rounds"]]
            if "b" in r:
                r["b_over_floor"] = r["b"]["us_median"] / out["floor_us"]
                r["b_over_floor_rounds"] = [u / out["floor_us"] for u in r["b"]["us_rounds"]]
                if "a" in r:
                    r["a_over_b_rounds"] = [x / y for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"])]
                    r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
                if "d" in r:
                    r["b_over_d_rounds"] = [x / y for x, y in zip(r["b"]["us_rounds"], r["d"]["us_rounds"])]
            out[f"{metric}{' + score' if score else ''}"] = r
    return out


def bench_net(ctx, calls, warmup, rounds):
    t = ctx.torch
    B, W, H, N, V, M = SHAPES["8x1920x1080 on 120x68"]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(2)
    img = t.as_tensor(rng.integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    net = aefft.Net(ctx, D, N, N, [8], 5, 2, batch=8)
    net.set_pair(0, 0.05 * rng.uniform(-1, 1, (8, D, 5, 5)), rng.uniform(-1, 1, 8), 0.05 * rng.uniform(-1, 1, (D, 8, 5, 5)), rng.uniform(-1, 1, D))
    Mx, My = aefft.cells_for_tile(W, H, TILE)
    out, m, s = t.empty_like(img), ctx.empty(B, Mx, My), ctx.empty(B)
    fns = {"infer_tiled": lambda: net.infer_tiled(img, V, M, out=out),
           "score_tiled mse": lambda: net.score_tiled(img, V, M, tile=TILE, metric="mse", map=m, score=s, out=out),
           "score_tiled ssim": lambda: net.score_tiled(img, V, M, tile=TILE, metric="ssim", map=m, score=s, out=out)}
    r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
    for k in ("score_tiled mse", "score_tiled ssim"):
        r[k + " over infer_tiled, rounds"] = [x / y for x, y in zip(r[k]["us_rounds"], r["infer_tiled"]["us_rounds"])]
    net.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b, b_cold or d alone")
    ap.add_argument("--net", action="store_true", help="also Net.score_tiled beside Net.infer_tiled on the 1080p case")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        out[name] = bench(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    if a.net:
        out["score_tiled 8x1920x1080"] = bench_net(ctx, max(1, a.calls // 8), max(1, a.warmup // 5), a.rounds)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
