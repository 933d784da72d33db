"""aefft_image_warp_affine and aefft_image_remap measurements, one process on one GPU; prints one JSON line.

8 images of 1920 x 1080 x 3 and 32 of 640 x 480 x 3 under a rotation of 5 degrees about the centre at the same size, nearest and linear, and 8 of
2448 x 2048 x 3 through the table of a barrel distortion (k1 = -0.12, k2 = 0.02); per row microseconds per call of
  a   the torch route on the same GPU, nothing pulled to the host: uint8 -> float NCHW, F.affine_grid / F.grid_sample(align_corners=True, zeros
      padding), round, clamp, back to interleaved uint8.  The affine rows build the grid inside the call (a pose per image arrives with the image);
      the table row uses a grid built once (a fixed calibration).  a is float arithmetic: it is the cost of the route, not the definition -- the
      largest difference from b in grey levels is reported beside the times
  b   the library's call: one launch, the affine or the table on the device, the destination reused
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also the bytes the call is accounted with (include/aefft.h) and the floor they set at the achievable HBM rate (6.3 TB/s).

    python tools/warp_bench.py [--calls 30] [--warmup 10] [--rounds 3] [--variant b]
"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
aefft = importlib.import_module("autoencoder-fft_amd")
from tools.image_bench import HBM_ACHIEVABLE, alternate, stats  # noqa: E402

AFFINE_SHAPES = {"8x1920x1080x3": (8, 1920, 1080, 3), "32x640x480x3": (32, 640, 480, 3)}      # B, W, H, D
TABLE_SHAPES = {"8x2448x2048x3": (8, 2448, 2048, 3)}
ANGLE = math.radians(5.0)


def rows(ctx, fns, nbytes, calls, warmup, rounds, variant, differ):
    fns = {k: v for k, v in fns.items() if not variant or k == variant}
    r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
    if "b" in r:
        r["b"].update(bytes=nbytes, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
    if "a" in r and "b" in r:
        r["a_over_b_rounds"] = [x / y for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"])]
        r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
        r["max_grey_levels_a_minus_b"] = differ()
    return r


def torch_route(t, F, img, grid_fn, mode):
    x = img.permute(0, 3, 1, 2).float()
    y = F.grid_sample(x, grid_fn(), mode=mode, padding_mode="zeros", align_corners=True)
    return y.round().clamp(0, 255).to(t.uint8).permute(0, 2, 3, 1).contiguous()


def bench_affine(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, W, H, D = AFFINE_SHAPES[name]
    dev = f"cuda:{ctx.device}"
    img = t.as_tensor(np.random.default_rng(len(name)).integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    c, s, cx, cy = math.cos(ANGLE), math.sin(ANGLE), (W - 1) / 2, (H - 1) / 2
    m = [[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]]             # destination -> source, about the centre
    q = t.as_tensor(aefft.affine_q(m), device=dev)
    # the same rotation in affine_grid's normalised coordinates (align_corners=True: x_n = 2 x / (W - 1) - 1)
    theta = t.tensor([[c, -s * (H - 1) / (W - 1), 0.0], [s * (W - 1) / (H - 1), c, 0.0]], device=dev).expand(B, 2, 3).contiguous()
    out = t.empty_like(img)
    res = {"B": B, "size": [W, H], "D": D}
    for interp, mode in (("nearest", "nearest"), ("linear", "bilinear")):
        fns = {"a": lambda: torch_route(t, F, img, lambda: F.affine_grid(theta, (B, D, H, W), align_corners=True), mode),
               "b": lambda: ctx.image_warp(img, q, interp=interp, out=out)}
        differ = lambda: int((fns["a"]().int() - fns["b"]().int()).abs().max().item())
        res[interp] = rows(ctx, fns, 2 * B * D * W * H + 48, calls, warmup, rounds, variant, differ)
    return res


def bench_table(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, W, H, D = TABLE_SHAPES[name]
    dev = f"cuda:{ctx.device}"
    img = t.as_tensor(np.random.default_rng(len(name)).integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    K = [[2200.0, 0, (W - 1) / 2], [0, 2200.0, (H - 1) / 2], [0, 0, 1]]
    table = aefft.undistort_table(K, (-0.12, 0.02, 0.0, 0.0, 0.0), (W, H))
    tab = t.as_tensor(table, device=dev)
    pos = tab.double() / 2048.0                                                   # the same positions, normalised for grid_sample
    grid = t.stack([2 * pos[..., 0] / (W - 1) - 1, 2 * pos[..., 1] / (H - 1) - 1], -1).float().expand(B, H, W, 2).contiguous()
    out = t.empty_like(img)
    fns = {"a": lambda: torch_route(t, F, img, lambda: grid, "bilinear"), "b": lambda: ctx.image_remap(img, tab, out=out)}
    differ = lambda: int((fns["a"]().int() - fns["b"]().int()).abs().max().item())
    return {"B": B, "size": [W, H], "D": D, "linear": rows(ctx, fns, 2 * B * D * W * H + 8 * W * H, calls, warmup, rounds, variant, differ)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a or b alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in AFFINE_SHAPES:
        out[name] = bench_affine(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    for name in TABLE_SHAPES:
        out[name] = bench_table(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
