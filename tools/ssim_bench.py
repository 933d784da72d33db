"""Block-SSIM and target-score measurements, one process on one GPU; prints one JSON line.

Two nets -- cfg3-P2's (D=3, maps 8/16/32/64, 5x5, s=2) at 512^2 with B = 32 and the same net at 640 x 480 (smooth sizes, operator form) -- and
per net ms per call of
  infer            aefft_net_infer, float frames in, float image out: the yardstick
  map              aefft_net_score_map(tile 8) without score_d and without recon_d (the C entry)
  map_target       aefft_net_score_map_target with the same arguments and a float target
  ssim8            aefft_net_ssim_map(tile 8, float target) without score_d and without recon_d
  ssim64           ... tile 64 (512^2 only: 64 does not divide 480; the 640 x 480 net takes 32, reported as ssim32)
  ssim8_u8         ... tile 8, 8-bit frames and 8-bit target
  infer_torch_ssim aefft_net_infer followed by torch's block SSIM (tile 8, avg_pool2d of the five moments) of the stored reconstruction: what a
                   caller does without aefft_net_ssim_map
The variants are alternated in the process: --rounds rounds of --calls calls each between events on the library's stream (torch's current
stream: the torch expression is ordered on it), after --warmup calls of each.

    python tools/ssim_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--only NAME] [--variant NAME]
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
from tools.infer_bench import NETS  # noqa: E402
from tools.sizes_bench import timed  # noqa: E402

NAMES = ("cfg3p2", "cfg3p2_640x480")


def bench_net(ctx, name, calls, warmup, rounds, variants):
    D, Nx, Ny, maps, Nk, s, B, smooth = NETS[name]
    t = ctx.torch
    rng = np.random.default_rng(len(name))
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, **(dict(smooth_sizes=True, operator_form=True) if smooth else {}))
    dD = D
    for l, dM in enumerate(maps):
        net.set_pair(l, rng.uniform(-1, 1, (dM, dD, Nk, Nk)), rng.uniform(-1, 1, dM), rng.uniform(-1, 1, (dD, dM, Nk, Nk)), rng.uniform(-1, 1, dD))
        dD = dM
    px, tg = (np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))) for _ in range(2))
    dev = f"cuda:{ctx.device}"
    f32, u8 = ctx.dev(px), t.as_tensor(px.astype(np.uint8), device=dev)
    t32, t8 = ctx.dev(tg), t.as_tensor(tg.astype(np.uint8), device=dev)
    o32 = ctx.empty(B, D, Nx, Ny)
    big = 64 if Nx % 64 == 0 and Ny % 64 == 0 else 32
    maps_ = {tile: ctx.empty(B, Nx // tile, Ny // tile) for tile in (8, big)}
    P = aefft._ptr
    L, C1, C2 = 255.0, (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2

    def c_ssim(frames, targets, is_u8, tile):
        return lambda: ctx.check(net.L.aefft_net_ssim_map(net.h, P(frames), is_u8, P(targets), is_u8, tile, L, P(maps_[tile]), None, None))

    def infer_torch_ssim():
        net.infer(f32, o32)
        pool = lambda a: t.nn.functional.avg_pool2d(a, 8)
        mx, mr = pool(t32), pool(o32)
        vx, vr, c = (pool(t32 * t32) - mx * mx).clamp_min(0), (pool(o32 * o32) - mr * mr).clamp_min(0), pool(t32 * o32) - mx * mr
        return ((2 * mx * mr + C1) * (2 * c + C2) / ((mx * mx + mr * mr + C1) * (vx + vr + C2))).mean(1)

    fns = {"infer": lambda: net.infer(f32, o32),
           "map": lambda: ctx.check(net.L.aefft_net_score_map(net.h, P(f32), 0, 8, P(maps_[8]), None, None)),
           "map_target": lambda: ctx.check(net.L.aefft_net_score_map_target(net.h, P(f32), 0, P(t32), 0, 8, P(maps_[8]), None, None)),
           "ssim8": c_ssim(f32, t32, 0, 8), f"ssim{big}": c_ssim(f32, t32, 0, big), "ssim8_u8": c_ssim(u8, t8, 1, 8),
           "infer_torch_ssim": infer_torch_ssim}
    fns = {k: v for k, v in fns.items() if not variants or k in variants}
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ctx.sync()
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(timed(ctx, fn, calls))
    form = net.step_form()
    net.close()
    return {"form": form, **{k: {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)} for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--variant", default="")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"lib": aefft.LIB_PATH, "calls": a.calls, "warmup": a.warmup}
    for name in NAMES:
        if a.only and name != a.only:
            continue
        out[name] = bench_net(ctx, name, a.calls, a.warmup, a.rounds, [a.variant] if a.variant else [])
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
