"""Per-frame reconstruction error measurements, one process on one GPU; prints one JSON line.

Three nets -- cfg3-P2's (D=3, maps 8/16/32/64, 5x5, s=2) at 512^2 with B = 32, the same net at 640 x 480 (smooth sizes, operator form), cfg2
(256^2, maps 8/16/32) at B = 1 -- and per net ms per call of
  infer            aefft_net_infer, float frames in, float image out: the yardstick
  infer_torch      ... followed by torch's ((x - r)**2).mean((1, 2, 3)) on the same stream: what a caller does without aefft_net_score
  score            aefft_net_score without recon_d
  score_recon      aefft_net_score with recon_d
  score_u8         aefft_net_score, 8-bit frames, without recon_d
  score_u8_recon   aefft_net_score, 8-bit frames, with recon_d
--group map measures the per-tile map instead, with --tile (default 16, which divides every net's grid):
  score_pool       (a) aefft_net_score(.., recon_d) followed by torch's avg_pool2d of ((x - r)**2).sum(1) / D: what a caller does without
                       aefft_net_score_map
  map              (b) aefft_net_score_map without score_d and without recon_d (the C entry: Net.score_map always hands a score buffer over)
  map_score        (b') ... with score_d (one launch more)
  map_recon        (c) ... without score_d, with recon_d
  map_u8           (d) ... 8-bit frames, without score_d and recon_d
  score            (e) aefft_net_score without recon_d: the base
The variants are alternated in the process: --rounds rounds of --calls calls each between events on the library's stream (torch's current
stream: the torch expression is ordered on it), after --warmup calls of each.

    python tools/score_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--only NAME] [--variant NAME] [--group score|map] [--tile T]
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


def bench_net(ctx, name, calls, warmup, rounds, variants, group="score", tile=16):
    D, Nx, Ny, maps, Nk, s, B, smooth = NETS[name]
    t = ctx.torch
    rng = np.random.default_rng(len(name))
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, **(dict(smooth_sizes=True, operator_form=True) if smooth else {}))
    dD = D
    for l, dM in enumerate(maps):
        net.set_pair(l, rng.uniform(-1, 1, (dM, dD, Nk, Nk)), rng.uniform(-1, 1, dM), rng.uniform(-1, 1, (dD, dM, Nk, Nk)), rng.uniform(-1, 1, dD))
        dD = dM
    px = np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))
    f32, u8 = ctx.dev(px), t.as_tensor(px.astype(np.uint8), device=f"cuda:{ctx.device}")
    o32, sc = ctx.empty(B, D, Nx, Ny), ctx.empty(B)

    def infer_torch():
        net.infer(f32, o32)
        return ((f32 - o32) ** 2).mean((1, 2, 3))

    fns = {"infer": lambda: net.infer(f32, o32), "infer_torch": infer_torch,
           "score": lambda: net.score(f32, sc), "score_recon": lambda: net.score(f32, sc, o32),
           "score_u8": lambda: net.score(u8, sc), "score_u8_recon": lambda: net.score(u8, sc, o32)}
    if group == "map":
        mp = ctx.empty(B, Nx // tile, Ny // tile)

        def score_pool():
            net.score(f32, sc, o32)
            return t.nn.functional.avg_pool2d(((f32 - o32) ** 2).sum(1, keepdim=True), tile) / D

        P = aefft._ptr

        def c_map(frames, is_u8, recon):
            return lambda: ctx.check(net.L.aefft_net_score_map(net.h, P(frames), is_u8, tile, P(mp), None, P(recon)))

        fns = {"score_pool": score_pool, "map": c_map(f32, 0, None), "map_score": lambda: net.score_map(f32, tile, mp, sc), "map_recon": c_map(f32, 0, o32),
               "map_u8": c_map(u8, 1, None), "score": lambda: net.score(f32, sc)}
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
    ap.add_argument("--group", default="score", choices=["score", "map"])
    ap.add_argument("--tile", type=int, default=16)
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"lib": aefft.LIB_PATH, "calls": a.calls, "warmup": a.warmup, "group": a.group}
    if a.group == "map":
        out["tile"] = a.tile
    for name in NETS:
        if a.only and name != a.only:
            continue
        out[name] = bench_net(ctx, name, a.calls, a.warmup, a.rounds, [a.variant] if a.variant else [], a.group, a.tile)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
