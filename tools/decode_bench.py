"""Decode measurements, one process on one GPU; prints one JSON line.

Three nets -- cfg3-P2's (D=3, maps 8/16/32/64, 5x5, s=2) at 512^2 with B = 32, the same net at 640 x 480 (smooth sizes, operator form), cfg2
(256^2, maps 8/16/32) at B = 1 -- and per net ms per call of
  infer       aefft_net_infer, float frames in, float image out (reconstruction only): the yardstick, of the same library on the same net
  infer_u8    ... 8-bit image out (float frames in)
  decode      aefft_net_decode from the innermost pair's hidden layer (--pair: another pair), float image out
  decode_u8   ... 8-bit image out
The variants are alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup
calls of each (the operators of both calls are cached by then).

    python tools/decode_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--only NAME] [--pair L]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/decode_bench.py --only cfg3p2 --variant decode --rounds 1
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
from tools.sizes_bench import timed  # noqa: E402
from tools.infer_bench import NETS  # noqa: E402


def bench_net(ctx, name, calls, warmup, rounds, variants, pair):
    D, Nx, Ny, maps, Nk, s, B, smooth = NETS[name]
    t = ctx.torch
    rng = np.random.default_rng(len(name))
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, **(dict(smooth_sizes=True, operator_form=True) if smooth else {}))
    dD = D
    for l, dM in enumerate(maps):
        net.set_pair(l, rng.uniform(-1, 1, (dM, dD, Nk, Nk)), rng.uniform(-1, 1, dM), rng.uniform(-1, 1, (dD, dM, Nk, Nk)), rng.uniform(-1, 1, dD))
        dD = dM
    l = len(maps) - 1 if pair < 0 else pair
    g = net.dims[l]
    f32 = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))))
    code = ctx.empty(B, g["dM"], g["Nx"], g["Ny"])
    o32, o8 = ctx.empty(B, D, Nx, Ny), ctx.empty(B, D, Nx, Ny, dtype=t.uint8)
    net.infer(f32, None, l, code)          # the code decode reads: the frames' own hidden layer
    fns = {"infer": lambda: net.infer(f32, o32), "infer_u8": lambda: net.infer(f32, o8),
           "decode": lambda: net.decode(code, l, o32), "decode_u8": lambda: net.decode(code, l, o8)}
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
    return {"form": form, "pair": l, **{k: {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)} for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--variant", default="")
    ap.add_argument("--pair", type=int, default=-1)
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"lib": aefft.LIB_PATH, "calls": a.calls, "warmup": a.warmup}
    for name in NETS:
        if a.only and name != a.only:
            continue
        out[name] = bench_net(ctx, name, a.calls, a.warmup, a.rounds, [a.variant] if a.variant else [], a.pair)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
