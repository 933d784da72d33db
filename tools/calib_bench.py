"""aefft_map_stats_update / _merge / _finish and aefft_map_peak measurements, one process on one GPU; prints one JSON line.

8 maps of 240 x 135 cells (1920 x 1080 at 8 pixels a cell), 32 of 40 x 30 (640 x 480 at 16) and one of 1024 x 1024 (the largest the calls take),
random float32 in 0..65025; per call and shape microseconds per call of
  a   the torch route on the same GPU, nothing pulled to the host: update -- map.double() sums over b added to float64 planes, and torch.topk
      (largest and smallest 4) over the kept extremes concatenated with the footage; merge -- two additions and two topk over eight; finish --
      the SIGMA formulas on float64 tensors (RANK: indexing the kept plane); peak -- (map - ref).flatten(1).max(1), value and index.  a does not
      skip non-finite values, count per cell or treat -0, and its sums reduce over b in torch's order: it is the cost of the route, not the
      definition
  b   the library's call: one launch, state and outputs reused
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also the bytes the call is accounted with (include/aefft.h) and the floor they set at the achievable HBM rate (6.3 TB/s).

    python tools/calib_bench.py [--calls 30] [--warmup 10] [--rounds 3] [--variant b]
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
from tools.image_bench import HBM_ACHIEVABLE, alternate, stats  # noqa: E402

SHAPES = {"8x240x135": (8, 240, 135), "32x40x30": (32, 40, 30), "1x1024x1024": (1, 1024, 1024)}      # B, Mx, My


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    B, Mx, My = SHAPES[name]
    n = Mx * My
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name))
    m = t.as_tensor((rng.random((B, Mx, My)) * 65025).astype(np.float32), device=dev)
    state, other = ctx.map_stats(Mx, My), ctx.map_stats(Mx, My)
    for _ in range(2):                                                           # (more than four values a cell: every slot live)
        ctx.map_stats_update(state, m)
        ctx.map_stats_update(other, m)
    ref = ctx.map_stats_finish(state, (Mx, My), "sigma", k=3.0)
    ref_rank = ctx.empty(Mx, My)
    peak, cell = ctx.map_peak(m, ref)
    S1, S2, hi, lo, c = (v.clone() for v in aefft.map_stats_view(state, Mx, My))
    o1, o2, ohi, olo, _ = (v.clone() for v in aefft.map_stats_view(other, Mx, My))
    cd = c.double()

    def a_update():
        d = m.double()
        S1.add_(d.sum(0))
        S2.add_((d * d).sum(0))
        c.add_(B)
        return t.topk(t.cat([hi, m]), 4, dim=0).values, t.topk(t.cat([lo, m]), 4, dim=0, largest=False).values

    def a_merge():
        return S1 + o1, S2 + o2, t.topk(t.cat([hi, ohi]), 4, dim=0).values, t.topk(t.cat([lo, olo]), 4, dim=0, largest=False).values

    def a_sigma():
        mean = S1 / cd
        sd = ((S2 - S1 * mean).clamp_min(0) / (cd - 1)).sqrt()
        return (mean + 3.0 * sd).float()

    cases = {
        "update": (4 * B * n + 104 * n, {"a": a_update, "b": lambda: ctx.map_stats_update(state, m)}),
        "merge": (156 * n, {"a": a_merge, "b": lambda: ctx.map_stats_merge(state, other)}),
        "finish_sigma": (56 * n, {"a": a_sigma, "b": lambda: ctx.map_stats_finish(state, (Mx, My), "sigma", k=3.0, ref=ref)}),
        "finish_rank": (56 * n, {"a": lambda: hi[1].clone(), "b": lambda: ctx.map_stats_finish(state, (Mx, My), "rank", rank=2, ref=ref_rank)}),
        "peak": (4 * B * n + 8 * B, {"a": lambda: m.flatten(1).max(1), "b": lambda: ctx.map_peak(m, peak=peak, cell=cell)}),
        "peak_ref": (4 * B * n + 4 * n + 8 * B, {"a": lambda: (m - ref).flatten(1).max(1), "b": lambda: ctx.map_peak(m, ref, peak=peak, cell=cell)}),
    }
    out = {"cells": [Mx, My], "B": B}
    for case, (nbytes, fns) in cases.items():
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            r["b"].update(bytes=nbytes, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
        if "a" in r and "b" in r:
            r["a_over_b_rounds"] = [x / y for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"])]
            r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
        out[case] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a or b alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        out[name] = bench(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
