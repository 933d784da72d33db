"""Image-boundary measurements, one process on one GPU; prints one JSON line.

Shapes 32 x 3 x 512 x 512 and 32 x 3 x 640 x 480, both directions, 8-bit and float frames; per case microseconds per call of
  a   what a torch host can do without the op: img.permute(0, 3, 2, 1).contiguous() (+ .float()); packing: (round / clamp / uint8 for float
      frames, then) frames.permute(0, 3, 2, 1).contiguous()
  b   aefft_image_to_frames / aefft_frames_to_image
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For
b also its algorithmic bytes B D Nx Ny (1 + element size) over the time, as a share of the HBM peak (8 TB/s) and of the achievable rate
(6.3 TB/s), and the floor those bytes set at the achievable rate.  Then `infer` from images -- unpack + aefft_net_infer (8-bit in and
out) + pack -- against `infer` on planar pixels for cfg3-P2's net at both shapes, and numpy's time for the same transposition on the host.

    python tools/image_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--no-infer] [--no-numpy] [--variant b] [--long]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/image_bench.py --variant b --no-infer --no-numpy --rounds 1
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
aefft = importlib.import_module("autoencoder-fft_amd")
from tools.sizes_bench import timed  # noqa: E402

SHAPES = {"512x512": (32, 3, 512, 512), "640x480": (32, 3, 640, 480)}      # B, D, Nx, Ny
LONG = {"512x512_B128": (128, 3, 512, 512)}                                  # --long: four resident rounds of workgroups instead of one (ops only)
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12                                    # bytes / s
NET = dict(maps=[8, 16, 32, 64], Nk=5, s=2)                                  # cfg3-P2


def alternate(ctx, fns, calls, warmup, rounds):
    """{name: [ms per call of each round]}: every variant warmed up, then the variants alternated round by round"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ctx.sync()
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(timed(ctx, fn, calls))
    return res


def stats(ms):
    us = [1e3 * v for v in ms]
    return {"us_median": float(np.median(us)), "us_min": min(us), "us_max": max(us), "us_rounds": us}


def bench_ops(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    B, D, Nx, Ny = {**SHAPES, **LONG}[name]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name))
    img = t.as_tensor(rng.integers(0, 256, (B, Ny, Nx, D), dtype=np.uint8), device=dev)
    f8 = ctx.image_to_frames(img)
    f32 = (f8.float() * 1.25 - 20.0).contiguous()                            # (a float image that spills over both ends of 0..255)
    o8, o32, oimg = t.empty_like(f8), t.empty_like(f32), t.empty_like(img)
    cases = {
        "unpack_u8": (1, {"a": lambda: img.permute(0, 3, 2, 1).contiguous(), "b": lambda: ctx.image_to_frames(img, out=o8)}),
        "unpack_f32": (4, {"a": lambda: img.permute(0, 3, 2, 1).contiguous().float(), "b": lambda: ctx.image_to_frames(img, out=o32)}),
        "pack_u8": (1, {"a": lambda: f8.permute(0, 3, 2, 1).contiguous(), "b": lambda: ctx.frames_to_image(f8, out=oimg)}),
        "pack_f32": (4, {"a": lambda: f32.round().clamp(0, 255).to(t.uint8).permute(0, 3, 2, 1).contiguous(), "b": lambda: ctx.frames_to_image(f32, out=oimg)}),
    }
    out = {}
    for case, (es, fns) in cases.items():
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            nbytes = B * D * Nx * Ny * (1 + es)
            rate = nbytes / (r["b"]["us_median"] * 1e-6)
            r["b"].update(bytes=nbytes, TBps=rate / 1e12, share_of_peak=rate / HBM_PEAK, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
        if "a" in r and "b" in r:
            r["b_not_slower_in_any_round"] = all(y <= x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
        out[case] = r
    return out


def bench_infer(ctx, name, calls, warmup, rounds):
    t = ctx.torch
    B, D, Nx, Ny = SHAPES[name]
    smooth = name != "512x512"
    rng = np.random.default_rng(7)
    net = aefft.Net(ctx, D, Nx, Ny, NET["maps"], NET["Nk"], NET["s"], batch=B, **(dict(smooth_sizes=True, operator_form=True) if smooth else {}))
    dD = D
    for l, dM in enumerate(NET["maps"]):
        net.set_pair(l, rng.uniform(-1, 1, (dM, dD, 5, 5)), rng.uniform(-1, 1, dM), rng.uniform(-1, 1, (dD, dM, 5, 5)), rng.uniform(-1, 1, dD))
        dD = dM
    img = t.as_tensor(rng.integers(0, 256, (B, Ny, Nx, D), dtype=np.uint8), device=f"cuda:{ctx.device}")
    f8 = ctx.image_to_frames(img)
    o8, oimg = t.empty_like(f8), t.empty_like(img)

    def from_images():
        ctx.image_to_frames(img, out=f8)
        net.infer(f8, o8)
        ctx.frames_to_image(o8, out=oimg)

    r = alternate(ctx, {"planar": lambda: net.infer(f8, o8), "images": from_images}, calls, warmup, rounds)
    net.close()
    out = {k: stats(v) for k, v in r.items()}
    out["overhead_us"] = out["images"]["us_median"] - out["planar"]["us_median"]
    return out


def bench_numpy(name, reps=3):
    """seconds numpy takes for one batch's transposition on the host, both directions (best of reps)"""
    B, D, Nx, Ny = SHAPES[name]
    px = np.random.default_rng(0).integers(0, 256, (B, Ny, Nx, D), dtype=np.uint8)
    best = {"unpack_ms": 1e30, "pack_ms": 1e30}
    for _ in range(reps):
        t0 = time.perf_counter(); fr = np.ascontiguousarray(px.transpose(0, 3, 2, 1)); t1 = time.perf_counter()
        back = np.ascontiguousarray(fr.transpose(0, 3, 2, 1)); t2 = time.perf_counter()
        best = {"unpack_ms": min(best["unpack_ms"], 1e3 * (t1 - t0)), "pack_ms": min(best["pack_ms"], 1e3 * (t2 - t1))}
    assert np.array_equal(back, px)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a or b alone")
    ap.add_argument("--no-infer", action="store_true")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--long", action="store_true", help="also the ops at B = 128: the rate with four rounds of workgroups")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        out[name] = {"ops": bench_ops(ctx, name, a.calls, a.warmup, a.rounds, a.variant)}
        if not a.no_infer:
            out[name]["infer"] = bench_infer(ctx, name, a.calls, a.warmup, a.rounds)
        if not a.no_numpy:
            out[name]["numpy"] = bench_numpy(name)
    for name in (LONG if a.long else {}):
        out[name] = {"ops": bench_ops(ctx, name, a.calls, a.warmup, a.rounds, a.variant)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
