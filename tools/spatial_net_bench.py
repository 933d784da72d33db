"""Spatial-mode training throughput on one GPU: (a) the resident spatial net (aefft_net_create_ex with AEFFT_NET_SPATIAL), step_grad +
step_apply, against (b) the same training through the public op calls -- aefft_pool_conv_spatial per encoder, aefft_conv_spatial and
aefft_pool_spatial per decoder, aefft_backprop_spatial per pair.  Prints one JSON line.

    python tools/spatial_net_bench.py [--steps 20] [--warmup 5] [--only net|ops] [--flags NORCORR,...]

--flags sets development switches (include/aefft.h AEFFT_F_*) for both forms: NORCORR keeps pair 0 of (a) off the region route, on the
back-convolution route that (b) takes (aefft_backprop_spatial does not know that its hidden layer is the pair's own convolution).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
aefft = importlib.import_module("autoencoder-fft_amd")

SHAPES = [dict(B=32, D=3, Nx=256, Ny=256), dict(B=16, D=3, Nx=640, Ny=480)]
MAPS, NK, SCALE, DEL0, ALPHA = [16, 32], 3, 2, 0.2, 0.9


def weights(rng, net):
    out = []
    for l, g in enumerate(net.dims):
        sc = 1.0 / NK
        c = rng.uniform(-sc, sc, (g["dM"], g["dD"], NK, NK)).astype(np.float32)
        f = rng.uniform(-sc, sc, (g["dD"], g["dM"], NK, NK)).astype(np.float32)
        b = rng.uniform(-1, 1, g["dM"]).astype(np.float32); p = rng.uniform(-1, 1, g["dD"]).astype(np.float32)
        net.set_pair(l, c, b, f, p)
        out.append((c, b, f, p))
    return out


def timed(ctx, fn, steps, warmup):
    st = ctx.torch_stream()
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def run_shape(ctx, sh, steps, warmup, only):
    B, D, Nx, Ny = sh["B"], sh["D"], sh["Nx"], sh["Ny"]
    rng = np.random.default_rng(0)
    x = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))).astype(np.float32))
    recon = ctx.empty(B, D, Nx, Ny)
    net = aefft.Net(ctx, D, Nx, Ny, MAPS, NK, SCALE, B, spatial=True)
    w = weights(rng, net)
    res = dict(shape=f"{B}x{D}x{Nx}x{Ny}", pairs=[D] + MAPS, kernel=f"{NK}x{NK}", scale=SCALE)
    if only in (None, "net"):
        def net_step():
            net.step_grad(x, recon)
            net.step_apply(DEL0, 0, 0, 1.0)
        ms = timed(ctx, net_step, steps, warmup)
        res["net_ms"], res["net_fps"] = ms, B * 1000.0 / ms
    net.close()
    if only in (None, "ops"):
        L, h, p_ = ctx.L, ctx.h, lambda t: C.c_void_p(t.data_ptr())
        dims, prs = [], []
        dD, nx, ny = D, Nx, Ny
        for l, (c, b, f, p) in enumerate(w):
            dM = MAPS[l]; nx //= SCALE; ny //= SCALE
            t = dict(c=ctx.dev(c), b=ctx.dev(b), f=ctx.dev(f), p=ctx.dev(p))
            for k in ("c", "b", "f", "p"):
                t["D" + k] = torch.zeros_like(t[k]); t["G" + k] = torch.zeros_like(t[k])
            t.update(pooled=ctx.empty(B, dD, nx, ny), hid=ctx.empty(B, dM, nx, ny), out=ctx.empty(B, dD, nx, ny),
                     up=ctx.empty(B, dD, nx * SCALE, ny * SCALE))
            dims.append((dD, dM, nx, ny)); prs.append(t)
            dD = dM

        def ops_step():
            src = x
            for (dD, dM, nx, ny), t in zip(dims, prs):
                ctx.check(L.aefft_pool_conv_spatial(h, p_(src), p_(t["pooled"]), p_(t["hid"]), p_(t["c"]), p_(t["b"]), B, dD, dM, nx, ny, SCALE, NK, NK, 0))
                src = t["hid"]
            for l in range(len(prs) - 1, -1, -1):
                (dD, dM, nx, ny), t = dims[l], prs[l]
                ctx.check(L.aefft_conv_spatial(h, p_(src), p_(t["out"]), p_(t["f"]), p_(t["p"]), B, dM, dD, nx, ny, NK, NK, 0))
                ctx.check(L.aefft_pool_spatial(h, p_(t["out"]), p_(t["up"]), B * dD, nx, ny, nx * SCALE, ny * SCALE, -SCALE))
                src = t["up"]          # the next decoder's input; pair 0's is the reconstruction
            for (dD, dM, nx, ny), t in zip(dims, prs):
                ctx.check(L.aefft_backprop_spatial(h, p_(t["pooled"]), p_(t["out"]), p_(t["hid"]), p_(t["c"]), p_(t["b"]), p_(t["f"]), p_(t["p"]),
                                                   p_(t["Dc"]), p_(t["Db"]), p_(t["Df"]), p_(t["Dp"]), p_(t["Gc"]), p_(t["Gb"]), p_(t["Gf"]), p_(t["Gp"]),
                                                   B, dD, dM, nx, ny, NK, NK, DEL0, ALPHA, 0, 0))
        ms = timed(ctx, ops_step, steps, warmup)
        res["ops_ms"], res["ops_fps"] = ms, B * 1000.0 / ms
    if "net_ms" in res and "ops_ms" in res:
        res["speedup"] = res["ops_ms"] / res["net_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["net", "ops"], default=None)
    ap.add_argument("--flags", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = aefft.Context(0)
    ctx.set_flags(*[f for f in a.flags.split(",") if f])
    out = dict(bench="spatial_net", steps=a.steps, warmup=a.warmup, flags=a.flags, results=[run_shape(ctx, sh, a.steps, a.warmup, a.only) for sh in SHAPES])
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
