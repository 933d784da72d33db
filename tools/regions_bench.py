"""aefft_map_regions measurements, one process on one GPU; prints one JSON line.

8 maps of 240 x 135 cells (1920 x 1080 at 8 pixels a cell), 32 of 40 x 30 (640 x 480 at 16) and one of 1024 x 1024 (the largest the call takes);
at each a sparse map (a few blobs on a quiet background) and a random map at density 0.6, next to the percolation threshold, where components
are many and winding; hysteresis 0.5 / 0.75, 8-connectivity, 256 regions; per case microseconds per call of
  a   the route the call replaces, on the same GPU: map.cpu() -- the synchronisation the call avoids is part of it -- and then
      scipy.ndimage.label + find_objects per image where scipy is there, otherwise an iterated max_pool2d label propagation in torch (which
      waits for the device every eight sweeps to see whether it is done).  a gives labels and boxes only: no hysteresis, area or peak
  b   the library's call: six launches (constant: csrc/regions_kernels.hip), outputs and workspace reused
  d   for scale: the aefft_image_compare_map call that writes such a map (D = 1 images of cells x 8 or 16 pixels, MSE, no score)
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.

    python tools/regions_bench.py [--calls 30] [--warmup 10] [--rounds 3] [--variant b]
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

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

SHAPES = {"8x240x135": (8, 240, 135, 8), "32x40x30": (32, 40, 30, 16), "1x1024x1024": (1, 1024, 1024, 8)}      # B, Mx, My, pixels a cell for d
LAUNCHES = 6
LO, HI = 0.5, 0.75


def make_map(kind, B, Mx, My, rng):
    if kind == "random60":
        fg = rng.random((B, Mx, My)) < 0.6
    else:                                                                        # a few blobs: discs of 2..6 cells, about one per 1500 cells
        fg = np.zeros((B, Mx, My), bool)
        I, J = np.indices((Mx, My))
        for b in range(B):
            for _ in range(max(2, Mx * My // 1500)):
                ci, cj, r = rng.integers(0, Mx), rng.integers(0, My), rng.integers(2, 7)
                fg[b] |= (I - ci) ** 2 + (J - cj) ** 2 <= r * r
    return np.where(fg, 0.5 + 0.5 * rng.random((B, Mx, My)), 0.4 * rng.random((B, Mx, My))).astype(np.float32)


def host_route(m):
    h = m.cpu().numpy()                                                          # waits for the device
    out = []
    for b in range(h.shape[0]):
        lab, n = ndimage.label(h[b] >= LO, structure=np.ones((3, 3)))
        out.append((lab, ndimage.find_objects(lab), n))
    return out


def torch_route(t, m):
    """label propagation: every foreground cell starts as its index + 1 and takes the largest label of its 3 x 3 neighbourhood until nothing changes"""
    F = t.nn.functional
    fg = (m >= LO)[:, None]
    lab = (t.arange(1, m[0].numel() + 1, device=m.device, dtype=t.float32).view(1, 1, *m.shape[1:]) * fg).contiguous()
    while True:
        old = lab
        for _ in range(8):
            lab = F.max_pool2d(lab, 3, 1, 1) * fg
        if bool((lab == old).all()):                                             # waits for the device
            return lab


def bench(ctx, name, kind, calls, warmup, rounds, variant):
    t = ctx.torch
    B, Mx, My, px = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name) + len(kind))
    m = t.as_tensor(make_map(kind, B, Mx, My, rng), device=dev)
    labels, regions, count = ctx.map_regions(m, LO, HI)
    ctx.sync()
    out = {"cells": [Mx, My], "launches": LAUNCHES, "components_kept": count.cpu().tolist()[:8], "route_a": "scipy" if ndimage else "torch max_pool2d"}
    if ndimage:
        plain = ctx.map_regions(m, LO, LO)                                       # a plain threshold: what scipy labels
        ctx.sync()
        got = host_route(m)
        out["equals_scipy"] = all(np.array_equal(plain[0][b].cpu().numpy(), got[b][0]) for b in range(B))
    W, H = Mx * px, My * px
    img = t.as_tensor(rng.integers(0, 256, (B, H, W, 1), dtype=np.uint8), device=dev)
    img2 = t.as_tensor(rng.integers(0, 256, (B, H, W, 1), dtype=np.uint8), device=dev)
    o_m = ctx.empty(B, Mx, My)
    fns = {"a": (lambda: host_route(m)) if ndimage else (lambda: torch_route(t, m)),
           "b": lambda: ctx.map_regions(m, LO, HI, labels=labels, regions=regions, count=count),
           "d": lambda: ctx.image_compare_map(img, img2, (Mx, My), "mse", map=o_m, score=False)}
    fns = {k: v for k, v in fns.items() if not variant or k == variant}
    r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
    if "a" in r and "b" in r:
        r["a_over_b_rounds"] = [x / y for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"])]
        r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
    if "d" in r and "b" in r:
        r["b_over_d_rounds"] = [x / y for x, y in zip(r["b"]["us_rounds"], r["d"]["us_rounds"])]
    out.update(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b or d alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        for kind in ("sparse", "random60"):
            out[f"{name} {kind}"] = bench(ctx, name, kind, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
