"""aefft_frames_degrade measurements, one process on one GPU; prints one JSON line.

B = 32, D = 3 at 256 x 256 and 512 x 512; noise only (sigma = 25) 8-bit -> 8-bit, blur = 2 + noise 8-bit -> 8-bit, noise only 8-bit -> float;
per case microseconds per call of
  a   what a torch caller does today on the same GPU: frames.float() -> (blurred: a depthwise conv2d with the same binomial kernel on a
      replicate-padded input) -> + sigma * randn_like -> (8-bit out: round().clamp(0, 255).to(uint8))
  b   aefft_frames_degrade
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also its algorithmic bytes (what the profile id `image` accounts) over the median as a share of the achievable rate (6.3 TB/s), and b as a
share of the training step it feeds: step_grad on 8-bit frames + step_apply of the 4-pair 8/16/32/64-map, 5 x 5, pooling 2 net at that size,
timed the same way in the same process.  a and b are different generators: only their times are compared.

    python tools/degrade_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant b]
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
from tools.image_bench import alternate, stats  # noqa: E402

SHAPES = {"256x256": (32, 3, 256, 256), "512x512": (32, 3, 512, 512)}           # B, D, Nx, Ny
CASES = {"noise_u8_u8": (0, False), "blur2_noise_u8_u8": (2, False), "noise_u8_f32": (0, True)}      # blur, float out
SIGMA = 25.0
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s


def step_fn(ctx, B, D, N):
    t = ctx.torch
    maps, Nk = [8, 16, 32, 64], 5
    net = aefft.Net(ctx, D, N, N, maps, Nk, 2, batch=B)
    rng = np.random.default_rng(1)
    dD = D
    for l, dM in enumerate(maps):
        net.set_pair(l, 0.05 * rng.uniform(-1, 1, (dM, dD, Nk, Nk)), 0.05 * rng.uniform(-1, 1, dM), 0.05 * rng.uniform(-1, 1, (dD, dM, Nk, Nk)),
                     0.05 * rng.uniform(-1, 1, dD))
        dD = dM
    frames = t.as_tensor(rng.integers(0, 256, (B, D, N, N), dtype=np.uint8), device=f"cuda:{ctx.device}")
    recon = ctx.empty(B, D, N, N)

    def step():
        net.step_grad(frames, recon); net.step_apply(1e-6, 0, 0, 1.0, None)
    return net, step


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, D, Nx, Ny = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    f8 = t.as_tensor(np.random.default_rng(len(name)).integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8), device=dev)
    w = t.tensor([math.comb(4, k) for k in range(5)], dtype=t.float32, device=dev) / 16.0
    kern = (w[:, None] * w[None, :]).expand(D, 1, 5, 5).contiguous()
    out = {}
    for case, (blur, f32_out) in CASES.items():
        o = ctx.empty(B, D, Nx, Ny, dtype=t.float32 if f32_out else t.uint8)
        calls_made = [0]

        def torch_way(blur=blur, f32_out=f32_out):
            x = f8.float()
            if blur:
                x = F.conv2d(F.pad(x, (blur,) * 4, mode="replicate"), kern, groups=D)
            x = x + SIGMA * t.randn_like(x)
            return x if f32_out else x.round().clamp(0, 255).to(t.uint8)

        def op(blur=blur, o=o):
            calls_made[0] += 1
            return ctx.frames_degrade(f8, blur, SIGMA, 0.0, 2024, calls_made[0] * B, out=o)

        fns = {k: v for k, v in {"a": torch_way, "b": op}.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            nbytes = B * D * Nx * Ny * (1 + (4 if f32_out else 1))
            rate = nbytes / (r["b"]["us_median"] * 1e-6)
            r["b"].update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
        if "a" in r and "b" in r:
            r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
            r["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
        out[case] = r
    net, step = step_fn(ctx, B, D, Nx)
    s = stats(alternate(ctx, {"step": step}, calls, warmup, rounds)["step"])
    net.close()
    out["step_grad_u8_plus_apply"] = s
    for case in CASES:
        if "b" in out[case]:
            out[case]["b_share_of_step"] = out[case]["b"]["us_median"] / s["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
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
