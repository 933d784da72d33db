"""aefft_image_resize_to_frames measurements, one process on one GPU; prints one JSON line.

B = 32, D = 3; 640 x 480 -> 256 x 256 and 1920 x 1080 -> 512 x 512; both modes; 8-bit and float frames; per case microseconds per call of
  a   what a torch caller can do without the op: img.permute(0, 3, 1, 2).float() -> torch.nn.functional.interpolate (mode="bilinear",
      align_corners=False against LINEAR; mode="area" against AREA) -> the transposition to [B][D][Nx][Ny] (.transpose(2, 3).contiguous()),
      and round().clamp(0, 255).to(uint8) for 8-bit frames
  b   aefft_image_resize_to_frames
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For
b also its algorithmic bytes B D (W H + Nx Ny sizeof(frame element)) over the median, as a share of the achievable rate (6.3 TB/s), and the
floor those bytes set at that rate; and how far a's values are from b's (they are different filters in float: reported, not asserted).

    python tools/resize_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant b]
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

SHAPES = {"640x480->256x256": (32, 3, 640, 480, 256, 256), "1920x1080->512x512": (32, 3, 1920, 1080, 512, 512)}      # B, D, W, H, Nx, Ny
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
TORCH_MODE = {"linear": dict(mode="bilinear", align_corners=False), "area": dict(mode="area")}


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, D, W, H, Nx, Ny = SHAPES[name]
    img = t.as_tensor(np.random.default_rng(len(name)).integers(0, 256, (B, H, W, D), dtype=np.uint8), device=f"cuda:{ctx.device}")
    out = {}
    for mode in ("linear", "area"):
        for dtype, es in ((t.uint8, 1), (t.float32, 4)):
            o = ctx.empty(B, D, Nx, Ny, dtype=dtype)

            def torch_way(mode=mode, dtype=dtype):
                r = F.interpolate(img.permute(0, 3, 1, 2).float(), size=(Ny, Nx), **TORCH_MODE[mode]).transpose(2, 3)
                return r.round().clamp(0, 255).to(t.uint8).contiguous() if dtype == t.uint8 else r.contiguous()

            fns = {"a": torch_way, "b": lambda mode=mode, o=o: ctx.image_resize_to_frames(img, (Nx, Ny), mode, out=o)}
            fns = {k: v for k, v in fns.items() if not variant or k == variant}
            r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
            if "b" in r:
                nbytes = B * D * (W * H + Nx * Ny * es)
                rate = nbytes / (r["b"]["us_median"] * 1e-6)
                r["b"].update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
            if "a" in r and "b" in r:
                r["b_faster_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
                r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
                d = (torch_way().float() - ctx.image_resize_to_frames(img, (Nx, Ny), mode, dtype=dtype).float()).abs()
                ctx.sync()
                r["torch_minus_op_max_abs"] = float(d.max())
            out[f"{mode}_{'u8' if es == 1 else 'f32'}"] = r
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
