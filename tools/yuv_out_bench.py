"""aefft_image_to_yuv / aefft_frames_resize_to_yuv measurements, one process on one GPU; prints one JSON line.

Order BGR, BT601, 8-bit frames; NV12 and YUYV; 32 frames of 3 x 256^2 -> 640 x 480 and 8 of 3 x 512^2 -> 1920 x 1080 (LINEAR: both enlarge),
32 of 3 x 1024^2 -> 640 x 480 (LINEAR and AREA: the one case in which both axes reduce); per case microseconds per call of
  a   what a caller of the library without the calls does: aefft_frames_resize_to_image, then torch ops to the planes (float(), a matmul with the
      float matrix, avg_pool2d for the chroma, round().clamp().to(uint8), the interleave)
  b   aefft_frames_resize_to_image + aefft_image_to_yuv
  c   aefft_frames_resize_to_yuv, the fused call
  d   for scale: aefft_frames_resize_to_image alone
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For c
also its bytes (frames + plane samples, what `image` accounts) over the median as a share of the achievable rate (6.3 TB/s), and how far a's
planes are from the fused call's (a float matrix against the Q20 table: reported, not asserted).

    python tools/yuv_out_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant c]
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

# name -> (B, Nx, Ny, W, H, modes)
SHAPES = {"32x256x256->640x480": (32, 256, 256, 640, 480, ("linear",)), "8x512x512->1920x1080": (8, 512, 512, 1920, 1080, ("linear",)),
          "32x1024x1024->640x480": (32, 1024, 1024, 640, 480, ("linear", "area"))}      # (AREA needs W <= Nx and H <= Ny: 512^2 -> 640 x 480 enlarges x)
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
# BT.601 limited range: rows Y, U, V over the channels as stored (B, G, R)
KR, KB = 0.299, 0.114
KG = 1.0 - KR - KB
SY, SC = 219.0 / 255.0, 224.0 / 255.0
M601 = [[KB * SY, KG * SY, KR * SY], [SC / 2, -KG * SC / (2 * (1 - KB)), -KR * SC / (2 * (1 - KB))], [-KB * SC / (2 * (1 - KR)), -KG * SC / (2 * (1 - KR)), SC / 2]]


def bench(ctx, name, fmt, calls, warmup, rounds, variant):
    t = ctx.torch
    B, Nx, Ny, W, H, modes = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    frames = t.as_tensor(np.random.default_rng(len(name) + len(fmt)).integers(0, 256, (B, 3, Nx, Ny), dtype=np.uint8), device=dev)
    M = t.tensor(M601, dtype=t.float32, device=dev)
    off = t.tensor([16.0, 128.0, 128.0], dtype=t.float32, device=dev)
    img = ctx.empty(B, H, W, 3, dtype=t.uint8)
    q8 = lambda v: v.round().clamp(0, 255).to(t.uint8)

    def torch_planes(image):
        yuv = image.float() @ M.T                                                # [B][H][W][3]: Y, U, V without their offsets
        y = q8(yuv[..., 0] + off[0])
        if fmt == "nv12":
            c = t.nn.functional.avg_pool2d(yuv[..., 1:].permute(0, 3, 1, 2), 2)  # [B][2][H/2][W/2]
            return y, q8(c + 128.0).permute(0, 2, 3, 1).contiguous()
        c = t.nn.functional.avg_pool2d(yuv[..., 1:].permute(0, 3, 1, 2), (1, 2))  # [B][2][H][W/2]
        u, v = q8(c[:, 0] + 128.0), q8(c[:, 1] + 128.0)
        return (t.stack([y[..., 0::2], u, y[..., 1::2], v], -1),)

    out = {}
    for mode in modes:
        planes = ctx.frames_resize_to_yuv(frames, (W, H), fmt, mode=mode)
        two = tuple(t.empty_like(p) for p in planes)
        ref = torch_planes(ctx.frames_resize_to_image(frames, (W, H), mode, out=img))
        ctx.sync()
        fns = {"a": lambda mode=mode: torch_planes(ctx.frames_resize_to_image(frames, (W, H), mode, out=img)),
               "b": lambda mode=mode: ctx.image_to_yuv(ctx.frames_resize_to_image(frames, (W, H), mode, out=img), fmt, out=two),
               "c": lambda mode=mode: ctx.frames_resize_to_yuv(frames, (W, H), fmt, mode=mode, out=planes),
               "d": lambda mode=mode: ctx.frames_resize_to_image(frames, (W, H), mode, out=img)}
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        r["torch_minus_op_max_abs"] = max(int((a.int() - p.int()).abs().max()) for a, p in zip(ref, planes))
        if "b" in r:
            ctx.sync()
            r["two_calls_equal_fused"] = all(bool(t.equal(a, p)) for a, p in zip(two, planes))
        if "c" in r:
            nbytes = B * 3 * Nx * Ny + (B * (W * H + 2 * (W // 2) * (H // 2)) if fmt == "nv12" else B * 2 * W * H)
            rate = nbytes / (r["c"]["us_median"] * 1e-6)
            r["c"].update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
            for k in ("a", "b", "d"):
                if k in r:
                    r[f"c_faster_than_{k}_in_every_round"] = all(y < x for x, y in zip(r[k]["us_rounds"], r["c"]["us_rounds"]))
            if "a" in r:
                r["a_over_c"] = r["a"]["us_median"] / r["c"]["us_median"]
            if "b" in r:
                r["b_over_c"] = r["b"]["us_median"] / r["c"]["us_median"]
            if "d" in r:
                r["c_over_d"] = r["c"]["us_median"] / r["d"]["us_median"]
        out[mode] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b, c or d alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        for fmt in ("nv12", "yuyv"):
            out[f"{fmt} {name}"] = bench(ctx, name, fmt, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
