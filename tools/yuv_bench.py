"""aefft_yuv_to_image / aefft_yuv_resize_to_frames measurements, one process on one GPU; prints one JSON line.

B = 32, order BGR, BT601, 8-bit frames; NV12 and YUYV; 640 x 480 -> 256 x 256 and 1920 x 1080 -> 512 x 512; both modes; per case microseconds per call of
  a   what a torch caller of the library without the calls does: torch ops to a BGR uint8 image (float copies of the planes, the chroma
      upsampled by repeat_interleave, a matmul with the float matrix, round, clamp, to(uint8)), then aefft_image_resize_to_frames
  b   aefft_yuv_to_image + aefft_image_resize_to_frames
  c   aefft_yuv_resize_to_frames, the fused call
  d   for scale: aefft_image_resize_to_frames alone on a ready BGR image
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For c
also its bytes (source samples + frames, what `image` accounts) over the median as a share of the achievable rate (6.3 TB/s), and how far a's
pixels are from yuv_to_image's (a float matrix against the Q20 table: reported, not asserted).

    python tools/yuv_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant c]
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

SHAPES = {"640x480->256x256": (32, 640, 480, 256, 256), "1920x1080->512x512": (32, 1920, 1080, 512, 512)}      # B, W, H, Nx, Ny
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
# BT.601 limited range, rows B, G, R over (Y - 16, U - 128, V - 128)
KR, KB = 0.299, 0.114
KG = 1.0 - KR - KB
SY, SC = 255.0 / 219.0, 255.0 / 224.0
M601 = [[SY, 2 * (1 - KB) * SC, 0.0], [SY, -2 * (1 - KB) * KB / KG * SC, -2 * (1 - KR) * KR / KG * SC], [SY, 0.0, 2 * (1 - KR) * SC]]


def bench(ctx, name, fmt, calls, warmup, rounds, variant):
    t = ctx.torch
    B, W, H, Nx, Ny = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name) + len(fmt))
    rand = lambda *s: t.as_tensor(rng.integers(0, 256, s, dtype=np.uint8), device=dev)
    planes = (rand(B, H, W), rand(B, H // 2, W // 2, 2)) if fmt == "nv12" else (rand(B, H, W // 2, 4),)
    M = t.tensor(M601, dtype=t.float32, device=dev)
    off = t.tensor([16.0, 128.0, 128.0], dtype=t.float32, device=dev)

    def torch_bgr():
        if fmt == "nv12":
            y, c = planes[0].float(), planes[1].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
            yuv = t.cat([y.unsqueeze(-1), c], -1)
        else:
            q = planes[0].float()
            y = q[..., 0::2].reshape(B, H, W)
            yuv = t.stack([y, q[..., 1].repeat_interleave(2, 2), q[..., 3].repeat_interleave(2, 2)], -1)
        return ((yuv - off) @ M.T).round().clamp(0, 255).to(t.uint8)

    bgr = ctx.yuv_to_image(planes, fmt)
    mid = t.empty_like(bgr)
    src_bytes = B * (W * H + 2 * (W // 2) * (H // 2)) if fmt == "nv12" else B * 2 * W * H
    out = {}
    d = (torch_bgr().int() - bgr.int()).abs()
    ctx.sync()
    out["torch_minus_op_max_abs"] = int(d.max())
    for mode in ("linear", "area"):
        o = ctx.empty(B, 3, Nx, Ny, dtype=t.uint8)
        fns = {"a": lambda mode=mode, o=o: ctx.image_resize_to_frames(torch_bgr(), (Nx, Ny), mode, out=o),
               "b": lambda mode=mode, o=o: ctx.image_resize_to_frames(ctx.yuv_to_image(planes, fmt, out=mid), (Nx, Ny), mode, out=o),
               "c": lambda mode=mode, o=o: ctx.yuv_resize_to_frames(planes, fmt, (Nx, Ny), mode=mode, out=o),
               "d": lambda mode=mode, o=o: ctx.image_resize_to_frames(bgr, (Nx, Ny), mode, out=o)}
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "c" in r:
            nbytes = src_bytes + B * 3 * Nx * Ny
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
