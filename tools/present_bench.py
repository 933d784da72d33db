"""aefft_frames_resize_to_image and aefft_map_overlay_image measurements, one process on one GPU; prints one JSON line.

B = 32, D = 3; 256 x 256 -> 640 x 480 and 512 x 512 -> 1920 x 1080; LINEAR, and AREA where it does not enlarge (neither case: the workload's
direction enlarges); 8-bit and float frames; per case microseconds per call of
  a   what a torch caller can do without the op: frames.float() -> torch.nn.functional.interpolate(mode="bilinear", align_corners=False) on the
      transposed planes -> round().clamp(0, 255).to(uint8) -> permute(0, 2, 3, 1).contiguous()
  c   the three existing calls the new one equals bit for bit: frames_to_image -> image_resize_to_frames(8-bit) -> frames_to_image
  b   aefft_frames_resize_to_image
and for the overlay (a 32 x 32 map per image, smooth and per tile, alpha = 128)
  a   torch: quantise the map, interpolate it to the image's size, index the table, blend in float, round, store
  b   aefft_map_overlay_image
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For
b also its algorithmic bytes (include/aefft.h: what the profile id `image` accounts) over the median, as a share of the achievable rate
(6.3 TB/s), and the floor those bytes set at that rate; b == c is asserted, and how far a's values are from b's is reported.

    python tools/present_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--variant b]
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

SHAPES = {"256x256->640x480": (32, 3, 256, 256, 640, 480), "512x512->1920x1080": (32, 3, 512, 512, 1920, 1080)}      # B, D, Nx, Ny, W, H
MAP = 32                                                                        # map entries per axis
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s


def _rate(r, nbytes):
    rate = nbytes / (r["us_median"] * 1e-6)
    r.update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, D, Nx, Ny, W, H = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(len(name))
    f8 = t.as_tensor(rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8), device=dev)
    out = {}
    for frames, es in ((f8, 1), ((f8.float() * 1.25 - 20.0).contiguous(), 4)):      # (a float frame that spills over both ends of 0..255)
        o = ctx.empty(B, H, W, D, dtype=t.uint8)
        mid_img, mid_frm = ctx.empty(B, Ny, Nx, D, dtype=t.uint8), ctx.empty(B, D, W, H, dtype=t.uint8)

        def torch_way(frames=frames):
            r = F.interpolate(frames.float().transpose(2, 3), size=(H, W), mode="bilinear", align_corners=False)
            return r.round().clamp(0, 255).to(t.uint8).permute(0, 2, 3, 1).contiguous()

        def three_calls(frames=frames, o=o):
            ctx.frames_to_image(frames, out=mid_img)
            ctx.image_resize_to_frames(mid_img, (W, H), "linear", out=mid_frm)
            return ctx.frames_to_image(mid_frm, out=o)

        fns = {"a": torch_way, "c": three_calls, "b": lambda frames=frames, o=o: ctx.frames_resize_to_image(frames, (W, H), "linear", out=o)}
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            _rate(r["b"], B * D * (Nx * Ny * es + W * H))
        if "b" in r and "c" in r:
            r["b_faster_than_c_in_every_round"] = all(y < x for x, y in zip(r["c"]["us_rounds"], r["b"]["us_rounds"]))
            r["c_over_b"] = r["c"]["us_median"] / r["b"]["us_median"]
            same = t.equal(three_calls().clone(), ctx.frames_resize_to_image(frames, (W, H), "linear"))
            ctx.sync()
            assert same, "the fused call and the three-call composition differ"
        if "a" in r and "b" in r:
            r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
            d = (torch_way().float() - ctx.frames_resize_to_image(frames, (W, H), "linear").float()).abs()
            ctx.sync()
            r["torch_minus_op_max_abs"] = float(d.max())
        out[f"resize_linear_{'u8' if es == 1 else 'f32'}"] = r
    # the overlay
    img0 = t.as_tensor(rng.integers(0, 256, (B, H, W, D), dtype=np.uint8), device=dev)
    m = t.as_tensor(rng.uniform(0, 1, (B, MAP, MAP)).astype(np.float32), device=dev)
    lut = t.as_tensor(aefft.heat_lut(D), device=dev)
    for smooth in (True, False):
        img = img0.clone()

        def torch_overlay(img=img, smooth=smooth):
            k0 = (m * 255.0).round().clamp(0, 255)
            k = F.interpolate(k0.transpose(1, 2).unsqueeze(1), size=(H, W), **(dict(mode="bilinear", align_corners=False) if smooth else dict(mode="nearest")))
            col = lut[k.squeeze(1).round().long()]
            img.copy_(((col.float() + img.float()) * 0.5).round().to(t.uint8))
            return img

        fns = {"a": torch_overlay, "b": lambda img=img, smooth=smooth: ctx.map_overlay(m, img, lut, 0.0, 1.0, alpha=128, smooth=smooth)}
        fns = {k: v for k, v in fns.items() if not variant or k == variant}
        r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
        if "b" in r:
            _rate(r["b"], B * (4 * MAP * MAP + 2 * W * H * D) + 256 * D)
        if "a" in r and "b" in r:
            r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
        out[f"overlay_{'smooth' if smooth else 'tile'}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b or c alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        out[name] = bench(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
