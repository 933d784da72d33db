"""aefft_raw_to_image measurements, one process on one GPU; prints one JSON line.

B = 8 images of 2448 x 2048 (a 5-megapixel GigE sensor) and of 4096 x 3000 (12 megapixels); RGGB; containers U8 and PACKED 12 (black 64 of 4095,
gains (1.9, 1, 1.4)); both demosaic methods; with and without the sRGB table; BGR out.  Per case microseconds per call of
  a   a torch restatement on the same GPU: unpack (PACKED), black level and gains in float, a BILINEAR demosaic as three conv2d over the
      colour-masked mosaic (reflect padding), round / clamp / uint8, the table as a gather -- whatever the case's method is, torch does BILINEAR
  b   aefft_raw_to_image
  c   aefft_raw_to_image + aefft_image_resize_to_frames (AREA, to 512 x 512, 8-bit frames)
  d   for scale: aefft_image_resize_to_frames alone on a ready BGR image
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also its bytes (source rows + image, what `image` accounts) over the median as a share of the achievable rate (6.3 TB/s) and the floor those
bytes set; c - d is what the intermediate image costs a pipeline that has no fused raw -> frames call.  How far a's pixels are from b's is
reported, not asserted (a float BILINEAR against the integer definition).

    python tools/bayer_bench.py [--calls 20] [--warmup 10] [--rounds 3] [--variant b]
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

SHAPES = {"8x2448x2048": (8, 2448, 2048), "8x4096x3000": (8, 4096, 3000)}       # B, W, H
FRAME = (512, 512)
HBM_ACHIEVABLE = 6.3e12                                                         # bytes / s
CONTAINERS = {"u8": dict(bits=8, packed=False, black=4, white=255), "packed12": dict(bits=12, packed=True, black=64, white=4095)}
GAINS = (1.9, 1.0, 1.4)


def bench(ctx, name, cont, calls, warmup, rounds, variant):
    t = ctx.torch
    F = t.nn.functional
    B, W, H = SHAPES[name]
    kw = CONTAINERS[cont]
    bits = kw["bits"]
    dev = f"cuda:{ctx.device}"
    live = W if cont == "u8" else W * bits // 8
    raw = t.as_tensor(np.random.default_rng(W + bits).integers(0, 256, (B, H, live), dtype=np.uint8), device=dev)
    lut = t.as_tensor(aefft.srgb_lut(), device=dev)
    # the colour masks of RGGB and the BILINEAR kernels: (R or B plane) * K_rb and (G plane) * K_g fill the missing sites
    yy, xx = t.meshgrid(t.arange(H, device=dev), t.arange(W, device=dev), indexing="ij")
    mask = t.stack([(yy % 2 == 0) & (xx % 2 == 0), (yy + xx) % 2 == 1, (yy % 2 == 1) & (xx % 2 == 1)]).float().unsqueeze(0)      # [1][3][H][W]: R, G, B
    k_rb = t.tensor([[0.25, 0.5, 0.25], [0.5, 1.0, 0.5], [0.25, 0.5, 0.25]], device=dev)
    k_g = t.tensor([[0.0, 0.25, 0.0], [0.25, 1.0, 0.25], [0.0, 0.25, 0.0]], device=dev)
    weight = t.stack([k_rb, k_g, k_rb]).unsqueeze(1)                                                                                 # depthwise [3][1][3][3]
    gain = t.tensor(GAINS, device=dev).view(1, 3, 1, 1) * (255.0 / (kw["white"] - kw["black"]))
    lutf = lut.long()

    def torch_bgr(with_lut):
        if cont == "u8":
            s = raw.float()
        else:
            q = raw.view(B, H, W // 2, 3).int()
            s = t.stack([q[..., 0] | (q[..., 1] & 15) << 8, q[..., 1] >> 4 | q[..., 2] << 4], -1).view(B, H, W).float()
        u = ((s - kw["black"]).clamp_(min=0).unsqueeze(1) * mask * gain).clamp_(max=255.0)
        rgb = F.conv2d(F.pad(u, (1, 1, 1, 1), mode="reflect"), weight, groups=3)
        if with_lut:
            return lutf[(rgb * 16.0).round_().clamp_(0, 4080).long()].to(t.uint8).flip(1).permute(0, 2, 3, 1).contiguous()
        return rgb.round_().clamp_(0, 255).to(t.uint8).flip(1).permute(0, 2, 3, 1).contiguous()

    src_bytes = B * H * live
    out = {}
    for method in ("bilinear", "mhc"):
        for with_lut in (False, True):
            args = dict(method=method, gains=GAINS, lut=lut if with_lut else None, **kw)
            bgr = ctx.raw_to_image(raw, "rggb", **args)
            mid = t.empty_like(bgr)
            o = ctx.empty(B, 3, *FRAME, dtype=t.uint8)
            fns = {"a": lambda: torch_bgr(with_lut),
                   "b": lambda: ctx.raw_to_image(raw, "rggb", out=mid, **args),
                   "c": lambda: ctx.image_resize_to_frames(ctx.raw_to_image(raw, "rggb", out=mid, **args), FRAME, "area", out=o),
                   "d": lambda: ctx.image_resize_to_frames(bgr, FRAME, "area", out=o)}
            fns = {k: v for k, v in fns.items() if not variant or k == variant}
            r = {k: stats(v) for k, v in alternate(ctx, fns, calls, warmup, rounds).items()}
            if "b" in r:
                nbytes = src_bytes + B * H * W * 3 + (4096 if with_lut else 0)
                rate = nbytes / (r["b"]["us_median"] * 1e-6)
                r["b"].update(bytes=nbytes, TBps=rate / 1e12, share_of_achievable=rate / HBM_ACHIEVABLE, floor_us=1e6 * nbytes / HBM_ACHIEVABLE)
                if "a" in r:
                    r["a_over_b"] = r["a"]["us_median"] / r["b"]["us_median"]
                if "c" in r and "d" in r:
                    r["c_over_d"] = r["c"]["us_median"] / r["d"]["us_median"]
                    r["c_minus_d_us"] = r["c"]["us_median"] - r["d"]["us_median"]
            if method == "bilinear" and (not variant or variant == "a"):
                d = (torch_bgr(with_lut)[:, 2:-2, 2:-2].int() - bgr[:, 2:-2, 2:-2].int()).abs()
                ctx.sync()
                r["torch_minus_op_max_abs_interior"] = int(d.max())
                r["torch_minus_op_differing_share"] = float((d > 0).float().mean())
            out[f"{method}{'+lut' if with_lut else ''}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a, b, c or d alone")
    ap.add_argument("--shape", default="", help="one of %s alone" % ", ".join(SHAPES))
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in SHAPES:
        if a.shape and name != a.shape:
            continue
        for cont in CONTAINERS:
            out[f"{cont} {name}"] = bench(ctx, name, cont, a.calls, a.warmup, a.rounds, a.variant)
            print(json.dumps({f"{cont} {name}": out[f"{cont} {name}"]}), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
