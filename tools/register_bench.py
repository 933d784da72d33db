"""aefft_frames_register measurements, one process on one GPU; prints one JSON line.

32 frames of 3 x 256 x 256 and 8 of 3 x 512 x 512, 8-bit, against one stored reference, HANN, cutoff 0.5, with the affines; per shape microseconds
per call of
  a   a torch route on the same GPU, nothing pulled to the host: channel sum and window (the window tensors made once), torch.fft.rfft2, the
      cross-power with the stored reference spectrum normalised by its modulus (the kept-bin mask made once), torch.fft.irfft2, argmax.  a stops
      at the integer peak: it has no centroid and writes no affine, so it does LESS than b
  b   the library's call through Context.frames_register (which takes its workspace and outputs from torch's caching allocator on every call)
alternated in the process: --rounds rounds of --calls calls each between events on the library's stream, after --warmup calls of each.  For b
also the share of the two transforms, from the library's profiler over --calls further calls (the profiler's events serialise the launches: the
share is of the profiled sum, not of the time above), and whether a's integer peak equals b's cell.

    python tools/register_bench.py [--calls 30] [--warmup 10] [--rounds 3] [--variant b]
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

SHAPES = {"32x3x256x256": (32, 3, 256, 256), "8x3x512x512": (8, 3, 512, 512)}        # B, D, Nx, Ny
CUTOFF = 0.5
TRANSFORM_IDS = ("r2c_rows", "r2c_cols", "c2r_cols", "c2r_rows")


def smooth_frames(rng, B, D, Nx, Ny):
    """a low-passed texture and B circularly shifted copies of it, 8-bit"""
    fx, fy = np.fft.fftfreq(Nx)[:, None], np.fft.fftfreq(Ny)[None, :]
    H = np.exp(-(fx * fx + fy * fy) / (2 * 0.08 ** 2))
    tex = np.stack([np.fft.ifft2(np.fft.fft2(rng.standard_normal((Nx, Ny))) * H).real for _ in range(D)])
    ref = np.clip(np.rint(128 + 48 * tex / tex.std()), 0, 255).astype(np.uint8)
    shifts = rng.integers(-20, 21, (B, 2))
    return ref[None], np.stack([np.roll(ref, tuple(s), (1, 2)) for s in shifts])


def bench(ctx, name, calls, warmup, rounds, variant):
    t = ctx.torch
    B, D, Nx, Ny = SHAPES[name]
    dev = f"cuda:{ctx.device}"
    ref_np, frames_np = smooth_frames(np.random.default_rng(len(name)), B, D, Nx, Ny)
    frames, ref_frames = t.as_tensor(frames_np, device=dev), t.as_tensor(ref_np, device=dev)
    ref = ctx.frames_register_ref(ref_frames, "hann")
    # the torch route's constants, made once
    win = (t.hann_window(Nx, periodic=True, device=dev)[:, None] * t.hann_window(Ny, periodic=True, device=dev)[None, :]).contiguous()
    u = t.minimum(t.arange(Nx, device=dev), Nx - t.arange(Nx, device=dev))[:, None]
    v = t.arange(Ny // 2 + 1, device=dev)[None, :]
    mask = ((2 * u <= CUTOFF * Nx) & (2 * v <= CUTOFF * Ny) & ~((u <= 1) & (v <= 1))).float()
    Gref = t.fft.rfft2(ref_frames.float().sum(1) * win).conj() * mask

    def torch_route():
        R = t.fft.rfft2(frames.float().sum(1) * win) * Gref
        s = t.fft.irfft2(R / R.abs().clamp_min(1e-30), s=(Nx, Ny))
        return s.flatten(1).argmax(1)

    fns = {"a": torch_route, "b": lambda: ctx.frames_register(frames, ref, cutoff=CUTOFF, affine=True)}
    fns = {k: f for k, f in fns.items() if not variant or k == variant}
    r = {k: stats(ms) for k, ms in alternate(ctx, fns, calls, warmup, rounds).items()}
    res = {"B": B, "D": D, "size": [Nx, Ny], **r}
    if "a" in r and "b" in r:
        res["a_over_b_rounds"] = [x / y for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"])]
        res["b_faster_than_a_in_every_round"] = all(y < x for x, y in zip(r["a"]["us_rounds"], r["b"]["us_rounds"]))
        cells = fns["b"]()[0].cpu().numpy().view(aefft.SHIFT)["cell"].ravel()
        res["a_peak_equals_b_cell"] = bool((fns["a"]().cpu().numpy() == cells).all())
    if "b" in r:
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(calls):
            fns["b"]()
        ctx.sync()
        prof = {k: p for k, p in ctx.prof_read().items() if p["launches"]}
        ctx.prof_enable(False)
        total = sum(p["ms"] for p in prof.values())
        res["b"]["profiled_us_per_call"] = {k: 1e3 * p["ms"] / calls for k, p in prof.items()}
        res["b"]["transform_share_of_profiled"] = sum(p["ms"] for k, p in prof.items() if k in TRANSFORM_IDS) / total if total else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", default="", help="a or b alone")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"calls": a.calls, "warmup": a.warmup, "rounds": a.rounds, "cutoff": CUTOFF}
    for name in SHAPES:
        out[name] = bench(ctx, name, a.calls, a.warmup, a.rounds, a.variant)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
