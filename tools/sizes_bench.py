"""Smooth-size measurements, all in one process on one GPU; prints one JSON line.

  op level : batched 2-D R2C and C2R of 96 planes of 640 x 480 and 32 planes of 1280 x 720, the mixed-radix transforms against the
             Bluestein route (AEFFT_F_CHIRPZ) on the same buffers, alternated: time per call, algorithmic bytes/s (read + write once),
             the share of HBM peak -- the per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script
  training : cfg3-P2's net (D=3, maps 8/16/32/64, 5x5, s=2, B=32) at 640 x 480 (smooth sizes, per-frame form) and at 512^2 under NOOPFORM
             (the same per-frame form on powers of two: the yardstick), alternated: ms/step and frames/s; vga_640x480_full is the 640 x 480
             net with the weight side on the full pad + R2C / C2R + shrink route (AEFFT_F_NOPRUNESMOOTH), the A/B of the pruned transforms;
             vga_640x480_opform is the 640 x 480 net created with AEFFT_NET_SMOOTH_OPFORM (operator form; left out, with a note in the
             result, when AEFFT_LIB names a library from before the option)

    python tools/sizes_bench.py [--reps 20] [--steps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/sizes_bench.py --no-train --rounds 1     (per-kernel split, op level)
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/sizes_bench.py --train-only vga_640x480   (per-kernel split of one step kind)
    python tools/sizes_bench.py --train --flags NOGROUP     (training only; development switches added to every net's own)
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
HBM_PEAK = 8.0e12     # MI355X HBM3E, bytes/s


def timed(ctx, fn, reps):
    """mean ms of fn() over reps calls, bracketed by events on the library's stream after a synchronisation"""
    t = ctx.torch
    ptr = ctx.L.aefft_stream(ctx.h)
    st = t.cuda.ExternalStream(ptr) if ptr else t.cuda.default_stream()      # (a context on torch's default stream)
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    ctx.sync()
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    ctx.sync()
    b.synchronize()
    return a.elapsed_time(b) / reps


def op_level(ctx, planes, Nx, Ny, reps, rounds):
    rng = np.random.default_rng(Nx)
    x = ctx.dev(np.floor(rng.uniform(0, 256, (planes, Nx, Ny))))
    X = ctx.r2c(x)
    y = ctx.c2r(X, Ny)
    r2c = lambda: ctx.check(ctx.L.aefft_r2c(ctx.h, x.data_ptr(), X.data_ptr(), planes, Nx, Ny))
    c2r = lambda: ctx.check(ctx.L.aefft_c2r(ctx.h, X.data_ptr(), y.data_ptr(), planes, Nx, Ny, 1.0 / (Nx * Ny)))
    res = {k: [] for k in ("r2c_mixed", "r2c_chirpz", "c2r_mixed", "c2r_chirpz")}
    for path in ("", "CHIRPZ"):                                 # warm-up: tables, code objects
        ctx.set_flags(*([path] if path else [])); r2c(); c2r(); ctx.sync()
    for _ in range(rounds):
        for path, tag in (("", "mixed"), ("CHIRPZ", "chirpz")):
            ctx.set_flags(*([path] if path else []))
            res["r2c_" + tag].append(timed(ctx, r2c, reps))
            res["c2r_" + tag].append(timed(ctx, c2r, reps))
    ctx.set_flags()
    nbytes = planes * (Nx * Ny * 4 + Nx * (Ny // 2 + 1) * 8)
    out = {"planes": planes, "Nx": Nx, "Ny": Ny, "bytes": nbytes}
    for k, v in res.items():
        ms = float(np.median(v))
        out[k + "_ms"] = round(ms, 4)
        out[k + "_GBps"] = round(nbytes / ms / 1e6, 1)
        out[k + "_hbm_share"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)
    out["r2c_speedup"] = round(out["r2c_chirpz_ms"] / out["r2c_mixed_ms"], 2)
    out["c2r_speedup"] = round(out["c2r_chirpz_ms"] / out["c2r_mixed_ms"], 2)
    return out


NETS = (("vga_640x480", 640, 480, True), ("vga_640x480_full", 640, 480, True), ("p2_512x512_noopform", 512, 512, False), ("p2_512x512", 512, 512, False),
        ("vga_640x480_opform", 640, 480, True))
FLAGS_OF = {"vga_640x480": [], "vga_640x480_full": ["NOPRUNESMOOTH"], "p2_512x512_noopform": ["NOOPFORM"], "p2_512x512": [], "vga_640x480_opform": []}


def training(ctx, steps, warmup, rounds, only=None, extra=()):
    D, maps, Nk, s, B = 3, [8, 16, 32, 64], 5, 2, 32
    rng = np.random.default_rng(3)
    nets = {}
    skipped = []
    for tag, Nx, Ny, smooth in NETS:
        if only and tag != only:
            continue
        try:
            net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, smooth_sizes=smooth, operator_form=tag.endswith("_opform"))
        except RuntimeError:
            if not tag.endswith("_opform"):
                raise
            skipped.append(tag)          # a library from before AEFFT_NET_SMOOTH_OPFORM refuses the option bit
            continue
        dD = D
        for l, dM in enumerate(maps):
            net.set_pair(l, rng.uniform(-1, 1, (dM, dD, Nk, Nk)) * 0.05, rng.uniform(-1, 1, dM), rng.uniform(-1, 1, (dD, dM, Nk, Nk)) * 0.05,
                         rng.uniform(-1, 1, dD))
            dD = dM
        frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))))
        recon = ctx.empty(B, D, Nx, Ny)
        nets[tag] = (net, frames, recon, Nx, Ny)

    def step(tag):
        net, frames, recon, _, _ = nets[tag]
        net.step_grad(frames, recon)
        net.step_apply(0.2)

    flags_of = {k: v + [f for f in extra if f not in v] for k, v in FLAGS_OF.items()}
    for tag in nets:
        ctx.set_flags(*flags_of[tag])
        for _ in range(warmup):
            step(tag)
        ctx.sync()
    res = {tag: [] for tag in nets}
    for _ in range(rounds):
        for tag in nets:
            ctx.set_flags(*flags_of[tag])
            res[tag].append(timed(ctx, lambda: step(tag), steps))
    ctx.set_flags()
    out = {}
    for tag, v in res.items():
        ms = float(np.median(v))
        ctx.set_flags(*flags_of[tag])
        out[tag] = {"ms_per_step": round(ms, 4), "rounds_ms": [round(x, 4) for x in v], "frames_per_s": round(B / ms * 1e3, 1), "form": nets[tag][0].step_form()}
    ctx.set_flags()
    if skipped:
        out["skipped"] = skipped
    if not only:
        if "vga_640x480_opform" in out:
            out["step_ratio_opform_over_per_frame"] = round(out["vga_640x480_opform"]["ms_per_step"] / out["vga_640x480"]["ms_per_step"], 3)
            out["step_ratio_opform_over_512_default"] = round(out["vga_640x480_opform"]["ms_per_step"] / out["p2_512x512"]["ms_per_step"], 3)
        out["step_ratio_vga_over_512"] = round(out["vga_640x480"]["ms_per_step"] / out["p2_512x512_noopform"]["ms_per_step"], 3)
        out["pixel_ratio"] = round(640 * 480 / 512 / 512, 3)
    for net, *_ in nets.values():
        net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-train", action="store_true", help="op level only (the profiler run)")
    ap.add_argument("--train-only", choices=[n[0] for n in NETS], default=None, help="the training steps of one net only (the profiler run)")
    ap.add_argument("--train", action="store_true", help="training only, every net, alternated")
    ap.add_argument("--flags", default="", help="comma-separated development switches (without AEFFT_F_) added to every net's own")
    a = ap.parse_args()
    extra = [f for f in a.flags.split(",") if f]
    ctx = aefft.Context(0)
    if a.train_only or a.train:
        print(json.dumps({"train": training(ctx, a.steps, a.warmup, a.rounds, a.train_only, extra)}))
        ctx.close()
        return
    out = {"op": [op_level(ctx, 96, 640, 480, a.reps, a.rounds), op_level(ctx, 32, 1280, 720, a.reps, a.rounds)]}
    if not a.no_train:
        out["train"] = training(ctx, a.steps, a.warmup, a.rounds, None, extra)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
