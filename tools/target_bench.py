"""Training toward a target frame: what the target costs, one process on one GPU; prints one JSON line.

Two nets -- cfg3-P2's (D=3, maps 8/16/32/64, 5x5, s=2) at 512^2 with B = 32 and the same net at 640 x 480 (smooth sizes, operator form) --
and per net ms per training step (gradient half + update half, MSE asked for) of
  plain             (a) aefft_net_step_grad + aefft_net_step_apply
  target            (b) aefft_net_step_grad_target + aefft_net_step_apply
  target_noopform   (c) ... under AEFFT_F_NOOPFORM (the per-frame form), on a net of its own
The variants are alternated in the process: --rounds rounds of --calls steps each between events on the library's stream, after --warmup
steps of each.  Then, with the profiler on (every launch bracketed by events: the side streams and the fused update are off, so these are
per-launch times, not a step time): the input transform's two launches (r2c_rows + r2c_cols, per transform), target_terms and target_mse,
the two new kernels also as algorithmic bytes over time against the 8 TB/s peak.

    python tools/target_bench.py [--calls 40] [--warmup 15] [--rounds 3] [--only NAME]
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
from tools.infer_bench import NETS  # noqa: E402
from tools.sizes_bench import timed  # noqa: E402

HBM_PEAK_GBS = 8000.0
BENCH_NETS = ("cfg3p2", "cfg3p2_640x480")


def _net(ctx, name, rng):
    D, Nx, Ny, maps, Nk, s, B, smooth = NETS[name]
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, **(dict(smooth_sizes=True, operator_form=True) if smooth else {}))
    dD = D
    for l, dM in enumerate(maps):
        net.set_pair(l, 0.1 * rng.uniform(-1, 1, (dM, dD, Nk, Nk)), rng.uniform(-1, 1, dM), 0.1 * rng.uniform(-1, 1, (dD, dM, Nk, Nk)), rng.uniform(-1, 1, dD))
        dD = dM
    return net


def bench_net(ctx, name, calls, warmup, rounds):
    D, Nx, Ny, maps, Nk, s, B, smooth = NETS[name]
    frames = ctx.dev(np.floor(np.random.default_rng(1).uniform(0, 256, (B, D, Nx, Ny))))
    targets = ctx.dev(np.floor(np.random.default_rng(2).uniform(0, 100, (B, D, Nx, Ny))))
    op_net, pf_net = _net(ctx, name, np.random.default_rng(len(name))), _net(ctx, name, np.random.default_rng(len(name)))
    mse = ctx.empty(len(maps))

    def plain():
        op_net.step_grad(frames, None); op_net.step_apply(0.2, 0, 0, 1.0, mse)

    def target():
        op_net.step_grad_target(frames, targets, None); op_net.step_apply(0.2, 0, 0, 1.0, mse)

    def target_noopform():
        pf_net.step_grad_target(frames, targets, None); pf_net.step_apply(0.2, 0, 0, 1.0, mse)

    fns = {"plain": (plain, ()), "target": (target, ()), "target_noopform": (target_noopform, ("NOOPFORM",))}
    forms = {}
    for k, (fn, fl) in fns.items():
        ctx.set_flags(*fl)
        forms[k] = (pf_net if fl else op_net).step_form()
        for _ in range(warmup):
            fn()
    ctx.sync()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, fl) in fns.items():
            ctx.set_flags(*fl)
            for _ in range(3):        # (the other variant ran last: its chain carried ahead, its caches)
                fn()
            res[k].append(timed(ctx, fn, calls))
    ctx.set_flags()
    # per-launch times: the gradient half and the update half profiled apart, so that the "target" id holds one kernel at a time
    ctx.prof_enable()
    acc = {"r2c": [0, 0.0], "target_terms": [0, 0.0, 0.0], "target_mse": [0, 0.0, 0.0]}
    for _ in range(calls):
        ctx.prof_reset()
        op_net.step_grad_target(frames, targets, None)
        p = ctx.prof_read()
        acc["r2c"][0] += p["r2c_rows"]["launches"]; acc["r2c"][1] += p["r2c_rows"]["ms"] + p["r2c_cols"]["ms"]
        for i, f in enumerate(("launches", "ms", "bytes")):
            acc["target_terms"][i] += p["target"][f]
        ctx.prof_reset()
        op_net.step_apply(0.2, 0, 0, 1.0, mse)
        p = ctx.prof_read()
        for i, f in enumerate(("launches", "ms", "bytes")):
            acc["target_mse"][i] += p["target"][f]
    ctx.prof_enable(False)
    launches = {"r2c_rows+r2c_cols": {"transforms": acc["r2c"][0], "us_per_transform": 1e3 * acc["r2c"][1] / max(acc["r2c"][0], 1)}}
    for k in ("target_terms", "target_mse"):
        n, ms, by = acc[k]
        launches[k] = {"launches": n, "us_per_launch": 1e3 * ms / max(n, 1), "mb_per_launch": by / max(n, 1) / 1e6,
                       "share_of_peak": (by / 1e9) / (ms / 1e3) / HBM_PEAK_GBS if ms > 0 else None}
    op_net.close(); pf_net.close()
    out = {"forms": forms, "launches": launches}
    for k, v in res.items():
        out[k] = {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "rounds": v}
    out["target_minus_plain_ms"] = out["target"]["ms_median"] - out["plain"]["ms_median"]
    out["target_below_noopform_every_round"] = all(b < c for b, c in zip(res["target"], res["target_noopform"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    ctx = aefft.Context(0)
    out = {"lib": aefft.LIB_PATH, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    for name in BENCH_NETS:
        if a.only and name != a.only:
            continue
        out[name] = bench_net(ctx, name, a.calls, a.warmup, a.rounds)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
