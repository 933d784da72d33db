"""The reconstruction on its side stream against the same step with everything in line.  What differs between the two is the queue the
inverse transform's kernels run in (fork and join by device-scope events, host.h AEFFT_X_QUEUE_EVENT_FLAGS) -- not a kernel's code, its launch
or the order of its sums -- so three training steps from identical weights must leave IDENTICAL bits whichever way they ran: reconstruction,
packed gradients, post-update MSE and every pair's weights.  The shapes are the
smallest that reach the code (conftest.py's SMALLOVERLAP sends them to the side stream): the four-pair net (not creatable below 128 x 128; its
row pass takes the sparse-head route), a two-pair net with an odd batch (the row pass's last workgroup partly live), and a smooth 96 x 96 net
whose row pass is the mixed-radix one.
(What pins the step to the reference are the oracle parity tests; this file pins the overlapped step to the in-line one, and the join to
include/aefft.h's ordering promise.)"""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from test_gpu_fft_path import host

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

D, POOL, STEPS = 3, 2, 3
SHAPES = {  # N, maps, Nk, B, Net keywords
    "128-four-pairs": (128, (8, 16, 32, 64), 5, 4, {}),
    "64-odd-batch": (64, (8, 16), 5, 3, {}),
    "96-smooth": (96, (4, 3), 3, 3, {"smooth_sizes": True, "operator_form": True}),
}
MODES = {"default": ([], False), "inline": (["NOOVERLAP"], False), "pipelined": ([], True)}   # development switches, set_input_ready


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _inputs(name):
    N, maps, Nk, B, _ = SHAPES[name]
    rng = np.random.default_rng(977 + N + len(maps))
    q32 = lambda a: a.astype(np.float32).astype(np.float64)
    ws, dD = [], D
    for dM in maps:
        ws.append((q32(rng.uniform(-1, 1, (dM, dD, Nk, Nk))), q32(rng.uniform(-1, 1, dM)),
                   q32(rng.uniform(-1, 1, (dD, dM, Nk, Nk))), q32(rng.uniform(-1, 1, dD))))
        dD = dM
    return ws, np.floor(rng.uniform(0, 256, (B, D, N, N)))


def _net(ctx, name, ws):
    N, maps, Nk, B, kw = SHAPES[name]
    net = aefft.Net(ctx, D, N, N, list(maps), Nk, POOL, batch=B, **kw)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    return net


_runs = {}


def _steps(ctx, name, mode):
    """STEPS training steps of a shape in one of MODES, from the same weights and frames; computed once per (shape, mode) and left unchanged:
    [packed gradients, post-update MSE, reconstruction] per step, then c, b, f, p of every pair"""
    if (name, mode) in _runs:
        return _runs[name, mode]
    switches, ready = MODES[mode]
    N, maps, Nk, B, _ = SHAPES[name]
    ws, xs = _inputs(name)
    ctx.set_flags(*switches)
    net = _net(ctx, name, ws)
    net.set_input_ready(ready)
    frames, recon = ctx.dev(xs), ctx.empty(B, D, N, N)
    out = []
    for _ in range(STEPS):
        recon.fill_(float("nan"))
        net.step_grad(frames, recon)
        out.append(host(net.grad_buffer()).copy())
        net.step_apply(0.2)                              # (the pipelined mode's deferred reconstruction is joined here)
        out.append(host(net.last_mse()).copy())
        out.append(host(recon).copy())
    for l in range(len(maps)):
        out.extend(np.asarray(a).copy() for a in net.get_pair(l))
    net.close()
    ctx.set_flags()
    assert len(out) == 3 * STEPS + 4 * len(maps)
    assert all(np.isfinite(a).all() for a in out), (name, mode)
    assert np.abs(out[-4] - ws[-1][0]).max() > 1e-4, "the update was not applied"
    _runs[name, mode] = out
    return out


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (i, float(np.abs(x.astype(np.float64) - y).max()))


@pytest.mark.parametrize("name", list(SHAPES))
def test_side_stream_step_gives_the_inline_step_s_bits(ctx, flags, name):
    _same(_steps(ctx, name, "default"), _steps(ctx, name, "inline"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_pipelined_step_gives_the_default_step_s_bits(ctx, flags, name):
    """set_input_ready(True): the input transform on aux[1] (ev_r2c, ev_mid, ev_end), the reconstruction deferred behind the gradient half"""
    _same(_steps(ctx, name, "default"), _steps(ctx, name, "pipelined"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_join_keeps_the_stream_order_promise(ctx, flags, name):
    """include/aefft.h: recon_d is complete, in stream order on the context stream, when step_grad's work is.  The context enqueues on torch's
    stream, so a torch copy enqueued right behind step_grad -- no synchronisation in between -- must see the finished reconstruction; and
    aefft_sync alone (no torch.cuda.synchronize()) must leave it readable from the host."""
    flags()
    N, maps, Nk, B, _ = SHAPES[name]
    ws, xs = _inputs(name)
    want = _steps(ctx, name, "inline")[2]               # the first step's reconstruction, everything in line
    net = _net(ctx, name, ws)
    frames, recon = ctx.dev(xs), ctx.empty(B, D, N, N)
    recon.fill_(float("nan"))
    ctx.sync()
    net.step_grad(frames, recon)
    copy = recon.clone()                                # on torch's current stream == the context stream
    ctx.sync()
    after_sync = host(recon).copy()
    got_copy = host(copy).copy()
    net.close()
    assert np.array_equal(after_sync, want), float(np.abs(after_sync - want).max())
    assert np.array_equal(got_copy, want), float(np.abs(got_copy - want).max())


@pytest.mark.parametrize("name", list(SHAPES))
def test_inline_reconstructions_are_what_they_were(ctx, flags, name):
    """infer and score launch their reconstruction in line, with no residency target: under the default switches they give what they give
    under NOOVERLAP"""
    N, maps, Nk, B, _ = SHAPES[name]
    ws, xs = _inputs(name)
    outs = []
    for switches in ([], ["NOOVERLAP"]):
        flags(*switches)
        net = _net(ctx, name, ws)
        frames = ctx.dev(xs)
        r_inf, r_sc = ctx.empty(B, D, N, N), ctx.empty(B, D, N, N)
        net.infer(frames, r_inf)
        score, _ = net.score(frames, None, r_sc)
        outs.append([host(r_inf).copy(), host(score).copy(), host(r_sc).copy()])
        net.close()
    _same(outs[0], outs[1])
    assert all(np.isfinite(a).all() for a in outs[0])
