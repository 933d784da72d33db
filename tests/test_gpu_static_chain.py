"""The tail launch's two step routes against each other: the per-bin steps from a compile-time table for the net's channel counts (static) and
the same steps decoded from the step list in the kernel's arguments (generic, AEFFT_F_NOSTATICCHAIN).  Both multiply the same elements in the
same order, so three training steps from identical weights must leave IDENTICAL bits: weights, packed gradients, post-update MSE, reconstruction.
(What pins either route to the reference are the oracle parity tests; this file only pins the routes to each other.)"""
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

D, NK, POOL, B, STEPS = 3, 5, 2, 2, 3


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context()
    yield c
    c.close()


def _smallest_chain_frame(ctx, maps):
    """the smallest square power-of-two frame at which the net exists and its step runs in the operator-chain form: 64 for the three-pair net,
    256 for the five-pair one, and 128 for the four-pair one (at 64 its innermost pooled grid would be 4 x 4: aefft_net_create refuses it)"""
    for N in (16, 32, 64, 128, 256, 512):
        try:
            net = aefft.Net(ctx, D, N, N, list(maps), NK, POOL, batch=B)
        except aefft.AefftError:
            continue
        form = net.step_form()
        net.close()
        if form == "operator_chain":
            return N
    raise AssertionError(f"no frame up to 512 runs maps {maps} in the operator-chain form")


N_WANT = {(8, 16, 32): 64, (8, 16, 32, 64): 128, (8, 16, 32, 64, 128): 256, (8, 16, 24): 64}


def _weights(maps, tied, seed, N):
    rng = np.random.default_rng(seed)
    q32 = lambda a: a.astype(np.float32).astype(np.float64)
    ws, dD = [], D
    for dM in maps:
        c = q32(rng.uniform(-1, 1, (dM, dD, NK, NK)))
        f = np.transpose(c, (1, 0, 2, 3)).copy() if tied else q32(rng.uniform(-1, 1, (dD, dM, NK, NK)))
        ws.append((c, q32(rng.uniform(-1, 1, dM)), f, q32(rng.uniform(-1, 1, dD)))); dD = dM
    return ws, np.floor(rng.uniform(0, 256, (B, D, N, N)))


def _run(ctx, flags, maps, switches, sym, maxdiff, ws, xs):
    """STEPS training steps; -> (route of the last tail launch, [arrays])"""
    flags(*switches)
    N = xs.shape[-1]
    net = aefft.Net(ctx, D, N, N, list(maps), NK, POOL, batch=B)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    assert net.step_form() == "operator_chain"
    frames, recon, mse = ctx.dev(xs), ctx.empty(B, D, N, N), ctx.empty(len(maps))
    out = []
    for _ in range(STEPS):
        net.step_grad(frames, recon)
        out.append(host(net.grad_buffer()).copy())
        net.step_apply(0.2, maxdiff, sym, 1.0, mse)
        out.append(host(mse).copy())
        out.append(host(recon).copy())
    route = net.tail_route()
    for l in range(len(maps)):
        out.extend(np.asarray(a).copy() for a in net.get_pair(l))
    net.close()
    return route, out


def _both_routes(ctx, flags, maps, extra, sym, maxdiff, want):
    flags()
    N = _smallest_chain_frame(ctx, maps)
    assert N == N_WANT[tuple(maps)], N
    ws, xs = _weights(maps, sym == 1, 4711 + len(maps), N)
    r_def, a = _run(ctx, flags, maps, extra, sym, maxdiff, ws, xs)
    r_gen, b = _run(ctx, flags, maps, extra + ["NOSTATICCHAIN"], sym, maxdiff, ws, xs)
    assert r_def == want and r_gen == "generic", (r_def, r_gen)
    assert len(a) == len(b) == 3 * STEPS + 4 * len(maps)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all(), i
        assert np.array_equal(x, y), (i, float(np.abs(x.astype(np.float64) - y).max()))
    assert np.abs(a[-4] - ws[-1][0]).max() > 1e-4, "the update was not applied"


@pytest.mark.parametrize("maps", [(8, 16, 32), (8, 16, 32, 64), (8, 16, 32, 64, 128)])
def test_static_route_gives_the_generic_route_s_bits(ctx, flags, maps):
    _both_routes(ctx, flags, maps, [], 0, 0, "static")


def test_static_route_with_the_fused_mse_as_config5_runs_it(ctx, flags):
    """the five-pair net with the innermost pair's MSE inside the chain items (CHAINMSE), tied weights and the multiobjective term"""
    _both_routes(ctx, flags, (8, 16, 32, 64, 128), ["CHAINMSE"], 1, 1, "static")


def test_net_without_a_table_takes_the_generic_route(ctx, flags):
    _both_routes(ctx, flags, (8, 16, 24), [], 0, 0, "generic")
