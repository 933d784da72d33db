"""The tail launch with the innermost pair's post-update MSE inside the chain's per-bin items (the fused route), for the nets whose fused kernel
is compiled from a static step table at six workgroups per CU.  Three pins, none of them against the oracle (tests/test_gpu_fft_path.py and
tests/test_gpu_round4.py hold the CHAINMSE path to it):
  * the four-pair net's fused static kernel against the fused generic kernel: same elements, same order, identical bits;
  * the three-pair net, which has no fused table, still runs the generic kernel under CHAINMSE;
  * fused against unfused from the same weights: the MSE feeds nothing back, so everything but the MSE is identical, and the MSE -- whose partial
    sums land in other slots, in another order -- agrees to the bound the oracle parity tests hold it to (so does its copy in the tail of the
    next step's gradient message, include/aefft.h aefft_net_grad_buffer)."""
import importlib

import numpy as np
import pytest

from test_gpu_static_chain import N_WANT, STEPS, _both_routes, _run, _smallest_chain_frame, _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

FOUR, THREE = (8, 16, 32, 64), (8, 16, 32)


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context()
    yield c
    c.close()


def test_four_pair_fused_static_route_gives_the_generic_route_s_bits(ctx, flags):
    """maps (8,16,32,64) at 128 x 128, B = 2, three steps under CHAINMSE: the static table's fused kernel against NOSTATICCHAIN"""
    _both_routes(ctx, flags, FOUR, ["CHAINMSE"], 0, 0, "static")


def test_three_pair_net_fuses_in_the_generic_kernel(ctx, flags):
    """maps (8,16,32) at 64 x 64 under CHAINMSE: no fused table, so the launch reports the generic route with and without NOSTATICCHAIN"""
    _both_routes(ctx, flags, THREE, ["CHAINMSE"], 0, 0, "generic")


def test_fused_against_unfused_on_the_default_route(ctx, flags):
    """The four-pair net as the launcher routes it by itself (at this size: the packed MSE in workgroups of its own, static steps) against the same
    net under CHAINMSE (the MSE inside the items, static steps).  MSE bound: |d| < 1e-5 * max(1, mse), as test_gpu_fft_path._step_vs_oracle."""
    flags()
    N = _smallest_chain_frame(ctx, FOUR)
    assert N == N_WANT[FOUR], N
    ws, xs = _weights(FOUR, False, 4711 + len(FOUR), N)
    r_def, a = _run(ctx, flags, FOUR, [], 0, 0, ws, xs)
    r_fus, b = _run(ctx, flags, FOUR, ["CHAINMSE"], 0, 0, ws, xs)
    assert r_def == "static" and r_fus == "static", (r_def, r_fus)
    assert len(a) == len(b) == 3 * STEPS + 4 * len(FOUR)
    L = len(FOUR)
    mse_close = lambda x, y: (np.abs(x.astype(np.float64) - y.astype(np.float64)) < 1e-5 * np.maximum(1.0, np.abs(x.astype(np.float64)))).all()
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all() and np.isfinite(y).all(), i
        if i < 3 * STEPS and i % 3 == 1:                           # the step's per-pair MSE
            assert x.shape == y.shape == (L,)
            print("step", i // 3, "mse", x, "fused", y, "max |d|", np.abs(x.astype(np.float64) - y).max())
            assert mse_close(x, y), (i, x, y)
        elif i < 3 * STEPS and i % 3 == 0:                         # the gradient message: [gradients | the previous step's MSE, one float per pair]
            assert np.array_equal(x[:-L], y[:-L]), (i, float(np.abs(x[:-L].astype(np.float64) - y[:-L]).max()))
            assert mse_close(x[-L:], y[-L:]), (i, x[-L:], y[-L:])
        else:
            assert np.array_equal(x, y), (i, float(np.abs(x.astype(np.float64) - y).max()))
    assert np.abs(a[-4] - ws[-1][0]).max() > 1e-4, "the update was not applied"
