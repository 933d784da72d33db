"""Every call that changes the weights drops every cache derived from them (weights_changed, csrc/net.h): set_pair, load_spectra, a
train_pair burst and step_grad + step_apply, each made on a net whose caches are all warm and current -- the step's operator sets, the
bin-major record, the inference operators (ops_valid), the hidden-layer operator and the decode operator.  What infer and then decode give
afterwards is held, bit for bit, to a fresh net of the same Context that was given the first net's weights and makes the same two calls
cold: a cache that survives shows as a difference.

load_spectra is the one call after which a warm and a cold net are not bit-identical (2.6e-7 .. 3.9e-7 of the largest value): the loaded
spectra ARE the first net's weights, while the fresh net forms its spectra from the taps that aefft_kernel_export derived from them -- one
float32 round trip apart.  That call's outputs are held to the float64 oracle of the first net's taps at test_gpu_infer.TOL instead (the
call halves a pair's weights: a surviving cache is far outside)."""
import importlib

import numpy as np
import pytest

import frozen_cases as F
from frozen_cases import CASES, _case, _oracle_layers, _scales, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import TOL, _infer
from test_gpu_decode import _codes, _decode, _decode_oracle

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu


def _hidden(name):
    """the pair whose hidden layer is asked for and decoded: the innermost.  Its hidden operator reads every encoder, its decode operator every
    decoder, and expanding its hidden layer overwrites no next pair's input operator (a pair of scale 1 keeps its input in the buffer of the
    hidden layer before it), so the inference operators are still current when the weight-changing call is made"""
    return len(CASES[name][3]) - 1


def _step(net, frames):
    net.step_grad(frames)
    net.step_apply(0.02)


def _set_pair(net, l, frames):
    net.set_pair(l, *[0.5 * a for a in net.get_pair(l)])


def _load_spectra(net, l, frames):
    c, b, f, p = net.get_pair(l)
    Cs, Fs = net.store_spectra(l)
    net.load_spectra(l, 0.5 * Cs, 0.5 * b, 0.5 * Fs, 0.5 * p)


def _train_pair(net, l, frames):
    net.train_pair(l, 2, 0.02)


def _step_call(net, l, frames):
    _step(net, frames)


ORACLE = {"load_spectra"}        # not bit-identical with a cold net (module docstring): against the float64 oracle
CALLS = {"set_pair": _set_pair, "load_spectra": _load_spectra, "train_pair": _train_pair, "step": _step_call}


def _warm(ctx, net, frames, code, h):
    """decode first (it overwrites activation buffers): infer then leaves every cache of the current weights in place, and a forward behind
    it, which a burst trains on"""
    _decode(ctx, net, code, h)
    _infer(ctx, net, frames, h)


def _outputs(ctx, net, frames, code, h):
    """infer first: it is the call that would run on the operators of the old weights"""
    rec, hid = _infer(ctx, net, frames, h)
    return {"recon": rec, "hidden": hid, "decode": _decode(ctx, net, code, h)}


def _oracle_outputs(name, ws, xs, code, h):
    ws = [tuple(a.astype(np.float64) for a in w) for w in ws]
    s = _scales(CASES[name][6], len(ws))
    layers = [_oracle_layers(x, ws, s) for x in xs]
    return {"recon": np.stack([q[-1] for q in layers]), "hidden": np.stack([q[2 * h + 2] for q in layers]),
            "decode": np.stack([_decode_oracle(c, ws, s, h) for c in code])}


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator")])
@pytest.mark.parametrize("name", ["64-2pairs", "64-4pairs"])
def test_no_cache_survives_a_weight_change(ctx, flags, name, path, form, call):
    flags(path)
    L = len(CASES[name][3])
    frames = ctx.dev(_case(name)[1][0])
    h = _hidden(name)
    code = ctx.dev(_codes(name, h)[0])
    for l in ([0] if call == "step" else sorted({0, 1, L - 1})):      # the pair whose weights the call changes (the step changes every pair's)
        net = F.net(ctx, name)
        assert net.step_form() == form
        _warm(ctx, net, frames, code, h)
        _step(net, frames)                        # warm: the step's operator sets and the bin-major record of the updated weights
        _warm(ctx, net, frames, code, h)          # ... the decode operator, the inference operators and the hidden operator of the same weights
        CALLS[call](net, l, frames)
        warm = _outputs(ctx, net, frames, code, h)
        ws = [net.get_pair(j) for j in range(L)]
        fresh = F.net(ctx, name, ws)
        cold = _outputs(ctx, fresh, frames, code, h)
        for k in warm:
            d = np.abs(warm[k].astype(np.float64) - cold[k]).max() / max(1.0, np.abs(cold[k]).max())
            print(f"{name} [{path}] {call} of pair {l}: {k} warm against cold {d:.2e}")
        ref = _oracle_outputs(name, ws, _case(name)[1][0], _codes(name, h)[0], h) if call in ORACLE else None
        for k in warm:
            assert np.isfinite(cold[k]).all(), (name, path, call, l, k)
            if ref is None:
                assert np.array_equal(warm[k], cold[k]), (name, path, call, l, k)
            else:
                e = relerr(warm[k], ref[k])
                print(f"{name} [{path}] {call} of pair {l}: {k} against the oracle {e:.2e}")
                assert e < TOL, (name, path, call, l, k, e)
        net.close(); fresh.close()
