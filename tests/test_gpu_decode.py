"""aefft_net_decode (Net.decode): the reconstruction from a stored hidden layer -- arbitrary codes against the float64 oracle in every
form and route, the round trip through Net.infer, the 8-bit output rule exactly, training undisturbed bit for bit, the operator cache by
the profiler's launch counts, state and errors, the spatial net."""
import functools
import importlib

import numpy as np
import pytest
import torch

import np_ref as R
import np_spatial as S
import frozen_cases as F
from frozen_cases import CASES, PATHS, _case, _rule, _scales, _weights, host, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import _infer, _train_streamed

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

TOL = 1e-4      # the project's bound on the step's and the inference's reconstruction (test_gpu_infer.TOL)
DECODE_CASES = ["64-1pair", "64-2pairs", "64-4pairs", "256-4pairs", "cfg2", "no-pooling", "640x480", "640x480-opform", "5x3", "D4", "tied"]


def _decode_oracle(code, ws, scales, l):
    """np_ref (float64): the rest of autoenc_fft (fft_backproplib.cu:1331-1376) from its loop index n = l + 1 with freq = fft(code) of ONE
    frame's layer 2l+2 -- pool then conv_k with c_n for the pairs below l, conv_k with f_n then pool(-s) for every decoder -- and fft_inv"""
    L = len(ws)
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]
    net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    sc = list(scales) + [-v for v in scales[::-1]]
    code = np.asarray(code, np.float64)
    Nx, Ny = code.shape[-2:]
    freq = R.fft(code)
    for n in range(l + 1, 2 * L):
        if n < L:
            freq, Nx, Ny = R.pool_fft(freq, Nx, Ny, sc[n])
        ofreq = R.conv_k(freq, R.kernel_spectrum(net_c[n], Nx, Ny), net_b[n], Nx, Ny)
        if n >= L:
            ofreq, Nx, Ny = R.pool_fft(ofreq, Nx, Ny, sc[n])
        freq = ofreq
    return R.fft_inv(freq, Nx, Ny)


def _code_shape(name, l):
    D, Nx, Ny, maps, Nk, Nl, s, B, *_ = CASES[name]
    for v in _scales(s, len(maps))[:l + 1]:
        Nx //= v; Ny //= v
    return B, maps[l], Nx, Ny


@functools.lru_cache(maxsize=None)
def _codes(name, l, k=0):
    """arbitrary codes (float32-exact uniform values, not an encoder's output) and their float64 decode under the case's weights"""
    ws, _ = _case(name)
    rng = np.random.default_rng(sum(map(ord, name)) + 17 * l + 1000 * k)
    code = rng.uniform(-64, 192, _code_shape(name, l)).astype(np.float32).astype(np.float64)
    s = _scales(CASES[name][6], len(ws))
    return code, np.stack([_decode_oracle(c, ws, s, l) for c in code])


def _decode(ctx, net, code, l, u8=False):
    """one Net.decode of a host array: the reconstruction as a host array; the output starts as NaN / 0xAA"""
    rec = ctx.empty(net.B, net.D, net.Nx, net.Ny, dtype=torch.uint8 if u8 else None)
    rec.fill_(0xAA if u8 else float("nan"))
    net.decode(code if torch.is_tensor(code) else ctx.dev(code), l, rec)
    ctx.sync()
    return host(rec).copy()


def _want_form(name, path):
    want = CASES[name][-1]
    if path == "NOOPFORM":
        return "per_frame"
    if path == "NOCHAIN" and want == "operator_chain":
        return "operator"
    return want


# ------------------------------------------------------------------------------------------
# 1. arbitrary codes against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", DECODE_CASES)
def test_decode_against_the_oracle(ctx, flags, name, path):
    flags(path)
    net = F.net(ctx, name)
    assert net.step_form() == _want_form(name, path)
    L = len(CASES[name][3])
    for rnd in range(2):            # the second pass over the pairs: every operator formed again after another pair's
        for l in range(L):
            code, ref = _codes(name, l)
            rec = _decode(ctx, net, code, l)
            e = relerr(rec, ref)
            print(f"{name} [{path}] pair {l} pass {rnd}: {e:.2e}")
            assert e < TOL, (name, path, l, e)
    # the same pair twice in a row: from the cached operator
    code, ref = _codes(name, L - 1)
    assert relerr(_decode(ctx, net, code, L - 1), ref) < TOL
    net.close()


@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("maps,scales", [([2, 2, 2], [2, 2, 2]), ([2, 2], [2, 1]), ([1, 2, 1], [2, 2, 1]), ([2], [2])])
def test_hidden_layers_narrower_than_the_input(ctx, flags, maps, scales, path, form):
    """every hidden layer has fewer channels than the frames (D = 3): the rows the operator is formed from are sized by the hidden widths, not
    by D (launch_decode_op holds every stage's row against the allocated column).  Every pair, twice over, against the oracle"""
    flags(path)
    D, N, B, L = 3, 64, 2, len(maps)
    rng = np.random.default_rng(7 + sum(maps) + L)
    ws = _weights(rng, D, maps, 3, 3)
    net = F.track(aefft.Net(ctx, D, N, N, maps, 3, scales, batch=B))
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    assert net.step_form() == form
    for rnd in range(2):
        n = N
        for l in range(L):
            n //= scales[l]
            code = rng.uniform(-64, 192, (B, maps[l], n, n)).astype(np.float32).astype(np.float64)
            ref = np.stack([_decode_oracle(c, ws, scales, l) for c in code])
            e = relerr(_decode(ctx, net, code, l), ref)
            print(f"narrow {maps} [{path}] pair {l} pass {rnd}: {e:.2e}")
            assert e < TOL, (maps, path, l, e)
    net.close()


# ------------------------------------------------------------------------------------------
# 2. round trip: infer(hidden_pair = l) then decode == the reconstruction of the same infer call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64-4pairs", "256-4pairs", "cfg2", "no-pooling", "640x480-opform", "640x480", "5x3", "D4"])
def test_round_trip(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    for l in range(len(ws)):
        g = net.dims[l]
        rec = ctx.empty(net.B, net.D, net.Nx, net.Ny); rec.fill_(float("nan"))
        hid = ctx.empty(net.B, g["dM"], g["Nx"], g["Ny"]); hid.fill_(float("nan"))
        net.infer(frames, rec, l, hid)
        out = _decode(ctx, net, hid, l)
        e = relerr(out, host(rec))
        print(f"{name} pair {l}: round trip {e:.2e}")
        assert e < TOL, (name, l, e)
    net.close()


# ------------------------------------------------------------------------------------------
# 3. the 8-bit output rule, exactly
# ------------------------------------------------------------------------------------------
HALVES = [-7.5, -0.5, 0.5, 1.5, 2.5, 100.5, 254.5, 255.5, 300.25, 77.0]


@pytest.mark.parametrize("Nx,Ny,smooth", [(64, 256, False), (240, 320, True)])
def test_u8_output_rule_is_exact(ctx, flags, Nx, Ny, smooth):
    """a power-of-two net and a mixed-radix net (the geometry of test_gpu_infer's 240x320-opform), both in the operator form"""
    flags()
    B, D, maps, s = 2, 3, [4, 3], 2
    L = len(maps)
    rng = np.random.default_rng(Nx + Ny)
    mk = lambda: F.track(aefft.Net(ctx, D, Nx, Ny, maps, 3, s, batch=B, smooth_sizes=smooth, operator_form=smooth))
    shape = lambda l: (B, maps[l], Nx // s ** (l + 1), Ny // s ** (l + 1))
    # (a) constant planes: zero decoder kernels of pair 0 leave recon[d] = p_0[d] / s^2 whatever the code holds.  Built on the CPU first: the
    # candidates that survive the library's float32 scale 1/(Nx Ny) exactly -- one below 0, one above 255, one exactly on .5 inside
    N = np.float32(Nx) * np.float32(Ny)
    inv = np.float32(1.0) / N
    keep = [v for v in HALVES if np.float32(np.float32(v) * N) * inv == np.float32(v)]
    pick = [[v for v in keep if v < 0][0], [v for v in keep if v > 255][0], [v for v in keep if 0 < v < 255 and v % 1 == 0.5][0]]
    net = mk()
    assert net.step_form() == "operator_chain"
    ws = _weights(rng, D, maps, 3, 3)
    ws[0] = (ws[0][0], ws[0][1], np.zeros_like(ws[0][2]), np.array(pick) * s * s)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    for l in range(L):
        code = rng.uniform(-50, 300, shape(l))
        img_f = _decode(ctx, net, code, l)
        img_8 = _decode(ctx, net, code, l, u8=True)
        frac = np.abs(img_f) % 1
        assert (img_f < 0).any() and (img_f > 255).any() and ((frac == 0.5) & (img_f > 0) & (img_f < 255)).any(), (Nx, l)
        assert np.array_equal(img_8, _rule(img_f)), (Nx, l)
    net.close()
    # (b) a random net whose image spills over both ends.  Built on the CPU first: the float64 oracle's image r0 of frame 0's code with
    # p_0 = 0, and -- the image being linear in f_0 and p_0 (which enters as p_0 / s^2) -- pair 0's decoder scaled per channel so that the
    # image spans [-128, 384]
    net = mk()
    ws = _weights(rng, D, maps, 3, 3)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    for l in range(L):
        code = q32(rng.uniform(0, 256, shape(l)))
        c0, b0, f0, _ = ws[0]
        r0 = _decode_oracle(code[0], [(c0, b0, f0, np.zeros(D))] + ws[1:], [s] * L, l)
        lo, hi = r0.min(axis=(1, 2)), r0.max(axis=(1, 2))
        assert (hi - lo > 1e-3 * np.abs(r0).max()).all(), (lo, hi)
        a = 512.0 / (hi - lo)
        wl = [(c0, b0, q32(f0 * a[:, None, None, None]), q32((-128.0 - a * lo) * s * s))] + ws[1:]
        for j, w in enumerate(wl):
            net.set_pair(j, *w)
        img_f = _decode(ctx, net, code, l)
        img_8 = _decode(ctx, net, code, l, u8=True)
        assert (img_f < 0).any() and (img_f > 255).any() and ((img_f > 1) & (img_f < 254)).any(), (Nx, l, img_f.min(), img_f.max())
        assert np.array_equal(img_8, _rule(img_f)), (Nx, l)
    # NaN -> 0
    net.set_pair(0, wl[0][0], wl[0][1], wl[0][2], np.array([np.nan, 1.0, 2.0]))
    img_8 = _decode(ctx, net, code, L - 1, u8=True)
    assert (img_8[:, 0] == 0).all()
    net.close()


# ------------------------------------------------------------------------------------------
# 4. training is undisturbed
# ------------------------------------------------------------------------------------------
def _decode_streamed(name, ctx, net, steps):
    """[step, decode, step, decode(8-bit, another pair), step]"""
    L = net.npairs
    codes = [ctx.dev(_codes(name, 0)[0]), ctx.dev(_codes(name, L - 1)[0])]
    img32, img8 = ctx.empty(net.B, net.D, net.Nx, net.Ny), ctx.empty(net.B, net.D, net.Nx, net.Ny, dtype=torch.uint8)

    def hook(k, x):
        if k == 0:
            net.decode(codes[0], 0, img32)
        if k == 1:
            net.decode(codes[1], L - 1, img8)
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed(ctx, flags, name, path, form, ready):
    """[step, decode, step, decode, step] against [step, step, step]: reconstructions, packed gradients with their MSE tail, MSEs and
    weights bit for bit"""
    flags(path)
    assert F.net(ctx, name).step_form() == form
    setup = functools.partial(_decode_streamed, name)
    plain = _train_streamed(ctx, name, ready, setup, False)
    mixed = _train_streamed(ctx, name, ready, setup, True)
    assert len(plain) == len(mixed)
    for i, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a, b), i
    L = len(CASES[name][3])
    assert np.isfinite(plain[5][-L:]).all() and (plain[5][-L:] > 0).all()      # the tail of the third step's buffer: the second step's MSE


# ------------------------------------------------------------------------------------------
# 5. the cache, by launch counts
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOCHAIN"])
def test_the_operator_is_cached_until_the_weights_or_the_pair_change(ctx, flags, path):
    """`moment` (the operator-form helpers' id) counts decode_op (1, when the operator is formed) and decode_apply (1)"""
    flags(path)
    name = "256-4pairs"
    ws, _ = _case(name)
    L = len(ws)
    s = _scales(CASES[name][6], L)
    net = F.net(ctx, name)
    code1, ref1 = _codes(name, 1)
    code2, ref2 = _codes(name, 2)
    _counted = lambda ctx, net, code, l: F.counted(ctx, lambda: _decode(ctx, net, code, l))

    def cached(c):
        assert c["moment"] == 1 and c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0, c
        assert c["r2c_rows"] == 1 and c["c2r_rows"] == 1, c

    out, c = _counted(ctx, net, code1, 1)
    assert relerr(out, ref1) < TOL and c["moment"] == 2, c
    out, c = _counted(ctx, net, code1, 1)              # unchanged weights, the same pair: five launches
    assert relerr(out, ref1) < TOL
    cached(c)
    out, c = _counted(ctx, net, code2, 2)              # another pair: its operator
    assert relerr(out, ref2) < TOL and c["moment"] == 2 and c["chain"] == 0 and c["contract"] == 0, c
    out, c = _counted(ctx, net, code2, 2)
    cached(c)
    # set_pair: the operator is formed again, and the result follows the new weights
    wsb = [w if l != 3 else tuple(0.5 * a for a in w) for l, w in enumerate(ws)]
    net.set_pair(3, *wsb[3])
    refb = np.stack([_decode_oracle(x, wsb, s, 2) for x in code2])
    out, c = _counted(ctx, net, code2, 2)
    assert relerr(out, refb) < TOL and c["moment"] == 2, c
    out, c = _counted(ctx, net, code2, 2)
    assert relerr(out, refb) < TOL
    cached(c)
    # step_apply: the weights change again
    frames = ctx.dev(_case(name)[1][0])
    net.step_grad(frames); net.step_apply(0.02); ctx.sync()
    wsc = [tuple(a.astype(np.float64) for a in net.get_pair(l)) for l in range(L)]
    refc = np.stack([_decode_oracle(x, wsc, s, 2) for x in code2])
    out, c = _counted(ctx, net, code2, 2)
    assert relerr(out, refc) < TOL and c["moment"] == 2, c
    out, c = _counted(ctx, net, code2, 2)
    assert relerr(out, refc) < TOL
    cached(c)
    net.close()


# ------------------------------------------------------------------------------------------
# 6. state and errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_and_state(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    L = len(ws)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    rec = ctx.empty(net.B, net.D, net.Nx, net.Ny)
    pad = ctx.empty(rec.numel() + 4)
    code = ctx.dev(_codes(name, 1)[0])
    cpad = ctx.empty(code.numel() + 4)
    for args in ((code, -1, rec), (code, L, rec), (None, 1, rec), (code, 1, None), (cpad[1:], 1, rec), (code, 1, pad[1:])):
        with pytest.raises(aefft.AefftError) as ei:
            net.decode(*args)
        assert f"aefft error {aefft.EINVAL}:" in str(ei.value), ei.value
    # the call ends a pending step_grad
    net.step_grad(frames)
    net.decode(code, 1, rec)
    with pytest.raises(aefft.AefftError) as ei:
        net.step_apply(0.02)
    assert f"aefft error {aefft.ESTATE}:" in str(ei.value), ei.value
    # no frame stands behind a decode: the layer exports wait for the next forward
    with pytest.raises(aefft.AefftError) as ei:
        net.get_layer(2)
    assert f"aefft error {aefft.ESTATE}:" in str(ei.value), ei.value
    with pytest.raises(aefft.AefftError) as ei:
        net.get_layers()
    assert f"aefft error {aefft.ESTATE}:" in str(ei.value), ei.value
    _infer(ctx, net, frames, 1)
    assert np.isfinite(host(net.get_layer(2))).all()
    net.close()


# ------------------------------------------------------------------------------------------
# 7. spatial net
# ------------------------------------------------------------------------------------------
def _sp_pool(x, s):
    """Pool(s > 0), netlib.cpp:114-164: max(0, trunc(window maximum))"""
    ch, nx, ny = x.shape
    return np.trunc(np.maximum(x.reshape(ch, nx // s, s, ny // s, s).max(axis=(2, 4)), 0))


def _sp_decode_oracle(code, ws, s, l):
    """np_spatial: the coordinate-space sequence from layer 2l+2 of one frame"""
    L = len(ws)
    h = np.asarray(code, np.float64)
    for j in range(l + 1, L):
        h = S.conv(_sp_pool(h, s), ws[j][0], ws[j][1])
    for j in range(L - 1, -1, -1):
        h = np.repeat(np.repeat(S.conv(h, ws[j][2], ws[j][3]), s, axis=1), s, axis=2)
    return h


def test_spatial_net(ctx, flags):
    """the net of test_gpu_infer.py::test_spatial_net"""
    flags()
    rng = np.random.default_rng(3)
    D, N, maps, B, s = 3, 64, [4, 6], 2, 2
    net = F.track(aefft.Net(ctx, D, N, N, maps, 3, s, B, spatial=True))
    ws = _weights(rng, D, maps, 3, 3)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    for l in range(len(maps)):
        n = N // s ** (l + 1)
        code = rng.uniform(-64, 192, (B, maps[l], n, n)).astype(np.float32).astype(np.float64)
        ref = np.stack([_sp_decode_oracle(c, ws, s, l) for c in code])
        rec = _decode(ctx, net, code, l)
        e = relerr(rec, ref)
        print(f"spatial pair {l}: {e:.2e}")
        assert e < TOL, (l, e)
    u8 = torch.zeros(B, D, N, N, dtype=torch.uint8, device=ctx.dev(np.zeros(4)).device)
    with pytest.raises(aefft.AefftError) as ei:
        net.decode(ctx.dev(code), len(maps) - 1, u8)
    assert f"aefft error {aefft.EINVAL}:" in str(ei.value), ei.value
    net.close()
