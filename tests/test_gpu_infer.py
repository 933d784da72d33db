"""aefft_net_infer (Net.infer): frozen-weight inference over a batch -- reconstruction and every hidden pair's layer against the float64
oracle in every form and route, infer == forward, the 8-bit output rule exactly on every row-pass route, 8-bit input bit for bit,
training undisturbed bit for bit, the operator cache by the profiler's launch counts, layer exports, the spatial net and the errors."""
import importlib

import numpy as np
import pytest
import torch

import frozen_cases as F
from frozen_cases import CASES, PATHS, _case, _oracle, _oracle_layers, _rule, _scales, _weights, host, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

TOL = 1e-4      # the bound _check_two_steps holds the step's reconstruction to
ORDER = ["64-1pair", "64-2pairs", "64-4pairs", "256-1pair", "256-2pairs", "256-4pairs", "cfg2", "no-pooling", "640x480", "640x480-opform", "240x320",
         "240x320-opform", "5x3", "D4", "tied"]


def _infer(ctx, net, frames, pair=None, recon=True, u8=False):
    """one Net.infer: (reconstruction or None, hidden layer or None) as host arrays; the outputs start as NaN / 0xAA"""
    rec = hid = None
    if recon:
        rec = ctx.empty(net.B, net.D, net.Nx, net.Ny, dtype=torch.uint8 if u8 else None)
        rec.fill_(0xAA if u8 else float("nan"))
    if pair is not None:
        g = net.dims[pair]
        hid = ctx.empty(net.B, g["dM"], g["Nx"], g["Ny"]); hid.fill_(float("nan"))
    net.infer(frames, rec, pair, hid)
    ctx.sync()
    return (None if rec is None else host(rec).copy()), (None if hid is None else host(hid).copy())


def _check_against_oracle(ctx, net, name, k=0):
    ws, xs = _case(name)
    ref = _oracle(name, k)
    frames = ctx.dev(xs[k])
    L = len(ws)
    for l in range(L):
        rec, hid = _infer(ctx, net, frames, l)
        e_r = relerr(rec, np.stack([q[-1] for q in ref]))
        e_h = relerr(hid, np.stack([q[2 * l + 2] for q in ref]))
        print(f"{name} pair {l}: recon {e_r:.2e} hidden {e_h:.2e}")
        assert e_r < TOL, (name, l, e_r)
        assert e_h < TOL, (name, l, e_h)


# ------------------------------------------------------------------------------------------
# 1. against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ORDER)
def test_infer_against_the_oracle(ctx, flags, name, path):
    flags(path)
    net = F.net(ctx, name)
    want = CASES[name][-1]
    if path == "NOOPFORM":
        want = "per_frame"
    elif path == "NOCHAIN" and want == "operator_chain":
        want = "operator"
    assert net.step_form() == want
    _check_against_oracle(ctx, net, name)
    # a second pass over the pairs, now from the cached operators
    _check_against_oracle(ctx, net, name)
    net.close()


# ------------------------------------------------------------------------------------------
# 2. infer == forward + get_layer; layer exports after infer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64-2pairs", "256-4pairs", "no-pooling", "640x480-opform", "640x480", "5x3", "D4"])
def test_infer_equals_forward(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    D, Nx, Ny, maps, *_ = CASES[name]
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    rec_f = ctx.empty(net.B, D, Nx, Ny)
    net.forward(frames, rec_f)
    layers_f = [host(t).copy() for t in net.get_layers()]
    rec_f = host(rec_f).copy()
    per_frame = net.step_form() == "per_frame"
    for l in range(len(maps)):
        rec, hid = _infer(ctx, net, frames, l)
        assert relerr(rec, rec_f) < TOL and relerr(hid, layers_f[2 * l + 2]) < TOL, (name, l)
        if per_frame:
            assert np.array_equal(rec, rec_f), (name, l, np.abs(rec - rec_f).max())
    # the layers aefft_net_get_layer(s) export after infer are those of the call
    _infer(ctx, net, frames, None)
    layers_i = [host(t).copy() for t in net.get_layers()]
    for i, (a, b) in enumerate(zip(layers_i, layers_f)):
        assert relerr(a, b) < TOL, (name, i)
    net.close()


# ------------------------------------------------------------------------------------------
# 3. the 8-bit output rule, exactly, on every row-pass route
# ------------------------------------------------------------------------------------------
# the power-of-two row pass: every N of RowCfg, dense (no pooling) and -- N >= 128, Wc <= N/16 -- sparse (pooling by 8);
# the mixed-radix row pass: one size per thread class T = 16 .. 256 (N <= 8 T), Wc = N/2 and Wc < N/2
ROW_ROUTES = ([("pow2-dense", 16, n, 1) for n in (8, 16, 32, 64, 128, 256, 512, 1024, 2048)] +
              [("pow2-sparse", 64, n, 8) for n in (128, 256, 512, 1024, 2048)] +
              [("mixed-dense", 40, n, 1) for n in (120, 240, 480, 960, 1920)] +
              [("mixed-sparse", 40, n, 2) for n in (120, 240, 480, 960, 1920)])
HALVES = [-7.5, -0.5, 0.5, 1.5, 2.5, 100.5, 254.5, 255.5, 300.25, 77.0]


@pytest.mark.parametrize("route,Nx,Ny,s", ROW_ROUTES)
def test_u8_output_rule_is_exact(ctx, flags, route, Nx, Ny, s):
    flags()
    smooth = route.startswith("mixed")
    B = 2
    rng = np.random.default_rng(Nx + Ny + s)
    # (a) constant planes: zero kernels leave recon[d] = p[d] / s^2 (the DC bin alone, zero-padded up from the pooled grid).  Built on the CPU first: the candidates that survive the
    # library's float32 scale 1/(Nx Ny) exactly, so that values below 0, above 255 and exactly on .5 are in the float image
    N = np.float32(Nx) * np.float32(Ny)
    inv = np.float32(1.0) / N
    keep = [v for v in HALVES if np.float32(np.float32(v) * N) * inv == np.float32(v)]
    assert any(v < 0 for v in keep) and any(v > 255 for v in keep) and any(v > 0 and v % 1 == 0.5 for v in keep), keep
    D = len(keep)
    net = F.track(aefft.Net(ctx, D, Nx, Ny, [2], 3, s, batch=B, smooth_sizes=smooth))
    z = lambda *sh: np.zeros(sh)
    net.set_pair(0, z(2, D, 3, 3), z(2), z(D, 2, 3, 3), np.array(keep) * s * s)
    frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))))
    img_f, _ = _infer(ctx, net, frames)
    img_8, _ = _infer(ctx, net, frames, u8=True)
    frac = np.abs(img_f) % 1
    assert (img_f < 0).any() and (img_f > 255).any() and ((frac == 0.5) & (img_f > 0) & (img_f < 255)).any(), route
    assert np.array_equal(img_8, _rule(img_f)), (route, Ny)
    net.close()
    # (b) a random net whose image spills over both ends, every pixel of every word in its place.  Built on the CPU first: frames with a
    # ramp under the noise (pooling keeps it), the float64 oracle's image r0 of frame 0 with p = 0, and -- the image being linear in f and p (which enters as p / s^2) --
    # the decoder scaled per channel so that frame 0's image spans [-128, 384]
    D = 3
    net = F.track(aefft.Net(ctx, D, Nx, Ny, [2], 3, s, batch=B, smooth_sizes=smooth))
    c, b, f, p = _weights(rng, D, [2], 3, 3)[0]
    ramp = np.add.outer(np.arange(Nx) / (Nx - 1.0), np.arange(Ny) / (Ny - 1.0)) / 2
    px = np.floor(255.0 * (0.75 * ramp + 0.25 * rng.uniform(0, 1, (B, D, Nx, Ny))))
    r0 = _oracle_layers(px[0], [(c, b, f, np.zeros(D))], [s])[-1]
    lo, hi = r0.min(axis=(1, 2)), r0.max(axis=(1, 2))
    assert (hi - lo > 1e-3 * np.abs(r0).max()).all(), (lo, hi)
    a = 512.0 / (hi - lo)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    f, p = q32(f * a[:, None, None, None]), q32((-128.0 - a * lo) * s * s)
    net.set_pair(0, c, b, f, p)
    frames = ctx.dev(px)
    img_f, _ = _infer(ctx, net, frames)
    img_8, _ = _infer(ctx, net, frames, u8=True)
    assert (img_f < 0).any() and (img_f > 255).any() and ((img_f > 1) & (img_f < 254)).any(), (route, img_f.min(), img_f.max())
    assert np.array_equal(img_8, _rule(img_f)), (route, Ny)
    # NaN -> 0
    net.set_pair(0, c, b, f, np.array([np.nan, 1.0, 2.0]))
    img_8, _ = _infer(ctx, net, frames, u8=True)
    assert (img_8[:, 0] == 0).all()
    net.close()


# ------------------------------------------------------------------------------------------
# 4. 8-bit input
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["256-4pairs", "640x480-opform", "640x480", "5x3"])
def test_u8_frames_give_the_float_frames_results_bit_for_bit(ctx, flags, name):
    """(640 x 480: the mixed-radix row pass converts 8-bit pixels on load as well -- the smooth case the header's sentence is pinned by)"""
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    f32 = ctx.dev(xs[0])
    u8 = torch.as_tensor(xs[0].astype(np.uint8), device=f32.device)
    for l in range(len(ws)):
        a = _infer(ctx, net, f32, l)
        b = _infer(ctx, net, u8, l)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, l)
        a8 = _infer(ctx, net, f32, None, u8=True)[0]
        b8 = _infer(ctx, net, u8, None, u8=True)[0]
        assert np.array_equal(a8, b8) and np.array_equal(a8, _rule(a[0]))
    net.close()


# ------------------------------------------------------------------------------------------
# 5. training is undisturbed
# ------------------------------------------------------------------------------------------
def _infer_between(ctx, net, steps):
    """behind the first step its own frames and pair 0, behind the second other frames, pair 1 % L and the 8-bit output"""
    others = [ctx.dev(o) for o in F.other_frames(steps[0].shape)]

    def hook(k, x):
        if k < 2:
            _infer(ctx, net, x if k == 0 else others[k], k % net.npairs, u8=bool(k))
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed(ctx, flags, name, path, form, ready):
    """[step, step, step] against [step, infer, step, infer(other frames), step]: reconstructions, packed gradients with their MSE tail,
    MSEs and weights after every step bit for bit (the momenta enter the next step's weights: there is no accessor of their own)"""
    flags(path)
    plain = F.train(ctx, name, ready, _infer_between)
    mixed = F.train(ctx, name, ready, _infer_between, at="readback")
    F.assert_same_training(plain, mixed)


def _train_streamed(ctx, name, ready, setup, mixed):
    """three steps with nothing between the calls that waits for the device or asks for the deferred MSE sums: every buffer exists up front,
    the packed buffer is copied on the library's stream, and results are read back after the last step alone.  setup(ctx, net, steps) makes
    the buffers of the interleaved calls, in both runs, and returns hook(k, x); mixed: it runs straight behind step_apply, straight in front
    of the next step_grad"""
    ws, xs = _case(name)
    L = len(ws)
    net = F.net(ctx, name)
    if ready:
        net.set_input_ready(True)
    steps = [ctx.dev(xs[0]), ctx.dev(xs[1]), ctx.dev(xs[0])]
    recons = [ctx.empty(net.B, net.D, net.Nx, net.Ny) for _ in steps]
    hook = setup(ctx, net, steps)
    gbuf = net.grad_buffer()
    grads = [torch.empty_like(gbuf) for _ in steps]
    ctx.sync()
    for k, x in enumerate(steps):
        net.step_grad(x, recons[k])
        grads[k].copy_(gbuf)                      # (in stream order: the gradients, and the MSE tail the previous step's sums rode in on)
        net.step_apply(0.02)                      # mse = None: the sums stay deferred
        if mixed:
            hook(k, x)
    ctx.sync()
    mse = ctx.empty(L); net.last_mse(mse); ctx.sync()
    out = [host(r).copy() for r in recons] + [host(g).copy() for g in grads] + [host(mse).copy()]
    out += [a for l in range(L) for a in net.get_pair(l)]
    net.close()
    return out


def _infer_streamed(ctx, net, steps):
    L = net.npairs
    other = F.u8(ctx, F.other_frames(steps[0].shape)[0], steps[0])
    img32, img8 = ctx.empty(net.B, net.D, net.Nx, net.Ny), ctx.empty(net.B, net.D, net.Nx, net.Ny, dtype=torch.uint8)
    g0, g1 = net.dims[0], net.dims[L - 1]
    hid0, hid1 = ctx.empty(net.B, g0["dM"], g0["Nx"], g0["Ny"]), ctx.empty(net.B, g1["dM"], g1["Nx"], g1["Ny"])

    def hook(k, x):
        if k == 0:
            net.infer(x, img32, 0, hid0)
        if k == 1:
            net.infer(other, img8, L - 1, hid1)
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed_without_synchronisation(ctx, flags, name, path, form, ready):
    """the same comparison with the calls issued back to back: infer runs while the deferred MSE sums of the step before are outstanding (they
    reach the next step's packed-buffer tail through its gradient launch, across the infer) and, with set_input_ready(1), while the next
    step's input transform may run ahead on its side stream into the other input-spectra buffer"""
    flags(path)
    assert F.net(ctx, name).step_form() == form
    plain = _train_streamed(ctx, name, ready, _infer_streamed, False)
    mixed = _train_streamed(ctx, name, ready, _infer_streamed, True)
    assert len(plain) == len(mixed)
    for i, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a, b), i
    L = len(CASES[name][3])
    assert np.isfinite(plain[5][-L:]).all() and (plain[5][-L:] > 0).all()      # the tail of the third step's buffer: the second step's MSE


@pytest.mark.parametrize("path,form", [("NOCHAIN", "operator"), ("", "operator_chain")])
def test_infer_behind_a_pending_step_grad_and_export_behind_a_hidden_layer(ctx, flags, path, form):
    """infer that ends a pending step_grad (operator form without the chain: the step's own operators are reused) against the oracle, then
    every layer export behind a call that asked for a hidden layer"""
    flags(path)
    name = "256-4pairs"
    ws, xs = _case(name)
    ref = _oracle(name)
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    assert net.step_form() == form
    net.step_grad(frames)
    for l in (1, 2):
        rec, hid = _infer(ctx, net, frames, l)
        assert relerr(rec, np.stack([q[-1] for q in ref])) < TOL, (path, l)
        assert relerr(hid, np.stack([q[2 * l + 2] for q in ref])) < TOL, (path, l)
        layers = [host(t).copy() for t in net.get_layers()]
        assert len(layers) == len(ref[0])
        for i, a in enumerate(layers):
            assert relerr(a, np.stack([q[i] for q in ref])) < TOL, (path, l, i)
    with pytest.raises(Exception):
        net.step_apply(0.02)
    net.close()


# ------------------------------------------------------------------------------------------
# 6. the cache, by launch counts
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOCHAIN"])
def test_operators_are_cached_until_the_weights_change(ctx, flags, path):
    """a pooled net (no expand launch): `moment` (the operator-form helpers' id) counts the hidden-operator kernel (1) and the expansion of the hidden planes (1)"""
    flags(path)
    name = "256-4pairs"
    ws, xs = _case(name)
    L = len(ws)
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    chain = path == ""
    heavy = ("chain", "kspec") if chain else ("contract", "kspec")
    ref = _oracle(name)
    _counted = lambda ctx, net, frames, pair: F.counted(ctx, lambda: _infer(ctx, net, frames, pair))

    def ok(out, l, ref=ref):
        assert relerr(out[0], np.stack([q[-1] for q in ref])) < TOL and relerr(out[1], np.stack([q[2 * l + 2] for q in ref])) < TOL

    out, c = _counted(ctx, net, frames, 1)
    ok(out, 1)
    assert c[heavy[0]] >= 1 and c["moment"] == 2, c
    out, c = _counted(ctx, net, frames, 1)             # unchanged weights: the two transforms, and the hidden planes
    ok(out, 1)
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0 and c["moment"] == 1, c
    assert c["r2c_rows"] == 1 and c["c2r_rows"] == 2, c
    out, c = _counted(ctx, net, frames, 2)             # another pair: its operator, nothing of the chain
    ok(out, 2)
    assert c["chain"] == 0 and c["contract"] == 0 and c["moment"] == 2, c
    out, c = _counted(ctx, net, frames, None)          # the reconstruction alone
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0 and c["moment"] == 0 and c["c2r_rows"] == 1, c
    # set_pair: everything comes back, and the results follow the new weights
    ws2 = [w if l != 1 else tuple(0.5 * a for a in w) for l, w in enumerate(ws)]
    net.set_pair(1, *ws2[1])
    s = _scales(CASES[name][6], L)
    ref2 = [_oracle_layers(x, ws2, s) for x in xs[0]]
    out, c = _counted(ctx, net, frames, 2)
    ok(out, 2, ref2)
    assert c[heavy[0]] >= 1 and c["moment"] == 2, c
    # step_apply: the weights change again (in the chain form the step's last launch has carried the chain ahead)
    net.step_grad(frames); net.step_apply(0.02); ctx.sync()
    ws3 = [net.get_pair(l) for l in range(L)]
    ref3 = [_oracle_layers(x, [tuple(a.astype(np.float64) for a in w) for w in ws3], s) for x in xs[0]]
    out, c = _counted(ctx, net, frames, 2)
    ok(out, 2, ref3)
    assert c["moment"] == 2, c
    if not chain:
        assert c["contract"] >= 1, c
    out, c = _counted(ctx, net, frames, 2)
    ok(out, 2, ref3)
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0 and c["moment"] == 1, c
    net.close()


# ------------------------------------------------------------------------------------------
# 7. spatial net, errors, state
# ------------------------------------------------------------------------------------------
def test_spatial_net(ctx, flags):
    flags()
    rng = np.random.default_rng(3)
    D, N, maps, B = 3, 64, [4, 6], 2
    net = F.track(aefft.Net(ctx, D, N, N, maps, 3, 2, B, spatial=True))
    for l, w in enumerate(_weights(rng, D, maps, 3, 3)):
        net.set_pair(l, *w)
    frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, N, N))))
    rec_f = ctx.empty(B, D, N, N)
    net.forward(frames, rec_f)
    hid_f = host(net.get_layer(4)).copy()
    rec, hid = _infer(ctx, net, frames, 1)
    assert np.array_equal(rec, host(rec_f)) and np.array_equal(hid, hid_f)
    u8 = torch.zeros(B, D, N, N, dtype=torch.uint8, device=frames.device)
    with pytest.raises(Exception):
        net.infer(u8, rec_f)
    with pytest.raises(Exception):
        net.infer(frames, u8)
    net.close()


def test_argument_errors_and_state(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    rec = ctx.empty(net.B, net.D, net.Nx, net.Ny)
    hid = ctx.empty(net.B, 3, 16, 16)
    for args in ((None, rec), (frames, None), (frames, rec, 2, hid), (frames, rec, -1, hid), (frames.reshape(-1)[1:], rec),
                 (frames, rec.reshape(-1)[1:])):
        with pytest.raises(Exception):
            net.infer(*args)
    # the call ends a pending step_grad
    net.step_grad(frames)
    net.infer(frames, rec)
    with pytest.raises(Exception):
        net.step_apply(0.02)
    net.close()
