"""What the tests of the frozen-weight calls share (test_gpu_infer, _decode, _score, _score_map, _score_target, _ssim, _weight_caches), each
once: the table of cases with its seeded weights and frames, the float64 oracle of a case, the list of open nets with the fixture that closes
them, the module's context, and the three-step training run that a call is interleaved with.  A plain module -- pytest collects nothing from
it; a test file imports the fixtures `ctx` and `_close_nets` into its own namespace.  The runner of each call (_infer, _score, ...) stays in
the file of that call."""
import functools
import importlib

import numpy as np
import pytest
import torch

import np_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")

q32 = lambda a: np.asarray(a, np.float32).astype(np.float64)


def relerr(got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def host(t):
    return t.detach().cpu().numpy()


def _weights(rng, D, maps, Nk, Nl):
    ws, dD = [], D
    for dM in maps:
        ws.append((q32(rng.uniform(-1, 1, (dM, dD, Nk, Nl))), q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, (dD, dM, Nk, Nl))),
                   q32(rng.uniform(-1, 1, dD))))
        dD = dM
    return ws


# ------------------------------------------------------------------------------------------
# the context and the open nets
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


_LIVE = []


def track(net):
    _LIVE.append(net)
    return net


@pytest.fixture(autouse=True)
def _close_nets(ctx):
    """every net of a test is destroyed before the module's context is, also when an assertion ends the test early (a net that outlives
    its context is destroyed by the garbage collector through a dangling context pointer)"""
    yield
    while _LIVE:
        _LIVE.pop().close()


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
# name: D, Nx, Ny, maps, Nk, Nl, scale, B, smooth_sizes, operator_form, tied, the form under the default switches (None: recorded, not asserted).
# Every file lists the names it runs (ORDER, OWN, DECODE_CASES, NAMES)
CASES = {
    "64-1pair": (3, 64, 64, [4], 5, 5, 2, 2, False, False, False, "operator_chain"),
    "64-2pairs": (3, 64, 64, [4, 3], 5, 5, 2, 3, False, False, False, "operator_chain"),
    "64-4pairs": (3, 64, 64, [4, 3, 4, 2], 3, 3, [2, 2, 1, 1], 2, False, False, False, "operator_chain"),
    "256-1pair": (3, 256, 256, [4], 5, 5, 2, 2, False, False, False, "operator_chain"),
    "256-2pairs": (1, 256, 256, [3, 4], 3, 3, 2, 2, False, False, False, "operator_chain"),
    "256-4pairs": (3, 256, 256, [4, 3, 4, 2], 5, 5, 2, 2, False, False, False, "operator_chain"),
    "cfg2": (3, 256, 256, [8, 16, 32], 5, 5, 2, 1, False, False, False, "operator_chain"),
    # 8*3*512*257*8 B = 25 MB > 16 MB: the expand route (and a coarsest grid beyond the chain launch's 16384 bins)
    "no-pooling": (3, 512, 512, [4], 5, 5, 1, 8, False, False, False, "operator"),
    "640x480": (3, 640, 480, [4, 3], 5, 5, 2, 2, True, False, False, "per_frame"),
    "640x480-opform": (3, 640, 480, [4, 3], 5, 5, 2, 2, True, True, False, "operator_chain"),
    "240x320": (3, 240, 320, [4, 3], 3, 3, 2, 2, True, False, False, "per_frame"),
    "240x320-opform": (3, 240, 320, [4, 3], 3, 3, 2, 2, True, True, False, "operator_chain"),
    "5x3": (3, 64, 64, [4, 3], 5, 3, 2, 2, False, False, False, "per_frame"),
    "D4": (4, 64, 64, [4, 3], 5, 5, 2, 2, False, False, False, "per_frame"),
    "tied": (3, 64, 64, [4, 3], 5, 5, 2, 2, False, False, True, "operator_chain"),
    # the per-frame score
    "64x128": (3, 64, 128, [4], 3, 3, 2, 2, False, False, False, "operator_chain"),       # rows and columns not interchangeable
    "10x24": (1, 10, 24, [2], 3, 3, 1, 3, True, False, False, "per_frame"),               # 5 row pairs per frame: partials across workgroup boundaries
    # the per-tile maps
    "24x40": (1, 24, 40, [2], 3, 3, 1, 3, True, False, False, None),        # mixed radix, T = 16; 12 row pairs per plane cross workgroup boundaries; the second j holds 4 live lanes of 16; only tile 8
    "8x1024": (1, 8, 1024, [2], 3, 3, 1, 1, False, False, False, None),     # a row pair is the whole workgroup
    "8x2048": (1, 8, 2048, [2], 3, 3, 1, 1, False, False, False, None),     # two positions per lane in different strips
    "64x192": (1, 64, 192, [2], 3, 3, 1, 1, True, False, False, None),      # T = 32 with tile 64: 32-lane segments
    "16x640": (1, 16, 640, [2], 3, 3, 1, 1, True, False, False, None),      # T = 128
    "16x1280": (1, 16, 1280, [2], 3, 3, 1, 1, True, False, False, None),    # T = 256
}
PATHS = ["", "NOOPFORM", "NOCHAIN", "NOOVERLAP", "GTAPS"]
TILES = (8, 16, 32, 64)


def _scales(s, L):
    return [s] * L if isinstance(s, int) else list(s)


def tiles(name):
    """every tile that divides both axes"""
    _, Nx, Ny, *_ = CASES[name]
    return [t for t in TILES if Nx % t == 0 and Ny % t == 0]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(weights, two batches of frames), seeded by the name: shared by every test, never written to"""
    D, Nx, Ny, maps, Nk, Nl, s, B, *_rest, tied, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    ws = _weights(rng, D, maps, Nk, Nl)
    if tied:        # decoder kernels are the encoder's, transposed over the channel pair
        ws = [(c, b, np.ascontiguousarray(c.transpose(1, 0, 2, 3)), p) for c, b, f, p in ws]
    xs = [np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))) for _ in range(2)]
    return ws, xs


def _oracle_layers(x, ws, scales):
    """np_ref.autoenc_fft (float64) of one frame: the list of layers 0..4L"""
    L = len(ws)
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]
    net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    return R.autoenc_fft(x, net_c, net_b, list(scales) + [-v for v in scales[::-1]])[0]


@functools.lru_cache(maxsize=None)
def _oracle(name, k=0):
    ws, xs = _case(name)
    s = _scales(CASES[name][6], len(ws))
    return [_oracle_layers(x, ws, s) for x in xs[k]]


@functools.lru_cache(maxsize=None)
def _oracle_recon(name):
    """the float64 oracle's reconstruction (layer 4L of np_ref.autoenc_fft) of the case's first batch, [B][D][Nx][Ny]"""
    return np.stack([q[-1] for q in _oracle(name)])


@functools.lru_cache(maxsize=None)
def _identity_case():
    """a one-pair net without pooling that nearly reproduces its input: c[m][d] = dM delta, f[d][m] = dD delta on the centre tap for m = d,
    plus 1e-3 of that everywhere, zero biases.  (The oracle's s_o is 2.6e-5 of the mean squared pixel: residual ~0.75 on pixels up to 255.)"""
    D, N, dM, Nk, B = 3, 64, 3, 3, 2
    rng = np.random.default_rng(4)
    c = np.zeros((dM, D, Nk, Nk)); f = np.zeros((D, dM, Nk, Nk))
    for m in range(dM):
        c[m, m, Nk // 2, Nk // 2] = dM; f[m, m, Nk // 2, Nk // 2] = D
    c = q32(c + 1e-3 * dM * rng.uniform(-1, 1, c.shape)); f = q32(f + 1e-3 * D * rng.uniform(-1, 1, f.shape))
    w = (c, np.zeros(dM), f, np.zeros(D))
    x = np.floor(rng.uniform(0, 256, (B, D, N, N)))
    rec_o = np.stack([_oracle_layers(xb, [w], [1])[-1] for xb in x])
    return (D, N, dM, Nk, B), w, x, rec_o


def net(ctx, name, ws=None):
    """the case's net, open until the test ends, with the case's weights or `ws`"""
    D, Nx, Ny, maps, Nk, Nl, s, B, smooth, opform, *_ = CASES[name]
    n = track(aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, batch=B, Nl=Nl, smooth_sizes=smooth, operator_form=opform))
    for l, w in enumerate(ws if ws is not None else _case(name)[0]):
        n.set_pair(l, *w)
    return n


def _form(net, name, path=""):
    """the form the net reports: asserted for the cases whose row names one, recorded for the others"""
    form, want = net.step_form(), CASES[name][-1]
    print(f"{name} {path}: step_form {form}")
    if want is None:
        return form
    if path == "NOOPFORM":
        want = "per_frame"
    elif path == "NOCHAIN" and want == "operator_chain":
        want = "operator"
    assert form == want, (name, path, form, want)
    return form


# ------------------------------------------------------------------------------------------
# small helpers
# ------------------------------------------------------------------------------------------
def nan(ctx, *shape):
    v = ctx.empty(*shape); v.fill_(float("nan"))
    return v


def u8(ctx, x, like):
    return torch.as_tensor(np.asarray(x).astype(np.uint8), device=like.device)


def _rule(v):
    """SpinToImage_C: clamp((int)round(v), 0, 255), halves away from zero, NaN -> 0"""
    v = np.asarray(v, np.float64)
    r = np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5))
    return np.clip(np.nan_to_num(r, nan=0.0), 0, 255).astype(np.uint8)


def counted(ctx, call):
    """(call(), {kernel id: launches the profiler counted during it})"""
    ctx.prof_enable(); ctx.prof_reset()
    out = call()
    counts = {k: v["launches"] for k, v in ctx.prof_read().items()}
    ctx.prof_enable(False)
    return out, counts


# ------------------------------------------------------------------------------------------
# training, with and without a frozen-weight call between the steps
# ------------------------------------------------------------------------------------------
def train(ctx, name, ready, setup, at=None):
    """three steps of the case's net, each read back: ([(reconstruction, packed gradients, MSEs, weights) per step], the packed buffer behind
    the last step).  setup(ctx, net, steps) allocates, in front of the first sync, what the interleaved calls need -- in the plain run (at =
    None) as well, so that both runs allocate alike -- and returns hook(k, x), the calls behind step k on its frames x.  Where the hook runs
    is part of what is tested: at = "apply" straight behind step_apply, before the sync, so that the deferred MSE sums are outstanding across
    the calls; at = "readback" after the step's results have been read back"""
    ws, xs = _case(name)
    L = len(ws)
    n = net(ctx, name)
    if ready:
        n.set_input_ready(True)
    steps = [ctx.dev(xs[0]), ctx.dev(xs[1]), ctx.dev(xs[0])]
    hook = setup(ctx, n, steps)
    ctx.sync()
    out = []
    for k, x in enumerate(steps):
        recon = ctx.empty(n.B, n.D, n.Nx, n.Ny)
        n.step_grad(x, recon)
        ctx.sync()
        g = host(n.grad_buffer()).copy()
        n.step_apply(0.02)                        # mse = None: the sums stay deferred across the calls
        if at == "apply":
            hook(k, x)
        ctx.sync()
        mse = ctx.empty(L); n.last_mse(mse); ctx.sync()
        out.append((host(recon).copy(), g, host(mse).copy(), [n.get_pair(l) for l in range(L)]))
        if at == "readback":
            hook(k, x)
    tail = host(n.grad_buffer()).copy()
    n.close()
    return out, tail


def other_frames(shape):
    """the two batches of 8-bit-valued pixels, unrelated to any case's, that the interleaved calls read"""
    rng = np.random.default_rng(5)
    return [np.floor(rng.uniform(0, 256, shape)) for _ in range(2)]


def assert_same_training(plain, mixed):
    """two results of train(): reconstructions, packed gradients with their MSE tail, MSEs and weights after every step bit for bit"""
    (plain, tail_p), (mixed, tail_m) = plain, mixed
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a[0], b[0]), (k, "recon")
        assert np.array_equal(a[1], b[1]), (k, "grads")
        assert np.array_equal(a[2], b[2]), (k, "mse")
        for l, (wa, wb) in enumerate(zip(a[3], b[3])):
            for u, v in zip(wa, wb):
                assert np.array_equal(u, v), (k, l)
    assert np.array_equal(tail_p, tail_m)
