"""Smooth sizes (even, no prime factor above 5: 640 x 480-class camera frames) on the GPU: the mixed-radix transforms against pocketfft,
the resident network created with AEFFT_NET_SMOOTH_SIZES against the float64 oracle, 8-bit frames, the creation rules and the reference's
own vector entry points at such a size."""
import ctypes as C
import importlib

import numpy as np
import pytest

import np_ref as R
from frozen_cases import _weights, q32  # noqa: F401  (defined there; the files that import them from here find them)
from test_gpu_fft_path import host, relerr, weight_step_tol
from test_shims import _p, wrap  # noqa: F401  (module fixture: the reference's entry points compiled against the product headers)

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------
# 1. transforms
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,planes", [(640, 480, 3), (480, 640, 2), (320, 240, 3), (1280, 720, 1), (2000, 16, 2), (10, 12, 5), (18, 30, 4),
                                          (640, 512, 2), (512, 480, 2)])
def test_mixed_radix_transforms_against_pocketfft(ctx, flags, Nx, Ny, planes):
    """R2C, C2R and a C2R of a spectrum that is not exactly Hermitian at the power-of-two path's bounds (2e-6 forward, 5e-6 inverse);
    2000 x 16 is beyond Bluestein's 1024, 640 x 512 and 512 x 480 mix a mixed-radix axis with a power-of-two one."""
    flags()
    rng = np.random.default_rng(Nx * 7 + Ny)
    x = np.floor(rng.uniform(0, 256, (planes, Nx, Ny))).astype(np.float32)
    ref = R.fft(x)
    assert relerr(host(ctx.r2c(ctx.dev(x))), ref) < 2e-6
    assert relerr(host(ctx.c2r(ctx.dev(ref), Ny)), R.fft_inv(ref, Nx, Ny)) < 5e-6
    Z = ref + 1e-3 * np.abs(ref).max() * (rng.normal(size=ref.shape) + 1j * rng.normal(size=ref.shape))
    assert relerr(host(ctx.c2r(ctx.dev(Z), Ny, scale=1.0)), R.c2r_unnorm(Z, Nx, Ny)) < 5e-6


@pytest.mark.parametrize("Nx,Ny", [(640, 480), (240, 320), (60, 36)])
def test_fused_pool_forms_at_smooth_sizes(ctx, flags, Nx, Ny):
    """r2c_pool / unpool_c2r by 2: the crop / zero-pad fused into the mixed-radix column and row passes, against R.pool_fft."""
    flags()
    rng = np.random.default_rng(Nx + Ny)
    x = np.floor(rng.uniform(0, 256, (2, Nx, Ny))).astype(np.float32)
    down, nx, ny = R.pool_fft(R.fft(x), Nx, Ny, 2)
    assert relerr(host(ctx.r2c_pool(ctx.dev(x), 2)), down) < 2e-6
    up, _, _ = R.pool_fft(down, nx, ny, -2)
    assert relerr(host(ctx.unpool_c2r(ctx.dev(down), ny, -2, 1.0 / (Nx * Ny))), R.fft_inv(up, Nx, Ny)) < 5e-6


@pytest.mark.parametrize("Nx,Ny,s", [(1280, 720, 2), (2000, 16, 2), (1920, 1080, 2)])
def test_pool_above_1024(ctx, Nx, Ny, s):
    """aefft_pool (only a resize) at smooth sizes beyond Bluestein's 1024: down and up, bit for bit against np_ref.resize."""
    rng = np.random.default_rng(Nx + s)
    X = (rng.normal(size=(2, Nx, Ny // 2 + 1)) + 1j * rng.normal(size=(2, Nx, Ny // 2 + 1))).astype(np.complex64)
    down, nx, ny = R.pool_fft(X.astype(np.complex128), Nx, Ny, s)
    Xd, gx, gy = ctx.pool(ctx.dev(X), Ny, s)
    assert (gx, gy) == (nx, ny) and np.array_equal(host(Xd), down.astype(np.complex64))
    up, ux, uy = R.pool_fft(down, nx, ny, -s)
    Xu, gx, gy = ctx.pool(ctx.dev(down), ny, -s)
    assert (gx, gy) == (ux, uy) and np.array_equal(host(Xu), up.astype(np.complex64))


def test_power_of_two_grids_keep_their_route(ctx, flags):
    """A power-of-two grid cropped to a size that is not a power of two (r2c_pool of 128^2 by 3: 42 x 42) stays on Bluestein + resize:
    AEFFT_F_CHIRPZ, which only moves grids with a smooth axis, changes nothing there, bit for bit."""
    rng = np.random.default_rng(1283)
    x = ctx.dev(np.floor(rng.uniform(0, 256, (3, 128, 128))))
    flags()
    a = host(ctx.r2c_pool(x, 3)).copy()
    flags("CHIRPZ")
    b = host(ctx.r2c_pool(x, 3)).copy()
    flags()
    assert np.array_equal(a, b)
    down, _, _ = R.pool_fft(R.fft(host(x)), 128, 128, 3)
    assert relerr(a, down) < 1e-5


def test_mixed_radix_and_chirpz_paths_agree(ctx, flags):
    """AEFFT_F_CHIRPZ sends 640 x 480 back to Bluestein: both paths give the same spectra and images to 1e-5."""
    rng = np.random.default_rng(64048)
    x = ctx.dev(np.floor(rng.uniform(0, 256, (2, 640, 480))))
    flags()
    Xm = host(ctx.r2c(x)).copy()
    ym = host(ctx.c2r(ctx.dev(Xm), 480)).copy()
    flags("CHIRPZ")
    Xb = host(ctx.r2c(x)).copy()
    yb = host(ctx.c2r(ctx.dev(Xm), 480)).copy()
    flags()
    assert relerr(Xm, Xb) < 1e-5 and relerr(ym, yb) < 1e-5
    assert not np.array_equal(Xm, Xb), "CHIRPZ took the same kernels"


# ------------------------------------------------------------------------------------------
# 2. the network against the oracle
# ------------------------------------------------------------------------------------------
def _net(ctx, D, Nx, Ny, ws, Nk, Nl, s, B):
    net = aefft.Net(ctx, D, Nx, Ny, [w[0].shape[0] for w in ws], Nk, s, batch=B, Nl=Nl, smooth_sizes=True)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    return net


@pytest.mark.parametrize("Nx,Ny,maps,Nk,Nl,B", [
    (640, 480, [3, 4, 3, 2], 5, 5, 2),      # down to 40 x 30
    (240, 320, [4, 3, 2], 5, 5, 2),
    (1280, 720, [2, 3, 2], 5, 5, 1),
    (96, 96, [4, 3], 5, 3, 2),              # Nk != Nl at a smooth size
])
def test_network_at_smooth_sizes_against_oracle(ctx, flags, Nx, Ny, maps, Nk, Nl, B):
    """forward (reconstruction + all 4L+1 layers), step_grad (packed gradients), step_apply (weights, per-pair MSE) and a 5-iteration
    train_pair burst of a net created with AEFFT_NET_SMOOTH_SIZES, which trains in the per-frame form."""
    flags()
    D, s = 3, 2
    L = len(maps)
    rng = np.random.default_rng(Nx * 5 + Ny + L)
    ws = _weights(rng, D, maps, Nk, Nl)
    xs = np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))
    net = _net(ctx, D, Nx, Ny, ws, Nk, Nl, s, B)
    assert net.step_form() == "per_frame"
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]
    net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    sp = [R.autoenc_fft(xs[i], net_c, net_b, [s] * L + [-s] * L) for i in range(B)]
    frames = ctx.dev(xs)
    recon = ctx.empty(B, D, Nx, Ny)
    net.forward(frames, recon)
    layers = [host(t).copy() for t in net.get_layers()]
    assert len(layers) == 4 * L + 1
    for i in range(B):
        assert relerr(host(recon)[i], sp[i][0][-1]) < 1e-4
        for k in range(4 * L + 1):
            assert relerr(layers[k][i], sp[i][0][k]) < 1e-4, k
    # one training step
    net.step_grad(frames, recon)
    for i in range(B):
        assert relerr(host(recon)[i], sp[i][0][-1]) < 1e-4
    gbuf = host(net.grad_buffer()).copy()
    mse = ctx.empty(L)
    net.step_apply(0.2, 0, 0, 1.0, mse)
    off = 0
    cf = sp[0][1]
    z = lambda a: np.zeros_like(a)
    for l in range(L):
        c, b, f, p = ws[l]
        dM, dDl = c.shape[:2]
        Xs = [sp[i][2][2 * l + 1] for i in range(B)]; Os = [sp[i][2][4 * L - 1 - 2 * l] for i in range(B)]
        r = R.batch_train_iter(Xs, Xs, Os, cf[l], cf[2 * L - 1 - l], c, f, b, p, (z(c), z(f), z(b), z(p)), 0.02)
        nk = c.size
        for seg, ref in zip((gbuf[off:off + nk], gbuf[off + nk:off + 2 * nk], gbuf[off + 2 * nk:off + 2 * nk + dM],
                             gbuf[off + 2 * nk + dM:off + 2 * nk + dM + dDl]), r["grads"]):
            assert relerr(seg, ref.ravel()) < 5e-5, l
        off += 2 * nk + dM + dDl
        c2, b2, f2, p2 = net.get_pair(l)
        for (a, k), gref in zip(((c2, "c"), (f2, "f"), (b2, "b"), (p2, "p")), r["grads"]):
            assert (np.abs(a - r[k]) < weight_step_tol(gref)).all(), (l, k, np.abs(a - r[k]).max())
        assert abs(host(mse)[l] - r["mse"]) < 1e-4 * max(1, r["mse"]), l
    net.close()
    # a 5-iteration burst on pair 0 of one frame (fft_backproplib.cu:1381-1511)
    net = _net(ctx, D, Nx, Ny, ws, Nk, Nl, s, 1)
    net.forward(ctx.dev(xs[:1]), None)
    got = net.train_pair(0, 5, 0.2)
    lay, cfr = sp[0][0], sp[0][1]
    c, b, f, p = ws[0]
    r = R.backprop_fft(lay[1], lay[1], lay[4 * L - 1], cfr[0], c, cfr[2 * L - 1], f, b, p, 0.2, n_iter=5)
    assert np.allclose(got, np.array(r["mse"]), rtol=1e-4), (got, r["mse"])
    c2, b2, f2, p2 = net.get_pair(0)
    for a, k in ((c2, "c"), (f2, "f"), (b2, "b"), (p2, "p")):
        assert np.abs(a - r[k]).max() < 1e-4, (k, np.abs(a - r[k]).max())
    net.close()


# ------------------------------------------------------------------------------------------
# 3. two steps, three ways
# ------------------------------------------------------------------------------------------
def _two_steps(ctx, net, frames, B, D, Nx, Ny, L):
    out = []
    for x in frames:
        recon = ctx.empty(B, D, Nx, Ny); recon.fill_(float("nan"))
        mse = ctx.empty(L)
        net.step_grad(x, recon)
        g = host(net.grad_buffer()).copy()
        net.step_apply(0.2, 0, 0, 1.0, mse)
        ctx.sync()
        out.append((host(recon).copy(), g, host(mse).copy()))
    out.append([np.concatenate([a.ravel() for a in net.get_pair(l)]) for l in range(L)])
    return out


def _same(a, b):
    for u, v in zip(a[:-1], b[:-1]):
        for x, y in zip(u, v):
            assert np.array_equal(x, y)
    for x, y in zip(a[-1], b[-1]):
        assert np.array_equal(x, y)


def test_input_ready_and_noopform_give_the_same_two_steps(ctx, flags):
    """At 640 x 480: aefft_net_set_input_ready(1) (the frame R2C on a side stream in its own workspace) and NOOPFORM (the form such a net
    runs anyway) give the results of the plain loop bit for bit over two steps."""
    D, Nx, Ny, maps, B = 3, 640, 480, [4, 3], 2
    L = len(maps)
    rng = np.random.default_rng(2 * 640)
    ws = _weights(rng, D, maps, 5, 5)
    frames = [ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))) for _ in range(2)]
    runs = []
    for ready, fl in ((False, ""), (True, ""), (False, "NOOPFORM")):
        flags(fl)
        net = _net(ctx, D, Nx, Ny, ws, 5, 5, 2, B)
        net.set_input_ready(ready)
        runs.append(_two_steps(ctx, net, frames, B, D, Nx, Ny, L))
        net.close()
    flags()
    assert np.isfinite(runs[0][0][0]).all()
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])


# ------------------------------------------------------------------------------------------
# 4. 8-bit frames
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,Nk,Nl,path,smooth", [
    (640, 480, 5, 5, "", True),
    (64, 64, 5, 3, "", False),              # power of two, no pruned transform: the kernels' pad + R2C must not read bytes
    (64, 64, 5, 3, "NOOPFORM", False),
])
def test_u8_frames_equal_float_frames(ctx, flags, Nx, Ny, Nk, Nl, path, smooth):
    """step_grad_u8 / forward_u8 == the float calls bit for bit: reconstruction, packed gradients, weights after 3 steps, layer 0.  Only the
    frame transforms read 8-bit input; the zero-padded float kernels of a non-pruned geometry go through the float path."""
    flags(path)
    D, maps, B = 3, [4, 3], 2
    L = len(maps)
    rng = np.random.default_rng(Nx + Nk * 10 + len(path))
    ws = _weights(rng, D, maps, Nk, Nl)
    x8 = np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))).astype(np.uint8)
    torch = ctx.torch
    res = []
    for u8 in (False, True):
        net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, 2, batch=B, Nl=Nl, smooth_sizes=smooth)
        for l, w in enumerate(ws):
            net.set_pair(l, *w)
        frames = torch.from_numpy(x8).to(f"cuda:{ctx.device}") if u8 else ctx.dev(x8.astype(np.float32))
        recs, grads = [], []
        for _ in range(3):
            recon = ctx.empty(B, D, Nx, Ny)
            net.step_grad(frames, recon)
            grads.append(host(net.grad_buffer()).copy())
            net.step_apply(0.2)
            recs.append(host(recon).copy())
        recon = ctx.empty(B, D, Nx, Ny)
        net.forward(frames, recon)
        ctx.sync()
        res.append((recs + [host(recon).copy()], grads, [net.get_pair(l) for l in range(L)], host(net.get_layer(0)).copy(),
                    host(net.get_layer(1)).copy()))
        net.close()
    flags()
    (ra, ga, wa, l0a, l1a), (rb, gb, wb, l0b, l1b) = res
    for u, v in zip(ra + ga, rb + gb):
        assert np.isfinite(u).all() and np.array_equal(u, v)
    for u, v in zip(wa, wb):
        for x, y in zip(u, v):
            assert np.array_equal(x, y)
    assert np.array_equal(l0a, l0b) and np.array_equal(l0a, x8.astype(np.float32)) and np.array_equal(l1a, l1b)


# ------------------------------------------------------------------------------------------
# 5. creation rules
# ------------------------------------------------------------------------------------------
def test_create_ex_options_on_a_power_of_two_net(ctx, flags):
    """aefft_net_create_ex(opts = 0) and (AEFFT_NET_SMOOTH_SIZES) on a 64^2 net == aefft_net_create, bit for bit over two steps."""
    flags()
    D, N, maps, B = 3, 64, [4, 3], 2
    rng = np.random.default_rng(6464)
    ws = _weights(rng, D, maps, 5, 5)
    frames = [ctx.dev(np.floor(rng.uniform(0, 256, (B, D, N, N)))) for _ in range(2)]
    L = len(maps)
    runs = []
    for opts in (None, 0, aefft.NET_SMOOTH_SIZES):
        d = aefft.NetDesc(D, N, N, L, (C.c_int * L)(*maps), (C.c_int * L)(5, 5), (C.c_int * L)(5, 5), (C.c_int * L)(2, 2), B)
        net = aefft.Net(ctx, D, N, N, maps, 5, 2, batch=B)
        if opts is not None:
            # the same net object around a handle made by aefft_net_create_ex
            h = C.c_void_p()
            ctx.check(ctx.L.aefft_net_create_ex(ctx.h, C.byref(d), opts, C.byref(h)))
            ctx.L.aefft_net_destroy(net.h)
            net.h = h
        for l, w in enumerate(ws):
            net.set_pair(l, *w)
        runs.append(_two_steps(ctx, net, frames, B, D, N, N, L))
        net.close()
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])


@pytest.mark.parametrize("Nx,Ny,L", [(14, 14, 1), (13, 12, 1), (2050, 16, 1), (480, 480, 5), (1080, 1080, 3)])
def test_create_ex_rejects(ctx, Nx, Ny, L):
    """14 = 2 * 7 and 13 are not smooth, 2050 is beyond 2048, 480 over 5 pairs ends on a 15-point grid, 1080 over 3 on 135."""
    d = aefft.NetDesc(3, Nx, Ny, L, (C.c_int * L)(*[2] * L), (C.c_int * L)(*[3] * L), (C.c_int * L)(*[3] * L), (C.c_int * L)(*[2] * L), 1)
    h = C.c_void_p()
    assert ctx.L.aefft_net_create_ex(ctx.h, C.byref(d), aefft.NET_SMOOTH_SIZES, C.byref(h)) == aefft.EINVAL and not h.value
    if L > 1:
        assert b"even and >= 8" in ctx.L.aefft_last_error(ctx.h)


# ------------------------------------------------------------------------------------------
# 6. the reference's vector entry points at a smooth size
# ------------------------------------------------------------------------------------------
def test_vector_entry_points_at_a_smooth_size(wrap):  # noqa: F811
    """autoenc_fft (the cached net, aefft_net_create_ex) and backprop_fft (the per-bin ops) through nested vectors at N = 240."""
    rng = np.random.default_rng(240)
    D, dM, N, Nk, s = 3, 4, 240, 5, 2
    n = N // s
    x = np.floor(rng.uniform(0, 256, (D, N, N))).astype(np.float32)
    c = rng.uniform(-1, 1, (dM, D, Nk, Nk)).astype(np.float32); f = rng.uniform(-1, 1, (D, dM, Nk, Nk)).astype(np.float32)
    b = rng.uniform(-1, 1, dM).astype(np.float32); p = rng.uniform(-1, 1, D).astype(np.float32)
    layers, cfreq, _ = R.autoenc_fft(x.astype(np.float64), [c.astype(np.float64), f.astype(np.float64)],
                                     [b.astype(np.float64), p.astype(np.float64)], [s, -s])
    sizes = [D * n * n, dM * n * n, D * n * n, D * N * N]
    lay = np.zeros(sum(sizes), np.float32)
    W = dM * D * n * (n // 2 + 1) * 2
    cf = np.zeros(2 * W, np.float32)
    nc = C.c_int(0)
    cc, bb, ff, pp = c.copy(), b.copy(), f.copy(), p.copy()
    wrap.w_fft_pair(_p(x), _p(lay), _p(cc), _p(bb), _p(ff), _p(pp), _p(cf), C.byref(nc), D, dM, N, Nk, s, 1, 0, C.c_float(0.2), 0)
    assert nc.value == 2
    off = 0
    for l, sz in enumerate(sizes, start=1):
        ref = layers[l].ravel()
        assert np.abs(lay[off:off + sz] - ref).max() < 1e-4 * np.abs(ref).max(), l
        off += sz
    lay2 = np.zeros_like(lay)
    wrap.w_fft_pair(_p(x), _p(lay2), _p(cc), _p(bb), _p(ff), _p(pp), _p(cf), C.byref(nc), D, dM, N, Nk, s, 1, 1, C.c_float(0.01), 0)
    r = R.backprop_fft(layers[1], layers[1], layers[3], cfreq[0], c.astype(np.float64), cfreq[1], f.astype(np.float64),
                       b.astype(np.float64), p.astype(np.float64), 0.01, n_iter=100)
    dw = np.abs(r["c"] - c).max()
    assert dw > 1e-3
    for a, k in ((cc, "c"), (ff, "f"), (bb, "b"), (pp, "p")):
        assert np.abs(a - r[k]).max() < 2e-5 + 1e-3 * dw, (k, np.abs(a - r[k]).max(), dw)
