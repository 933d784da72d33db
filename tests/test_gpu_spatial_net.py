"""The spatial net (aefft_net_create_ex with AEFFT_NET_SPATIAL): the reference's coordinate-space training mode as a resident, batched,
data-parallel network, against oracle/np_spatial.py.  Pool and nearest up-sampling (netlib.cpp:114-164) are restated here in numpy."""
import ctypes as C
import importlib

import numpy as np
import pytest

import np_spatial as S

pytestmark = pytest.mark.gpu
aefft = importlib.import_module("autoencoder-fft_amd")
dp = importlib.import_module("autoencoder-fft_amd.dp")


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def host(t):
    return t.detach().cpu().numpy()


def pool(x, s):
    """Pool(s > 0): max(0, trunc(window maximum)) -- the reference's `int smax = 0` accumulator"""
    B, ch, nx, ny = x.shape
    m = x.reshape(B, ch, nx // s, s, ny // s, s).max(axis=(3, 5))
    return np.trunc(np.maximum(m, 0)).astype(np.float32)


def upsample(x, s):
    return np.repeat(np.repeat(x, s, axis=2), s, axis=3)


def make_net(ctx, D, Nx, Ny, maps, Nk, Nl, s, B, seed=0, spatial=True):
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, s, B, Nl=Nl, spatial=spatial)
    rng = np.random.default_rng(seed)
    for l, g in enumerate(net.dims):
        sc = 1.0 / np.sqrt(g["Nk"] * g["Nl"])
        c = rng.uniform(-sc, sc, (g["dM"], g["dD"], g["Nk"], g["Nl"])).astype(np.float32)
        f = rng.uniform(-sc, sc, (g["dD"], g["dM"], g["Nk"], g["Nl"])).astype(np.float32)
        b = rng.uniform(-1, 1, g["dM"]).astype(np.float32); p = rng.uniform(-1, 1, g["dD"]).astype(np.float32)
        net.set_pair(l, c, b, f, p)
    return net


def frames(rng, B, D, Nx, Ny):
    return np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))).astype(np.float32)


def relerr(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(1.0, np.abs(b).max())


# (D, Nx, Ny, maps, Nk, Nl, scale)
SHAPES = [
    (1, 128, 128, [4], 3, 3, 1),
    (3, 64, 64, [4, 6], 3, 3, 2),
    (3, 96, 80, [3, 5, 4], 5, 5, 2),
    (3, 96, 96, [4], 3, 3, 3),
    (3, 640, 480, [4, 8], 3, 3, 2),
    (3, 60, 36, [4, 3], 5, 3, 2),
]


@pytest.mark.parametrize("D,Nx,Ny,maps,Nk,Nl,s", SHAPES)
def test_forward_layer_by_layer(ctx, D, Nx, Ny, maps, Nk, Nl, s):
    """every layer from the GPU's own previous layer: Pool and up-sampling bit for bit, the convolutions against Conv_gpu"""
    B, L = 2, len(maps)
    net = make_net(ctx, D, Nx, Ny, maps, Nk, Nl, s, B, seed=Nx + Ny)
    assert net.step_form() == "spatial"
    x = ctx.dev(frames(np.random.default_rng(Nx * Ny), B, D, Nx, Ny))
    recon = ctx.empty(B, D, Nx, Ny)
    net.forward(x, recon)
    lay = [host(t) for t in net.get_layers()]
    offs = (C.c_size_t * (4 * L + 2))()
    ctx.check(ctx.L.aefft_net_layers_layout(net.h, offs))
    for i, t in enumerate(lay):
        assert t.size == offs[i + 1] - offs[i]
    assert np.array_equal(lay[0], host(x))
    pairs = [net.get_pair(l) for l in range(L)]
    for l in range(L):
        c, b, f, p = pairs[l]
        assert np.array_equal(lay[2 * l + 1], pool(lay[2 * l], s)), l
        for i in range(B):
            assert relerr(lay[2 * l + 2][i], S.conv(lay[2 * l + 1][i], c, b)) < 1e-5, l
            assert relerr(lay[4 * L - 1 - 2 * l][i], S.conv(lay[4 * L - 2 - 2 * l][i], f, p)) < 1e-5, l
        assert np.array_equal(lay[4 * L - 2 * l], upsample(lay[4 * L - 1 - 2 * l], s)), l
    assert np.array_equal(host(recon), lay[4 * L])
    net.close()


def _oracle_pair(lay, L, l, w, mom, del0, alpha, tied):
    c, b, f, p = w
    x, out, hin = (lay[2 * l + 1].astype(np.float64), lay[4 * L - 1 - 2 * l].astype(np.float64), lay[2 * l + 2].astype(np.float64))
    r = S.backprop_gpu(x, out, hin, c, b, f, p, *mom, del0, alpha, tied=tied, B_mean=True)
    return r[:4], r[4:8]


def _grad_segments(buf, dims):
    _, n = dp.grad_layout(dims)
    return [dict(zip(("dck", "dfk", "db", "dp"), t)) for t in dp.unpack_grads(buf, dims)], buf[n:n + len(dims)]


def _steps_against_backprop_gpu(ctx, sym, D, Nx, Ny, maps, Nk, Nl, s, B, steps):
    L, del0 = len(maps), 0.2
    net = make_net(ctx, D, Nx, Ny, maps, Nk, Nl, s, B, seed=3)
    if sym:
        for l in range(L):
            c, b, f, p = net.get_pair(l)
            net.set_pair(l, c, b, np.ascontiguousarray(c.transpose(1, 0, 2, 3)), p)
    alpha = 0.5 if sym else 0.9
    if sym:
        net.set_inertia(alpha)
    x = ctx.dev(frames(np.random.default_rng(5), B, D, Nx, Ny))
    mom = [[np.zeros((g["dM"], g["dD"], Nk, Nl)), np.zeros(g["dM"]), np.zeros((g["dD"], g["dM"], Nk, Nl)), np.zeros(g["dD"])] for g in net.dims]
    mse = ctx.empty(L)
    for step in range(steps):
        w = [net.get_pair(l) for l in range(L)]
        net.step_grad(x)
        lay = [host(t) for t in net.get_layers()]
        segs, tail = _grad_segments(host(net.grad_buffer()).astype(np.float64), net.dims)
        net.step_apply(del0, 0, sym, 1.0, mse)
        got_mse = host(mse)
        for l, g in enumerate(net.dims):
            xin, out, hin = lay[2 * l + 1], lay[4 * L - 1 - 2 * l], lay[2 * l + 2]
            gs = [S.gradients(xi, oi, hi, w[l][2]) for xi, oi, hi in zip(xin, out, hin)]
            gc, gf, gb, gp = (sum(t) / B for t in zip(*gs))
            for name, ref in (("dck", gc), ("dfk", gf), ("db", gb), ("dp", gp)):
                assert np.abs(segs[l][name] - ref).max() <= 5e-5 * np.abs(ref).max(), (step, l, name)
            norm = g["dD"] * g["dM"] * Nk * Nl * g["Nx"] * g["Ny"]
            ref_mse = ((xin.astype(np.float64) - out) ** 2).sum() / norm / B
            assert abs(tail[l] - ref_mse) <= 1e-4 * ref_mse, (step, l)
            assert abs(got_mse[l] - ref_mse * (0.5 if sym else 1.0)) <= 1e-4 * ref_mse, (step, l)
            new, mom[l] = _oracle_pair(lay, L, l, w[l], mom[l], del0, alpha, bool(sym))
            now = net.get_pair(l)
            for a, o, old in zip(now, new, w[l]):
                dw = np.abs(o - old).max()
                assert np.abs(a - o).max() <= 1e-6 * max(1.0, np.abs(o).max()) + 2e-3 * dw, (step, l)
            if sym:
                assert np.array_equal(now[2], np.ascontiguousarray(now[0].transpose(1, 0, 2, 3)))
        assert np.array_equal(host(net.last_mse()), got_mse)
    net.close()


# (D, Nx, Ny, maps, Nk, Nl, scale, B, steps) and the weight-gradient route of each pair (launch_spatial_grad)
STEP_SHAPES = [
    (3, 64, 48, [8, 12], 3, 3, 2, 2, 3),      # pair 0 on 32x24: region sums (rcorr<3>); pair 1 on 16x12, dD = 8: mcorr<3>
    (3, 40, 24, [8, 10], 5, 5, 2, 2, 2),      # pair 0 on 20x12: mcorr<5>; pair 1 on 10x6, Ny % 4 != 0: wcorr<5>
    (1, 28, 32, [9], 7, 7, 2, 1, 2),          # 14x16: mcorr<7>
    (3, 36, 60, [4, 3], 5, 3, 2, 2, 2),       # Nk != Nl: the naive kernels; Pool and up-sampling run as launches of their own
]


@pytest.mark.parametrize("sym", [0, 1])
def test_steps_against_backprop_gpu(ctx, sym):
    """three step_grad / step_apply rounds against backprop_gpu[_cc] per pair on the GPU's own layers: the packed gradients, the MSE
    tail, the weights (momentum carried across steps); set_inertia reaches the update"""
    _steps_against_backprop_gpu(ctx, sym, *STEP_SHAPES[0])


@pytest.mark.parametrize("D,Nx,Ny,maps,Nk,Nl,s,B,steps,sym", [STEP_SHAPES[1] + (0,), STEP_SHAPES[1] + (1,), STEP_SHAPES[2] + (0,), STEP_SHAPES[3] + (0,)])
def test_steps_against_backprop_gpu_other_supports_and_routes(ctx, D, Nx, Ny, maps, Nk, Nl, s, B, steps, sym):
    """the same checks, two steps each, where the pairs' gradients take the other routes: 5x5 supports on the matrix cores and through
    the VALU correlation (untied and tied), 7x7 on the matrix cores, and a 5x3 support, which only the naive kernels serve"""
    _steps_against_backprop_gpu(ctx, sym, D, Nx, Ny, maps, Nk, Nl, s, B, steps)


def test_reset_momentum_on_a_spatial_net(ctx):
    """after two steps and reset_momentum, the next step gives the weights -- to the bit -- that a fresh net gives when it starts
    from the same weights: the momentum buffers are zero again and nothing else of the two steps is carried over"""
    D, Nx, Ny, maps, Nk, s, B = 3, 40, 24, [8, 10], 5, 2, 2
    L = len(maps)
    x = ctx.dev(frames(np.random.default_rng(71), B, D, Nx, Ny))
    net = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=70)
    w0 = [net.get_pair(l) for l in range(L)]
    for _ in range(2):
        net.step_grad(x); net.step_apply(0.2, 0, 0, 1.0)
    w2 = [net.get_pair(l) for l in range(L)]
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(w0, w2))
    net.reset_momentum()
    net.step_grad(x); net.step_apply(0.2, 0, 0, 1.0)
    got = [net.get_pair(l) for l in range(L)]
    net.close()
    fresh = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=1)
    for l in range(L):
        fresh.set_pair(l, *w2[l])
    fresh.step_grad(x); fresh.step_apply(0.2, 0, 0, 1.0)
    want = [fresh.get_pair(l) for l in range(L)]
    fresh.close()
    for a, o in zip(got, want):
        for u, v in zip(a, o):
            assert np.array_equal(u, v)
    # the momentum mattered: without the reset the third step differs
    cont = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=70)
    for _ in range(3):
        cont.step_grad(x); cont.step_apply(0.2, 0, 0, 1.0)
    assert not np.array_equal(cont.get_pair(0)[0], got[0][0])
    cont.close()


def _train(ctx, flags, fl, steps=2, shape=(3, 64, 48, [8, 12], 3, 2, 2)):
    D, Nx, Ny, maps, Nk, s, B = shape
    flags(fl)
    net = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=11)
    x = ctx.dev(frames(np.random.default_rng(12), B, D, Nx, Ny))
    bufs = []
    for _ in range(steps):
        net.step_grad(x)
        bufs.append(host(net.grad_buffer()).copy())
        net.step_apply(0.2, 0, 0, 1.0)
    ws = [net.get_pair(l) for l in range(len(maps))]
    net.close()
    flags()
    return bufs, ws


def test_routes_agree(ctx, flags):
    """the default routes (region sums, matrix-core convolutions with Pool / up-sampling on load), NOTILEDSPATIAL (naive kernels, Pool and
    Pool(-s) launches of their own) and NORCORR (dC through the back-convolved error) give the same step; POISON changes no bit"""
    base_b, base_w = _train(ctx, flags, "")
    L = 2
    for fl in ("NOTILEDSPATIAL", "NORCORR"):
        b, w = _train(ctx, flags, fl)
        for u, v in zip(b, base_b):
            assert np.abs(u - v).max() <= 1e-5 * np.abs(v).max(), fl
            # the MSE tail: pair 0 sums it inside the region launch by default, in the standalone reduction under both switches
            assert np.allclose(u[-L:], v[-L:], rtol=1e-5, atol=0), fl
        for a, o in zip(w, base_w):
            for u, v in zip(a, o):
                assert np.abs(u - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), fl
    b, w = _train(ctx, flags, "POISON")
    for u, v in zip(b, base_b):
        assert np.array_equal(u, v)
    for a, o in zip(w, base_w):
        for u, v in zip(a, o):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("D,N,dM,Nk,s", [(3, 64, 16, 3, 2), (3, 48, 4, 5, 1)])
def test_one_pair_net_equals_step_spatial(ctx, D, N, dM, Nk, s):
    """an L = 1 net == aefft_step_spatial on its pooled input with the same weights and momentum (two steps)"""
    import torch
    B, del0, alpha = 2, 0.2, 0.9
    net = make_net(ctx, D, N, N, [dM], Nk, Nk, s, B, seed=21)
    c, b, f, p = (ctx.dev(a) for a in net.get_pair(0))
    mom = [torch.zeros_like(t) for t in (c, b, f, p)]
    grads = [torch.zeros_like(t) for t in (c, b, f, p)]
    x = ctx.dev(frames(np.random.default_rng(22), B, D, N, N))
    for _ in range(2):
        net.step_grad(x)
        xin = net.get_layer(1)
        net.step_apply(del0, 0, 0, 1.0)
        hin, out = ctx.step_spatial(xin, c, b, f, p, (mom[0], mom[1], mom[2], mom[3]), grads, del0, alpha)
        ctx.sync()
        assert relerr(host(net.get_layer(2)), host(hin)) < 1e-6
        assert relerr(host(net.get_layer(3)), host(out)) < 1e-6
        for a, o in zip(net.get_pair(0), (host(c), host(b), host(f), host(p))):
            assert np.abs(a - o).max() <= 1e-6 * max(1.0, np.abs(o).max())
    net.close()


def test_data_parallel_on_one_gpu(ctx):
    """two replicas with B/2 frames each, buffers summed, step_apply(grad_scale = 1/2): bit-identical replicas, equal to one net over the
    whole batch to the bound test_gpu_dp.py uses"""
    D, Nx, Ny, maps, Nk, s, B = 3, 64, 64, [8, 6], 3, 2, 4
    x = frames(np.random.default_rng(31), B, D, Nx, Ny)
    full = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=30)
    w0 = [full.get_pair(l) for l in range(len(maps))]
    reps = [make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B // 2, seed=30) for _ in range(2)]
    xs = [ctx.dev(x[:B // 2]), ctx.dev(x[B // 2:])]
    xf = ctx.dev(x)
    for _ in range(2):
        full.step_grad(xf)
        full.step_apply(0.2, 0, 0, 1.0)
        for r, xr in zip(reps, xs):
            r.step_grad(xr)
        total = reps[0].grad_buffer() + reps[1].grad_buffer()
        for r in reps:
            r.grad_buffer().copy_(total)
            r.step_apply(0.2, 0, 0, 0.5)
    ctx.sync()
    for l in range(len(maps)):
        a, b2, ref = reps[0].get_pair(l), reps[1].get_pair(l), full.get_pair(l)
        for u, v, o, w in zip(a, b2, ref, w0[l]):
            assert np.array_equal(u, v)
            assert np.abs(u - o).max() <= 1e-6 + 2e-3 * np.abs(o - w).max()
    for n in reps + [full]:
        n.close()


def test_mse_of_two_emulated_ranks(ctx):
    """two replicas with B/2 frames each, buffers summed (the all-reduce), step_apply(grad_scale = 1/2): every rank's tail, the floats behind
    the buffer, last_mse and mse_d hold the global-batch pre-update MSE of the step; a further all-reduce of the tails times 1/2 (what
    dp.DataParallelStep.flush_mse does) gives it back -- equal to one net over the whole batch"""
    D, Nx, Ny, maps, Nk, s, B = 3, 64, 64, [8, 6], 3, 2, 4
    L = len(maps)
    x = frames(np.random.default_rng(61), B, D, Nx, Ny)
    full = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=60)
    reps = [make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B // 2, seed=60) for _ in range(2)]
    xs = [ctx.dev(x[:B // 2]), ctx.dev(x[B // 2:])]
    mse_full, mse_r = ctx.empty(L), [ctx.empty(L), ctx.empty(L)]
    full.step_grad(ctx.dev(x))
    full.step_apply(0.2, 0, 0, 1.0, mse_full)
    for r, xr in zip(reps, xs):
        r.step_grad(xr)
    total = reps[0].grad_buffer() + reps[1].grad_buffer()
    for r, m in zip(reps, mse_r):
        r.grad_buffer().copy_(total)
        r.step_apply(0.2, 0, 0, 0.5, m)
    ctx.sync()
    want = host(mse_full).astype(np.float64)
    tails = [host(r.grad_buffer())[-L:].astype(np.float64) for r in reps]
    assert np.allclose((tails[0] + tails[1]) * 0.5, want, rtol=1e-5, atol=0)
    for r, m, t in zip(reps, mse_r, tails):
        assert np.allclose(t, want, rtol=1e-5, atol=0)
        assert np.array_equal(host(m), t.astype(np.float32))
        assert np.array_equal(host(r.mse_prev_global()), t.astype(np.float32))
        assert np.array_equal(host(r.last_mse()), t.astype(np.float32))
    for n in reps + [full]:
        n.close()


def test_rccl_step_at_world_size_one(ctx):
    """dp.RcclStep (libaefft_dp.so) on a spatial net == plain step_grad / step_apply bit for bit over 3 steps"""
    D, Nx, Ny, maps, Nk, s, B = 3, 64, 64, [8, 6], 3, 2, 2
    x = ctx.dev(frames(np.random.default_rng(41), B, D, Nx, Ny))
    recon = ctx.empty(B, D, Nx, Ny)
    mse = ctx.empty(len(maps))
    plain = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=40)
    for _ in range(3):
        plain.step_grad(x, recon); plain.step_apply(0.2, 0, 0, 1.0, mse)
    ctx.sync()
    want, want_mse = [plain.get_pair(l) for l in range(len(maps))], host(mse).copy()
    plain.close()
    net = make_net(ctx, D, Nx, Ny, maps, Nk, Nk, s, B, seed=40)
    step = dp.RcclStep(net, 0, 1)
    step(x, recon, 0.2)
    step.run(x, recon, 0.2, 1)
    step(x, recon, 0.2, mse=mse)
    ctx.sync()
    for a, b in zip(want, [net.get_pair(l) for l in range(len(maps))]):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert np.array_equal(host(mse), want_mse)
    assert np.allclose(step.flush_mse(), want_mse, rtol=1e-6)
    step.close(); net.close()


def _create(ctx, D, Nx, Ny, maps, Nk, s, B=1, opts=aefft.NET_SPATIAL):
    L = len(maps)
    arr = lambda v: (C.c_int * L)(*v)
    keep = [arr(maps), arr([Nk] * L), arr([Nk] * L), arr([s] * L)]
    d = aefft.NetDesc(D, Nx, Ny, L, *keep, B)
    h = C.c_void_p()
    rc = ctx.L.aefft_net_create_ex(ctx.h, C.byref(d), opts, C.byref(h))
    return rc, h


def test_rules_and_refused_entry_points(ctx):
    for (N, maps, s, pair) in ((66, [2, 2], 2, 1), (10, [2], 3, 0)):
        rc, h = _create(ctx, 1, N, N, maps, 3, s)
        assert rc == aefft.EINVAL and not h.value
        msg = ctx.L.aefft_last_error(ctx.h).decode()
        assert "divide" in msg and f"pair {pair}" in msg, msg
    rc, h = _create(ctx, 1, 16, 16, [2], 3, 4)              # 4 x 4 pooled grid holds the 3 x 3 support
    assert rc == aefft.OK
    ctx.L.aefft_net_destroy(h)
    rc, h = _create(ctx, 1, 16, 16, [2], 5, 4)
    assert rc == aefft.EINVAL and "support" in ctx.L.aefft_last_error(ctx.h).decode()
    rc, h = _create(ctx, 3, 30, 18, [4], 3, 3, opts=aefft.NET_SPATIAL | aefft.NET_SMOOTH_SIZES)
    assert rc == aefft.OK
    ctx.L.aefft_net_destroy(h)

    D, N, B = 3, 32, 1
    net = make_net(ctx, D, N, N, [4], 3, 3, 2, B)
    x = ctx.dev(frames(np.random.default_rng(51), B, D, N, N))
    net.step_grad(x)
    Lb, h = ctx.L, net.h
    pp = C.c_void_p()
    buf = np.zeros(1 << 16, np.float32)
    hp = buf.ctypes.data_as(C.c_void_p)
    assert Lb.aefft_net_pair_spectra(h, 0, C.byref(pp), C.byref(pp)) == aefft.EINVAL
    assert "spatial" in Lb.aefft_last_error(ctx.h).decode()
    assert Lb.aefft_net_store_spectra(h, 0, hp, hp) == aefft.EINVAL
    assert Lb.aefft_net_load_spectra(h, 0, hp, hp, hp, hp) == aefft.EINVAL
    assert Lb.aefft_net_train_pair(h, 0, 1, 0.2, 0, 0, None) == aefft.EINVAL
    assert Lb.aefft_net_step_grad_u8(h, C.c_void_p(x.data_ptr()), None) == aefft.EINVAL
    assert Lb.aefft_net_forward_u8(h, C.c_void_p(x.data_ptr()), None) == aefft.EINVAL
    assert Lb.aefft_net_set_input_ready(h, 1) == aefft.EINVAL
    assert Lb.aefft_net_set_input_ready(h, 0) == aefft.OK
    assert Lb.aefft_net_step_apply(h, 0.2, 1, 0, 1.0, None) == aefft.EINVAL
    assert Lb.aefft_net_set_inertia(h, 1.5) == aefft.EINVAL
    assert Lb.aefft_net_set_inertia(h, -0.1) == aefft.EINVAL
    net.set_inertia(0.0); net.set_inertia(1.0)
    assert Lb.aefft_net_step_apply(h, 0.2, 0, 0, 1.0, None) == aefft.OK
    ctx.sync()
    net.close()

    fft = make_net(ctx, D, N, N, [4], 3, 3, 2, B, spatial=False)
    assert fft.step_form() != "spatial"
    assert ctx.L.aefft_net_set_inertia(fft.h, 0.5) == aefft.EINVAL
    fft.close()
