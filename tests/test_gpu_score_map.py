"""aefft_net_score_map (Net.score_map): the per-tile reconstruction error under frozen weights -- the segmented reduction against the
returned float reconstruction on every row-pass route and every tile, with and without the store, 8-bit frames bit for bit, score_d as a
function of the map, against the float64 oracle in every form, a trained net's small residual, frames independent of one another, training
undisturbed bit for bit, the launch counts by the profiler, state and errors, and the unfused routes (spatial net, chirp-z transforms)."""
import importlib

import numpy as np
import pytest
import torch

import frozen_cases as F
from frozen_cases import CASES, PATHS, TILES, _case, _identity_case, _oracle_recon, _weights, host, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import TOL, _infer        # 1e-4: the bound test_gpu_infer.py holds the reconstruction to
from test_gpu_score import _score

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# A map entry against the returned float reconstruction: the project's bound 4 k 2^-24 with k <= 32.  The float32 chains (DESIGN.md section
# 16): power-of-two row kernel 8 terms in the lane + at most 4 butterfly levels = 12; mixed-radix row kernel 4 + at most 5 = 9; the finish and
# the unfused route in double.  4 * 32 * 2^-24 = 7.6e-6 < 1e-5.
RTOL = 1e-5
OWN = ["64-2pairs", "64x128", "256-4pairs", "no-pooling", "240x320", "240x320-opform", "D4"]          # test_gpu_score.py's
ORDER = OWN + ["24x40", "8x1024", "8x2048", "64x192", "16x640", "16x1280"]


def _map(ctx, net, frames, tile, recon=True, score=True):
    """one aefft_net_score_map: (map, score or None, reconstruction or None) as host arrays; the outputs start as NaN.  (Net.score_map always
    hands a score buffer over: score_d = NULL goes through the C entry.)"""
    m = ctx.empty(net.B, net.Nx // tile, net.Ny // tile); m.fill_(float("nan"))
    sc = rec = None
    if score:
        sc = ctx.empty(net.B); sc.fill_(float("nan"))
    if recon:
        rec = ctx.empty(net.B, net.D, net.Nx, net.Ny); rec.fill_(float("nan"))
    if score:
        out = net.score_map(frames, tile, m, sc, rec)
        assert out[0] is m and out[1] is sc and out[2] is rec
    else:
        ctx.check(net.L.aefft_net_score_map(net.h, aefft._ptr(frames), int(frames.dtype == torch.uint8), tile, aefft._ptr(m), None, aefft._ptr(rec)))
    ctx.sync()
    return host(m).copy(), (None if sc is None else host(sc).copy()), (None if rec is None else host(rec).copy())


def _block_mean_sq(x, r, t):
    """numpy's float64 block mean of (x - r)^2 over channels and t x t tiles: [B][Nx/t][Ny/t]"""
    d = (np.asarray(x, np.float64) - np.asarray(r, np.float64)) ** 2
    B, D, Nx, Ny = d.shape
    return d.reshape(B, D, Nx // t, t, Ny // t, t).sum((1, 3, 5)) / (D * t * t)


def _check_reduction(name, x, m, rec, t):
    ref = _block_mean_sq(x, rec, t)
    assert m.shape == ref.shape, (name, m.shape, ref.shape)
    assert (ref > 0).all(), name
    err = np.abs(m.astype(np.float64) - ref) / ref
    print(f"{name} tile {t}: map {m.shape} against the returned reconstruction: relative {err.max():.2e}")
    assert np.isfinite(m).all() and (err <= RTOL).all(), (name, t, err.max())


def _check_oracle(name, x, m, rec_o, t):
    m_o = _block_mean_sq(x, rec_o, t)
    d = np.abs(np.sqrt(m.astype(np.float64)) - np.sqrt(m_o))
    bound = TOL * np.abs(rec_o).max() + 1e-5 * np.sqrt(m_o)
    print(f"{name} tile {t}: max |sqrt(m) - sqrt(m_o)| {d.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.isfinite(m).all() and (d <= bound).all(), (name, t, (d - bound).max())


def test_the_cases_tiles_divide_their_grids():
    for name in ORDER:
        _, Nx, Ny, *_ = CASES[name]
        assert F.tiles(name), name
        assert all(Nx % t == 0 and Ny % t == 0 for t in F.tiles(name))
    assert F.tiles("24x40") == [8] and F.tiles("64x192") == [8, 16, 32, 64] and F.tiles("240x320") == [8, 16] and F.tiles("8x2048") == [8]


# ------------------------------------------------------------------------------------------
# 1. the reduction, 2. with and without the store, 8-bit frames
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER)
def test_map_is_the_block_mean_square_of_the_returned_reconstruction(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    F._form(net, name)
    f32 = ctx.dev(xs[0])
    u8 = F.u8(ctx, xs[0], f32)
    rec_i, _ = _infer(ctx, net, f32)
    for t in F.tiles(name):
        m_f, _, rec_f = _map(ctx, net, f32, t)
        m_8, _, rec_8 = _map(ctx, net, u8, t)
        assert np.array_equal(rec_f, rec_i), (name, t, np.abs(rec_f - rec_i).max())
        assert np.array_equal(rec_8, rec_i), (name, t)
        _check_reduction(name, xs[0], m_f, rec_f, t)
        # 2. without the store; 8-bit frames against the same pixels as floats
        m_f0, _, _ = _map(ctx, net, f32, t, recon=False)
        m_80, _, _ = _map(ctx, net, u8, t, recon=False)
        assert np.array_equal(m_8, m_f) and np.array_equal(m_f0, m_f) and np.array_equal(m_80, m_f), (name, t)


# ------------------------------------------------------------------------------------------
# 3. score_d
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER)
def test_score_is_the_mean_of_the_map(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    f32 = ctx.dev(xs[0])
    s_ref, _ = _score(ctx, net, f32, recon=False)          # aefft_net_score on the same frames
    for t in F.tiles(name):
        m, s, _ = _map(ctx, net, f32, t, recon=False)
        want = np.float32(m.astype(np.float64).mean((1, 2)))
        print(f"{name} tile {t}: score {s}, mean of the map {want}, aefft_net_score {s_ref}")
        assert (np.abs(s - want) <= np.spacing(np.abs(want))).all(), (name, t, s, want)
        assert (np.abs(s.astype(np.float64) - s_ref) <= 2 * RTOL * s_ref).all(), (name, t, s, s_ref)
        m0, s0, _ = _map(ctx, net, f32, t, recon=False, score=False)
        assert s0 is None and np.array_equal(m0, m), (name, t)


# ------------------------------------------------------------------------------------------
# 4. the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [(n, p) for n in ("64-2pairs", "256-4pairs") for p in PATHS] + [(n, "") for n in ORDER if n not in ("64-2pairs", "256-4pairs")])
def test_map_against_the_oracle(ctx, flags, name, path):
    """the RMS norm's triangle inequality holds per tile as it does per frame: the per-pixel bound TOL * max|recon_o| of test_gpu_infer.py"""
    flags(path)
    ws, xs = _case(name)
    net = F.net(ctx, name)
    F._form(net, name, path)
    frames = ctx.dev(xs[0])
    for k in range(2):          # the second call from the cached operators
        for t in F.tiles(name):
            m, _, _ = _map(ctx, net, frames, t, recon=bool(k), score=bool(k))
            _check_oracle(f"{name} {path}", xs[0], m, _oracle_recon(name), t)


# ------------------------------------------------------------------------------------------
# 5. a small residual
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [8, 64])
def test_a_small_residual(ctx, flags, tile):
    """the case a difference contracted into an FMA with the unrounded product fails: the residual is ~3e-3 of the pixels"""
    flags()
    (D, N, dM, Nk, B), w, x, rec_o = _identity_case()
    net = F.track(aefft.Net(ctx, D, N, N, [dM], Nk, 1, batch=B))
    net.set_pair(0, *w)
    f32 = ctx.dev(x)
    rec_i, _ = _infer(ctx, net, f32)
    m, _, rec = _map(ctx, net, f32, tile)
    m8, _, rec8 = _map(ctx, net, F.u8(ctx, x, f32), tile)
    m0, _, _ = _map(ctx, net, f32, tile, recon=False)
    assert np.array_equal(rec, rec_i) and np.array_equal(rec8, rec_i)
    _check_reduction("identity", x, m, rec, tile)
    assert np.array_equal(m0, m) and np.array_equal(m8, m)
    _check_oracle("identity", x, m, rec_o, tile)


# ------------------------------------------------------------------------------------------
# 6. frames are independent
# ------------------------------------------------------------------------------------------
def test_a_frames_map_does_not_depend_on_the_others(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    m_a, _, _ = _map(ctx, net, ctx.dev(xs[0]), 16, recon=False)
    x = xs[0].copy()
    x[1] = xs[1][1]
    m_b, _, _ = _map(ctx, net, ctx.dev(x), 16, recon=False)
    assert np.array_equal(m_a[0], m_b[0]) and np.array_equal(m_a[2], m_b[2]) and not np.array_equal(m_a[1], m_b[1])


# ------------------------------------------------------------------------------------------
# 7. training is undisturbed
# ------------------------------------------------------------------------------------------
def _map_between(ctx, net, steps):
    other = F.u8(ctx, F.other_frames(steps[0].shape)[0], steps[0])
    m8, m32 = ctx.empty(net.B, net.Nx // 8, net.Ny // 8), ctx.empty(net.B, net.Nx // 32, net.Ny // 32)
    sc, rec = ctx.empty(net.B), ctx.empty(net.B, net.D, net.Nx, net.Ny)

    def hook(k, x):
        if k == 0:
            net.score_map(x, 8, m8, sc, rec)      # straight behind step_apply: the frames of the step, with the store
        if k == 1:
            net.score_map(other, 32, m32, sc)     # other frames, 8-bit, without the store
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed(ctx, flags, name, path, form, ready):
    """[step, step, step] against [step, map, step, map(other frames, 8-bit, no recon), step]: reconstructions, packed gradients with their
    MSE tail, MSEs and weights after every step bit for bit"""
    flags(path)
    assert F.net(ctx, name).step_form() == form
    plain = F.train(ctx, name, ready, _map_between)
    mixed = F.train(ctx, name, ready, _map_between, at="apply")
    F.assert_same_training(plain, mixed)


def test_score_is_the_same_before_and_after_a_map(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    s_a, _ = _score(ctx, net, frames, recon=False)
    _map(ctx, net, ctx.dev(xs[1]), 8)
    s_b, _ = _score(ctx, net, frames, recon=False)
    assert np.array_equal(s_a, s_b)


# ------------------------------------------------------------------------------------------
# 8. launch counts
# ------------------------------------------------------------------------------------------
def _five(c):
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0, c
    return c["r2c_rows"] == 1 and c["r2c_cols"] == 1 and c["c2r_cols"] == 1 and c["c2r_rows"] == 1 and c["score_map"] == 1


def test_launch_counts(ctx, flags):
    flags()
    name = "256-4pairs"
    ws, xs = _case(name)
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    assert net.step_form() == "operator_chain"
    _counted = lambda ctx, net, frames, score: F.counted(ctx, lambda: _map(ctx, net, frames, 16, recon=False, score=score))
    (m1, _, _), c = _counted(ctx, net, frames, False)
    assert c["chain"] >= 1 and c["score_map"] == 1 and c["score"] == 0, c
    # the chain form with the operators at hand: R2C rows and columns, inverse columns with the operator on load, the mapping row pass, the map finish
    (m2, _, _), c = _counted(ctx, net, frames, False)
    assert _five(c) and c["score"] == 0 and sum(c.values()) == 5, c
    assert np.array_equal(m1, m2)
    (m3, _, _), c = _counted(ctx, net, frames, True)
    assert _five(c) and c["score"] == 1 and sum(c.values()) == 6, c
    assert np.array_equal(m3, m2)
    # behind step_apply the step's last launch has carried the chain ahead
    net.step_grad(frames); net.step_apply(0.02); ctx.sync()
    (m4, _, _), c = _counted(ctx, net, frames, False)
    assert _five(c) and c["score"] == 0 and sum(c.values()) == 5, c
    (m5, _, _), c = _counted(ctx, net, frames, True)
    assert _five(c) and c["score"] == 1 and sum(c.values()) == 6, c
    assert np.isfinite(m4).all() and not np.array_equal(m4, m2) and np.array_equal(m5, m4)


# ------------------------------------------------------------------------------------------
# 9. state and errors
# ------------------------------------------------------------------------------------------
def _refused(ctx, net, frames, tile, what="tile"):
    """AEFFT_EINVAL with the rule in the message, every output still NaN"""
    m = ctx.empty(net.B * max(net.Nx // 8, 1) * max(net.Ny // 8, 1)); m.fill_(float("nan"))
    sc = ctx.empty(net.B); sc.fill_(float("nan"))
    rec = ctx.empty(net.B, net.D, net.Nx, net.Ny); rec.fill_(float("nan"))
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*{what}"):
        net.score_map(frames, tile, m, sc, rec)
    ctx.sync()
    assert np.isnan(host(m)).all() and np.isnan(host(sc)).all() and np.isnan(host(rec)).all(), tile


def test_state_and_errors(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    L = len(ws)
    # the call ends a pending step_grad
    net.step_grad(frames)
    m, _, rec = _map(ctx, net, frames, 8)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.02)
    # layer exports are those of the call
    top = host(net.get_layer(4 * L)).copy()
    print("get_layer(4L) against recon: bit-equal", np.array_equal(top, rec), "relative", relerr(top, rec))
    assert relerr(top, rec) < TOL
    # tiles
    for tile in (4, 12, 128, 0):
        _refused(ctx, net, frames, tile)
    for other, tiles in (("240x320", (32,)), ("24x40", (64,))):
        n2 = F.net(ctx, other)
        for tile in tiles:
            _refused(ctx, n2, ctx.dev(_case(other)[1][0]), tile)
    n3 = F.net(ctx, "10x24")
    for tile in TILES:
        _refused(ctx, n3, ctx.dev(_case("10x24")[1][0]), tile)
    # pointers: AEFFT_EINVAL, outputs untouched
    mp = ctx.empty(net.B, net.Nx // 8, net.Ny // 8); mp.fill_(float("nan"))
    sc = ctx.empty(net.B); sc.fill_(float("nan"))
    rc_ = ctx.empty(net.B, net.D, net.Nx, net.Ny); rc_.fill_(float("nan"))
    einval = f"aefft error {aefft.EINVAL}:"
    for args in ((None, 8, mp, sc, rc_), (frames.reshape(-1)[1:], 8, mp, sc, rc_), (frames, 8, mp.reshape(-1)[1:], sc, rc_),
                 (frames, 8, mp, ctx.empty(net.B + 1)[1:], rc_), (frames, 8, mp, sc, rc_.reshape(-1)[1:])):
        with pytest.raises(aefft.AefftError, match=einval):
            net.score_map(*args)
    P = aefft._ptr
    assert net.L.aefft_net_score_map(net.h, P(frames), 0, 8, None, P(sc), P(rc_)) == aefft.EINVAL       # null map_d
    assert net.L.aefft_net_score_map(None, P(frames), 0, 8, P(mp), P(sc), P(rc_)) == aefft.EINVAL       # null net
    ctx.sync()
    assert np.isnan(host(mp)).all() and np.isnan(host(sc)).all() and np.isnan(host(rc_)).all()


# ------------------------------------------------------------------------------------------
# 10. the unfused routes
# ------------------------------------------------------------------------------------------
def test_spatial_net(ctx, flags):
    flags()
    rng = np.random.default_rng(3)
    D, N, maps, B = 3, 32, [4], 2
    net = F.track(aefft.Net(ctx, D, N, N, maps, 3, 2, B, spatial=True))
    for l, w in enumerate(_weights(rng, D, maps, 3, 3)):
        net.set_pair(l, *w)
    x = np.floor(rng.uniform(0, 256, (B, D, N, N)))
    frames = ctx.dev(x)
    rec_i, _ = _infer(ctx, net, frames)
    for t in (8, 16):
        m, s, rec = _map(ctx, net, frames, t)
        assert np.array_equal(rec, rec_i)
        _check_reduction("spatial", x, m, rec, t)
        assert (np.abs(s - np.float32(m.astype(np.float64).mean((1, 2)))) <= np.spacing(s)).all()
    mp = ctx.empty(B, N // 8, N // 8); mp.fill_(float("nan"))
    einval = f"aefft error {aefft.EINVAL}:"
    with pytest.raises(aefft.AefftError, match=einval + ".*recon_d"):
        net.score_map(frames, 8, mp, None, None)
    rc_ = ctx.empty(B, D, N, N); rc_.fill_(float("nan"))
    with pytest.raises(aefft.AefftError, match=einval):
        net.score_map(F.u8(ctx, x, frames), 8, mp, None, rc_)
    ctx.sync()
    assert np.isnan(host(mp)).all() and np.isnan(host(rc_)).all()


def test_chirpz_route(ctx, flags):
    flags("CHIRPZ")
    name = "240x320"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    rec_i, _ = _infer(ctx, net, frames)
    m, _, rec = _map(ctx, net, frames, 16)
    assert np.array_equal(rec, rec_i)
    _check_reduction("chirpz", xs[0], m, rec, 16)
    mp = ctx.empty(net.B, net.Nx // 16, net.Ny // 16); mp.fill_(float("nan"))
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*recon_d"):
        net.score_map(frames, 16, mp, None, None)
    ctx.sync()
    assert np.isnan(host(mp)).all()
