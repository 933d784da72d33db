"""aefft_net_ssim_map (Net.ssim_map): block SSIM of the reconstruction under frozen weights -- the five-moment strip reduction against float64
block SSIM of the returned float reconstruction on every row-pass route and every tile, bit equality across the variants, score_d as a
function of the map, against the float64 oracle in every form, frames independent of one another, training undisturbed bit for bit, the
launch counts by the profiler, state and errors, and the unfused routes (spatial net, chirp-z transforms)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import frozen_cases as F
from frozen_cases import PATHS, _case, _identity_case, _oracle_recon, _weights, host, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import TOL, _infer
from test_gpu_score_map import ORDER

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# 1. A map entry against float64 block SSIM of the RETURNED float reconstruction.  The largest absolute deviation measured on the MI355X over
# every case and tile below is MEASURED_MAP; the bound is 4 x that, rounded up to one digit -- the margin is for the
# rounding patterns of other inputs.  The measured value itself stays within 1e-4, the resolution SSIM is quoted at.
MEASURED_MAP = 4.75e-5
ATOL_MAP = 2e-4
# 4. A map entry against block SSIM of the float64 ORACLE reconstruction: the reconstruction differs from the oracle's by up to TOL * max|recon|
# per pixel, and SSIM's sensitivity to that depends on each window's variance, so the bound is 4 x the largest deviation measured (section 19),
# rounded up to one digit.
MEASURED_ORACLE = 4.75e-5
ATOL_ORACLE = 2e-4


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _ssim_ref(x, r, t, L):
    """numpy's float64 block SSIM -- uniform weights, population statistics, t x t windows -- averaged over the channels: [B][Nx/t][Ny/t]"""
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    B, D, Nx, Ny = x.shape
    w = lambda a: a.reshape(B, D, Nx // t, t, Ny // t, t).mean((3, 5))
    mx, mr = w(x), w(r)
    vx, vr, c = np.maximum(w(x * x) - mx * mx, 0), np.maximum(w(r * r) - mr * mr, 0), w(x * r) - mx * mr
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    return ((2 * mx * mr + C1) * (2 * c + C2) / ((mx * mx + mr * mr + C1) * (vx + vr + C2))).mean(1)


@functools.lru_cache(maxsize=None)
def _targets(name, t):
    """the float64 oracle's reconstruction plus Gaussian noise whose amplitude is, per window of the map (the D channels of a t x t tile), a
    factor from U(0, 2) times that window's standard deviation -- the factors a stratified sample with both ends, one per window of the
    batch in random order, so that three windows spread as a thousand do.  (float32 values, data_range = max - min)"""
    rec = _oracle_recon(name)
    B, D, Nx, Ny = rec.shape
    rng = np.random.default_rng(77 + t + sum(map(ord, name)))
    return _noisy(rng, rec, t)


def _noisy(rng, rec, t):
    B, D, Nx, Ny = rec.shape
    nw = B * (Nx // t) * (Ny // t)
    a = rng.permutation(np.arange(nw) * (2.0 / (nw - 1))).reshape(B, 1, Nx // t, 1, Ny // t, 1)
    sd = np.asarray(rec, np.float64).reshape(B, D, Nx // t, t, Ny // t, t).std((1, 3, 5), keepdims=True)
    tg = _f32(rec + (a * sd * rng.standard_normal((B, D, Nx // t, t, Ny // t, t))).reshape(rec.shape))
    return tg, float(np.float32(tg.max() - tg.min()))


def _spread(name, t):
    """the reference map, from the float64 oracle alone, spans at least [0.5, 0.95]: a map that is ~0 or ~1 everywhere tests nothing"""
    tg, L = _targets(name, t)
    ref = _ssim_ref(tg, _oracle_recon(name), t, L)
    assert ref.min() <= 0.5 and ref.max() >= 0.95, (name, t, ref.min(), ref.max())
    return ref


def _ssim(ctx, net, frames, tile, targets=None, L=255.0, recon=True, score=True):
    """one aefft_net_ssim_map: (map, score or None, reconstruction or None) as host arrays; the outputs start as NaN.  (Net.ssim_map always hands
    a score buffer over: score_d = NULL goes through the C entry.)"""
    m = F.nan(ctx, net.B, net.Nx // tile, net.Ny // tile)
    sc = F.nan(ctx, net.B) if score else None
    rec = F.nan(ctx, net.B, net.D, net.Nx, net.Ny) if recon else None
    if score:
        out = net.ssim_map(frames, tile, targets, L, m, sc, rec)
        assert out[0] is m and out[1] is sc and out[2] is rec
    else:
        P = aefft._ptr
        ctx.check(net.L.aefft_net_ssim_map(net.h, P(frames), int(frames.dtype == torch.uint8), P(targets), int(targets is not None and targets.dtype == torch.uint8),
                                           tile, float(L), P(m), None, P(rec)))
    ctx.sync()
    return host(m).copy(), (None if sc is None else host(sc).copy()), (None if rec is None else host(rec).copy())


def _check_map(what, m, ref, atol):
    assert m.shape == ref.shape, (what, m.shape, ref.shape)
    err = np.abs(m.astype(np.float64) - ref)
    print(f"SSIM {what}: map {m.shape} in [{ref.min():.3f}, {ref.max():.3f}], largest absolute deviation {err.max():.3e}")
    assert np.isfinite(m).all() and (err <= atol).all(), (what, err.max())


def test_the_recorded_deviation_is_within_the_resolution_ssim_is_quoted_at():
    assert 0 < MEASURED_MAP <= 1e-4 and 4 * MEASURED_MAP <= ATOL_MAP < 4 * MEASURED_MAP + 10 ** np.floor(np.log10(4 * MEASURED_MAP))
    assert 0 < MEASURED_ORACLE and 4 * MEASURED_ORACLE <= ATOL_ORACLE < 4 * MEASURED_ORACLE + 10 ** np.floor(np.log10(4 * MEASURED_ORACLE))


# ------------------------------------------------------------------------------------------
# 1. the map against the returned reconstruction, 2. bit equality across the variants
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER)
def test_map_is_the_block_ssim_of_the_returned_reconstruction(ctx, flags, name):
    refs = {t: _spread(name, t) for t in F.tiles(name)}          # (before the GPU is touched)
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    F._form(net, name)
    f32 = ctx.dev(xs[0])
    rec_i, _ = _infer(ctx, net, f32)
    for t in F.tiles(name):
        tg, L = _targets(name, t)
        t32 = ctx.dev(tg)
        m, _, rec = _ssim(ctx, net, f32, t, t32, L)
        assert np.array_equal(rec, rec_i), (name, t)
        _check_map(f"{name} tile {t}", m, _ssim_ref(tg, rec, t, L), ATOL_MAP)
        # 2. without the store, 8-bit frames, a repeated call
        m0, _, _ = _ssim(ctx, net, f32, t, t32, L, recon=False)
        m8, _, _ = _ssim(ctx, net, F.u8(ctx, xs[0], f32), t, t32, L, recon=False)
        m1, _, _ = _ssim(ctx, net, f32, t, t32, L)
        assert np.array_equal(m0, m) and np.array_equal(m8, m) and np.array_equal(m1, m), (name, t)
        # float and 8-bit targets of the same (integer-valued) pixels
        ti = np.clip(np.rint((tg - tg.min()) * (255.0 / L)), 0, 255)
        mi, _, rec = _ssim(ctx, net, f32, t, ctx.dev(ti), 255.0)
        mi8, _, _ = _ssim(ctx, net, f32, t, F.u8(ctx, ti, f32), 255.0, recon=False)
        _check_map(f"{name} tile {t} (8-bit range)", mi, _ssim_ref(ti, rec, t, 255.0), ATOL_MAP)
        assert np.array_equal(mi8, mi), (name, t)
        # the frames as the target against no target (random weights: a map near 0, which does not count toward the spread)
        mf, _, rec = _ssim(ctx, net, f32, t, f32, 255.0)
        mn, _, _ = _ssim(ctx, net, f32, t, None, 255.0, recon=False)
        mn8, _, _ = _ssim(ctx, net, F.u8(ctx, xs[0], f32), t, None, 255.0, recon=False)
        _check_map(f"{name} tile {t} (no target)", mf, _ssim_ref(xs[0], rec, t, 255.0), ATOL_MAP)
        assert np.array_equal(mn, mf) and np.array_equal(mn8, mf), (name, t)
    assert refs


@pytest.mark.parametrize("tile", [8, 64])
def test_a_small_residual(ctx, flags, tile):
    """targets = None, L = 255 on a net that nearly reproduces its input: SSIM ~ 1 from a small residual"""
    flags()
    (D, N, dM, Nk, B), w, x, rec_o = _identity_case()
    net = F.track(aefft.Net(ctx, D, N, N, [dM], Nk, 1, batch=B))
    net.set_pair(0, *w)
    f32 = ctx.dev(x)
    rec_i, _ = _infer(ctx, net, f32)
    m, _, rec = _ssim(ctx, net, f32, tile)
    m8, _, rec8 = _ssim(ctx, net, F.u8(ctx, x, f32), tile)
    m0, _, _ = _ssim(ctx, net, f32, tile, recon=False)
    assert np.array_equal(rec, rec_i) and np.array_equal(rec8, rec_i)
    ref = _ssim_ref(x, rec, tile, 255.0)
    assert ref.min() > 0.99 and ref.max() < 1.0
    _check_map(f"identity tile {tile}", m, ref, ATOL_MAP)
    assert np.array_equal(m0, m) and np.array_equal(m8, m)
    _check_map(f"identity tile {tile} (oracle)", m, _ssim_ref(x, rec_o, tile, 255.0), ATOL_ORACLE)


# ------------------------------------------------------------------------------------------
# 3. score_d
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER)
def test_score_is_the_mean_of_the_map(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    f32 = ctx.dev(xs[0])
    for t in F.tiles(name):
        tg, L = _targets(name, t)
        t32 = ctx.dev(tg)
        m, s, _ = _ssim(ctx, net, f32, t, t32, L, recon=False)
        want = np.float32(m.astype(np.float64).mean((1, 2)))
        print(f"{name} tile {t}: score {s}, mean of the map {want}")
        assert (np.abs(s - want) <= np.spacing(np.abs(want))).all(), (name, t, s, want)
        m0, s0, _ = _ssim(ctx, net, f32, t, t32, L, recon=False, score=False)
        assert s0 is None and np.array_equal(m0, m), (name, t)


# ------------------------------------------------------------------------------------------
# 4. the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [(n, p) for n in ("64-2pairs", "256-4pairs") for p in PATHS] + [(n, "") for n in ORDER if n not in ("64-2pairs", "256-4pairs")])
def test_map_against_the_oracle(ctx, flags, name, path):
    refs = {t: _spread(name, t) for t in F.tiles(name)}
    flags(path)
    ws, xs = _case(name)
    net = F.net(ctx, name)
    F._form(net, name, path)
    frames = ctx.dev(xs[0])
    for k in range(2):          # the second call from the cached operators
        for t in F.tiles(name):
            tg, L = _targets(name, t)
            m, _, _ = _ssim(ctx, net, frames, t, ctx.dev(tg), L, recon=bool(k), score=bool(k))
            _check_map(f"{name} {path} tile {t} (oracle)", m, refs[t], ATOL_ORACLE)


# ------------------------------------------------------------------------------------------
# 5. frames are independent
# ------------------------------------------------------------------------------------------
def test_a_frames_map_does_not_depend_on_the_others(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    tg, L = _targets(name, 16)
    net = F.net(ctx, name)
    m_a, _, _ = _ssim(ctx, net, ctx.dev(xs[0]), 16, ctx.dev(tg), L, recon=False)
    x, t2 = xs[0].copy(), tg.copy()
    x[1] = xs[1][1]
    m_b, _, _ = _ssim(ctx, net, ctx.dev(x), 16, ctx.dev(t2), L, recon=False)
    assert np.array_equal(m_a[0], m_b[0]) and np.array_equal(m_a[2], m_b[2]) and not np.array_equal(m_a[1], m_b[1])
    t2[1] = tg[0]
    m_c, _, _ = _ssim(ctx, net, ctx.dev(xs[0]), 16, ctx.dev(t2), L, recon=False)
    assert np.array_equal(m_a[0], m_c[0]) and np.array_equal(m_a[2], m_c[2]) and not np.array_equal(m_a[1], m_c[1])


# ------------------------------------------------------------------------------------------
# 6. training is undisturbed
# ------------------------------------------------------------------------------------------
def _ssim_between(ctx, net, steps):
    other, target = (F.u8(ctx, o, steps[0]) for o in F.other_frames(steps[0].shape))
    m8, m32 = ctx.empty(net.B, net.Nx // 8, net.Ny // 8), ctx.empty(net.B, net.Nx // 32, net.Ny // 32)
    sc, rec = ctx.empty(net.B), ctx.empty(net.B, net.D, net.Nx, net.Ny)

    def hook(k, x):
        if k == 0:
            net.ssim_map(x, 8, target, 255.0, m8, sc, rec)          # straight behind step_apply: the frames of the step, with the store
            net.score_map_target(x, target, 8, m8, sc)
        if k == 1:
            net.score_map_target(other, target, 32, m32, sc, rec)
            net.ssim_map(other, 32, None, 255.0, m32, sc)           # other frames, 8-bit, without the store
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed(ctx, flags, name, path, form, ready):
    """[step, step, step] against [step, ssim + map_target, step, map_target + ssim (other frames, 8-bit, no recon), step]: reconstructions,
    packed gradients with their MSE tail, MSEs and weights after every step bit for bit"""
    flags(path)
    assert F.net(ctx, name).step_form() == form
    plain = F.train(ctx, name, ready, _ssim_between)
    mixed = F.train(ctx, name, ready, _ssim_between, at="apply")
    F.assert_same_training(plain, mixed)


# ------------------------------------------------------------------------------------------
# 7. launch counts
# ------------------------------------------------------------------------------------------
def _five(c):
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0 and c["score_map"] == 0, c
    return c["r2c_rows"] == 1 and c["r2c_cols"] == 1 and c["c2r_cols"] == 1 and c["c2r_rows"] == 1 and c["ssim"] == 1


def test_launch_counts(ctx, flags):
    flags()
    name = "256-4pairs"
    ws, xs = _case(name)
    frames = ctx.dev(xs[0])
    targets = F.u8(ctx, xs[1], frames)
    net = F.net(ctx, name)
    assert net.step_form() == "operator_chain"
    _counted = lambda ctx, net, frames, targets, score: F.counted(ctx, lambda: _ssim(ctx, net, frames, 16, targets, 255.0, recon=False, score=score))
    (m1, _, _), c = _counted(ctx, net, frames, targets, False)
    assert c["chain"] >= 1 and c["ssim"] == 1 and c["score"] == 0 and c["score_map"] == 0, c
    # the chain form with the operators at hand: R2C rows and columns, inverse columns with the operator on load, the SSIM row pass, the finish
    (m2, _, _), c = _counted(ctx, net, frames, targets, False)
    assert _five(c) and c["score"] == 0 and sum(c.values()) == 5, c
    assert np.array_equal(m1, m2)
    (m3, _, _), c = _counted(ctx, net, frames, targets, True)
    assert _five(c) and c["score"] == 1 and sum(c.values()) == 6, c
    assert np.array_equal(m3, m2)
    (m4, _, _), c = _counted(ctx, net, frames, None, False)
    assert _five(c) and c["score"] == 0 and sum(c.values()) == 5, c
    # behind step_apply the step's last launch has carried the chain ahead
    net.step_grad(frames); net.step_apply(0.02); ctx.sync()
    (m5, _, _), c = _counted(ctx, net, frames, targets, True)
    assert _five(c) and c["score"] == 1 and sum(c.values()) == 6, c
    assert np.isfinite(m5).all() and not np.array_equal(m5, m2)


# ------------------------------------------------------------------------------------------
# 8. state and errors
# ------------------------------------------------------------------------------------------
def _refused(ctx, net, frames, targets, tile, L, what):
    """AEFFT_EINVAL with the rule in the message, every output still NaN"""
    m = F.nan(ctx, net.B * max(net.Nx // 8, 1) * max(net.Ny // 8, 1))
    sc, rec = F.nan(ctx, net.B), F.nan(ctx, net.B, net.D, net.Nx, net.Ny)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*{what}"):
        net.ssim_map(frames, tile, targets, L, m, sc, rec)
    ctx.sync()
    assert np.isnan(host(m)).all() and np.isnan(host(sc)).all() and np.isnan(host(rec)).all(), (tile, L)


def test_state_and_errors(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    tg, L = _targets(name, 8)
    targets = ctx.dev(tg)
    nL = len(ws)
    # refused in front of the net's first SSIM call as well
    _refused(ctx, net, frames, targets, 8, 0.0, "data_range")
    # the call ends a pending step_grad
    net.step_grad(frames)
    m, _, rec = _ssim(ctx, net, frames, 8, targets, L)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.02)
    # layer exports are those of the call
    top = host(net.get_layer(4 * nL)).copy()
    assert relerr(top, rec) < TOL
    for tile in (4, 12, 128, 0):
        _refused(ctx, net, frames, targets, tile, L, "tile")
    for other, tiles in (("240x320", (32,)), ("24x40", (64,))):
        n2 = F.net(ctx, other)
        for tile in tiles:
            _refused(ctx, n2, ctx.dev(_case(other)[1][0]), None, tile, 255.0, "tile")
    for bad in (0.0, -255.0, float("nan"), float("inf")):
        _refused(ctx, net, frames, targets, 8, bad, "data_range")
    # pointers: AEFFT_EINVAL, outputs untouched
    mp, sc, rc_ = F.nan(ctx, net.B, net.Nx // 8, net.Ny // 8), F.nan(ctx, net.B), F.nan(ctx, net.B, net.D, net.Nx, net.Ny)
    einval = f"aefft error {aefft.EINVAL}:"
    off = lambda t: t.reshape(-1)[1:]
    for args in ((None, 8, targets, L, mp, sc, rc_), (off(frames), 8, targets, L, mp, sc, rc_), (frames, 8, off(targets), L, mp, sc, rc_),
                 (frames, 8, targets, L, off(mp), sc, rc_), (frames, 8, targets, L, mp, ctx.empty(net.B + 1)[1:], rc_), (frames, 8, targets, L, mp, sc, off(rc_))):
        with pytest.raises(aefft.AefftError, match=einval):
            net.ssim_map(*args)
    P = aefft._ptr
    assert net.L.aefft_net_ssim_map(net.h, P(frames), 0, P(targets), 0, 8, L, None, P(sc), P(rc_)) == aefft.EINVAL       # null map_d
    assert net.L.aefft_net_ssim_map(None, P(frames), 0, P(targets), 0, 8, L, P(mp), P(sc), P(rc_)) == aefft.EINVAL       # null net
    ctx.sync()
    assert np.isnan(host(mp)).all() and np.isnan(host(sc)).all() and np.isnan(host(rc_)).all()
    # and the calls around it give what they gave
    m_b, _, _ = _ssim(ctx, net, frames, 8, targets, L, recon=False)
    assert np.array_equal(m_b, m)


# ------------------------------------------------------------------------------------------
# 9. the unfused routes
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
        # (targets from the net's own reconstruction: no oracle of the spatial net is needed for a spread)
        tg, L = _noisy(np.random.default_rng(t), rec_i, t)
        m, s, rec = _ssim(ctx, net, frames, t, ctx.dev(tg), L)
        assert np.array_equal(rec, rec_i)
        ref = _ssim_ref(tg, rec, t, L)
        assert ref.min() <= 0.5 and ref.max() >= 0.95, (ref.min(), ref.max())
        _check_map(f"spatial tile {t}", m, ref, ATOL_MAP)
        assert (np.abs(s - np.float32(m.astype(np.float64).mean((1, 2)))) <= np.spacing(s)).all()
        mn, _, rec = _ssim(ctx, net, frames, t, None, 255.0)
        _check_map(f"spatial tile {t} (no target)", mn, _ssim_ref(x, rec, t, 255.0), ATOL_MAP)
    mp, rc_ = F.nan(ctx, B, N // 8, N // 8), F.nan(ctx, B, D, N, N)
    einval = f"aefft error {aefft.EINVAL}:"
    with pytest.raises(aefft.AefftError, match=einval + ".*recon_d"):
        net.ssim_map(frames, 8, None, 255.0, mp, None, None)
    with pytest.raises(aefft.AefftError, match=einval):
        net.ssim_map(F.u8(ctx, x, frames), 8, None, 255.0, mp, None, rc_)
    with pytest.raises(aefft.AefftError, match=einval):
        net.ssim_map(frames, 8, F.u8(ctx, x, frames), 255.0, mp, None, rc_)
    ctx.sync()
    assert np.isnan(host(mp)).all() and np.isnan(host(rc_)).all()


def test_chirpz_route(ctx, flags):
    name = "240x320"
    ref_o = _spread(name, 16)
    flags("CHIRPZ")
    ws, xs = _case(name)
    tg, L = _targets(name, 16)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    rec_i, _ = _infer(ctx, net, frames)
    m, _, rec = _ssim(ctx, net, frames, 16, ctx.dev(tg), L)
    assert np.array_equal(rec, rec_i)
    _check_map("chirpz", m, _ssim_ref(tg, rec, 16, L), ATOL_MAP)
    ti = np.clip(np.rint((tg - tg.min()) * (255.0 / L)), 0, 255)
    mi, _, _ = _ssim(ctx, net, frames, 16, ctx.dev(ti), 255.0)
    mi8, _, _ = _ssim(ctx, net, frames, 16, F.u8(ctx, ti, frames), 255.0)
    assert np.array_equal(mi8, mi)
    mp = F.nan(ctx, net.B, net.Nx // 16, net.Ny // 16)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*recon_d"):
        net.ssim_map(frames, 16, None, 255.0, mp, None, None)
    ctx.sync()
    assert np.isnan(host(mp)).all() and ref_o.shape == m.shape
