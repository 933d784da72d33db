"""aefft_net_score_target / aefft_net_score_map_target (Net.score_target, Net.score_map_target): the score calls with the reconstruction
compared against a target instead of the frame the net read -- the plain calls' bits when the target is the frame, the reduction against the
returned float reconstruction with an independent target, float and 8-bit targets bit for bit, with and without the store, the unfused routes
(spatial net, chirp-z transforms), and errors that leave the outputs untouched."""
import functools
import importlib

import numpy as np
import pytest
import torch

import frozen_cases as F
from frozen_cases import CASES, _case, _weights, host
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import _infer
from test_gpu_score import _check_reduction as _check_score, _score
from test_gpu_score_map import _check_reduction as _check_map, _map

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

NAMES = ["64-2pairs", "240x320", "D4"]


@functools.lru_cache(maxsize=None)
def _target(name):
    """8-bit-valued pixels that have nothing to do with the case's frames"""
    D, Nx, Ny, maps, Nk, Nl, s, B, *_ = CASES[name]
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    return np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))


def _score_t(ctx, net, frames, targets, recon=True):
    sc = F.nan(ctx, net.B)
    rec = F.nan(ctx, net.B, net.D, net.Nx, net.Ny) if recon else None
    out = net.score_target(frames, targets, sc, rec)
    assert out[0] is sc and out[1] is rec
    ctx.sync()
    return host(sc).copy(), (None if rec is None else host(rec).copy())


def _map_t(ctx, net, frames, targets, tile, recon=True, score=True):
    m = F.nan(ctx, net.B, net.Nx // tile, net.Ny // tile)
    sc = F.nan(ctx, net.B) if score else None
    rec = F.nan(ctx, net.B, net.D, net.Nx, net.Ny) if recon else None
    if score:
        out = net.score_map_target(frames, targets, tile, m, sc, rec)
        assert out[0] is m and out[1] is sc and out[2] is rec
    else:
        P = aefft._ptr
        ctx.check(net.L.aefft_net_score_map_target(net.h, P(frames), int(frames.dtype == torch.uint8), P(targets), int(targets.dtype == torch.uint8), tile,
                                                   P(m), None, P(rec)))
    ctx.sync()
    return host(m).copy(), (None if sc is None else host(sc).copy()), (None if rec is None else host(rec).copy())


@pytest.mark.parametrize("name", NAMES)
def test_the_frames_as_target_give_the_plain_calls_bits(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    f32 = ctx.dev(xs[0])
    u8 = F.u8(ctx, xs[0], f32)
    for fr in (f32, u8):
        s, rec = _score(ctx, net, fr)
        s_t, rec_t = _score_t(ctx, net, fr, fr)
        assert np.array_equal(s_t, s) and np.array_equal(rec_t, rec), name
        s_x, _ = _score_t(ctx, net, f32, fr, recon=False)            # (the same pixels in the other type)
        assert np.array_equal(s_x, s), name
        for t in F.tiles(name):
            m, sm, _ = _map(ctx, net, fr, t)
            m_t, sm_t, rec_t = _map_t(ctx, net, fr, fr, t)
            assert np.array_equal(m_t, m) and np.array_equal(sm_t, sm) and np.array_equal(rec_t, rec), (name, t)


@pytest.mark.parametrize("name", NAMES)
def test_an_independent_target(ctx, flags, name):
    """the bounds of test_gpu_score.py / test_gpu_score_map.py (_check_reduction, RTOL) with the target in the frame's place"""
    flags()
    ws, xs = _case(name)
    tg = _target(name)
    net = F.net(ctx, name)
    f32 = ctx.dev(xs[0])
    f8 = F.u8(ctx, xs[0], f32)
    t32 = ctx.dev(tg)
    t8 = F.u8(ctx, tg, f32)
    rec_i, _ = _infer(ctx, net, f32)
    s, rec = _score_t(ctx, net, f32, t32)
    assert np.array_equal(rec, rec_i), name
    _check_score(name + " (target)", tg, s, rec)
    s_plain, _ = _score(ctx, net, f32, recon=False)
    assert not np.array_equal(s, s_plain), name                      # (the target entered)
    for fr, t in ((f32, t8), (f8, t32), (f8, t8)):
        s_b, rec_b = _score_t(ctx, net, fr, t)
        assert np.array_equal(s_b, s) and np.array_equal(rec_b, rec_i), name
    s_0, _ = _score_t(ctx, net, f32, t32, recon=False)
    s_80, _ = _score_t(ctx, net, f32, t8, recon=False)
    assert np.array_equal(s_0, s) and np.array_equal(s_80, s), name
    for tile in F.tiles(name):
        m, sm, rec_m = _map_t(ctx, net, f32, t32, tile)
        assert np.array_equal(rec_m, rec_i), (name, tile)
        _check_map(name + " (target)", tg, m, rec_m, tile)
        want = np.float32(m.astype(np.float64).mean((1, 2)))
        assert (np.abs(sm - want) <= np.spacing(np.abs(want))).all(), (name, tile)
        for fr, t, rc in ((f32, t8, True), (f8, t8, True), (f32, t32, False), (f32, t8, False)):
            m_b, sm_b, _ = _map_t(ctx, net, fr, t, tile, recon=rc)
            assert np.array_equal(m_b, m) and np.array_equal(sm_b, sm), (name, tile)
        m_n, s_n, _ = _map_t(ctx, net, f32, t32, tile, recon=False, score=False)
        assert s_n is None and np.array_equal(m_n, m), (name, tile)


def test_spatial_net(ctx, flags):
    flags()
    rng = np.random.default_rng(3)
    D, N, maps, B = 3, 32, [4], 2
    net = F.track(aefft.Net(ctx, D, N, N, maps, 3, 2, B, spatial=True))
    for l, w in enumerate(_weights(rng, D, maps, 3, 3)):
        net.set_pair(l, *w)
    x = np.floor(rng.uniform(0, 256, (B, D, N, N)))
    tg = np.floor(rng.uniform(0, 256, (B, D, N, N)))
    frames, targets = ctx.dev(x), ctx.dev(tg)
    rec_i, _ = _infer(ctx, net, frames)
    s, rec = _score_t(ctx, net, frames, targets)
    assert np.array_equal(rec, rec_i)
    _check_score("spatial (target)", tg, s, rec)
    s_p, _ = _score_t(ctx, net, frames, frames)
    assert np.array_equal(s_p, _score(ctx, net, frames)[0])
    for t in (8, 16):
        m, sm, rec = _map_t(ctx, net, frames, targets, t)
        assert np.array_equal(rec, rec_i)
        _check_map("spatial (target)", tg, m, rec, t)
    # float frames and float targets only; the stored reconstruction is needed
    einval = f"aefft error {aefft.EINVAL}:"
    sc, mp, rc_ = F.nan(ctx, B), F.nan(ctx, B, N // 8, N // 8), F.nan(ctx, B, D, N, N)
    with pytest.raises(aefft.AefftError, match=einval):
        net.score_target(frames, F.u8(ctx, tg, frames), sc, rc_)
    with pytest.raises(aefft.AefftError, match=einval):
        net.score_map_target(F.u8(ctx, x, frames), targets, 8, mp, sc, rc_)
    with pytest.raises(aefft.AefftError, match=einval + ".*recon_d"):
        net.score_target(frames, targets, sc, None)
    with pytest.raises(aefft.AefftError, match=einval + ".*recon_d"):
        net.score_map_target(frames, targets, 8, mp, sc, None)
    ctx.sync()
    assert np.isnan(host(sc)).all() and np.isnan(host(mp)).all() and np.isnan(host(rc_)).all()


def test_chirpz_route(ctx, flags):
    flags("CHIRPZ")
    name = "240x320"
    ws, xs = _case(name)
    tg = _target(name)
    net = F.net(ctx, name)
    frames, targets = ctx.dev(xs[0]), ctx.dev(tg)
    rec_i, _ = _infer(ctx, net, frames)
    s, rec = _score_t(ctx, net, frames, targets)
    assert np.array_equal(rec, rec_i)
    _check_score("chirpz (target)", tg, s, rec)
    s8, _ = _score_t(ctx, net, frames, F.u8(ctx, tg, frames))
    assert np.array_equal(s8, s)
    m, _, rec = _map_t(ctx, net, frames, targets, 16)
    assert np.array_equal(rec, rec_i)
    _check_map("chirpz (target)", tg, m, rec, 16)
    sc, mp = F.nan(ctx, net.B), F.nan(ctx, net.B, net.Nx // 16, net.Ny // 16)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*recon_d"):
        net.score_target(frames, targets, sc, None)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*recon_d"):
        net.score_map_target(frames, targets, 16, mp, sc, None)
    ctx.sync()
    assert np.isnan(host(sc)).all() and np.isnan(host(mp)).all()


def test_errors_leave_the_outputs_untouched(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames, targets = ctx.dev(xs[0]), ctx.dev(_target(name))
    sc, mp, rc_ = F.nan(ctx, net.B), F.nan(ctx, net.B, net.Nx // 8, net.Ny // 8), F.nan(ctx, net.B, net.D, net.Nx, net.Ny)
    einval = f"aefft error {aefft.EINVAL}:"
    off = lambda t: t.reshape(-1)[1:]
    for args in ((frames, None), (frames, off(targets)), (None, targets), (off(frames), targets)):
        with pytest.raises(aefft.AefftError, match=einval):
            net.score_target(*args, sc, rc_)
        with pytest.raises(aefft.AefftError, match=einval):
            net.score_map_target(*args, 8, mp, sc, rc_)
    for tile in (4, 12, 128, 0):
        with pytest.raises(aefft.AefftError, match=einval + ".*tile"):
            net.score_map_target(frames, targets, tile, mp, sc, rc_)
    P = aefft._ptr
    assert net.L.aefft_net_score_target(net.h, P(frames), 0, P(targets), 0, None, P(rc_)) == aefft.EINVAL            # null score_d
    assert net.L.aefft_net_score_map_target(net.h, P(frames), 0, P(targets), 0, 8, None, P(sc), P(rc_)) == aefft.EINVAL  # null map_d
    assert net.L.aefft_net_score_target(None, P(frames), 0, P(targets), 0, P(sc), P(rc_)) == aefft.EINVAL
    ctx.sync()
    assert np.isnan(host(sc)).all() and np.isnan(host(mp)).all() and np.isnan(host(rc_)).all()
    # the call ends a pending step_grad, as the plain one
    net.step_grad(frames)
    _score_t(ctx, net, frames, targets)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.02)
