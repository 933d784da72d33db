"""aefft_net_score (Net.score): the per-frame reconstruction error under frozen weights -- the reduction against the returned float
reconstruction on every row-pass route, with and without the store, 8-bit frames bit for bit, against the float64 oracle in every form,
a trained net's small residual, frames independent of one another, training undisturbed bit for bit, the operator cache by the profiler's
launch counts, state and errors, and the unfused routes (spatial net, chirp-z transforms)."""
import importlib

import numpy as np
import pytest

import frozen_cases as F
from frozen_cases import CASES, PATHS, _case, _identity_case, _oracle_recon, _weights, host, relerr
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)
from test_gpu_infer import TOL, _infer        # 1e-4: the bound test_gpu_infer.py holds the reconstruction to

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# The score against the returned float reconstruction.  Non-negative float32 terms summed along a chain of depth k carry at most k 2^-24
# relative error; each term (x - r)^2 carries two more roundings.  The chains: power-of-two row kernel 8 terms in the
# lane + 6 butterfly levels + at most 4 waves = 18; mixed-radix row kernel 16 + 6 + 4 = 26; score_diff_kernel and the finish in double.
# 4 * 32 * 2^-24 = 7.6e-6 < 1e-5.
RTOL = 1e-5
ORDER = ["64-2pairs", "64x128", "256-4pairs", "no-pooling", "240x320", "240x320-opform", "10x24", "D4"]


def _score(ctx, net, frames, recon=True):
    """one Net.score: (score, reconstruction or None) as host arrays; the outputs start as NaN"""
    sc = ctx.empty(net.B); sc.fill_(float("nan"))
    rec = None
    if recon:
        rec = ctx.empty(net.B, net.D, net.Nx, net.Ny); rec.fill_(float("nan"))
    out = net.score(frames, sc, rec)
    assert out[0] is sc and out[1] is rec
    ctx.sync()
    return host(sc).copy(), (None if rec is None else host(rec).copy())


def _mean_sq(x, r):
    return ((np.asarray(x, np.float64) - np.asarray(r, np.float64)) ** 2).mean(axis=(1, 2, 3))


def _check_reduction(name, x, s, rec):
    ref = _mean_sq(x, rec)
    err = np.abs(s.astype(np.float64) - ref) / ref
    print(f"{name}: score {s} against the returned reconstruction: relative {err.max():.2e}")
    assert np.isfinite(s).all() and (err <= RTOL).all(), (name, err)


def _check_oracle(name, x, s, rec_o):
    s_o = _mean_sq(x, rec_o)
    d = np.abs(np.sqrt(s.astype(np.float64)) - np.sqrt(s_o))
    bound = TOL * np.abs(rec_o).max() + 1e-5 * np.sqrt(s_o)
    print(f"{name}: |sqrt(s) - sqrt(s_o)| {d} bound {bound}")
    assert (d <= bound).all(), (name, d, bound)


# ------------------------------------------------------------------------------------------
# 1. the reduction, 2. with and without the store, 8-bit frames
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER)
def test_score_is_the_mean_square_of_the_returned_reconstruction(ctx, flags, name):
    flags()
    ws, xs = _case(name)
    net = F.net(ctx, name)
    assert net.step_form() == CASES[name][-1]
    f32 = ctx.dev(xs[0])
    u8 = F.u8(ctx, xs[0], f32)
    rec_i, _ = _infer(ctx, net, f32)
    s_f, rec_f = _score(ctx, net, f32)
    s_8, rec_8 = _score(ctx, net, u8)
    assert np.array_equal(rec_f, rec_i), (name, np.abs(rec_f - rec_i).max())
    assert np.array_equal(rec_8, rec_i), name
    _check_reduction(name, xs[0], s_f, rec_f)
    _check_reduction(name + " (8-bit)", xs[0], s_8, rec_8)
    # 2. without the store; 8-bit frames against the same pixels as floats
    s_f0, _ = _score(ctx, net, f32, recon=False)
    s_80, _ = _score(ctx, net, u8, recon=False)
    assert np.array_equal(s_f0, s_f) and np.array_equal(s_80, s_8), name
    assert np.array_equal(s_8, s_f), name


# ------------------------------------------------------------------------------------------
# 3. the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [(n, p) for n in ("64-2pairs", "256-4pairs") for p in PATHS] + [(n, "") for n in ORDER if n not in ("64-2pairs", "256-4pairs")])
def test_score_against_the_oracle(ctx, flags, name, path):
    """the RMS norm's triangle inequality turns the per-pixel bound TOL * max|recon_o| of test_gpu_infer.py into this one"""
    flags(path)
    ws, xs = _case(name)
    net = F.net(ctx, name)
    want = CASES[name][-1]
    if path == "NOOPFORM":
        want = "per_frame"
    elif path == "NOCHAIN" and want == "operator_chain":
        want = "operator"
    assert net.step_form() == want
    frames = ctx.dev(xs[0])
    for k in range(2):          # the second call from the cached operators
        s, _ = _score(ctx, net, frames, recon=bool(k))
        _check_oracle(f"{name} {path}", xs[0], s, _oracle_recon(name))


# ------------------------------------------------------------------------------------------
# 4. a small residual
# ------------------------------------------------------------------------------------------
def test_a_small_residual(ctx, flags):
    """the case a difference contracted into an FMA with the unrounded product fails: the residual is ~3e-3 of the pixels"""
    flags()
    (D, N, dM, Nk, B), w, x, rec_o = _identity_case()
    s_o = _mean_sq(x, rec_o)
    assert (s_o < 1e-4 * (x ** 2).mean(axis=(1, 2, 3))).all(), s_o
    net = F.track(aefft.Net(ctx, D, N, N, [dM], Nk, 1, batch=B))
    net.set_pair(0, *w)
    f32 = ctx.dev(x)
    rec_i, _ = _infer(ctx, net, f32)
    s, rec = _score(ctx, net, f32)
    s8, rec8 = _score(ctx, net, F.u8(ctx, x, f32))
    s0, _ = _score(ctx, net, f32, recon=False)
    assert np.array_equal(rec, rec_i) and np.array_equal(rec8, rec_i)
    _check_reduction("identity", x, s, rec)
    assert np.array_equal(s0, s) and np.array_equal(s8, s)
    _check_oracle("identity", x, s, rec_o)


# ------------------------------------------------------------------------------------------
# 5. frames are independent
# ------------------------------------------------------------------------------------------
def test_a_frames_score_does_not_depend_on_the_others(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    s_a, _ = _score(ctx, net, ctx.dev(xs[0]), recon=False)
    x = xs[0].copy()
    x[1] = xs[1][1]
    s_b, _ = _score(ctx, net, ctx.dev(x), recon=False)
    assert s_a[0] == s_b[0] and s_a[2] == s_b[2] and s_a[1] != s_b[1], (s_a, s_b)


# ------------------------------------------------------------------------------------------
# 6. training is undisturbed
# ------------------------------------------------------------------------------------------
def _score_between(ctx, net, steps):
    other = F.u8(ctx, F.other_frames(steps[0].shape)[0], steps[0])
    sc, rec = ctx.empty(net.B), ctx.empty(net.B, net.D, net.Nx, net.Ny)

    def hook(k, x):
        if k == 0:
            net.score(x, sc, rec)                 # straight behind step_apply: the frames of the step, with the store
        if k == 1:
            net.score(other, sc, None)            # other frames, 8-bit, without the store
    return hook


@pytest.mark.parametrize("ready", [False, True])
@pytest.mark.parametrize("path,form", [("", "operator_chain"), ("NOCHAIN", "operator"), ("NOOPFORM", "per_frame")])
@pytest.mark.parametrize("name", ["256-4pairs", "64-2pairs"])
def test_training_is_not_disturbed(ctx, flags, name, path, form, ready):
    """[step, step, step] against [step, score, step, score(other frames), step]: reconstructions, packed gradients with their MSE tail,
    MSEs and weights after every step bit for bit"""
    flags(path)
    assert F.net(ctx, name).step_form() == form
    plain = F.train(ctx, name, ready, _score_between)
    mixed = F.train(ctx, name, ready, _score_between, at="apply")
    F.assert_same_training(plain, mixed)


# ------------------------------------------------------------------------------------------
# 7. the cache, by launch counts
# ------------------------------------------------------------------------------------------
def test_operators_are_reused(ctx, flags):
    flags()
    name = "256-4pairs"
    ws, xs = _case(name)
    frames = ctx.dev(xs[0])
    net = F.net(ctx, name)
    assert net.step_form() == "operator_chain"
    _counted = lambda ctx, net, frames, recon: F.counted(ctx, lambda: _score(ctx, net, frames, recon))
    (s1, _), c = _counted(ctx, net, frames, True)
    assert c["chain"] >= 1 and c["score"] == 1, c
    (s2, _), c = _counted(ctx, net, frames, False)
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0, c
    # the chain form with the operators at hand: R2C rows and columns, inverse columns with the operator on load, the scoring row pass, finish
    assert c["r2c_rows"] == 1 and c["r2c_cols"] == 1 and c["c2r_cols"] == 1 and c["c2r_rows"] == 1 and c["score"] == 1 and sum(c.values()) == 5, c
    assert np.array_equal(s1, s2)
    # behind step_apply the step's last launch has carried the chain ahead
    net.step_grad(frames); net.step_apply(0.02); ctx.sync()
    (s3, _), c = _counted(ctx, net, frames, False)
    assert c["chain"] == 0 and c["kspec"] == 0 and c["contract"] == 0 and sum(c.values()) == 5, c
    assert np.isfinite(s3).all() and not np.array_equal(s3, s2)


# ------------------------------------------------------------------------------------------
# 8. state and errors
# ------------------------------------------------------------------------------------------
def test_state_and_errors(ctx, flags):
    flags()
    name = "64-2pairs"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    L = len(ws)
    # the call ends a pending step_grad
    net.step_grad(frames)
    s, rec = _score(ctx, net, frames)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.02)
    # layer exports are those of the call
    top = host(net.get_layer(4 * L)).copy()
    print("get_layer(4L) against recon: bit-equal", np.array_equal(top, rec), "relative", relerr(top, rec))
    assert relerr(top, rec) < TOL
    # argument errors: AEFFT_EINVAL, outputs untouched
    sc = ctx.empty(net.B); sc.fill_(float("nan"))
    rc_ = ctx.empty(net.B, net.D, net.Nx, net.Ny); rc_.fill_(float("nan"))
    einval = f"aefft error {aefft.EINVAL}:"
    for args in ((None, sc, rc_), (frames.reshape(-1)[1:], sc, rc_), (frames, sc, rc_.reshape(-1)[1:]), (frames, ctx.empty(net.B + 1)[1:], rc_)):
        with pytest.raises(aefft.AefftError, match=einval):
            net.score(*args)
    assert net.L.aefft_net_score(net.h, aefft._ptr(frames), 0, None, aefft._ptr(rc_)) == aefft.EINVAL      # null score_d
    assert net.L.aefft_net_score(None, aefft._ptr(frames), 0, aefft._ptr(sc), aefft._ptr(rc_)) == aefft.EINVAL
    ctx.sync()
    assert np.isnan(host(sc)).all() and np.isnan(host(rc_)).all()


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
    s, rec = _score(ctx, net, frames)
    assert np.array_equal(rec, rec_i)
    _check_reduction("spatial", x, s, rec)
    sc = ctx.empty(B); sc.fill_(float("nan"))
    einval = f"aefft error {aefft.EINVAL}:"
    with pytest.raises(aefft.AefftError, match=einval + ".*recon_d"):
        net.score(frames, sc, None)
    rc_ = ctx.empty(B, D, N, N); rc_.fill_(float("nan"))
    with pytest.raises(aefft.AefftError, match=einval):
        net.score(F.u8(ctx, x, frames), sc, rc_)
    ctx.sync()
    assert np.isnan(host(sc)).all() and np.isnan(host(rc_)).all()


def test_chirpz_route(ctx, flags):
    flags("CHIRPZ")
    name = "240x320"
    ws, xs = _case(name)
    net = F.net(ctx, name)
    frames = ctx.dev(xs[0])
    rec_i, _ = _infer(ctx, net, frames)
    s, rec = _score(ctx, net, frames)
    assert np.array_equal(rec, rec_i)
    _check_reduction("chirpz", xs[0], s, rec)
    sc = ctx.empty(net.B); sc.fill_(float("nan"))
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.EINVAL}:.*recon_d"):
        net.score(frames, sc, None)
    ctx.sync()
    assert np.isnan(host(sc)).all()
