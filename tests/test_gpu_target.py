"""aefft_net_step_grad_target on the GPU: the resident net's training step toward a target frame (pair 0's expected output is the target's
spectrum, fft_backproplib.cu:395-475 with expout != in) against the float64 oracle -- autoenc_fft per frame, then per pair
np_ref.batch_train_iter(Xs, Ts, Os, ..) with Ts = pool_fft(fft(target)) for pair 0 and Ts = Xs for the others.

Inputs.  Weights in (-1, 1) with an independent uniform target hide the target (it moves the gradients by 5e-4 .. 4e-3 of their largest entry),
so the kernels are drawn as 0.1 * U(-1, 1) and every case runs two target kinds: `dark` = floor(U(0, 100)) (moves all four gradient segments
and the MSE at the 0.5 level) and `indep` = floor(U(0, 256)) (same mean as the frames: the non-DC bins carry the difference).  Every test
asserts from the oracle that the target is visible at 100 x the gradient tolerance before it looks at the GPU.

Bounds (the project's own): packed gradients relerr < 5e-5 per segment, weights weight_step_tol, reconstruction 1e-4, pair 0's MSE
|mse - ref| < 1e-5 * max(1, ref_self + ref_n2) with ref_self = mean_b mse_fft(X_b, O'_b), ref_n2 = mean_b mse_fft(T_b, X_b): the MSE is the sum
of three terms that cancel (up to 7x on the dark targets), so the bound is on the terms."""
import functools
import importlib

import numpy as np
import pytest

import np_ref as R
from test_gpu_fft_path import STEP_PATHS, TOL, weight_step_tol

pytestmark = pytest.mark.gpu
aefft = importlib.import_module("autoencoder-fft_amd")
GTOL = 5e-5
KINDS = ["dark", "indep"]


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def relerr(got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def host(t):
    return t.detach().cpu().numpy()


def q32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _weights(rng, D, maps, Nk, tied=False):
    ws, dD = [], D
    for dM in maps:
        c = q32(0.1 * rng.uniform(-1, 1, (dM, dD, Nk, Nk)))
        f = np.transpose(c, (1, 0, 2, 3)).copy() if tied else q32(0.1 * rng.uniform(-1, 1, (dD, dM, Nk, Nk)))
        ws.append((c, q32(rng.uniform(-1, 1, dM)), f, q32(rng.uniform(-1, 1, dD))))
        dD = dM
    return ws


def _targets(rng, shape, kind):
    return np.floor(rng.uniform(0, 100 if kind == "dark" else 256, shape))


def _segments(buf, ws):
    """the packed buffer [dck | dfk | db | dp] per pair -> list over pairs of the four segments"""
    out, off = [], 0
    for c, b, f, p in ws:
        nk, dM, dD = c.size, c.shape[0], c.shape[1]
        out.append((buf[off:off + nk], buf[off + nk:off + 2 * nk], buf[off + 2 * nk:off + 2 * nk + dM], buf[off + 2 * nk + dM:off + 2 * nk + dM + dD]))
        off += 2 * nk + dM + dD
    return out


def oracle_step(xs, ts, ws, moms, s, dele=0.02, sym=0):
    """One target step in float64, the shape of np_ref.net_step: autoenc_fft per frame, then per pair one loop-body iteration with
    Ts = the target's spectra on pair 0's grid for pair 0 and Ts = Xs for the others.  Returns per pair a dict with the gradients of the
    target step and of the plain step, the updated weights and momentum, the post-update MSE against Ts, and its terms."""
    L, B = len(ws), len(xs)
    Nx, Ny = xs.shape[-2:]
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]
    net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    cf, sp = None, []
    for x in xs:
        layers, cf, spec = R.autoenc_fft(x, net_c, net_b, [s] * L + [-s] * L, net_cfreq=cf)
        sp.append((layers, spec))
    T0 = [R.pool_fft(R.fft(t), Nx, Ny, s)[0] for t in ts]
    out = []
    for l in range(L):
        c, b, f, p = ws[l]
        dM, dD, Nk, Nl = c.shape
        Xs = [q[1][2 * l + 1] for q in sp]; Os = [q[1][4 * L - 1 - 2 * l] for q in sp]
        Ts = T0 if l == 0 else Xs
        nx = Xs[0].shape[-2]; ny = (Xs[0].shape[-1] - 1) * 2
        mom = moms[l] if moms is not None else tuple(np.zeros_like(a) for a in (c, f, b, p))
        C, F = cf[l], cf[2 * L - 1 - l]
        if not sym:
            r = R.batch_train_iter(Xs, Ts, Os, C, F, c, f, b, p, mom, dele)
            d = dict(grads=r["grads"], w=(r["c"], r["b"], r["f"], r["p"]), mom=r["mom"], mse=float(r["mse"]), Os2=r["Os"])
        else:
            g = R.batch_grad(Xs, Ts, Os, C, F, b, Nk, Nl)
            c2, f2, b2, p2, Dc, Df, Db, Dp = R.backprop_sym(c, f, b, p, *g, *mom, dele)
            C2 = R.fft(R.pad_k(c2, nx, ny)); F2 = R.fft(R.pad_k(f2, nx, ny))
            Os2 = [R.conv_k(R.conv_k(X, C2, b2, nx, ny), F2, p2, nx, ny) for X in Xs]
            d = dict(grads=g, w=(c2, b2, f2, p2), mom=(Dc, Df, Db, Dp), Os2=Os2,
                     mse=float(np.mean([R.mse_fft(T, O, dM, dD, nx, ny) for T, O in zip(Ts, Os2)])))
        d["plain"] = R.batch_grad(Xs, Xs, Os, C, F, b, Nk, Nl) if l == 0 else d["grads"]
        d["ref_self"] = float(np.mean([R.mse_fft(X, O, dM, dD, nx, ny) for X, O in zip(Xs, d["Os2"])]))
        d["ref_n2"] = float(np.mean([R.mse_fft(T, X, dM, dD, nx, ny) for T, X in zip(Ts, Xs)]))
        out.append(d)
    return out, np.stack([q[0][-1] for q in sp])


@functools.lru_cache(maxsize=None)
def _case(D, Nx, Ny, maps, Nk, s, B, kind, tied=False):
    """seeded frames, targets, weights and their oracle step, computed once per case and shared (never modified)"""
    rng = np.random.default_rng(1000 * Nx + 10 * Ny + 7 * Nk + B + len(maps) + (0 if kind == "dark" else 500))
    xs = np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))
    ws = _weights(rng, D, list(maps), Nk, tied)
    ts = _targets(rng, xs.shape, kind)
    ref, recon = oracle_step(xs, ts, ws, None, s, sym=1 if tied else 0)
    return xs, ts, ws, ref, recon


def _assert_target_visible(ref, kind):
    """the precondition: the target moves pair 0's gradients by at least 100 x the gradient tolerance"""
    moved = [relerr(t, p) for t, p in zip(ref[0]["grads"], ref[0]["plain"])]
    need = moved if kind == "dark" else moved[:2]
    assert min(need) >= 100 * GTOL, (kind, moved)


def _mse_bound(d):
    return 1e-5 * max(1.0, d["ref_self"] + d["ref_n2"])


def _net(ctx, D, Nx, Ny, maps, Nk, s, B, ws, **kw):
    net = aefft.Net(ctx, D, Nx, Ny, list(maps), Nk, s, batch=B, **kw)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    return net


def _step_vs_oracle(ctx, D, Nx, Ny, maps, Nk, s, B, kind, form=None, **kw):
    xs, ts, ws, ref, recon_ref = _case(D, Nx, Ny, tuple(maps), Nk, s, B, kind)
    _assert_target_visible(ref, kind)
    L = len(maps)
    net = _net(ctx, D, Nx, Ny, maps, Nk, s, B, ws, **kw)
    if form is not None:
        assert net.step_form() == form, net.step_form()
    recon = ctx.empty(B, D, Nx, Ny)
    net.step_grad_target(ctx.dev(xs), ctx.dev(ts), recon)
    assert relerr(host(recon), recon_ref) < TOL
    segs = _segments(host(net.grad_buffer()).copy(), ws)
    mse = ctx.empty(L)
    net.step_apply(0.2, 0, 0, 1.0, mse)
    got_mse = host(mse)
    for l in range(L):
        d = ref[l]
        errs = [relerr(seg, g.ravel()) for seg, g in zip(segs[l], d["grads"])]
        print(f"pair {l} {kind}: gradient relerr {errs}, mse {got_mse[l]:.9g} ref {d['mse']:.9g} (self {d['ref_self']:.6g}, n2 {d['ref_n2']:.6g})")
        assert max(errs) < GTOL, (l, errs)
        for a, r, g in zip(net.get_pair(l), d["w"], (d["grads"][0], d["grads"][2], d["grads"][1], d["grads"][3])):
            assert (np.abs(a - r) < weight_step_tol(g)).all(), (l, np.abs(a - r).max())
        assert np.abs(net.get_pair(l)[0] - ws[l][0]).max() > 1e-5, "the update was not applied"
        assert abs(got_mse[l] - d["mse"]) < _mse_bound(d), (l, got_mse[l], d["mse"], d["ref_self"], d["ref_n2"])
    net.close()


def _want_form(path):
    names = set(path.split(","))
    if names & {"NOOPFORM", "NOQPATH"}:
        return "per_frame"
    if names & {"NOCHAIN", "NOLAZY", "NOCOMPACT", "NOGROUP", "NOMFMA", "NOFUSECROP"}:
        return "operator"
    return "operator_chain"


# ------------------------------------------------------------------------------------------
# 1. every code path of the step
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", STEP_PATHS + ["NOLAZYMSE"])
@pytest.mark.parametrize("B", [1, 3])
def test_target_step_equals_oracle_on_every_path(ctx, flags, B, path, kind):
    flags(*path.split(","))
    _step_vs_oracle(ctx, 3, 32, 32, [4, 6], 5, 2, B, kind, form=_want_form(path))


# ------------------------------------------------------------------------------------------
# 2. shapes
# ------------------------------------------------------------------------------------------
SHAPES = [
    (3, 32, 32, (4, 6), 3, 2, 2, "operator_chain", {}),
    (3, 32, 32, (4,), 7, 2, 2, "per_frame", {}),                 # single pair, no Q path: pair 0 is the innermost
    (1, 32, 64, (5, 3), 5, 2, 3, "operator_chain", {}),
    (2, 64, 32, (3, 9), 3, 2, 5, "operator_chain", {}),          # B = 5: not a multiple of the batch slices
    (3, 32, 32, (4, 6), 5, 1, 2, "operator_chain", {}),          # no crop
    (3, 64, 64, (4, 6, 5), 5, 2, 2, "operator_chain", {}),
    (2, 128, 128, (8, 16), 5, 2, 1, "operator_chain", {}),       # P0 = 64 * 33: not a multiple of 256
    (4, 32, 32, (4,), 5, 2, 2, "per_frame", {}),                 # D = 4
    (1, 20, 24, (2,), 3, 1, 3, "per_frame", dict(smooth_sizes=True)),       # 260 bins
    (3, 48, 80, (4, 6), 5, 2, 2, "operator_chain", dict(smooth_sizes=True, operator_form=True)),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,Nx,Ny,maps,Nk,s,B,form,kw", SHAPES)
def test_target_step_shapes_vs_oracle(ctx, flags, D, Nx, Ny, maps, Nk, s, B, form, kw, kind):
    flags()
    _step_vs_oracle(ctx, D, Nx, Ny, maps, Nk, s, B, kind, form=form, **kw)


# ------------------------------------------------------------------------------------------
# 3. target == frames: the plain step by value
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOCHAIN", "NOOPFORM"])
@pytest.mark.parametrize("B", [1, 3])
def test_target_equal_to_the_frames_is_the_plain_step_by_value(ctx, flags, path, B):
    flags(*path.split(","))
    D, N, maps, Nk, s = 3, 32, (4, 6), 5, 2
    xs, _, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    x = ctx.dev(xs)
    res = []
    for target in (False, True):
        net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
        if target:
            net.step_grad_target(x, x.clone(), None)
        else:
            net.step_grad(x, None)
        g = host(net.grad_buffer()).copy()
        mse = ctx.empty(len(maps))
        net.step_apply(0.2, 0, 0, 1.0, mse)
        res.append((g, [net.get_pair(l) for l in range(len(maps))], host(mse).copy()))
        net.close()
    (g0, w0, m0), (g1, w1, m1) = res
    assert np.array_equal(g0, g1)                 # the corrections are exact zeros
    for a, b in zip(w0, w1):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert np.allclose(m0, m1, rtol=1e-6) and np.all(m0 > 0)      # (the slot adds are atomics)


# ------------------------------------------------------------------------------------------
# 4. 8-bit frames and targets
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOOPFORM"])
def test_8bit_frames_and_targets_equal_the_float_call(ctx, flags, path):
    import torch
    flags(*path.split(","))
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 3
    xs, ts, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "indep")
    xf, tf = ctx.dev(xs), ctx.dev(ts)
    x8, t8 = xf.to(torch.uint8), tf.to(torch.uint8)
    res = []
    for fr, tg in ((xf, tf), (x8, t8), (xf, t8)):
        net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
        recon = ctx.empty(B, D, N, N)
        net.step_grad_target(fr, tg, recon)
        res.append((host(net.grad_buffer()).copy(), host(recon).copy()))
        net.close()
    for g, r in res[1:]:
        assert np.array_equal(g, res[0][0]) and np.array_equal(r, res[0][1])
    assert np.abs(res[0][0]).max() > 0


# ------------------------------------------------------------------------------------------
# 5. deferred MSE sums
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOOPFORM", "NOLAZYMSE"])
def test_deferred_mse_is_the_target_mse(ctx, flags, path):
    flags(*path.split(","))
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 3
    L = len(maps)
    xs, ts, ws, ref, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    _assert_target_visible(ref, "dark")
    x, t = ctx.dev(xs), ctx.dev(ts)
    # (a) last_mse after step_apply(mse = None)
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    net.step_grad_target(x, t, None)
    net.step_apply(0.2, 0, 0, 1.0, None)
    got = host(net.last_mse())
    for l in range(L):
        assert abs(got[l] - ref[l]["mse"]) < _mse_bound(ref[l]), (l, got[l], ref[l]["mse"])
    assert abs(got[0] - ref[0]["ref_self"]) > 100 * _mse_bound(ref[0])       # (not the plain step's MSE)
    net.close()
    # (b) the next step's packed tail
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    net.step_grad_target(x, t, None)
    net.step_apply(0.2, 0, 0, 1.0, None)
    net.step_grad(x, None)
    tail = host(net.grad_buffer())[-L:]
    assert np.allclose(tail, got, rtol=1e-6), (tail, got)
    net.close()


# ------------------------------------------------------------------------------------------
# 6. tied weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tied_weights_target_step(ctx, flags, kind):
    flags()
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 2
    L = len(maps)
    xs, ts, ws, ref, _ = _case(D, N, N, maps, Nk, s, B, kind, True)
    _assert_target_visible(ref, kind)
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    net.step_grad_target(ctx.dev(xs), ctx.dev(ts), None)
    segs = _segments(host(net.grad_buffer()).copy(), ws)
    mse = ctx.empty(L)
    net.step_apply(0.2, 0, 1, 1.0, mse)
    for l in range(L):
        d = ref[l]
        dck, dfk, db, dp = d["grads"]
        for seg, g in zip(segs[l], d["grads"]):
            assert relerr(seg, g.ravel()) < GTOL, l
        c2, b2, f2, p2 = net.get_pair(l)
        rc, rb, rf, rp = d["w"]
        assert np.array_equal(f2, np.transpose(c2, (1, 0, 2, 3))), l
        assert (np.abs(c2 - rc) < weight_step_tol(0.5 * (dck + np.transpose(dfk, (1, 0, 2, 3))))).all(), l
        assert (np.abs(b2 - rb) < weight_step_tol(0.5 * db)).all() and (np.abs(p2 - rp) < weight_step_tol(0.5 * dp)).all(), l
        assert abs(host(mse)[l] - d["mse"]) < _mse_bound(d), (l, host(mse)[l], d["mse"])
    net.close()


# ------------------------------------------------------------------------------------------
# 7. five consecutive target steps, momentum carried
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trajectory():
    rng = np.random.default_rng(2024)
    D, N, maps, Nk, s, B, steps = 3, 32, (4, 6), 5, 2, 2, 5
    ws = _weights(rng, D, list(maps), Nk)
    frames = [np.floor(rng.uniform(0, 256, (B, D, N, N))) for _ in range(steps)]
    targets = [_targets(rng, frames[0].shape, "dark") for _ in range(steps)]
    w, moms, mses = ws, None, []
    for x, t in zip(frames, targets):
        ref, _ = oracle_step(x, t, w, moms, s)
        w = [d["w"] for d in ref]; moms = [d["mom"] for d in ref]
        mses.append([d["mse"] for d in ref])
    return (D, N, maps, Nk, s, B), ws, frames, targets, np.array(mses)


@pytest.mark.parametrize("path", ["", "NOOPFORM"])
def test_five_target_steps_vs_float64_oracle(ctx, flags, path):
    flags(*path.split(","))
    (D, N, maps, Nk, s, B), ws, frames, targets, ref = _trajectory()
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    assert net.step_form() == _want_form(path)
    mse = ctx.empty(len(frames), len(maps))
    for i, (x, t) in enumerate(zip(frames, targets)):
        net.step_grad_target(ctx.dev(x), ctx.dev(t), None)
        net.step_apply(0.2, 0, 0, 1.0, mse[i])
    got = host(mse).astype(np.float64)
    net.close()
    print("per-step pair MSEs, relative difference to the oracle:", np.abs(got / ref - 1).max(axis=0))
    assert np.allclose(got, ref, rtol=1e-4), np.abs(got / ref - 1).max()


def test_input_prefetch_gives_identical_target_training(ctx, flags):
    """aefft_net_set_input_ready(1): the frames' transform runs ahead on a side stream, the target's stays on the context stream (its own
    workspace, never prefetched) -- five target steps leave exactly the weights of the stream-ordered run"""
    flags()
    (D, N, maps, Nk, s, B), ws, frames, targets, _ = _trajectory()
    xs, ts = [ctx.dev(x) for x in frames], [ctx.dev(t) for t in targets]
    out = []
    for ready in (False, True):
        net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
        net.set_input_ready(ready)
        recon, mse = ctx.empty(B, D, N, N), ctx.empty(len(maps))
        for x, t in zip(xs, ts):
            net.step_grad_target(x, t, recon); net.step_apply(0.2, 0, 0, 1.0, mse)
        ctx.sync()
        out.append(([net.get_pair(l) for l in range(len(maps))], host(recon).copy(), host(mse).copy()))
        net.close()
    for wa, wb in zip(out[0][0], out[1][0]):
        for a, b in zip(wa, wb):
            assert np.array_equal(a, b)
    assert np.array_equal(out[0][1], out[1][1])
    assert np.allclose(out[0][2], out[1][2], rtol=1e-5)


# ------------------------------------------------------------------------------------------
# 8. state
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "NOCHAIN", "NOOPFORM"])
def test_plain_step_after_a_target_step_equals_a_fresh_net(ctx, flags, path):
    """the target leaves nothing behind: a plain step_grad after a completed target step gives the reconstruction and packed gradients of
    a fresh net that starts from the live net's weights (the comparison of test_second_step_equals_fresh_net_with_updated_weights)"""
    flags(*path.split(","))
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 3
    L = len(maps)
    xs, ts, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    x2 = ctx.dev(np.floor(np.random.default_rng(9).uniform(0, 256, xs.shape)))
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    net.step_grad_target(ctx.dev(xs), ctx.dev(ts), None); net.step_apply(0.2)
    weights = [net.get_pair(l) for l in range(L)]
    r_live = ctx.empty(B, D, N, N)
    net.step_grad(x2, r_live)
    g_live = host(net.grad_buffer()).copy()
    fresh = _net(ctx, D, N, N, maps, Nk, s, B, weights)
    r_fresh = ctx.empty(B, D, N, N)
    fresh.step_grad(x2, r_fresh)
    g_fresh = host(fresh.grad_buffer())
    assert relerr(host(r_live), host(r_fresh)) < 2e-5
    assert relerr(g_live[:-L], g_fresh[:-L]) < 5e-5
    # ... and that plain step reports the plain MSE: a twin whose second step is a target step with target == frames (exact zero corrections)
    # carries the same momentum and must report the same sums -- stale target terms of the first step would show at the 0.5 level
    twin = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    twin.step_grad_target(ctx.dev(xs), ctx.dev(ts), None); twin.step_apply(0.2)
    twin.step_grad_target(x2, x2.clone(), None)
    m_live, m_twin = ctx.empty(L), ctx.empty(L)
    net.step_apply(0.2, 0, 0, 1.0, m_live); twin.step_apply(0.2, 0, 0, 1.0, m_twin)
    assert np.allclose(host(m_live), host(m_twin), rtol=1e-6) and np.all(host(m_live) > 0)
    net.close(); fresh.close(); twin.close()


def test_a_call_that_ends_the_pending_step_ends_the_target(ctx, flags):
    flags()
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 2
    xs, ts, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    x, t = ctx.dev(xs), ctx.dev(ts)
    net.step_grad_target(x, t, None)
    net.infer(x, ctx.empty(B, D, N, N))
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.2)
    net.close()


def test_argument_errors_enqueue_nothing(ctx, flags):
    flags()
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 2
    xs, ts, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    x, t = ctx.dev(xs), ctx.dev(ts)
    einval = f"aefft error {aefft.EINVAL}:"
    net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
    recon = ctx.empty(B, D, N, N); recon.fill_(-7.0)
    n = x.numel()
    odd = ctx.empty(n + 4)
    odd[1:n + 1] = t.reshape(-1)
    for fr, tg, rc in ((x, None, recon), (None, t, recon), (x, odd[1:n + 1], recon), (odd[1:n + 1], t, recon), (x, t, odd[1:n + 1])):
        with pytest.raises(aefft.AefftError, match=einval):
            net.step_grad_target(fr, tg, rc)
    with pytest.raises(aefft.AefftError, match=f"aefft error {aefft.ESTATE}:"):
        net.step_apply(0.2)                                    # nothing was enqueued: no step is pending
    net.close()
    sp = aefft.Net(ctx, D, N, N, [4], 3, 2, batch=B, spatial=True)
    with pytest.raises(aefft.AefftError, match=einval):
        sp.step_grad_target(x, t, recon)
    sp.close()
    wide = aefft.Net(ctx, 5, N, N, [4], 5, 2, batch=1)
    x5 = ctx.empty(1, 5, N, N); x5.fill_(1.0)
    with pytest.raises(aefft.AefftError, match=einval):
        wide.step_grad_target(x5, x5.clone(), None)
    wide.close()
    ctx.sync()
    assert (host(recon) == -7.0).all()


# ------------------------------------------------------------------------------------------
# 9. launch counts
# ------------------------------------------------------------------------------------------
def test_a_target_step_is_four_launches_more(ctx, flags):
    flags()
    D, N, maps, Nk, s, B = 3, 32, (4, 6), 5, 2, 3
    xs, ts, ws, _, _ = _case(D, N, N, maps, Nk, s, B, "dark")
    x, t = ctx.dev(xs), ctx.dev(ts)
    counts = []
    for target in (False, True):
        net = _net(ctx, D, N, N, maps, Nk, s, B, ws)
        assert net.step_form() == "operator_chain"
        mse = ctx.empty(len(maps))
        for it in range(2):            # (the second step is counted: the chain of its weights is at hand, the target's workspaces exist)
            if it == 1:
                ctx.sync(); ctx.prof_enable(); ctx.prof_reset()
            if target:
                net.step_grad_target(x, t, None)
            else:
                net.step_grad(x, None)
            net.step_apply(0.2, 0, 0, 1.0, mse)
        counts.append({k: v["launches"] for k, v in ctx.prof_read().items()})
        ctx.prof_enable(False)
        net.close()
    plain, tgt = counts
    assert plain["target"] == 0 and tgt["target"] == 2, (plain, tgt)
    assert tgt["r2c_rows"] == plain["r2c_rows"] + 1 and tgt["r2c_cols"] == plain["r2c_cols"] + 1, (plain, tgt)
    for k in plain:
        if k not in ("target", "r2c_rows", "r2c_cols"):
            assert tgt[k] == plain[k], (k, plain, tgt)
    assert sum(tgt.values()) == sum(plain.values()) + 4
