"""The support-pruned kernel transforms (kspec: taps -> spectrum, kgrad: gradient spectrum -> taps) on grids with a smooth axis (even, no
prime factor above 5: 640 x 480, 90 x 160, 640 x 512 ...): the ops against the float64 oracle, the routes a smooth net's per-frame step
takes (by the profiler's launch counts), and pruned == full (AEFFT_F_NOPRUNESMOOTH) == oracle over two steps of such nets.  Power-of-two
grids must not see the switch at all."""
import functools
import importlib

import numpy as np
import pytest

import np_ref as R
from test_gpu_fft_path import host, relerr, weight_step_tol
from test_gpu_sizes import _net, _same, _two_steps, _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu
FULL = "NOPRUNESMOOTH"


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------
# 1. the ops
# ------------------------------------------------------------------------------------------
# (nA, nB): plane counts that give the single-problem kgrad one row chunk (many plane groups), several, and many (few planes on a
# long axis: the `pblocks < 96` branch of kgrad_geom); 90 rows split into 4 chunks of 23 (the last one 21), 360 and 30 likewise odd cases
GRIDS = [(640, 480, 4, 3), (480, 640, 2, 3), (240, 320, 4, 3), (60, 36, 2, 1), (90, 160, 4, 3), (30, 40, 40, 32), (1280, 360, 2, 2),
         (2000, 16, 4, 3), (640, 512, 3, 2)]


@pytest.mark.parametrize("Nk", [3, 5, 7])
@pytest.mark.parametrize("Nx,Ny,nA,nB", GRIDS)
def test_kernel_spectrum_and_export_on_smooth_grids(ctx, flags, Nx, Ny, nA, nB, Nk):
    """aefft_kernel_spectrum against np_ref.kernel_spectrum at the power-of-two route's bound (2e-6 relative), aefft_kernel_export back to
    the taps at 1e-5.  (7 x 7 on 2000 rows exceeds the kgrad LDS bound and keeps the full route: it must stay correct.)"""
    flags()
    rng = np.random.default_rng(Nx * 3 + Ny + Nk)
    c = rng.uniform(-3, 3, (nA, nB, Nk, Nk)).astype(np.float32)
    K = ctx.kernel_spectrum(ctx.dev(c), Nx, Ny)
    e_spec = relerr(host(K), R.kernel_spectrum(c, Nx, Ny))
    back = ctx.kernel_export(K, Nk, Nk, Ny)
    e_back = np.abs(host(back) - c).max()
    print(f"kspec {Nx}x{Ny} {Nk}x{Nk} planes {nA * nB}: spectrum {e_spec:.3g} (2e-6), export {e_back:.3g} (1e-5)")
    assert e_spec < 2e-6
    assert e_back < 1e-5


@pytest.mark.parametrize("planes", [(1, 1), (3, 2), (16, 12)])
def test_kernel_export_row_chunks(ctx, flags, planes):
    """The adjoint alone on a gradient-like (not exactly Hermitian) spectrum at 360 x 90 and 90 x 160 -- row counts no chunk count divides -- with
    one, six and 192 planes, against shrink_k(c2r_unnorm) scaled as kfft_inv scales it, 5x5 support, at the inverse transforms' 5e-6."""
    flags()
    for Nx, Ny in ((360, 90), (90, 160)):
        rng = np.random.default_rng(Nx + planes[0])
        Z = (rng.normal(size=(*planes, Nx, Ny // 2 + 1)) + 1j * rng.normal(size=(*planes, Nx, Ny // 2 + 1))).astype(np.complex64)
        ref = R.shrink_k(R.c2r_unnorm(Z.astype(np.complex128), Nx, Ny), 5, 5) / (Nx * Ny)
        got = host(ctx.kernel_export(ctx.dev(Z), 5, 5, Ny))
        assert relerr(got, ref) < 5e-6, (Nx, Ny)


@pytest.mark.parametrize("maxdiff", [0, 1])
@pytest.mark.parametrize("Nx,Ny,Nk,dD,dM", [(60, 36, 5, 3, 4), (90, 160, 3, 2, 3)])
def test_update_on_smooth_grids(ctx, flags, Nx, Ny, Nk, dD, dM, maxdiff):
    """aefft_update (adjoint of both gradient spectra, clipped-momentum update, new spectra) at test_update's bounds."""
    flags()
    rng = np.random.default_rng(5 + dD + maxdiff + Nx)
    q = lambda a: a.astype(np.float32).astype(np.float64)
    xs = np.floor(rng.uniform(0, 256, (dD, Nx, Ny)))
    c, f = q(rng.uniform(-1, 1, (dM, dD, Nk, Nk))), q(rng.uniform(-1, 1, (dD, dM, Nk, Nk)))
    b, p = q(rng.uniform(-1, 1, dM)), q(rng.uniform(-1, 1, dD))
    outs = xs + rng.uniform(-20, 20, xs.shape)
    X, O = R.fft(xs), R.fft(outs)
    Cs, Fs = R.kernel_spectrum(c, Nx, Ny), R.kernel_spectrum(f, Nx, Ny)
    dc, df, db, dp = R.gradient_k_io(X, X, O, Cs, Fs, b, Nx, Ny)
    mom = [0.01 * rng.normal(size=a.shape) for a in (c, f, b, p)]
    ref = R.backprop(c, f, b, p, dc, df, db, dp, *mom, Nx, Ny, 0.02, maxdiff)
    t = [ctx.dev(a) for a in (c, f, b, p, Cs, Fs, dc, df, db, dp, *mom)]
    ctx.update(*t, Ny, 0.02, maxdiff)
    names = ["c", "f", "b", "p", "Dc", "Df", "Db", "Dp"]
    got = dict(zip(["c", "f", "b", "p", "C", "F"], t[:6])); got.update(dict(zip(["Dc", "Df", "Db", "Dp"], t[10:])))
    refd = dict(zip(names + ["C", "F"], ref))
    start = dict(c=c, f=f, b=b, p=p, Dc=mom[0], Df=mom[1], Db=mom[2], Dp=mom[3])
    for k in names:
        dw = max(np.abs(refd[k] - start[k]).max(), 1e-12)
        assert np.abs(host(got[k]) - refd[k]).max() < 1e-6 + 1e-3 * dw, k
    assert relerr(host(got["C"]), refd["C"]) < 5e-6 and relerr(host(got["F"]), refd["F"]) < 5e-6


# ------------------------------------------------------------------------------------------
# 2. the routes
# ------------------------------------------------------------------------------------------
def _step_profile(ctx, Nx, Ny, maps, seed):
    rng = np.random.default_rng(seed)
    D, B, L = 3, 2, len(maps)
    ws = _weights(rng, D, maps, 5, 5)
    frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))))
    net = _net(ctx, D, Nx, Ny, ws, 5, 5, 2, B)
    form = net.step_form()
    recon, mse = ctx.empty(B, D, Nx, Ny), ctx.empty(L)
    ctx.prof_enable(); ctx.prof_reset()
    net.step_grad(frames, recon)
    net.step_apply(0.2, 0, 0, 1.0, mse)
    ctx.sync()
    pr = ctx.prof_read(); ctx.prof_enable(False)
    net.close()
    assert np.isfinite(host(mse)).all()
    return form, {k: v["launches"] for k, v in pr.items()}


def test_smooth_net_takes_the_pruned_routes(ctx, flags):
    """One step_grad + step_apply of the 640 x 480, four-pair, 5x5 net: no pad, no shrink, kspec and kgrad launched, and exactly the frame
    transforms of the same pairs at 512^2 in the per-frame form (NOOPFORM) remain.  Under NOPRUNESMOOTH pad and shrink are back; under
    GTAPS the G' launch joins the pruned ones."""
    maps = [3, 4, 3, 2]
    flags()
    form, sm = _step_profile(ctx, 640, 480, maps, 64048)
    flags("NOOPFORM")
    _, p2 = _step_profile(ctx, 512, 512, maps, 64048)
    flags(FULL)
    form_full, full = _step_profile(ctx, 640, 480, maps, 64048)
    flags("GTAPS")
    _, gt = _step_profile(ctx, 640, 480, maps, 64048)
    flags()
    print("640x480:", sm, "\n512^2 NOOPFORM:", p2, "\n640x480 full:", full, "\n640x480 GTAPS:", gt)
    assert form == "per_frame" and form_full == "per_frame"
    assert sm["pad"] == 0 and sm["shrink"] == 0 and sm["kspec"] > 0 and sm["kgrad"] > 0
    for k in ("r2c_rows", "r2c_cols", "c2r_cols", "c2r_rows"):
        assert sm[k] == p2[k], (k, sm[k], p2[k])
    assert full["pad"] > 0 and full["shrink"] > 0
    # G' from the taps (what an HBM-sized smooth net chooses by itself): more pruned launches, still no full transform of a kernel plane
    assert gt["kspec"] > sm["kspec"] and gt["pad"] == 0 and gt["shrink"] == 0
    for k in ("r2c_rows", "r2c_cols", "c2r_cols", "c2r_rows"):
        assert gt[k] == sm[k], k


def test_kernel_spectrum_op_takes_the_pruned_route(ctx, flags):
    rng = np.random.default_rng(7)
    c = ctx.dev(rng.uniform(-1, 1, (4, 3, 5, 5)).astype(np.float32))
    counts = []
    for fl in ("", FULL):
        flags(fl)
        ctx.prof_enable(); ctx.prof_reset()
        ctx.kernel_spectrum(c, 640, 480)
        ctx.sync()
        counts.append({k: v["launches"] for k, v in ctx.prof_read().items()}); ctx.prof_enable(False)
    flags()
    assert counts[0]["pad"] == 0 and counts[0]["shrink"] == 0 and counts[0]["kspec"] > 0
    assert counts[0]["r2c_rows"] == 0 and counts[0]["r2c_cols"] == 0
    assert counts[1]["pad"] > 0 and counts[1]["kspec"] == 0


# ------------------------------------------------------------------------------------------
# 3. pruned == full == oracle on a net
# ------------------------------------------------------------------------------------------
CASES = {  # Nx, Ny, maps, Nk, B
    "640x480": (640, 480, [3, 4, 3, 2], 5, 2),
    "240x320": (240, 320, [4, 3, 2], 5, 2),
    "240x320-3x3": (240, 320, [4, 3, 2], 3, 2),
    "1280x720": (1280, 720, [2, 3, 2], 5, 1),
}


def _case(name):
    Nx, Ny, maps, Nk, B = CASES[name]
    rng = np.random.default_rng(Nx * 5 + Ny + len(maps) + Nk)
    ws = _weights(rng, 3, maps, Nk, Nk)
    xs = [np.floor(rng.uniform(0, 256, (B, 3, Nx, Ny))) for _ in range(2)]
    return ws, xs


def _oracle_step(xs, ws, moms, s, L):
    """one step of np_ref.net_step's arithmetic, keeping the gradients: (ws', moms', mse, recon, grads, first frame's forward)"""
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]
    net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    sp = [R.autoenc_fft(x, net_c, net_b, [s] * L + [-s] * L) for x in xs]
    cf = sp[0][1]
    w2, m2, mse, grads = [], [], [], []
    for l in range(L):
        c, b, f, p = ws[l]
        Xs = [q[2][2 * l + 1] for q in sp]; Os = [q[2][4 * L - 1 - 2 * l] for q in sp]
        r = R.batch_train_iter(Xs, Xs, Os, cf[l], cf[2 * L - 1 - l], c, f, b, p, moms[l], 0.02)
        w2.append((r["c"], r["b"], r["f"], r["p"])); m2.append(r["mom"]); mse.append(r["mse"]); grads.append(r["grads"])
    return w2, m2, mse, np.stack([q[0][-1] for q in sp]), grads, sp[0]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """two oracle steps of a case (the second from the oracle's own state after the first), computed once for every flag set"""
    ws, xs = _case(name)
    L = len(ws)
    z = [tuple(np.zeros_like(a) for a in (w[0], w[2], w[1], w[3])) for w in ws]
    s1 = _oracle_step(xs[0], ws, z, 2, L)
    s2 = _oracle_step(xs[1], s1[0], s1[1], 2, L)
    return s1, s2


def _two_steps_w(ctx, net, frames, B, D, Nx, Ny, L):
    """_two_steps that also reads every pair's weights (get_pair: c, b, f, p) after EACH step: [(recon, grads, mse, weights)] * 2"""
    out = []
    for x in frames:
        recon = ctx.empty(B, D, Nx, Ny); recon.fill_(float("nan"))
        mse = ctx.empty(L)
        net.step_grad(x, recon)
        g = host(net.grad_buffer()).copy()
        net.step_apply(0.2, 0, 0, 1.0, mse)
        ctx.sync()
        out.append((host(recon).copy(), g, host(mse).copy(), [[np.array(a, copy=True) for a in net.get_pair(l)] for l in range(L)]))
    return out


def _check_two_steps(name, run, tag):
    """run: _two_steps_w's output.  BOTH steps at test_network_at_smooth_sizes_against_oracle's tolerances: reconstruction and MSE 1e-4,
    packed gradients 5e-5, and every weight tensor of every pair within weight_step_tol of the oracle's after step 1 AND after step 2 (the
    second oracle step runs from the oracle's own state after the first, momentum carried).  The largest |w - oracle| / weight_step_tol
    per step is printed before it is asserted."""
    Nx, Ny, maps, Nk, B = CASES[name]
    ws, _ = _case(name)
    L = len(ws)
    steps = _oracle(name)
    for k, (w_or, m2, mse, recon, grads, _) in enumerate(steps):
        rec_g, gbuf, mse_g, w_g = run[k]
        assert relerr(rec_g, recon) < 1e-4, (tag, k)
        off = 0
        worst = 0.0
        for l in range(L):
            c = ws[l][0]
            dM, dDl = c.shape[:2]
            nk = c.size
            for seg, ref in zip((gbuf[off:off + nk], gbuf[off + nk:off + 2 * nk], gbuf[off + 2 * nk:off + 2 * nk + dM],
                                 gbuf[off + 2 * nk + dM:off + 2 * nk + dM + dDl]), grads[l]):
                assert relerr(seg, ref.ravel()) < 5e-5, (tag, k, l)
            off += 2 * nk + dM + dDl
            assert abs(mse_g[l] - mse[l]) < 1e-4 * max(1, mse[l]), (tag, k, l)
            # weights: get_pair order (c, b, f, p); gradient order (c, f, b, p)
            for a, ref, gi in zip(w_g[l], w_or[l], (0, 2, 1, 3)):
                worst = max(worst, float((np.abs(a - ref) / weight_step_tol(grads[l][gi])).max()))
        print(f"{tag} step {k + 1}: max |w - oracle| / weight_step_tol = {worst:.3f}")
        for l in range(L):
            for a, ref, gi in zip(w_g[l], w_or[l], (0, 2, 1, 3)):
                assert (np.abs(a - ref) < weight_step_tol(grads[l][gi])).all(), (tag, k, l, gi, np.abs(a - ref).max())


@pytest.mark.parametrize("path", ["", "NOQPATH", "NOGROUP", "GTAPS"])
@pytest.mark.parametrize("name", list(CASES))
def test_pruned_full_and_oracle_agree_over_two_steps(ctx, flags, name, path):
    """Two steps of a smooth net with the pruned weight side and with the full pad + R2C / C2R + shrink one, under the default routes
    (grouped S -> Q -> weight taps), NOQPATH (dc|df with the grouped kgrad), NOGROUP (pair by pair) and GTAPS (the post-update MSE's G' as
    the spectrum of the (2Nk-1)^2-tap kernel f (*) c, which HBM-sized nets choose by themselves: taps formed once per plane and a 9 x 9 / 5 x 5
    launch where a grid has more than 64 rows, formed inside the transforming workgroups otherwise): both against the oracle."""
    Nx, Ny, maps, Nk, B = CASES[name]
    ws, xs = _case(name)
    frames = [ctx.dev(x) for x in xs]
    runs = {}
    for sw in ("", FULL):
        flags(path, sw)
        net = _net(ctx, 3, Nx, Ny, ws, Nk, Nk, 2, B)
        assert net.step_form() == "per_frame"
        runs[sw] = _two_steps_w(ctx, net, frames, B, 3, Nx, Ny, len(maps))
        net.close()
    flags()
    assert not np.array_equal(runs[""][0][1], runs[FULL][0][1]), "the switch changed nothing"
    for sw in ("", FULL):
        _check_two_steps(name, runs[sw], (name, path, sw))


@pytest.mark.parametrize("name", ["640x480", "240x320-3x3"])
def test_train_pair_burst_both_routes(ctx, flags, name):
    """a 5-iteration burst on pair 0 of one frame (fft_backproplib.cu:1381-1511): per-pair kgrad / kspec in a loop, both routes"""
    Nx, Ny, maps, Nk, B = CASES[name]
    ws, xs = _case(name)
    L = len(maps)
    lay, cfr = _oracle(name)[0][5][0], _oracle(name)[0][5][1]
    c, b, f, p = ws[0]
    r = R.backprop_fft(lay[1], lay[1], lay[4 * L - 1], cfr[0], c, cfr[2 * L - 1], f, b, p, 0.2, n_iter=5)
    for sw in ("", FULL):
        flags(sw)
        net = _net(ctx, 3, Nx, Ny, ws, Nk, Nk, 2, 1)
        net.forward(ctx.dev(xs[0][:1]), None)
        got = net.train_pair(0, 5, 0.2)
        assert np.allclose(got, np.array(r["mse"]), rtol=1e-4), (sw, got, r["mse"])
        for a, k in zip(net.get_pair(0), ("c", "b", "f", "p")):
            assert np.abs(a - r[k]).max() < 1e-4, (sw, k, np.abs(a - r[k]).max())
        net.close()
    flags()


def test_tied_weights_and_multiobjective_step(ctx, flags):
    """sym = 1, maxdiff = 1 at 240 x 320, one step, both routes against np_ref.net_step; the weight bound is weight_step_tol of the
    effective gradient backprop_sym forms (W0 * (g_c + g_f^T) / 2 - W1 * (cd + fd^T) / 2, halved bias gradients likewise)."""
    Nx, Ny, maps, B, s = 240, 320, [4, 3, 2], 2, 2
    L = len(maps)
    rng = np.random.default_rng(2403)
    ws = _weights(rng, 3, maps, 5, 5)
    ws = [(c, b, np.transpose(c, (1, 0, 2, 3)).copy(), p) for c, b, f, p in ws]
    xs = np.floor(rng.uniform(0, 256, (B, 3, Nx, Ny)))
    w1, _, mses, recon = R.net_step(xs, ws, None, s, 0.2, maxdiff=1, sym=1)
    net_c = [w[0] for w in ws] + [w[2] for w in ws[::-1]]; net_b = [w[1] for w in ws] + [w[3] for w in ws[::-1]]
    sp = [R.autoenc_fft(x, net_c, net_b, [s] * L + [-s] * L) for x in xs]
    tols = []
    for l in range(L):
        c, b, f, p = ws[l]
        Xs = [q[2][2 * l + 1] for q in sp]; Os = [q[2][4 * L - 1 - 2 * l] for q in sp]
        dck, dfk, db, dp = R.batch_grad(Xs, Xs, Os, sp[0][1][l], sp[0][1][2 * L - 1 - l], b, 5, 5)
        cd, fd, bd, pd = R.gradient_diff_fast(c, f, b, p)
        g = R.W0 * 0.5 * (dck + np.transpose(dfk, (1, 0, 2, 3))) - R.W1 * 0.5 * (cd + np.transpose(fd, (1, 0, 2, 3)))
        tols.append((weight_step_tol(g), weight_step_tol(R.W0 * 0.5 * db - R.W1 * bd), weight_step_tol(R.W0 * 0.5 * dp - R.W1 * pd)))
    for sw in ("", FULL):
        flags(sw)
        net = _net(ctx, 3, Nx, Ny, ws, 5, 5, s, B)
        rec, mse = ctx.empty(B, 3, Nx, Ny), ctx.empty(L)
        net.step_grad(ctx.dev(xs), rec)
        net.step_apply(0.2, 1, 1, 1.0, mse)
        ctx.sync()
        assert net.step_form() == "per_frame"
        assert relerr(host(rec), recon) < 1e-4
        for l in range(L):
            c2, b2, f2, p2 = net.get_pair(l)
            tc, tb, tp = tols[l]
            assert (np.abs(c2 - w1[l][0]) < tc).all() and (np.abs(f2 - w1[l][2]) < np.transpose(tc, (1, 0, 2, 3))).all(), (sw, l)
            assert (np.abs(b2 - w1[l][1]) < tb).all() and (np.abs(p2 - w1[l][3]) < tp).all(), (sw, l)
            assert abs(host(mse)[l] - mses[l]) < 1e-4 * max(1, mses[l]), (sw, l)
        net.close()
    flags()


# ------------------------------------------------------------------------------------------
# 4. power-of-two grids
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny", [(64, 64), (512, 256)])
def test_power_of_two_nets_do_not_see_the_switch(ctx, flags, Nx, Ny):
    """two steps of a power-of-two net, bit for bit with and without NOPRUNESMOOTH"""
    D, maps, B = 3, [4, 3], 2
    rng = np.random.default_rng(Nx + Ny)
    ws = _weights(rng, D, maps, 5, 5)
    frames = [ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny)))) for _ in range(2)]
    runs, forms = [], []
    for fl in ("", FULL):
        flags(fl)
        net = aefft.Net(ctx, D, Nx, Ny, maps, 5, 2, batch=B)
        for l, w in enumerate(ws):
            net.set_pair(l, *w)
        forms.append(net.step_form())
        runs.append(_two_steps(ctx, net, frames, B, D, Nx, Ny, len(maps)))
        net.close()
    flags()
    assert forms[0] == forms[1] and np.isfinite(runs[0][0][0]).all()
    _same(runs[0], runs[1])
