"""AEFFT_NET_SMOOTH_OPFORM: the operator-form training step of a net on a grid with a smooth axis (640 x 480-class camera frames) -- the
form it reports, two steps against the float64 oracle under every operator-form route, operator form == per-frame form with both
reconstruction routes, the routes by the profiler's launch counts, layer exports, pipelined mode, tied weights with the multiobjective
term, and the data-parallel library."""
import importlib

import numpy as np
import pytest

import np_ref as R
from test_gpu_fft_path import host, relerr, weight_step_tol
from test_gpu_pruned_smooth import CASES, _case, _check_two_steps, _oracle, _oracle_step, _two_steps_w  # noqa: F401
from test_gpu_sizes import _same, _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# the operator-form members of test_gpu_fft_path.STEP_PATHS
OP_PATHS = ["", "NOCHAIN", "NOAHEAD", "NOFUSEUPD", "NOOVERLAP", "CHAINMSE", "NOCHAIN,NOFUSEUPD,GTAPS"]
# two more cases with their own oracle run (same helpers): a mixed-axis grid, and 96 x 96 whose coarsest grid is 24 x 24
EXTRA = {  # Nx, Ny, maps, Nk, B
    "640x512": (640, 512, [3, 4, 3], 5, 2),
    "96x96-3x3": (96, 96, [4, 3], 3, 3),
}


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


@pytest.fixture
def cases(monkeypatch):
    """the helpers of test_gpu_pruned_smooth look a case up by name in CASES: the two extra ones are entered for the test's duration"""
    for k, v in EXTRA.items():
        monkeypatch.setitem(CASES, k, v)
    return CASES


def _net(ctx, Nx, Ny, ws, Nk, Nl, s, B, opform=True, D=3):
    net = aefft.Net(ctx, D, Nx, Ny, [w[0].shape[0] for w in ws], Nk, s, batch=B, Nl=Nl, smooth_sizes=True, operator_form=opform)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
    return net


def _form(ctx, Nx, Ny, maps, Nk, Nl, B, opform, D=3):
    net = aefft.Net(ctx, D, Nx, Ny, maps, Nk, 2, batch=B, Nl=Nl, smooth_sizes=True, operator_form=opform)
    f = net.step_form()
    net.close()
    return f


# ------------------------------------------------------------------------------------------
# 1. the form
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_form_of_an_opted_in_net(ctx, flags, name):
    Nx, Ny, maps, Nk, B = CASES[name]
    flags()
    assert _form(ctx, Nx, Ny, maps, Nk, Nk, B, True) == "operator_chain"
    assert _form(ctx, Nx, Ny, maps, Nk, Nk, B, False) == "per_frame"
    flags("NOCHAIN")
    assert _form(ctx, Nx, Ny, maps, Nk, Nk, B, True) == "operator"
    for sw in ("NOOPFORM", "NOQPATH", "NOPRUNESMOOTH"):
        flags(sw)
        assert _form(ctx, Nx, Ny, maps, Nk, Nk, B, True) == "per_frame", sw
    # the switches act on a live net as well
    flags()
    net = aefft.Net(ctx, 3, Nx, Ny, maps, Nk, 2, batch=B, smooth_sizes=True, operator_form=True)
    assert net.step_form() == "operator_chain"
    flags("NOPRUNESMOOTH")
    assert net.step_form() == "per_frame"
    flags()
    assert net.step_form() == "operator_chain"
    net.close()


def _oracle_check_plain(ctx, D, Nx, Ny, maps, Nk, Nl, B, seed):
    """two steps of a net outside the operator form's rules against the oracle, at _check_two_steps' tolerances"""
    rng = np.random.default_rng(seed)
    ws = _weights(rng, D, maps, Nk, Nl)
    xs = [np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))) for _ in range(2)]
    L = len(maps)
    net = _net(ctx, Nx, Ny, ws, Nk, Nl, 2, B, True, D)
    assert net.step_form() == "per_frame"
    run = _two_steps_w(ctx, net, [ctx.dev(x) for x in xs], B, D, Nx, Ny, L)
    assert net.step_form() == "per_frame"
    net.close()
    z = [tuple(np.zeros_like(a) for a in (w[0], w[2], w[1], w[3])) for w in ws]
    s1 = _oracle_step(xs[0], ws, z, 2, L)
    s2 = _oracle_step(xs[1], s1[0], s1[1], 2, L)
    for k, (w_or, _, mse, recon, grads, _) in enumerate((s1, s2)):
        rec_g, gbuf, mse_g, w_g = run[k]
        assert relerr(rec_g, recon) < 1e-4, k
        off = 0
        for l in range(L):
            c = ws[l][0]
            dM, dDl = c.shape[:2]
            nk = c.size
            for seg, ref in zip((gbuf[off:off + nk], gbuf[off + nk:off + 2 * nk], gbuf[off + 2 * nk:off + 2 * nk + dM],
                                 gbuf[off + 2 * nk + dM:off + 2 * nk + dM + dDl]), grads[l]):
                assert relerr(seg, ref.ravel()) < 5e-5, (k, l)
            off += 2 * nk + dM + dDl
            assert abs(mse_g[l] - mse[l]) < 1e-4 * max(1, mse[l]), (k, l)
            for a, ref, gi in zip(w_g[l], w_or[l], (0, 2, 1, 3)):
                assert (np.abs(a - ref) < weight_step_tol(grads[l][gi])).all(), (k, l, gi, np.abs(a - ref).max())


def test_nets_outside_the_rules_fall_back_to_the_per_frame_form(ctx, flags):
    """5 x 3 kernels at 96 x 96 and four input channels: per_frame with the option, and still the oracle's two steps"""
    flags()
    _oracle_check_plain(ctx, 3, 96, 96, [4, 3], 5, 3, 2, 9696)
    _oracle_check_plain(ctx, 4, 96, 96, [4, 3], 5, 5, 2, 9697)
    assert _form(ctx, 96, 96, [4, 3], 7, 7, 2, True) == "per_frame"


def test_option_without_smooth_sizes_or_on_a_power_of_two_net(ctx, flags):
    flags()
    with pytest.raises(Exception):
        aefft.Net(ctx, 3, 640, 480, [4, 3], 5, 2, batch=2, operator_form=True)
    forms = []
    for op in (False, True):
        net = aefft.Net(ctx, 3, 64, 64, [4, 3], 5, 2, batch=2, smooth_sizes=True, operator_form=op)
        forms.append(net.step_form())
        net.close()
    assert forms[0] == forms[1] == "operator_chain"


# ------------------------------------------------------------------------------------------
# 2. two steps against the float64 oracle, every operator-form route
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", OP_PATHS)
@pytest.mark.parametrize("name", list(CASES) + list(EXTRA))
def test_two_steps_against_the_oracle(ctx, flags, cases, name, path):
    """_check_two_steps unchanged: reconstruction and MSE 1e-4, packed gradients 5e-5, every weight within weight_step_tol after each step"""
    Nx, Ny, maps, Nk, B = cases[name]
    ws, xs = _case(name)
    flags(*path.split(","))
    net = _net(ctx, Nx, Ny, ws, Nk, Nk, 2, B)
    want = "operator" if "NOCHAIN" in path else "operator_chain"
    assert net.step_form() == want
    run = _two_steps_w(ctx, net, [ctx.dev(x) for x in xs], B, 3, Nx, Ny, len(maps))
    assert net.step_form() == want
    net.close()
    flags()
    _check_two_steps(name, run, (name, path, "opform"))


# ------------------------------------------------------------------------------------------
# 3. operator form == per-frame form, both reconstruction routes
# ------------------------------------------------------------------------------------------
def _one_step(ctx, net, frames, B, Nx, Ny, L, prof):
    recon = ctx.empty(B, 3, Nx, Ny); recon.fill_(float("nan"))
    if prof:
        ctx.prof_enable(); ctx.prof_reset()
    net.step_grad(frames, recon)
    ctx.sync()
    counts = None
    if prof:
        counts = {k: v["launches"] for k, v in ctx.prof_read().items()}; ctx.prof_enable(False)
    g = host(net.grad_buffer()).copy()
    layers = [host(t).copy() for t in net.get_layers()]
    return host(recon).copy(), g, layers, counts


@pytest.mark.parametrize("route,Nx,Ny,maps,s,B", [
    ("fused", 640, 480, [3, 4, 3, 2], 2, 2),      # decoder output on the coarsest grid (40 x 30): evaluated inside the column pass
    ("fused", 240, 320, [4, 3, 2], 2, 2),
    ("expand", 640, 480, [4], 1, 8),              # no pooling: 8 * 3 * 640 * 241 * 8 B = 29.6 MB > 16 MB, per-frame spectra written out
])
def test_operator_form_equals_per_frame_form(ctx, flags, route, Nx, Ny, maps, s, B):
    """one step of the same net on the same frames in both forms: reconstruction 2e-5, packed gradients 5e-5, every exported layer 5e-5
    (test_second_step_equals_fresh_net_with_updated_weights' bounds); the reconstruction route by the profiler's launch counts"""
    L = len(maps)
    rng = np.random.default_rng(Nx + Ny + L)
    ws = _weights(rng, 3, maps, 5, 5)
    frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, 3, Nx, Ny))))
    flags()
    net = _net(ctx, Nx, Ny, ws, 5, 5, s, B, True)
    assert net.step_form() in ("operator_chain", "operator")
    # (the profiled step decides its routes like any other but runs on one stream)
    _, _, _, counts = _one_step(ctx, net, frames, B, Nx, Ny, L, True)
    net.close()
    net = _net(ctx, Nx, Ny, ws, 5, 5, s, B, True)
    rec_o, g_o, lay_o, _ = _one_step(ctx, net, frames, B, Nx, Ny, L, False)
    net.close()
    net = _net(ctx, Nx, Ny, ws, 5, 5, s, B, False)
    assert net.step_form() == "per_frame"
    rec_p, g_p, lay_p, _ = _one_step(ctx, net, frames, B, Nx, Ny, L, False)
    net.close()
    print(route, counts)
    # "moment" counts the operator form's expansion launches (recon_expand, op_expand)
    if route == "expand":
        assert counts["moment"] == 1 and counts["c2r_cols"] == 1 and counts["c2r_rows"] == 1
    else:
        assert counts["moment"] == 0 and counts["c2r_cols"] == 1 and counts["c2r_rows"] == 1
    assert np.isfinite(rec_o).all()
    assert relerr(rec_o, rec_p) < 2e-5
    assert relerr(g_o[:-L], g_p[:-L]) < 5e-5
    assert len(lay_o) == len(lay_p) == 4 * L + 1
    for k, (a, b) in enumerate(zip(lay_o, lay_p)):
        assert relerr(a, b) < 5e-5, k


# ------------------------------------------------------------------------------------------
# 4. the routes by launch counts
# ------------------------------------------------------------------------------------------
def _step_profile(ctx, Nx, Ny, maps, seed, **kw):
    D, B = 3, 2
    L = len(maps)
    rng = np.random.default_rng(seed)
    ws = _weights(rng, D, maps, 5, 5)
    frames = ctx.dev(np.floor(rng.uniform(0, 256, (B, D, Nx, Ny))))
    net = aefft.Net(ctx, D, Nx, Ny, maps, 5, 2, batch=B, **kw)
    for l, w in enumerate(ws):
        net.set_pair(l, *w)
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


def test_opted_in_net_launches_what_the_power_of_two_net_launches(ctx, flags):
    """one step of the 640 x 480 [3, 4, 3, 2] net with the option, kernel id by kernel id, against the 512^2 net of the same maps in its
    default form; without the option the same net keeps the per-frame routes"""
    maps = [3, 4, 3, 2]
    flags()
    form, sm = _step_profile(ctx, 640, 480, maps, 64048, smooth_sizes=True, operator_form=True)
    form2, p2 = _step_profile(ctx, 512, 512, maps, 64048)
    form_pf, pf = _step_profile(ctx, 640, 480, maps, 64048, smooth_sizes=True)
    print("640x480 opted in:", sm, "\n512^2:", p2, "\n640x480:", pf)
    assert form == form2 == "operator_chain" and form_pf == "per_frame"
    assert sm == p2
    assert sm["pad"] == 0 and sm["shrink"] == 0 and sm["contract"] == 0 and sm["chain"] + sm["opmse"] > 0
    assert pf["contract"] > 0 and pf["chain"] == 0 and pf["sgrad"] == 0


# ------------------------------------------------------------------------------------------
# 5. layer exports
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["640x480", "240x320-3x3"])
def test_layer_exports_after_grad_and_after_apply(ctx, flags, name):
    """get_layers after step_grad and again after step_apply (operator-chain form: the layers of the step's forward, pre-update weights)
    against a per-frame net given the same weights and frames, 5e-5"""
    Nx, Ny, maps, Nk, B = CASES[name]
    ws, xs = _case(name)
    L = len(maps)
    frames = ctx.dev(xs[0])
    flags()
    ref = _net(ctx, Nx, Ny, ws, Nk, Nk, 2, B, False)
    ref.step_grad(frames, None)
    want = [host(t).copy() for t in ref.get_layers()]
    ref.close()
    net = _net(ctx, Nx, Ny, ws, Nk, Nk, 2, B, True)
    assert net.step_form() == "operator_chain"
    net.step_grad(frames, None)
    got1 = [host(t).copy() for t in net.get_layers()]
    net.step_apply(0.2)
    got2 = [host(t).copy() for t in net.get_layers()]
    single = host(net.get_layer(2 * L)).copy()
    net.close()
    assert len(want) == len(got1) == len(got2) == 4 * L + 1
    for k in range(4 * L + 1):
        assert relerr(got1[k], want[k]) < 5e-5, ("after step_grad", k)
        assert relerr(got2[k], want[k]) < 5e-5, ("after step_apply", k)
    assert relerr(single, want[2 * L]) < 5e-5


# ------------------------------------------------------------------------------------------
# 6. pipelined mode
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


def test_input_ready_gives_the_same_two_steps(ctx, flags):
    Nx, Ny, maps, B = 640, 480, [4, 3], 2
    L = len(maps)
    rng = np.random.default_rng(2 * 640 + 1)
    ws = _weights(rng, 3, maps, 5, 5)
    frames = [ctx.dev(np.floor(rng.uniform(0, 256, (B, 3, Nx, Ny)))) for _ in range(2)]
    flags()
    runs = []
    for ready in (False, True):
        net = _net(ctx, Nx, Ny, ws, 5, 5, 2, B, True)
        assert net.step_form() == "operator_chain"
        net.set_input_ready(ready)
        runs.append(_two_steps(ctx, net, frames, B, 3, Nx, Ny, L))
        net.close()
    assert np.isfinite(runs[0][0][0]).all()
    _same(runs[0], runs[1])


# ------------------------------------------------------------------------------------------
# 7. tied weights and the multiobjective term
# ------------------------------------------------------------------------------------------
def test_tied_weights_and_multiobjective_step(ctx, flags):
    """sym = 1, maxdiff = 1 at 240 x 320, one step of an opted-in net against np_ref.net_step (and a per-frame net beside it), at
    test_gpu_pruned_smooth.test_tied_weights_and_multiobjective_step's tolerances"""
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
    flags()
    for opform in (True, False):
        net = _net(ctx, Nx, Ny, ws, 5, 5, s, B, opform)
        assert net.step_form() == ("operator_chain" if opform else "per_frame")
        rec, mse = ctx.empty(B, 3, Nx, Ny), ctx.empty(L)
        net.step_grad(ctx.dev(xs), rec)
        net.step_apply(0.2, 1, 1, 1.0, mse)
        ctx.sync()
        assert relerr(host(rec), recon) < 1e-4
        for l in range(L):
            c2, b2, f2, p2 = net.get_pair(l)
            tc, tb, tp = tols[l]
            assert (np.abs(c2 - w1[l][0]) < tc).all() and (np.abs(f2 - w1[l][2]) < np.transpose(tc, (1, 0, 2, 3))).all(), (opform, l)
            assert (np.abs(b2 - w1[l][1]) < tb).all() and (np.abs(p2 - w1[l][3]) < tp).all(), (opform, l)
            assert abs(host(mse)[l] - mses[l]) < 1e-4 * max(1, mses[l]), (opform, l)
        net.close()


# ------------------------------------------------------------------------------------------
# 8. data parallel
# ------------------------------------------------------------------------------------------
def test_data_parallel_library_at_world_size_one(ctx, flags):
    """two steps through libaefft_dp.so on a communicator of one rank == two steps without the collective, bit for bit; replicas agree"""
    dp = importlib.import_module("autoencoder-fft_amd.dp")
    Nx, Ny, maps, B = 240, 320, [4, 3, 2], 2
    L = len(maps)
    rng = np.random.default_rng(41 + Nx)
    ws = _weights(rng, 3, maps, 5, 5)
    x = ctx.dev(np.floor(rng.uniform(0, 256, (B, 3, Nx, Ny))))
    recon = ctx.empty(B, 3, Nx, Ny)
    flags()
    plain = _net(ctx, Nx, Ny, ws, 5, 5, 2, B, True)
    mse = ctx.empty(L)
    for _ in range(2):
        plain.step_grad(x, recon); plain.step_apply(0.2, 0, 0, 1.0, mse)
    ctx.sync()
    want, want_mse = [plain.get_pair(l) for l in range(L)], host(mse).copy()
    plain.close()
    net = _net(ctx, Nx, Ny, ws, 5, 5, 2, B, True)
    assert net.step_form() == "operator_chain"
    step = dp.RcclStep(net, 0, 1)
    step(x, recon, 0.2)
    step(x, recon, 0.2, mse=mse)
    ctx.sync()
    for a, b in zip(want, [net.get_pair(l) for l in range(L)]):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert np.array_equal(host(mse), want_mse)
    assert step.replicas_agree()
    assert net.step_form() == "operator_chain"
    step.close(); net.close()
