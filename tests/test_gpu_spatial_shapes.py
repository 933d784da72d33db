"""Spatial-mode kernels on non-square grids (Nx != Ny), non-square supports (Nk != Nl) and the routes of launch_spatial_grad /
launch_dconv that square, small-dM cases never reach: 5x5 and 7x7 gradients on the matrix cores, run_mcorr's second row and column
tiles, tiles that hold only the ones column / the ones row, the CPU tap range (lo = 1), the naive kernels' gradients.

Everything is compared with oracle/np_spatial.py in float64 (cross-pinned at these kinds of shapes to the compiled CPU reference by
tests/test_oracle_crosspin.py::test_spatial_*).  Every case names the route it is meant to reach; `expected_route` restates
launch_spatial_grad's rule and `expected_conv` launch_dconv's, and the tables are asserted against them -- the profiler brackets a whole
route in one count, so the route is not observable from outside and the rule is restated instead.

Inputs: x = floor(U(0,256)), weights and biases U(-1,1); where the hidden layer is free, hin = U(-50,50) and out = x + U(-20,20).
Bounds: gradients 3e-5 of the tensor's largest reference element (the bound of
test_backprop_kernel_gradient_through_the_error_input_correlation), the fused step 5e-5 (its hidden layer is float32), weights and
momentum as test_backprop_gpu, convolutions 1e-5 * max(1, max|ref|).  np_spatial.gradients evaluated in float32 differs from float64
by at most 7.3e-7 of max|ref| at these inputs, so the bounds leave the reference's own conditioning 40x of room (the kernels' own
largest difference, measured on an MI355X when the module was written: 1.3e-6 of max|ref|)."""
import importlib

import numpy as np
import pytest

import cpu
import np_spatial as S

pytestmark = pytest.mark.gpu
aefft = importlib.import_module("autoencoder-fft_amd")


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def host(t):
    return t.detach().cpu().numpy()


# ---- the dispatch rules, restated ---------------------------------------------------------------------------------------------------
def _tiled(Nk, Nl, flags):
    """dconv_ok && !NOTILEDSPATIAL: the tiled kernels serve square 3x3, 5x5, 7x7 supports"""
    return Nk == Nl and Nk in (3, 5, 7) and "NOTILEDSPATIAL" not in flags


def expected_route(dD, dM, Nx, Ny, Nk, Nl, flags=()):
    """launch_spatial_grad: which kernel forms dC (aefft_backprop_spatial always passes the partial-sum and region workspaces)"""
    if not _tiled(Nk, Nl, flags):
        return "naive"                                   # backconv_kernel, wgrad_kernel, bgrad_kernel
    mfma = "NOMFMA" not in flags
    # rcorr_ok (ak == al == 0 and lo <= 1 hold for 3x3 under both boundary semantics)
    if Nk == 3 and dD in (1, 3) and dM >= 8 and Nx >= 8 and Ny >= 8 and Ny % 4 == 0 and mfma and "NORCORR" not in flags:
        return f"rcorr<{dD}>"                            # dC, dB from the region sums; dF, dP by mcorr<3> (fused step: region sums too)
    if dM >= 8 and Ny % 4 == 0 and mfma:
        return f"mcorr<{Nk}>"
    return f"wcorr<{Nk}>"


def expected_conv(dD, dM, Nx, Ny, Nk, Nl, flags=(), pool=False):
    """launch_conv_spatial / launch_dconv / run_dconv: which convolution kernel runs (dD input planes, dM output maps)"""
    if not _tiled(Nk, Nl, flags):
        return "conv_spatial_kernel"
    if (dM >= 8 and "NOMFMA" not in flags) or pool:
        return "mconv<2>" if dM > 32 else "mconv<1>"
    if dM <= 4 and Ny >= 64 and Nx * Ny * 4 < 2 ** 31 and dD * Nk * ((Nk * 4 + 3) & ~3) * 4 <= 32 * 1024 and "NOFAST" not in flags:
        return "dconv4"
    return "dconv<16>" if dM >= 12 else ("dconv<8>" if dM >= 6 else "dconv<4>")


def _settings(dD, dM, Nx, Ny, Nk, Nl):
    """the default and every switch that changes the case's route: (flags, route)"""
    base = expected_route(dD, dM, Nx, Ny, Nk, Nl)
    out = [((), base)]
    for fl in ("NORCORR", "NOMFMA", "NOTILEDSPATIAL"):
        r = expected_route(dD, dM, Nx, Ny, Nk, Nl, (fl,))
        if r != base:
            out.append(((fl,), r))
    return out


# ---- A. gradients through aefft_backprop_spatial, hidden layer free -------------------------------------------------------------------
# (B, dD, dM, Nx, Ny, Nk, Nl, tied, semantics), the default route, what the case reaches
GRAD_CASES = [
    ((2, 3, 8, 20, 36, 5, 5, False, "gpu"), "mcorr<5>"),    # 76 columns = NCB 3; NRB 1; last band 4 of 8 rows; Ny < one 64-column chunk
    ((1, 4, 40, 12, 72, 5, 5, False, "gpu"), "mcorr<5>"),   # 101 columns = two column tiles; the first spans 4 planes: plane groups staged in
                                                            # turn (!one_group); NRB 2; second column chunk 8 wide
    ((1, 2, 70, 10, 16, 7, 7, False, "gpu"), "mcorr<7>"),   # two column tiles (99 columns); 70 / 71 rows = second row tile
    ((2, 3, 9, 9, 12, 7, 7, True, "gpu"), "mcorr<7>"),      # tied (gc + gf^T)
    ((2, 3, 12, 20, 36, 5, 5, True, "gpu"), "mcorr<5>"),    # tied
    ((1, 2, 66, 14, 24, 3, 3, False, "gpu"), "mcorr<3>"),   # dC by mcorr<3> with dD = 2 (not the region route); two row tiles
    ((1, 32, 64, 10, 12, 3, 3, False, "gpu"), "mcorr<3>"),  # 288 + 1 columns: the last column tile holds only the ones column (dB);
                                                            # 64 + 1 rows for dF: the second row tile holds only the ones row (dP)
    ((1, 3, 32, 12, 16, 5, 5, False, "gpu"), "mcorr<5>"),   # dC 32 rows (NRB 1), dF 33 rows (NRB 2)
    ((1, 3, 10, 22, 28, 5, 5, False, "cpu"), "mcorr<5>"),   # lo = 1, taps -3..1
    ((1, 2, 9, 18, 20, 7, 7, False, "cpu"), "mcorr<7>"),    # lo = 1, taps -5..1
    ((2, 3, 5, 18, 30, 7, 7, False, "gpu"), "wcorr<7>"),    # dM < 8
    ((1, 2, 12, 21, 17, 5, 5, False, "gpu"), "wcorr<5>"),   # Ny odd, although dM >= 8
    ((2, 3, 4, 33, 10, 3, 3, True, "gpu"), "wcorr<3>"),     # third 16-row band has one row
    ((1, 3, 6, 19, 26, 7, 7, False, "cpu"), "wcorr<7>"),    # lo = 1
    ((2, 3, 8, 12, 40, 3, 3, False, "gpu"), "rcorr<3>"),    # wide grid
    ((1, 1, 9, 40, 12, 3, 3, True, "gpu"), "rcorr<1>"),     # tall grid, tied
    ((2, 3, 12, 24, 16, 3, 3, False, "cpu"), "rcorr<3>"),   # lo = 1
    ((1, 3, 8, 10, 268, 3, 3, False, "gpu"), "rcorr<3>"),   # two 256-column blocks on a 10-row image
    ((1, 2, 3, 10, 14, 5, 3, False, "gpu"), "naive"),       # Nk != Nl
    ((2, 3, 4, 12, 9, 3, 7, False, "gpu"), "naive"),
    ((1, 3, 9, 16, 12, 5, 3, True, "gpu"), "naive"),        # tied
]
GRAD_RUNS = [(case, fl, route) for case, _ in GRAD_CASES for fl, route in _settings(*case[1:7])]


def test_route_tables_follow_the_dispatch_rule():
    """the routes written beside the cases are what launch_spatial_grad's / launch_dconv's rule gives, and every switch sends a case where
    the module says: NORCORR to the matrix-core correlation, NOMFMA to wcorr, NOTILEDSPATIAL to the naive kernels"""
    for case, route in GRAD_CASES:
        B, dD, dM, Nx, Ny, Nk, Nl, tied, sem = case
        assert expected_route(dD, dM, Nx, Ny, Nk, Nl) == route, case
        for fl, r in _settings(dD, dM, Nx, Ny, Nk, Nl)[1:]:
            want = {"NORCORR": "mcorr<3>", "NOMFMA": f"wcorr<{Nk}>", "NOTILEDSPATIAL": "naive"}[fl[0]]
            assert r == want, (case, fl)
        if route.startswith("rcorr"):
            assert [fl for fl, _ in _settings(dD, dM, Nx, Ny, Nk, Nl)] == [(), ("NORCORR",), ("NOMFMA",), ("NOTILEDSPATIAL",)]
        elif route.startswith("mcorr"):
            assert [fl for fl, _ in _settings(dD, dM, Nx, Ny, Nk, Nl)] == [(), ("NOMFMA",), ("NOTILEDSPATIAL",)]
        elif route.startswith("wcorr"):
            assert [fl for fl, _ in _settings(dD, dM, Nx, Ny, Nk, Nl)] == [(), ("NOTILEDSPATIAL",)]
        else:
            assert _settings(dD, dM, Nx, Ny, Nk, Nl) == [((), "naive")]
    for case, route in STEP_CASES:
        assert expected_route(*case[1:7]) == route, case
    for case, kernel in CONV_CASES:
        dD, dM, Nx, Ny, Nk, Nl, B, sem = case
        assert expected_conv(dD, dM, Nx, Ny, Nk, Nl) == kernel, case
    for (dD, dM, Nxi, Nyi, s, Nk, sem), kernel in POOL_CONV_CASES:
        assert expected_conv(dD, dM, Nxi // s, Nyi // s, Nk, Nk, pool=True) == kernel


def _seed(case):
    return sum((i + 1) * int(v) for i, v in enumerate(case[:7])) + (1000 if case[7] else 0) + (2000 if case[8] == "cpu" else 0)


def _step(g, d, delmax, alpha):
    return S._step(g, d, delmax, alpha, np.float64)


def _ref_backprop(x, out, hin, c, b, f, p, mom, delmax, alpha, tied, sem):
    """(c, b, f, p, dc, db, df, dp, ddc, ddb, ddf, ddp) in float64: S.backprop_gpu(B_mean=True) for the GPU geometry; for the CPU geometry the
    batch mean of S.gradients(lo=1, cpu_geom=True) through the same clipped-momentum update"""
    if sem == "gpu":
        return S.backprop_gpu(list(x), list(out), list(hin), c, b, f, p, *mom, delmax, alpha, tied=tied, B_mean=True)
    gs = [S.gradients(xx, oo, hh, f, tied, lo=1, cpu_geom=True) for xx, oo, hh in zip(x, out, hin)]
    gc, gf, gb, gp = (sum(t) / len(gs) for t in zip(*gs))
    c = np.asarray(c, np.float64); f = np.asarray(f, np.float64)
    dc, db, df, dp = mom
    if tied:
        g = gc + np.transpose(gf, (1, 0, 2, 3))
        dc = _step(g, dc, delmax, alpha); c = c - dc
        f = np.transpose(c, (1, 0, 2, 3)).copy()
        ddc, ddf = g, None
    else:
        dc = _step(gc, dc, delmax, alpha); c = c - dc
        df = _step(gf, df, delmax, alpha); f = f - df
        ddc, ddf = gc, gf
    db = _step(gb, db, delmax, alpha); dp = _step(gp, dp, delmax, alpha)
    return c, np.asarray(b, np.float64) - db, f, np.asarray(p, np.float64) - dp, dc, db, df, dp, ddc, gb, ddf, gp


_grad_inputs = {}


def _grad_case(case):
    """inputs and float64 reference of a case, computed once and shared by the runs under every switch (never written to)"""
    if case not in _grad_inputs:
        B, dD, dM, Nx, Ny, Nk, Nl, tied, sem = case
        rng = np.random.default_rng(_seed(case))
        x = np.floor(rng.uniform(0, 256, (B, dD, Nx, Ny))).astype(np.float32)
        c = rng.uniform(-1, 1, (dM, dD, Nk, Nl)).astype(np.float32); f = rng.uniform(-1, 1, (dD, dM, Nk, Nl)).astype(np.float32)
        b = rng.uniform(-1, 1, dM).astype(np.float32); p = rng.uniform(-1, 1, dD).astype(np.float32)
        hin = rng.uniform(-50, 50, (B, dM, Nx, Ny)).astype(np.float32)
        out = (x + rng.uniform(-20, 20, x.shape)).astype(np.float32)
        mom = [0.01 * rng.normal(size=a.shape).astype(np.float32) for a in (c, b, f, p)]      # dc, db, df, dp
        ref = _ref_backprop(x, out, hin, c, b, f, p, mom, 0.2, 0.9, tied, sem)
        _grad_inputs[case] = ((x, out, hin, c, b, f, p), mom, ref)
    return _grad_inputs[case]


NAMES = ["c", "b", "f", "p", "dc", "db", "df", "dp", "ddc", "ddb", "ddf", "ddp"]


@pytest.mark.parametrize("case,fl,route", GRAD_RUNS, ids=[f"{'-'.join(str(v) for v in c)}-{'+'.join(fl) or 'default'}-{r}" for c, fl, r in GRAD_RUNS])
def test_gradients_on_every_route(ctx, flags, case, fl, route):
    """aefft_backprop_spatial with a hidden layer that is not conv(in), under the default and under each switch that changes the route:
    ddc, ddb, ddf, ddp each against the oracle, then the weights and the momentum from a non-zero momentum; tied: f == c^T to the bit"""
    B, dD, dM, Nx, Ny, Nk, Nl, tied, sem = case
    assert expected_route(dD, dM, Nx, Ny, Nk, Nl, fl) == route
    arrs, mom, ref = _grad_case(case)
    flags(*fl)
    t = [ctx.dev(a) for a in arrs]
    tm = [ctx.dev(a) for a in mom]
    tg = [ctx.dev(np.zeros_like(a)) for a in arrs[3:]]
    ctx.backprop_spatial(*t, tm, tg, 0.2, 0.9, tied=tied, semantics=sem)
    got = dict(zip(NAMES, [host(a) for a in (t[3], t[4], t[5], t[6], *tm, *tg)]))
    refd = dict(zip(NAMES, ref))
    for k in ("ddc", "ddb", "ddf", "ddp"):
        if refd[k] is None:
            continue                                    # tied: ddc holds gc + gf^T and ddf is not written
        err, scale = np.abs(got[k] - refd[k]).max(), np.abs(refd[k]).max()
        print(f"{k}: err {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}")
        assert err < 3e-5 * scale, (k, err, scale)
    for k in NAMES[:8]:
        if tied and k == "df":
            continue
        scale = max(np.abs(refd[k]).max(), 1e-6) if k.startswith("d") else max(np.abs(refd["dc"]).max(), 1e-6)
        assert np.abs(got[k] - refd[k]).max() < 1e-6 + 1e-3 * scale, k
    if tied:
        assert np.array_equal(got["f"], np.transpose(got["c"], (1, 0, 2, 3)))


# ---- B. the fused step ----------------------------------------------------------------------------------------------------------------
STEP_CASES = [
    ((2, 3, 8, 12, 40, 3, 3, False, "gpu"), "rcorr<3>"),    # region sums give dF and dP too
    ((1, 3, 9, 40, 12, 3, 3, True, "cpu"), "rcorr<3>"),
    ((1, 3, 10, 14, 20, 5, 5, False, "gpu"), "mcorr<5>"),   # plain sequence inside the call
    ((1, 2, 9, 16, 12, 7, 7, False, "gpu"), "mcorr<7>"),
    ((1, 2, 3, 10, 14, 5, 3, False, "gpu"), "naive"),       # plain sequence, naive kernels
]


@pytest.mark.parametrize("case,route", STEP_CASES, ids=["-".join(str(v) for v in c) + "-" + r for c, r in STEP_CASES])
def test_fused_step_on_non_square_grids(ctx, flags, case, route):
    """aefft_step_spatial as in test_fused_spatial_step_gradients_from_the_region_sums, with Nx != Ny and the supports the region route
    declines: layers == the separate conv_spatial calls bit for bit; gradients, weights, momentum == the three separate calls == the oracle"""
    B, dD, dM, Nx, Ny, Nk, Nl, tied, sem = case
    rng = np.random.default_rng(_seed(case))
    x = np.floor(rng.uniform(0, 256, (B, dD, Nx, Ny))).astype(np.float32)
    c = rng.uniform(-1, 1, (dM, dD, Nk, Nl)).astype(np.float32); f = rng.uniform(-1, 1, (dD, dM, Nk, Nl)).astype(np.float32)
    b = rng.uniform(-1, 1, dM).astype(np.float32); p = rng.uniform(-1, 1, dD).astype(np.float32)
    mom = [0.01 * rng.normal(size=a.shape).astype(np.float32) for a in (c, b, f, p)]
    flags()
    tw = [ctx.dev(a) for a in (c, b, f, p)]
    tm = [ctx.dev(a) for a in mom]
    tg = [ctx.dev(np.zeros_like(a)) for a in (c, b, f, p)]
    xd = ctx.dev(x)
    h0 = ctx.conv_spatial(xd, tw[0], tw[1], semantics=sem)
    o0 = ctx.conv_spatial(h0, tw[2], tw[3], semantics=sem)
    ctx.backprop_spatial(xd, o0, h0, *tw, tm, tg, 0.2, 0.9, tied=tied, semantics=sem)
    sep = [host(t).copy() for t in tw + tm + tg]
    tw = [ctx.dev(a) for a in (c, b, f, p)]
    tm = [ctx.dev(a) for a in mom]
    tg = [ctx.dev(np.zeros_like(a)) for a in (c, b, f, p)]
    h1, o1 = ctx.step_spatial(xd, *tw, tm, tg, 0.2, 0.9, tied=tied, semantics=sem)
    fus = [host(t).copy() for t in tw + tm + tg]
    assert np.array_equal(host(h1), host(h0)) and np.array_equal(host(o1), host(o0))
    for k, a, r in zip(NAMES, fus, sep):
        if tied and k in ("df", "ddf"):
            continue
        ref_scale = max(np.abs(sep[8]).max(), 1e-30) if k in ("ddc", "ddf") else max(np.abs(r).max(), 1e-30)
        if k.startswith("dd"):
            assert np.abs(a - r).max() < 5e-5 * ref_scale, (k, np.abs(a - r).max(), ref_scale)
        else:
            # one clipped-momentum step from the same gradients up to 5e-5: 0.02 * dg / 10
            assert np.abs(a - r).max() < 1e-6 + 0.02 / 10 * 5e-5 * max(np.abs(sep[8]).max(), np.abs(sep[10]).max(), np.abs(sep[9]).max(), np.abs(sep[11]).max()), k
    cs = sem == "cpu"
    hin = [S.conv(x[i], c, b, cpu_semantics=cs) for i in range(B)]
    out = [S.conv(hin[i], f, p, cpu_semantics=cs) for i in range(B)]
    ref = _ref_backprop(x, out, hin, c, b, f, p, mom, 0.2, 0.9, tied, sem)
    for k, g, r in zip(NAMES[8:], fus[8:], ref[8:]):
        if r is not None:
            err, scale = np.abs(g - r).max(), max(np.abs(r).max(), 1e-30)
            print(f"{k}: err {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}")
            assert err < 5e-5 * scale, (k, err, scale)


# ---- C. convolutions ------------------------------------------------------------------------------------------------------------------
# (dD, dM, Nx, Ny, Nk, Nl, B, semantics), the default kernel
CONV_CASES = [
    ((3, 10, 12, 40, 5, 5, 2, "gpu"), "mconv<1>"),
    ((4, 40, 9, 36, 7, 7, 1, "gpu"), "mconv<2>"),           # ragged 8x32 tiles
    ((5, 3, 10, 72, 3, 3, 2, "gpu"), "dconv4"),             # short and wide
    ((5, 3, 10, 72, 3, 3, 2, "cpu"), "dconv4"),
    ((2, 6, 21, 17, 5, 5, 1, "gpu"), "dconv<8>"),
    ((3, 5, 14, 9, 5, 3, 1, "gpu"), "conv_spatial_kernel"),
    ((2, 4, 9, 15, 3, 7, 1, "cpu"), "conv_spatial_kernel"),
]


@pytest.mark.parametrize("case,kernel", CONV_CASES, ids=["-".join(str(v) for v in c) + "-" + k for c, k in CONV_CASES])
def test_conv_on_non_square_grids(ctx, flags, case, kernel):
    """aefft_conv_spatial against the oracle under the default and under NOMFMA / NOFAST where the switch changes the kernel"""
    dD, dM, Nx, Ny, Nk, Nl, B, sem = case
    rng = np.random.default_rng(_seed((B,) + case[:6] + (False, sem)))
    x = np.floor(rng.uniform(0, 256, (B, dD, Nx, Ny))).astype(np.float32)
    c = rng.uniform(-1, 1, (dM, dD, Nk, Nl)).astype(np.float32); b = rng.uniform(-1, 1, dM).astype(np.float32)
    ref = [S.conv(x[i], c, b, cpu_semantics=(sem == "cpu")) for i in range(B)]
    runs = [()] + [(fl,) for fl in ("NOMFMA", "NOFAST") if expected_conv(dD, dM, Nx, Ny, Nk, Nl, (fl,)) != kernel]
    assert len(runs) == (1 if kernel == "conv_spatial_kernel" or kernel.startswith("dconv<") else 2)
    for fl in runs:
        flags(*fl)
        got = host(ctx.conv_spatial(ctx.dev(x), ctx.dev(c), ctx.dev(b), semantics=sem))
        for i in range(B):
            assert np.abs(got[i] - ref[i]).max() < 1e-5 * max(1, np.abs(ref[i]).max()), (fl, i)


# (dD, dM, input Nx, input Ny, scale, Nk, semantics): Pool exists only in the matrix-core kernel
POOL_CONV_CASES = [((3, 9, 24, 40, 2, 3, "gpu"), "mconv<1>"), ((2, 4, 18, 30, 3, 5, "cpu"), "mconv<1>")]


@pytest.mark.parametrize("case,kernel", POOL_CONV_CASES, ids=["-".join(str(v) for v in c) for c, k in POOL_CONV_CASES])
def test_fused_pool_conv_on_non_square_grids(ctx, case, kernel):
    """as test_fused_pool_conv_equals_pool_then_conv: the pooled layer bit for bit against the reference Pool, the output against the oracle"""
    dD, dM, Nxi, Nyi, s, Nk, sem = case
    L = cpu.reference() or cpu.port()
    rng = np.random.default_rng(Nxi * 7 + Nyi + Nk + s)
    B = 2
    x = rng.uniform(-40, 260, (B, dD, Nxi, Nyi)).astype(np.float32)
    c = rng.uniform(-1, 1, (dM, dD, Nk, Nk)).astype(np.float32); b = rng.uniform(-1, 1, dM).astype(np.float32)
    pooled, out = ctx.pool_conv_spatial(ctx.dev(x), ctx.dev(c), ctx.dev(b), s, semantics=sem)
    nx, ny = Nxi // s, Nyi // s
    for i in range(B):
        pref = L.pool(x[i], (dD, nx, ny), s)
        assert np.array_equal(host(pooled)[i], pref)
        ref = S.conv(pref, c, b, cpu_semantics=(sem == "cpu"))
        assert np.abs(host(out)[i] - ref).max() < 1e-5 * max(1, np.abs(ref).max())
    _, out2 = ctx.pool_conv_spatial(ctx.dev(x), ctx.dev(c), ctx.dev(b), s, semantics=sem, want_pooled=False)
    assert np.array_equal(host(out2), host(out))
