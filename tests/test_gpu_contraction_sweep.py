"""The per-bin channel contraction route by route, and gradient_diff where kernels are close, at the reference's float32.

A.  aefft_conv / aefft_gradient / aefft_mse.  One entry point (launch_contract2) fans out into the matrix-core kernel (VEC 1/2, tiles 1x1 /
1x2 / 2x2, DIFF, split-K), the lean scalar kernel (classes conv / S / dc|df, tiles 2x2 .. 4x4, VEC 1/2, split-K) and the generic scalar
kernel, chosen from R, C, K, P by thresholds.  Every case of CASES names the instantiation it is meant for; `contract_route` restates the
selection rules in Python, each case asserts that the restatement gives the route its id names, and a CPU test asserts that the table
reaches every instantiation the three ops can select.

Metric, as tests/test_gpu_transform_sweep.py: relative L2 error and worst bin max|err| / rms(ref) against the float64 oracle, on inputs where
no bin sets the scale (complex normal spectra and kernel spectra; O = T + 0.3 noise for the DIFF operand); the DC bin, which carries
b Nx Ny (conv) and the b0 term (df), is measured apart from the AC bins.  The bound is the error of the oracle's own float32 replay of the same
call (np_ref.conv_k / gradient_k_io with dtype=float32) times FACTOR, plus the transform sweep's floors.

FACTOR = 4 for both ops.  conv is the same sum in the same order as the replay (split-K and the matrix cores' 4-term groups only shorten the
chains).  The gradient is re-associated -- S = sum_b (O - T) X^H first, then F^H S and S C^H (ops.hip do_gradient) -- but each output still goes
through one chain of length B and one of length dD, like the literal loop nest that sums over d1 per frame and then averages the B frames;
with error ~ sqrt(chain length) * eps for either order, the two forms sit at the same level and no factor beyond the transform sweep's 4 follows
from the operation counts.  The worst GPU / peer ratio per route is printed at the end of the module (pytest -s).

The 2x2 matrix-core tile needs w2 >= 32768: 512x512, dM = 16, B = 8, dD = 3 for conv (w2 = 32896); for the DIFF form S has R = C = dD, so
dD >= 9 at 512x512 (B = 1, dM = 1 keeps the float64 oracle at ~1 s).

aefft_mse: the oracle sums in float64, so it gives no float32 level; the project's stated 1e-5 is applied relative to the MSE itself
at input scales that give MSE ~ 1e-3, 1 and 1e4.

B.  gradient_diff (update_kernels.hip gdiff_part_body) through aefft_update with maxdiff = 1, zero gradient spectra and zero momentum: the weight
change is -0.1 del g / max(10, |g|) with g = -10 g_diff.  The kernels are one base kernel + eps U(-1, 1) (the regime the repulsion term exists
for), or U(-1, 1) kernels with one near-duplicate pair.  Almost every tap is clipped, so what is observable is the sign of the step and
finiteness: `assert_update` compares every tap clearly above the knee with the oracle's clipped step, every tap clearly below at
weight_step_tol, and leaves out at most 1 % of a tensor's taps (those within 1e-3 of the knee).  A CPU test puts the oracle's float32 replay
(np_ref.gradient_diff + backprop_double with dtype=float32) of exactly the same inputs through the same assertion: the inputs are ones the
reference's own float32 arithmetic stays within."""
import importlib

import numpy as np
import pytest

import np_ref as R
from test_gpu_fft_path import host, weight_step_tol
from test_gpu_transform_sweep import DC_FLOOR, FLOOR_L2, FLOOR_MAX, PEER_FACTOR, cnormal, metrics

aefft = importlib.import_module("autoencoder-fft_amd")
gpu = pytest.mark.gpu

FACTOR = PEER_FACTOR      # 4.0: see the module docstring
WORST = {}                # route -> [worst ratio to the peer, case, GPU l2, GPU max/rms]


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nworst GPU error per contraction route (ratio to the float32 peer; GPU relative L2; GPU max|err|/rms(ref)):")
        for k in sorted(WORST):
            r, case, l2, mx = WORST[k]
            print(f"  {k:64s} {r:6.2f}  {l2:.2e}  {mx:.2e}  {case}")


def check(route, case, got, ref, peer, factor=FACTOR, floors=(FLOOR_L2, FLOOR_MAX)):
    """test_gpu_transform_sweep.check with this module's table.  got, peer: float32 results of the same input; ref: float64."""
    g2, gm = metrics(got, ref)
    p2, pm = metrics(peer, ref)
    if p2 > 0 and pm > 0:
        ratio = max(g2 / p2, gm / pm)
        w = WORST.get(route)
        if w is None or ratio > w[0]:
            WORST[route] = [ratio, case, g2, gm]
    assert g2 <= factor * p2 + floors[0] and gm <= factor * pm + floors[1], \
        f"{route} {case}: relative L2 {g2:.3e} (peer {p2:.3e}), max/rms {gm:.3e} (peer {pm:.3e})"


# ------------------------------------------------------------------------------------------
# the selection rules, restated
# ------------------------------------------------------------------------------------------
CLASSES = ("conv", "S", "dcdf")


def _cdiv(a, b):
    return -(-a // b)


def contract_route(probs, cls, flags=()):
    """Which instantiation serves one launch of launch_contract2: a Python restatement of
        contract_mfma.hip:383-416   launch_contract_mfma (VEC, split-K, tile)
        spectral_kernels.hip:533-552  contract_fast_class (0 conv, 1 S, 2 dc|df -- what the three ops build, ops.hip:173-241)
        spectral_kernels.hip:559-618  launch_contract2 (tile shrinking, lean / generic, split-K)
    for the descriptors of aefft_conv and aefft_gradient: no remap, biasAfterFirst, every stride a multiple of P (so `even` is P % 2 == 0),
    tensors below the 32-bit offset limit (asserted).  It can drift from the C++: it is a second statement of the rules, kept in step by hand.
    probs: [(R, C, K, P)] (two for dc|df); cls: index into CLASSES; flags: names of development switches.
    Returns (family, VEC, "TRxTC", KS, class name); the generic kernel has no classes (None)."""
    diff = cls == 1
    even = all(P % 2 == 0 for _, _, _, P in probs)
    for Rr, Cc, K, P in probs:
        assert min(Rr, Cc, K, P) > 0 and max(Rr, Cc) * K * P * 8.0 < 4.0e9
    if "NOMFMA" not in flags:
        w2 = sum(_cdiv(P, 32) * _cdiv(Rr, 4) * _cdiv(Cc, 4) for Rr, Cc, K, P in probs)
        vec = 2 if even and w2 >= 2048 else 1
        ks = [4 if K >= 32 and Rr * Cc <= 1024 and P <= 4096 else 1 for Rr, Cc, K, P in probs]
        Rmax, Cmax = max(q[0] for q in probs), max(q[1] for q in probs)
        trb, tcb = 1, (2 if Cmax >= 8 and max(ks) == 1 and not diff else 1)
        if w2 >= 32768 and Rmax >= 8 and Cmax >= 8:
            trb = tcb = 2
        assert len(set(ks)) == 1
        return ("mfma", vec, f"{trb}x{tcb}", ks[0], CLASSES[cls])
    Rmin, Cmin, Kmin = (min(q[i] for q in probs) for i in range(3))
    tr = 4 if Rmin >= 4 else (2 if Rmin >= 2 else 1)
    tc = 4 if Cmin >= 4 else (2 if Cmin >= 2 else 1)
    vec = 2 if even else 1
    waves = lambda v, r, c: sum(_cdiv(P, 64 * v) * _cdiv(Rr, r) * _cdiv(Cc, c) for Rr, Cc, K, P in probs)
    if waves(vec, tr, tc) < 4096 and tr == 4:
        tr = 2
    if waves(vec, tr, tc) < 1024 and vec == 2:
        vec = 1
    if "NOFAST" not in flags and tr >= 2 and tc >= 2:
        splitk = "NOSPLITK" not in flags and Kmin >= 16 and waves(vec, tr, tc) < 4096 and vec * tr * tc <= 16
        return ("lean", vec, f"{tr}x{tc}", 4 if splitk else 1, CLASSES[cls])
    return ("generic", vec, f"{tr}x{tc}", 1, None)


def route_name(r):
    fam, vec, tile, ks, cls = r
    return f"{fam} v{vec} {tile} ks{ks}" + (f" {cls}" if cls else "")


def op_routes(op, Nx, Ny, dM, dD, B, flags=()):
    """the launches of one op call as [(R, C, K, P)] per launch (ops.hip mk_conv, mk_S, mk_dc | mk_df) -> their routes"""
    P = Nx * (Ny // 2 + 1)
    if op == "conv":
        return [contract_route([(dM, B, dD, P)], 0, flags)]
    return [contract_route([(dD, dD, B, P)], 1, flags), contract_route([(dM, dD, dD, P), (dD, dM, dD, P)], 2, flags)]


def reachable_routes():
    """every instantiation the restated rules select for aefft_conv / aefft_gradient over the sizes the ops take (Nx even, so P is even) and
    the switch sets that change the choice"""
    out = set()
    grids = [(8, 8), (16, 8), (10, 12), (48, 20), (64, 64), (256, 256), (640, 480), (512, 512), (2048, 2048)]
    chans = [1, 2, 3, 4, 8, 9, 16, 32, 64, 128]
    for Nx, Ny in grids:
        for dM in chans:
            for dD in chans:
                for B in chans:
                    if max(dM, B) * dD * Nx * (Ny // 2 + 1) * 8.0 >= 4.0e9 or dD * max(dD, dM, B) * Nx * (Ny // 2 + 1) * 8.0 >= 4.0e9:
                        continue
                    for fl in ((), ("NOMFMA",), ("NOMFMA", "NOSPLITK"), ("NOMFMA", "NOFAST")):
                        out.update(op_routes("conv", Nx, Ny, dM, dD, B, fl))
                        out.update(op_routes("grad", Nx, Ny, dM, dD, B, fl))
    return out


# ------------------------------------------------------------------------------------------
# the case table: (op, Nx, Ny, dM, dD, B, flags, route names -- one for conv; S and dc|df for the gradient)
# ------------------------------------------------------------------------------------------
MF, NM, NS, NF = "", "NOMFMA", "NOMFMA,NOSPLITK", "NOMFMA,NOFAST"
CASES = [
    # ---- matrix-core kernel, conv: VEC x tile x split-K; K remainder groups; clamped rows / columns; P not a multiple of 16 VEC
    ("conv", 8, 8, 4, 1, 1, MF, ["mfma v1 1x1 ks1 conv"]),
    ("conv", 8, 8, 3, 2, 5, MF, ["mfma v1 1x1 ks1 conv"]),
    ("conv", 16, 8, 5, 3, 3, MF, ["mfma v1 1x1 ks1 conv"]),
    ("conv", 10, 12, 9, 7, 1, MF, ["mfma v1 1x1 ks1 conv"]),
    ("conv", 10, 12, 1, 13, 9, MF, ["mfma v1 1x2 ks1 conv"]),
    ("conv", 48, 20, 70, 3, 3, MF, ["mfma v1 1x1 ks1 conv"]),
    ("conv", 48, 20, 5, 13, 9, MF, ["mfma v1 1x2 ks1 conv"]),
    ("conv", 8, 8, 9, 33, 5, MF, ["mfma v1 1x1 ks4 conv"]),
    ("conv", 10, 12, 3, 37, 70, MF, ["mfma v1 1x1 ks4 conv"]),
    ("conv", 48, 20, 1, 33, 1, MF, ["mfma v1 1x1 ks4 conv"]),
    ("conv", 64, 64, 70, 7, 5, MF, ["mfma v2 1x1 ks1 conv"]),
    ("conv", 64, 64, 9, 2, 70, MF, ["mfma v2 1x2 ks1 conv"]),
    ("conv", 48, 20, 70, 13, 9, MF, ["mfma v1 1x2 ks1 conv"]),
    ("conv", 64, 64, 32, 37, 32, MF, ["mfma v2 1x1 ks4 conv"]),
    ("conv", 640, 480, 3, 5, 2, MF, ["mfma v2 1x1 ks1 conv"]),
    ("conv", 640, 480, 9, 3, 8, MF, ["mfma v2 1x2 ks1 conv"]),
    ("conv", 640, 480, 9, 3, 9, MF, ["mfma v2 2x2 ks1 conv"]),
    ("conv", 512, 512, 16, 3, 8, MF, ["mfma v2 2x2 ks1 conv"]),
    # ---- matrix-core kernel, gradient: DIFF 1x1 / 2x2, split-K with and without DIFF, the dc|df pair on every tile
    ("grad", 8, 8, 4, 3, 1, MF, ["mfma v1 1x1 ks1 S", "mfma v1 1x1 ks1 dcdf"]),
    ("grad", 16, 8, 9, 5, 7, MF, ["mfma v1 1x1 ks1 S", "mfma v1 1x2 ks1 dcdf"]),
    ("grad", 10, 12, 3, 9, 33, MF, ["mfma v1 1x1 ks4 S", "mfma v1 1x2 ks1 dcdf"]),
    ("grad", 8, 8, 5, 32, 2, MF, ["mfma v1 1x1 ks1 S", "mfma v1 1x1 ks4 dcdf"]),
    ("grad", 48, 20, 1, 3, 37, MF, ["mfma v1 1x1 ks4 S", "mfma v1 1x1 ks1 dcdf"]),
    ("grad", 64, 64, 4, 13, 3, MF, ["mfma v1 1x1 ks1 S", "mfma v1 1x2 ks1 dcdf"]),
    ("grad", 64, 64, 16, 16, 3, MF, ["mfma v1 1x1 ks1 S", "mfma v2 1x2 ks1 dcdf"]),
    ("grad", 64, 64, 1, 24, 33, MF, ["mfma v2 1x1 ks4 S", "mfma v1 1x2 ks1 dcdf"]),
    ("grad", 64, 64, 32, 32, 2, MF, ["mfma v2 1x1 ks1 S", "mfma v2 1x1 ks4 dcdf"]),
    ("grad", 64, 64, 70, 3, 5, MF, ["mfma v1 1x1 ks1 S", "mfma v2 1x2 ks1 dcdf"]),
    ("grad", 640, 480, 2, 3, 2, MF, ["mfma v2 1x1 ks1 S", "mfma v2 1x1 ks1 dcdf"]),
    ("grad", 640, 480, 8, 9, 1, MF, ["mfma v2 2x2 ks1 S", "mfma v2 2x2 ks1 dcdf"]),
    ("grad", 512, 512, 1, 9, 1, MF, ["mfma v2 2x2 ks1 S", "mfma v2 1x2 ks1 dcdf"]),
    # ---- lean scalar kernel (NOMFMA): classes conv / S / dc|df, VEC 1 / 2, tiles 2x2 .. 4x4, split-K on and off
    ("conv", 8, 8, 3, 2, 2, NM, ["lean v1 2x2 ks1 conv"]),
    ("conv", 10, 12, 2, 37, 3, NM, ["lean v1 2x2 ks4 conv"]),
    ("conv", 10, 12, 2, 37, 3, NS, ["lean v1 2x2 ks1 conv"]),
    ("conv", 16, 8, 5, 7, 9, NM, ["lean v1 2x4 ks1 conv"]),
    ("conv", 48, 20, 9, 33, 5, NM, ["lean v1 2x4 ks4 conv"]),
    ("conv", 48, 20, 9, 33, 5, NS, ["lean v1 2x4 ks1 conv"]),
    ("conv", 640, 480, 3, 2, 2, NM, ["lean v2 2x2 ks1 conv"]),
    ("conv", 64, 64, 70, 16, 3, NM, ["lean v2 2x2 ks4 conv"]),
    ("conv", 64, 64, 9, 3, 70, NM, ["lean v2 2x4 ks1 conv"]),
    ("conv", 64, 64, 9, 33, 70, NM, ["lean v2 2x4 ks4 conv"]),
    ("conv", 64, 64, 9, 33, 70, NS, ["lean v2 2x4 ks1 conv"]),
    ("conv", 640, 480, 9, 3, 3, NM, ["lean v2 4x2 ks1 conv"]),
    ("conv", 640, 480, 9, 2, 5, NM, ["lean v2 4x4 ks1 conv"]),
    ("grad", 8, 8, 3, 2, 3, NM, ["lean v1 2x2 ks1 S", "lean v1 2x2 ks1 dcdf"]),
    ("grad", 10, 12, 2, 3, 37, NM, ["lean v1 2x2 ks4 S", "lean v1 2x2 ks1 dcdf"]),
    ("grad", 10, 12, 2, 3, 37, NS, ["lean v1 2x2 ks1 S", "lean v1 2x2 ks1 dcdf"]),
    ("grad", 16, 8, 9, 5, 3, NM, ["lean v1 2x4 ks1 S", "lean v1 2x4 ks1 dcdf"]),
    ("grad", 48, 20, 5, 16, 33, NM, ["lean v1 2x4 ks4 S", "lean v1 2x4 ks4 dcdf"]),
    ("grad", 48, 20, 5, 16, 33, NS, ["lean v1 2x4 ks1 S", "lean v1 2x4 ks1 dcdf"]),
    ("grad", 8, 8, 3, 16, 2, NM, ["lean v1 2x4 ks1 S", "lean v1 2x2 ks4 dcdf"]),
    ("grad", 640, 480, 2, 3, 2, NM, ["lean v2 2x2 ks1 S", "lean v2 2x2 ks1 dcdf"]),
    ("grad", 64, 64, 3, 16, 2, NM, ["lean v1 2x4 ks1 S", "lean v1 2x2 ks4 dcdf"]),
    ("grad", 256, 256, 2, 3, 16, NM, ["lean v2 2x2 ks4 S", "lean v2 2x2 ks1 dcdf"]),
    ("grad", 64, 64, 3, 70, 16, NM, ["lean v2 4x4 ks1 S", "lean v2 2x2 ks4 dcdf"]),
    ("grad", 64, 64, 5, 33, 16, NM, ["lean v2 2x4 ks4 S", "lean v2 2x4 ks4 dcdf"]),
    ("grad", 64, 64, 5, 33, 16, NS, ["lean v2 2x4 ks1 S", "lean v2 2x4 ks1 dcdf"]),
    ("grad", 640, 480, 5, 3, 2, NM, ["lean v2 2x2 ks1 S", "lean v2 2x2 ks1 dcdf"]),
    ("grad", 640, 480, 9, 5, 1, NM, ["lean v2 4x4 ks1 S", "lean v2 4x4 ks1 dcdf"]),
    # ---- generic scalar kernel: NOMFMA,NOFAST, or R or C = 1 under NOMFMA
    ("conv", 8, 8, 1, 3, 5, NM, ["generic v1 1x4 ks1"]),
    ("conv", 10, 12, 5, 7, 1, NM, ["generic v1 2x1 ks1"]),
    ("conv", 48, 20, 1, 2, 1, NM, ["generic v1 1x1 ks1"]),
    ("conv", 16, 8, 3, 13, 3, NF, ["generic v1 2x2 ks1"]),
    ("conv", 8, 8, 1, 3, 2, NF, ["generic v1 1x2 ks1"]),
    ("conv", 16, 8, 9, 5, 5, NF, ["generic v1 2x4 ks1"]),
    ("conv", 640, 480, 9, 2, 5, NF, ["generic v2 4x4 ks1"]),
    ("conv", 640, 480, 1, 2, 1, NM, ["generic v2 1x1 ks1"]),
    ("conv", 640, 480, 1, 3, 3, NM, ["generic v2 1x2 ks1"]),
    ("conv", 640, 480, 1, 2, 5, NM, ["generic v2 1x4 ks1"]),
    ("conv", 640, 480, 3, 2, 1, NM, ["generic v2 2x1 ks1"]),
    ("conv", 640, 480, 16, 2, 1, NM, ["generic v2 4x1 ks1"]),
    ("conv", 640, 480, 3, 2, 2, NF, ["generic v2 2x2 ks1"]),
    ("conv", 640, 480, 3, 2, 5, NF, ["generic v2 2x4 ks1"]),
    ("conv", 640, 480, 9, 3, 3, NF, ["generic v2 4x2 ks1"]),
    ("grad", 10, 12, 1, 5, 3, NM, ["lean v1 2x4 ks1 S", "generic v1 1x1 ks1"]),
    ("grad", 8, 8, 4, 1, 2, NM, ["generic v1 1x1 ks1", "generic v1 1x1 ks1"]),
    ("grad", 48, 20, 9, 5, 7, NF, ["generic v1 2x4 ks1", "generic v1 2x4 ks1"]),
]


def case_id(c):
    op, Nx, Ny, dM, dD, B, fl, routes = c
    return f"{op}-{Nx}x{Ny}-dM{dM}-dD{dD}-B{B}-{fl or 'default'}-" + "+".join(r.replace(" ", "_") for r in routes)


def test_case_table_reaches_every_selectable_instantiation():
    """CPU: every case's routes are what the restated rules give, and the table covers every matrix-core and lean instantiation that
    aefft_conv / aefft_gradient can select (found by sweeping the rules over grids from 8x8 to 2048x2048 and channel counts 1 .. 128), and
    every (VEC, tile) of the generic kernel"""
    covered = set()
    for c in CASES:
        op, Nx, Ny, dM, dD, B, fl, routes = c
        got = [route_name(r) for r in op_routes(op, Nx, Ny, dM, dD, B, tuple(x for x in fl.split(",") if x))]
        assert got == routes, (case_id(c), got)
        covered.update(got)
    want = {route_name(r) for r in reachable_routes()}
    assert len(want) >= 40                                # (the sweep itself found the families)
    missing = sorted(want - covered)
    assert not missing, missing
    assert not covered - want, sorted(covered - want)


# ------------------------------------------------------------------------------------------
# A. conv, gradient, mse
# ------------------------------------------------------------------------------------------
def _split_dc(a):
    """(AC bins, DC bins) of [..., Nx, Nyr]"""
    a = np.asarray(a)
    ac = np.ones(a.shape, bool)
    ac[..., 0, 0] = False
    return a[ac], a[..., 0, 0].ravel()


def _check_spectrum(route, case, got, ref, peer):
    (ga, gd), (ra, rd), (pa, pd) = _split_dc(got), _split_dc(ref), _split_dc(peer)
    check(route + " AC", case, ga, ra, pa)
    check(route + " DC", case, gd, rd, pd, floors=(DC_FLOOR, DC_FLOOR))


def _seed(c):
    op, Nx, Ny, dM, dD, B, fl, _ = c
    return [Nx, Ny, dM, dD, B, len(fl), len(op)]


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_contraction_route(ctx, flags, case):
    op, Nx, Ny, dM, dD, B, fl, routes = case
    fset = tuple(x for x in fl.split(",") if x)
    assert [route_name(r) for r in op_routes(op, Nx, Ny, dM, dD, B, fset)] == routes
    flags(*fset)
    rng = np.random.default_rng(_seed(case))
    Nyr = Ny // 2 + 1
    cid = f"{Nx}x{Ny} dM{dM} dD{dD} B{B}"
    f32 = np.float32
    X = cnormal(rng, (B, dD, Nx, Nyr))
    Cs = cnormal(rng, (dM, dD, Nx, Nyr))
    b = rng.uniform(-1, 1, dM).astype(f32)
    if op == "conv":
        ref = np.stack([R.conv_k(X[i], Cs, b, Nx, Ny) for i in range(B)])
        peer = np.stack([R.conv_k(X[i], Cs, b, Nx, Ny, dtype=f32) for i in range(B)])
        got = host(ctx.conv(ctx.dev(X), ctx.dev(Cs), ctx.dev(b), Ny))
        _check_spectrum(routes[0], cid, got, ref, peer)
        return
    Fs = cnormal(rng, (dD, dM, Nx, Nyr))
    T = cnormal(rng, (B, dD, Nx, Nyr))
    O = (T + f32(0.3) * cnormal(rng, (B, dD, Nx, Nyr))).astype(np.complex64)

    def mean_grad(dtype):
        acc = None
        for i in range(B):
            g = R.gradient_k_io(X[i], T[i], O[i], Cs, Fs, b, Nx, Ny, dtype=dtype)
            acc = list(g) if acc is None else [a + t for a, t in zip(acc, g)]
        return [a / dtype(B) for a in acc]

    ref, peer = mean_grad(np.float64), mean_grad(f32)
    got = [host(g) for g in ctx.gradient(ctx.dev(X), ctx.dev(T), ctx.dev(O), ctx.dev(Cs), ctx.dev(Fs), ctx.dev(b), Ny)]
    name = f"{routes[0]} > {routes[1]}"
    _check_spectrum(name + " dc", cid, got[0], ref[0], peer[0])
    _check_spectrum(name + " df", cid, got[1], ref[1], peer[1])
    check("bias_grad db", cid, got[2], ref[2], peer[2], floors=(DC_FLOOR, DC_FLOOR))
    check("bias_grad dp", cid, got[3], ref[3], peer[3], floors=(DC_FLOOR, DC_FLOOR))


MSE_GRIDS = [(8, 8, 1, 3, 4), (16, 8, 3, 2, 5), (12, 10, 32, 3, 2), (48, 18, 3, 1, 3), (48, 20, 32, 2, 4), (64, 30, 1, 5, 8),
             (640, 480, 3, 3, 4), (512, 512, 3, 3, 8)]


@gpu
@pytest.mark.parametrize("target", [1e-3, 1.0, 1e4])
@pytest.mark.parametrize("Nx,Ny,B,dD,dM", MSE_GRIDS)
def test_mse_relative(ctx, flags, Nx, Ny, B, dD, dM, target):
    """aefft_mse against np_ref.mse_fft, 1e-5 relative to the MSE itself: non-square grids, Ny/2 + 1 odd (8, 20, 480, 512 -> 5, 11, 241, 257)
    and even (10, 18, 30 -> 6, 10, 16: the interior columns count twice, fft.cu:495), B = 1, 3, 32.  |O - T|^2 has mean 2 s^2 per bin, so
    MSE ~ s^2 / (dM Nx Ny)."""
    flags()
    rng = np.random.default_rng([Nx, Ny, B, dD])
    s = np.float32(np.sqrt(target * dM * Nx * Ny))
    Nyr = Ny // 2 + 1
    T = (np.float32(3) * s * cnormal(rng, (B, dD, Nx, Nyr))).astype(np.complex64)
    O = (T + s * cnormal(rng, (B, dD, Nx, Nyr))).astype(np.complex64)
    ref = np.mean([R.mse_fft(T[i], O[i], dM, dD, Nx, Ny) for i in range(B)])
    assert target / 2 < ref < target * 2
    got = float(host(ctx.mse(ctx.dev(T), ctx.dev(O), dM, Ny))[0])
    print(f"mse {Nx}x{Ny} B{B} dD{dD} target {target:g}: ref {ref:.9e} got {got:.9e} rel {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 1e-5 * ref, (got, ref, abs(got - ref) / ref)


# ------------------------------------------------------------------------------------------
# B. gradient_diff where kernels are close
# ------------------------------------------------------------------------------------------
DEL = 0.02
EPS = [1.0, 1e-1, 1e-2, 1e-3, 3e-4]
SUPPORTS = [(3, 3), (5, 5), (7, 7), (3, 5)]            # 3x5: the stored-distance route (difference form), the control
SHAPES = [(6, 5), (30, 12)]                            # dM x dD = 30 (one partner chunk, one row tile) and 360 (3 chunks x 2 row tiles)
# (family, Nk, Nl, dM, dD, eps or relative distance of the pair, tied)
GD_CASES = [("near", Nk, Nl, dM, dD, eps, tied) for (Nk, Nl) in SUPPORTS for (dM, dD) in SHAPES for eps in EPS for tied in (False, True)
            if (dM, dD) == (6, 5) or not tied or (Nk, Nl) == (5, 5)]
GD_CASES += [("pair", Nk, Nl, 6, 5, rel, False) for (Nk, Nl) in SUPPORTS for rel in (1e-3, 1e-4)]
GD_CASES += [("pair", 5, 5, 30, 12, rel, tied) for rel in (1e-3, 1e-4) for tied in (False, True)]


def gd_id(c):
    fam, Nk, Nl, dM, dD, eps, tied = c
    return f"{fam}-{Nk}x{Nl}-{dM}x{dD}-{eps:g}-{'tied' if tied else 'untied'}"


def gd_inputs(case):
    """float32 weights of one case.  near: every kernel = one base kernel + eps U(-1, 1).  pair: U(-1, 1) kernels, one of them (m1 != m,
    d1 != d) a copy of another + rel U(-1, 1).  tied: f = c^T."""
    fam, Nk, Nl, dM, dD, eps, tied = case
    rng = np.random.default_rng([Nk, Nl, dM, dD, int(round(1e6 * eps)), int(tied), len(fam)])
    f32 = np.float32

    def tensor(n0, n1):
        if fam == "near":
            return (rng.uniform(-1, 1, (Nk, Nl)) + eps * rng.uniform(-1, 1, (n0, n1, Nk, Nl))).astype(f32)
        w = rng.uniform(-1, 1, (n0, n1, Nk, Nl))
        w[n0 - 2, n1 - 1] = w[1, 2] + eps * rng.uniform(-1, 1, (Nk, Nl))
        return w.astype(f32)

    c = tensor(dM, dD)
    f = np.ascontiguousarray(np.transpose(c, (1, 0, 2, 3))) if tied else tensor(dD, dM)
    return c, f, rng.uniform(-1, 1, dM).astype(f32), rng.uniform(-1, 1, dD).astype(f32)


def gd_oracle(c, f, b, p):
    """float64: g_diff, and the weights after the step"""
    c64, f64, b64, p64 = (a.astype(np.float64) for a in (c, f, b, p))
    cd, fd, bd, pd = R.gradient_diff_fast(c64, f64, b64, p64)
    z = [np.zeros_like(a) for a in (c64, f64, b64, p64)]
    new = R.backprop_double(c64, f64, b64, p64, *z, *z, cd, fd, bd, pd, DEL)[:4]
    return (cd, fd, bd, pd), new


def assert_update(name, w0, w1, gd_ref, w_ref):
    """w0: weights before (float32), w1: after (the result under test), gd_ref / w_ref: the oracle's g_diff and weights after, float64.
    g = -10 g_diff.  Taps with |g| > 10 (1 + 1e-3) moved by the clipped step, sign included, to 1e-6 + 1e-4 |step|; taps with
    |g| <= 10 (1 - 1e-3) at weight_step_tol; the taps in between (within 1e-3 of the knee) are left out, at most 1 % of the tensor.  No tap is
    left out for a small |g|.  Everything finite."""
    w0 = w0.astype(np.float64)
    w1 = np.asarray(w1, np.float64)
    assert np.isfinite(w_ref).all(), name + ": the oracle itself is not finite"
    assert np.isfinite(w1).all(), f"{name}: {np.count_nonzero(~np.isfinite(w1))} of {w1.size} weights not finite"
    g = -10.0 * gd_ref
    step = w_ref - w0
    clipped = np.abs(g) > 10.0 * (1 + 1e-3)
    free = np.abs(g) <= 10.0 * (1 - 1e-3)
    left_out = ~(clipped | free)
    assert left_out.mean() <= 0.01, f"{name}: {left_out.mean():.3%} of the taps within 1e-3 of the knee"
    err = np.abs((w1 - w0) - step)
    bad = clipped & (err > 1e-6 + 1e-4 * np.abs(step))
    flips = clipped & (np.sign(w1 - w0) != np.sign(step))
    assert not bad.any(), f"{name}: {np.count_nonzero(bad)} of {np.count_nonzero(clipped)} clipped taps off ({np.count_nonzero(flips)} with the wrong sign), max error {err[clipped].max():.3e}"
    if free.any():
        tol = weight_step_tol(g, del_eff=0.1 * DEL)
        assert (err[free] < tol[free]).all(), f"{name}: unclipped taps off by {err[free].max():.3e}"


def _assert_all(case, got):
    c, f, b, p = gd_inputs(case)
    (cd, fd, bd, pd), (c1, f1, b1, p1) = gd_oracle(c, f, b, p)
    cid = gd_id(case)
    assert_update(cid + " c", c, got[0], cd, c1)
    assert_update(cid + " f", f, got[1], fd, f1)
    assert_update(cid + " b", b, got[2], bd, b1)
    assert_update(cid + " p", p, got[3], pd, p1)
    assert np.abs(np.asarray(got[0], np.float64) - c).max() > 1e-4, "the update was not applied"


def _gpu_update(ctx, c, f, b, p, N=8):
    dM, dD = c.shape[:2]
    zc = np.zeros((dM, dD, N, N // 2 + 1), np.complex64); zf = np.zeros((dD, dM, N, N // 2 + 1), np.complex64)
    t = [ctx.dev(a) for a in (c, f, b, p, zc, zf, zc, zf, np.zeros(dM, np.float32), np.zeros(dD, np.float32),
                              np.zeros_like(c), np.zeros_like(f), np.zeros_like(b), np.zeros_like(p))]
    ctx.update(*t, N, DEL, 1)
    return [host(a) for a in t[:4]]


@gpu
@pytest.mark.parametrize("case", GD_CASES, ids=gd_id)
def test_gradient_diff_close_kernels(ctx, flags, case):
    flags()
    _assert_all(case, _gpu_update(ctx, *gd_inputs(case)))


@pytest.mark.parametrize("case", GD_CASES, ids=gd_id)
def test_gradient_diff_float32_replay_stays_within_the_bound(case):
    """CPU, the peer rule: the oracle's own arithmetic in float32 (the reference's difference form) on exactly the GPU test's inputs passes
    the same assertion, so what the GPU test asks is what the reference achieves"""
    f32 = np.float32
    c, f, b, p = gd_inputs(case)
    cd, fd, bd, pd = R.gradient_diff(c, f, b, p, dtype=f32)
    z = [np.zeros_like(a) for a in (c, f, b, p)]
    got = R.backprop_double(c, f, b, p, *z, *z, cd, fd, bd, pd, DEL, dtype=f32)[:4]
    assert all(a.dtype == f32 for a in got)
    _assert_all(case, got)


@gpu
@pytest.mark.parametrize("Nk,Nl", SUPPORTS)
def test_gradient_diff_coinciding_kernels_give_nan_like_the_reference(ctx, flags, Nk, Nl):
    """two exactly equal kernels (m1 != m, d1 != d): the reference divides 0 by 0 (fft.cu:724-746); the taps of those two kernels are
    NaN after the step, as the oracle's, and every other tap is finite and equals the oracle's"""
    flags()
    rng = np.random.default_rng(Nk * 7 + Nl)
    dM, dD = 6, 5
    c = rng.uniform(-1, 1, (dM, dD, Nk, Nl)).astype(np.float32)
    f = rng.uniform(-1, 1, (dD, dM, Nk, Nl)).astype(np.float32)
    c[4, 4] = c[1, 2]
    b = rng.uniform(-1, 1, dM).astype(np.float32); p = rng.uniform(-1, 1, dD).astype(np.float32)
    (cd, fd, bd, pd), (c1, f1, b1, p1) = gd_oracle(c, f, b, p)
    nan = np.zeros(c.shape, bool); nan[4, 4] = nan[1, 2] = True
    assert np.array_equal(np.isnan(c1), nan)
    got = _gpu_update(ctx, c, f, b, p)
    assert np.array_equal(np.isnan(got[0]), nan)
    assert np.abs(got[0][~nan] - c1[~nan]).max() < 1e-6 + 1e-3 * 0.1 * DEL
    assert np.isfinite(got[1]).all() and np.abs(got[1] - f1).max() < 1e-6 + 1e-3 * 0.1 * DEL
