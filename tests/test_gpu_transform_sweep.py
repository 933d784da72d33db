"""The 2-D R2C / C2R transforms through the C ABI at every size and route they serve, at per-bin float32 precision.

Every FFT-mode result goes through these transforms: the power-of-two Stockham passes, the mixed-radix passes (75 even 5-smooth sizes,
1 to 7 radix passes, T = 16 .. 256 threads per transform), Bluestein's chirp-z form for the other even sizes, and the fused crop / zero-pad
of spectral pooling.  Each axis picks its kernel on its own, so the sweep runs every size as the row axis and as the column axis.

Metric.  The inputs are zero-mean (uniform(-1, 1) signals, complex normal spectra), so that no DC bin sets the scale.  Two quantities are
compared against the float64 reference (oracle/np_ref.py): the relative L2 error ||err|| / ||ref|| and the worst bin max|err| / rms(ref).
Both are bound by what a float32 FFT achieves on the same input -- torch's CPU transforms (pocketfft / MKL), measured per case -- times
PEER_FACTOR (BLU_FACTOR on Bluestein's route), plus a small floor.  A butterfly constant wrong in its 4th digit, or a twiddle or chirp
1e-4 rad off, is ~100x over that at every size it touches; under a DC-dominated max|err| / max|ref| bound, as the older transform tests
use, such errors stay a few times 1e-6 and can pass.  One 8-bit-range frame (mean ~128) per route keeps the frames' input regime, its AC
bins measured apart from the DC bin.

The worst GPU / peer ratio per route is printed at the end of the module (pytest -s)."""
import importlib

import numpy as np
import pytest
import torch

import np_ref as R
from test_gpu_fft_path import host

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

PEER_FACTOR = 4.0
# Bluestein: per axis two float32 transforms of length M >= 2n - 1 and three products with the chirp, where the peer runs one n-point
# transform -- measured 3-4.6x the peer with the chirp tables exact to float32 rounding (the chirp evaluated in float on the device was
# 4.4-7x); a chirp or filter wrong by 1e-4 rad is ~100x over
BLU_FACTOR = 6.0
FLOOR_L2 = 3e-8           # floors: for the smallest sizes, where the peer's own error is ~6e-8 / ~2e-7
FLOOR_MAX = 2e-7
DC_FLOOR = 1e-6

SMOOTH = [10, 12, 18, 20, 24, 30, 36, 40, 48, 50, 54, 60, 72, 80, 90, 96, 100, 108, 120, 144, 150, 160, 162, 180, 192, 200, 216, 240, 250, 270,
          288, 300, 320, 324, 360, 384, 400, 432, 450, 480, 486, 500, 540, 576, 600, 640, 648, 720, 750, 768, 800, 810, 864, 900, 960, 972, 1000,
          1080, 1152, 1200, 1250, 1280, 1296, 1350, 1440, 1458, 1500, 1536, 1600, 1620, 1728, 1800, 1920, 1944, 2000]
POW2 = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
# even sizes with a prime factor above 5, on both sides of each edge of the Bluestein length M = 2^q >= 2n - 1 (16 .. 2048)
BLUESTEIN = [14, 22, 34, 62, 66, 126, 130, 254, 258, 510, 514, 1018, 1022]

WORST = {}      # route -> [worst ratio to the peer, case, GPU l2, GPU max/rms]


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nworst GPU error per route (ratio to the float32 peer; GPU relative L2; GPU max|err|/rms(ref)):")
        for k in sorted(WORST):
            r, case, l2, mx = WORST[k]
            print(f"  {k:42s} {r:6.2f}  {l2:.2e}  {mx:.2e}  {case}")


# ------------------------------------------------------------------------------------------
# metric
# ------------------------------------------------------------------------------------------
def metrics(got, ref):
    d = np.abs(np.asarray(got, np.complex128 if np.iscomplexobj(got) else np.float64) - ref)
    nref = np.sqrt(np.sum(np.abs(ref) ** 2))
    rms = nref / np.sqrt(ref.size)
    return np.sqrt(np.sum(d ** 2)) / nref, d.max() / rms


def check(route, case, got, ref, peer, factor=PEER_FACTOR, floors=(FLOOR_L2, FLOOR_MAX)):
    """got, peer: float32 results of the same input; ref: the float64 reference.  Records the ratio, then asserts both bounds."""
    g2, gm = metrics(got, ref)
    p2, pm = metrics(peer, ref)
    if p2 > 0 and pm > 0:
        ratio = max(g2 / p2, gm / pm)
        w = WORST.get(route)
        if w is None or ratio > w[0]:
            WORST[route] = [ratio, case, g2, gm]
    assert g2 <= factor * p2 + floors[0] and gm <= factor * pm + floors[1], \
        f"{route} {case}: relative L2 {g2:.3e} (peer {p2:.3e}), max/rms {gm:.3e} (peer {pm:.3e})"


def peer_r2c(x):
    return torch.fft.rfft2(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def peer_c2r(Z, Nx, Ny, unnorm):
    """float32 C2R of the complex64 spectrum Z: unnormalised (scale 1) or times 1/(Nx Ny)"""
    z = torch.from_numpy(np.ascontiguousarray(Z, np.complex64))
    return torch.fft.irfft2(z, s=(Nx, Ny), norm="forward" if unnorm else "backward").numpy()


def c64(a):
    return np.asarray(a).astype(np.complex64)


def cnormal(rng, shape):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


def transforms(ctx, route, Nx, Ny, planes, seed, factor=PEER_FACTOR, c2r_checks=True):
    """R2C of a zero-mean frame; C2R of its spectrum (default scale and scale = 1); C2R of a spectrum with AC-level noise on every bin,
    the self-conjugate ones included (their imaginary parts are to be ignored, pocketfft semantics)."""
    rng = np.random.default_rng(seed)
    case = f"{Nx}x{Ny}x{planes}"
    x = rng.uniform(-1, 1, (planes, Nx, Ny)).astype(np.float32)
    ref = R.fft(x)
    check(route + " r2c", case, host(ctx.r2c(ctx.dev(x))), ref, peer_r2c(x), factor)
    if not c2r_checks:
        return
    Z = c64(ref)
    Zd = ctx.dev(Z)
    check(route + " c2r", case, host(ctx.c2r(Zd, Ny)), R.fft_inv(Z, Nx, Ny), peer_c2r(Z, Nx, Ny, False), factor)
    check(route + " c2r scale=1", case, host(ctx.c2r(Zd, Ny, scale=1.0)), R.c2r_unnorm(Z, Nx, Ny), peer_c2r(Z, Nx, Ny, True), factor)
    W = cnormal(rng, Z.shape)
    check(route + " c2r non-Hermitian", case, host(ctx.c2r(ctx.dev(W), Ny, scale=1.0)), R.c2r_unnorm(W, Nx, Ny), peer_c2r(W, Nx, Ny, True),
          factor)


def frames_8bit(ctx, route, Nx, Ny, planes, seed, factor=PEER_FACTOR):
    """The frames' regime (pixels in [0, 256), DC ~950x the AC rms): the AC bins and the DC bin measured apart; the C2R output measured
    against the rms of the image's AC part."""
    rng = np.random.default_rng(seed)
    case = f"{Nx}x{Ny}x{planes} 8-bit"
    x = np.floor(rng.uniform(0, 256, (planes, Nx, Ny))).astype(np.float32)
    ref = R.fft(x)
    got, peer = host(ctx.r2c(ctx.dev(x))), peer_r2c(x)
    ac = np.ones(ref.shape, bool)
    ac[:, 0, 0] = False
    check(route + " r2c 8-bit AC", case, got[ac], ref[ac], peer[ac], factor)
    # the DC bin alone: a sum of Nx Ny pixels, which the peer may get exactly -- float32 relative accuracy as the floor
    check(route + " r2c 8-bit DC", case, got[:, 0, 0], ref[:, 0, 0], peer[:, 0, 0], factor, floors=(DC_FLOOR, DC_FLOOR))
    Z = c64(ref)
    yref = R.fft_inv(Z, Nx, Ny)
    mean = yref.mean(axis=(-2, -1), keepdims=True)
    check(route + " c2r 8-bit", case, host(ctx.c2r(ctx.dev(Z), Ny)) - mean, yref - mean, peer_c2r(Z, Nx, Ny, False) - mean, factor)


# ------------------------------------------------------------------------------------------
# 1. every smooth size on each axis (mixed-radix passes; the other axis' kernel as the dispatch picks it)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMOOTH)
def test_smooth_size_as_row_axis(ctx, flags, n):
    """8 x n, 3 planes: n-point mixed-radix rows, 12 row pairs of a 16-pair workgroup at T = 16 (partly filled); the 8-point columns on
    the power-of-two passes when Wc = n/2 is a multiple of 16, on the mixed-radix passes at a power-of-two n otherwise (odd Wc included)"""
    flags()
    transforms(ctx, "smooth rows (8 x n)", 8, n, 3, n)


@pytest.mark.parametrize("n", SMOOTH)
def test_smooth_size_as_column_axis(ctx, flags, n):
    """n x 36, 3 planes: n-point mixed-radix columns over Wc = 18 packed columns -- narrow last tiles at every T (mix_cw 16, 8, 4, 2)"""
    flags()
    transforms(ctx, "smooth cols (n x 36)", n, 36, 3, 1000 + n)


# ------------------------------------------------------------------------------------------
# 2. every power of two on each axis (Stockham passes)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", POW2)
def test_power_of_two_as_row_axis(ctx, flags, n):
    flags()
    transforms(ctx, "pow2 rows (8 x n)", 8, n, 3, 2000 + n)


@pytest.mark.parametrize("n", POW2)
def test_power_of_two_as_column_axis(ctx, flags, n):
    flags()
    transforms(ctx, "pow2 cols (n x 8)", n, 8, 3, 3000 + n)


@pytest.mark.parametrize("Nx,Ny", [(64, 64), (256, 128), (512, 512), (2048, 256)])
def test_power_of_two_grids(ctx, flags, Nx, Ny):
    flags()
    transforms(ctx, "pow2 grids", Nx, Ny, 3, Nx + Ny)


# ------------------------------------------------------------------------------------------
# 3. the mixed-radix kernels at a power-of-two n (packed width Wc neither a power of two nor a multiple of 16)
# ------------------------------------------------------------------------------------------
def test_mixed_columns_at_a_power_of_two(ctx, flags):
    """512 x 600: Wc = 300, so the 512-point columns take the mixed-radix pass"""
    flags()
    transforms(ctx, "mixed kernels at pow2 n", 512, 600, 3, 512600)


def test_mixed_rows_at_a_power_of_two_odd_width(ctx, flags):
    """480 x 512 pooled by 3 (160 x 170): the 512-point rows on the mixed-radix pass with an odd Wc = 85"""
    flags()
    rng = np.random.default_rng(4805)
    x = rng.uniform(-1, 1, (3, 480, 512)).astype(np.float32)
    ref, nx, ny = R.pool_fft(R.fft(x), 480, 512, 3)
    assert (nx, ny) == (160, 170)
    peer, _, _ = R.pool_fft(peer_r2c(x), 480, 512, 3)
    check("mixed kernels at pow2 n r2c", "480x512/3", host(ctx.r2c_pool(ctx.dev(x), 3)), ref, peer)


def test_mixed_kernels_packed_width_below_4(ctx, flags):
    """unpool 6 x 2 by 4 -> 24 x 8: Wc = 1 -- the 8-point rows on the mixed-radix pass -- and 1-column tiles of the 24-point columns"""
    flags()
    rng = np.random.default_rng(628)
    Xs = cnormal(rng, (3, 6, 2))
    up, Nx, Ny = R.pool_fft(Xs.astype(np.complex128), 6, 2, -4)
    assert (Nx, Ny) == (24, 8)
    peer = peer_c2r(R.resize(Xs, 6, 2, 24, 8), 24, 8, True)
    check("mixed kernels at pow2 n c2r", "6x2 up 4", host(ctx.unpool_c2r(ctx.dev(Xs), 2, -4, 1.0)), R.c2r_unnorm(up, 24, 8), peer)


# ------------------------------------------------------------------------------------------
# 4. Bluestein
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BLUESTEIN)
def test_bluestein_sizes(ctx, flags, n):
    """n on each axis against 8 (which then takes Bluestein too)"""
    flags()
    transforms(ctx, "bluestein", 8, n, 3, 4000 + n, BLU_FACTOR)
    transforms(ctx, "bluestein", n, 8, 3, 5000 + n, BLU_FACTOR)


@pytest.mark.parametrize("Nx,Ny", [(12, 480), (640, 10), (1000, 24), (96, 64)])
def test_smooth_sizes_under_chirpz(ctx, flags, Nx, Ny):
    flags("CHIRPZ")
    transforms(ctx, "bluestein (CHIRPZ)", Nx, Ny, 3, Nx * 7 + Ny, BLU_FACTOR)


# ------------------------------------------------------------------------------------------
# 5. the 8-bit frame regime, one case per route
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,Nx,Ny,flag,factor", [("pow2", 256, 512, None, PEER_FACTOR), ("smooth", 480, 640, None, PEER_FACTOR),
                                                     ("mixed at pow2 n", 512, 600, None, PEER_FACTOR),
                                                     ("bluestein", 126, 254, None, BLU_FACTOR), ("bluestein (CHIRPZ)", 480, 640, "CHIRPZ", BLU_FACTOR)])
def test_8bit_frames_per_route(ctx, flags, route, Nx, Ny, flag, factor):
    flags(flag)
    frames_8bit(ctx, route, Nx, Ny, 2, Nx + 3 * Ny, factor)


# ------------------------------------------------------------------------------------------
# 6. crop and zero-pad (spectral pooling fused into the transforms, or Bluestein + resize)
# ------------------------------------------------------------------------------------------
def _servable(Nx, Ny):
    pow2 = lambda n: n in POW2
    smooth = lambda n: n in SMOOTH
    if (pow2(Nx) or smooth(Nx)) and (pow2(Ny) or smooth(Ny)):
        return True
    return Nx % 2 == 0 and Ny % 2 == 0 and 8 <= min(Nx, Ny) and max(Nx, Ny) <= 1024


def _route(Nx, Ny, nx, ny):
    if Nx in POW2 and Ny in POW2:
        return "crop/pad pow2" if nx in POW2 and ny in POW2 else "crop/pad bluestein + resize"
    if (Nx in SMOOTH or Ny in SMOOTH) and all(n in POW2 or n in SMOOTH for n in (Nx, Ny)):
        return "crop/pad mixed"
    return "crop/pad bluestein + resize"


POOL_GRIDS = [(128, 128), (256, 512), (1024, 64), (480, 640), (240, 320), (640, 512), (512, 480), (120, 40), (96, 96)]
POOL_CASES = []
for _Nx, _Ny in POOL_GRIDS:
    for _s in range(2, 7):
        _nx, _ny = R.pooled_size(_Nx, _Ny, _s)
        if _nx % 2 or _ny % 2 or min(_nx, _ny) < 8 or not _servable(_Nx, _Ny):
            continue
        if _route(_Nx, _Ny, _nx, _ny).startswith("crop/pad bluestein") and max(_Nx, _Ny) > 1024:
            continue
        POOL_CASES.append((_Nx, _Ny, _s))


@pytest.mark.parametrize("Nx,Ny,s", POOL_CASES)
def test_r2c_pool(ctx, flags, Nx, Ny, s):
    flags()
    rng = np.random.default_rng(Nx * 11 + Ny * 3 + s)
    x = rng.uniform(-1, 1, (3, Nx, Ny)).astype(np.float32)
    ref, nx, ny = R.pool_fft(R.fft(x), Nx, Ny, s)
    peer, _, _ = R.pool_fft(peer_r2c(x), Nx, Ny, s)
    got = host(ctx.r2c_pool(ctx.dev(x), s))
    assert got.shape == ref.shape
    route = _route(Nx, Ny, nx, ny)
    check(route + " r2c_pool", f"{Nx}x{Ny}/{s}", got, ref, peer, BLU_FACTOR if "bluestein" in route else PEER_FACTOR)


UNPOOL_CASES = []
for _Nx, _Ny, _s in POOL_CASES + [(128, 128, 8), (256, 512, 8), (512, 256, 16)]:
    _nx, _ny = R.pooled_size(_Nx, _Ny, _s)
    _ux, _uy = R.pooled_size(_nx, _ny, -_s)
    if (_ux, _uy) == (_nx * _s, _ny * _s) and _ux % 2 == 0 and _uy % 2 == 0 and _servable(_ux, _uy):
        UNPOOL_CASES.append((_nx, _ny, _s))


@pytest.mark.parametrize("nx,ny,s", UNPOOL_CASES)
def test_unpool_c2r(ctx, flags, nx, ny, s):
    """the zero-pad of a (non-Hermitian) pooled spectrum fused into the C2R; scales 8 and 16 reach the sparse first pass of the
    power-of-two rows (Wc <= N/16)"""
    flags()
    rng = np.random.default_rng(nx * 13 + ny * 5 + s)
    Xs = cnormal(rng, (3, nx, ny // 2 + 1))
    up, Nx, Ny = R.pool_fft(Xs.astype(np.complex128), nx, ny, -s)
    peer = peer_c2r(R.resize(Xs, nx, ny, Nx, Ny), Nx, Ny, True)
    got = host(ctx.unpool_c2r(ctx.dev(Xs), ny, -s, 1.0))
    route = _route(Nx, Ny, nx, ny)
    check(route + " unpool_c2r", f"{nx}x{ny}*{s}", got, R.c2r_unnorm(up, Nx, Ny), peer, BLU_FACTOR if "bluestein" in route else PEER_FACTOR)


def _remap_served(Nx, Ny, s):
    nx, ny = R.pooled_size(Nx, Ny, s)
    return nx % 2 == 0 and ny % 2 == 0 and min(nx, ny) >= 8 and max(nx, ny) <= 2048 and (s > 0 or (nx, ny) == (Nx * -s, Ny * -s))


@pytest.mark.parametrize("Nx,Ny,s", [(g[0], g[1], s) for g in POOL_GRIDS + [(1280, 720), (2000, 16)] for s in (2, 3, 4, 5, 6, -2, -3)
                                     if _remap_served(g[0], g[1], s)])
def test_pool_remap_bit_for_bit(ctx, Nx, Ny, s):
    """aefft_pool (only the index remap) against np_ref.resize, bit for bit, wherever the pooled size is even and in range"""
    nx, ny = R.pooled_size(Nx, Ny, s)
    rng = np.random.default_rng(Nx + Ny + s)
    X = cnormal(rng, (2, Nx, Ny // 2 + 1))
    down, _, _ = R.pool_fft(X, Nx, Ny, s)
    Xd, gx, gy = ctx.pool(ctx.dev(X), Ny, s)
    assert (gx, gy) == (nx, ny) and np.array_equal(host(Xd), down)


def test_pool_of_a_power_of_two_grid_above_1024_to_another_size_is_refused(ctx):
    """r2c_pool of 2048^2 by 3 (682^2): neither the power-of-two passes (a crop that is not a power of two) nor Bluestein (<= 1024)
    serve it -- AEFFT_EINVAL naming the rule, not a HIP error"""
    x = ctx.dev(np.zeros((1, 2048, 2048), np.float32))
    with pytest.raises(aefft.AefftError, match=r"aefft error 1: .*1024"):
        ctx.r2c_pool(x, 3)
    ctx.sync()


# ------------------------------------------------------------------------------------------
# 7. more planes than a grid dimension's 65535
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,Nx,Ny,factor", [("pow2", 8, 8, PEER_FACTOR), ("smooth", 10, 12, PEER_FACTOR), ("bluestein", 14, 14, BLU_FACTOR)])
def test_more_than_65535_planes(ctx, flags, route, Nx, Ny, factor):
    flags()
    planes = 70001
    rng = np.random.default_rng(planes + Nx)
    x = rng.uniform(-1, 1, (planes, Nx, Ny)).astype(np.float32)
    ref = R.fft(x)
    case = f"{Nx}x{Ny}x{planes}"
    check(f"{route} >65535 planes r2c", case, host(ctx.r2c(ctx.dev(x))), ref, peer_r2c(x), factor)
    Z = c64(ref)
    check(f"{route} >65535 planes c2r", case, host(ctx.c2r(ctx.dev(Z), Ny)), R.fft_inv(Z, Nx, Ny), peer_c2r(Z, Nx, Ny, False), factor)
