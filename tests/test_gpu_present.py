"""aefft_frames_resize_to_image (Context.frames_resize_to_image) and aefft_map_overlay_image (Context.map_overlay): the way out of the net.
Call 1 against the integer formulas of include/aefft.h (the numpy `oracle` of test_gpu_resize.py with the roles swapped) -- EXACT equality for
8-bit and float frames, both modes, every shape with a tight, a 64-aligned and an unaligned pitch (the last from a base off by one byte), the
image allocation pre-filled with random bytes that must come back unchanged outside the live pixels; px_u8's special values; a region of
interest; the same-size and constant-frame consequences; the composition identity on the device; a net's reconstruction carried back to the
camera's size.  Call 2 against a numpy restatement written here, float32 operations one at a time; a map from Net.score_map.  One graph capture
and replay of each call, every AEFFT_EINVAL rule, and the profile entries."""
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_fft_path import host
from test_gpu_resize import _linear_axis, oracle
from test_gpu_sizes import _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (B, D, Nx, Ny, W, H): identity; enlarging to an odd destination with W D no dword multiple (edge clamps); reducing to odd; exact 2x (AREA = the
# rounded block mean); several tiles with remainders, Ny % 4 == 2 (the element route on the frame side); ratios 20 and 12.5 (bands); the workload's
# own direction; 255 Nx Ny >= 2^32 (AREA only: the 64-bit sum); an x-reduction of 128 whose tiles need more source columns than a band holds, so
# that the sums run across bands (fr_geometry: to 16 x 4 AREA needs 512 columns with XB = 322, LINEAR needs 386 and XB is 386 -- one band --; to
# 16 x 8 LINEAR needs 386 with XB = 322 too)
SHAPES = [(1, 1, 8, 8, 8, 8), (2, 3, 8, 8, 11, 9), (1, 3, 16, 8, 7, 5), (2, 4, 64, 64, 32, 32), (1, 3, 66, 34, 130, 70), (1, 2, 200, 150, 10, 12),
          (2, 3, 256, 256, 640, 480), (1, 1, 8192, 2064, 8, 6), (1, 3, 2048, 64, 16, 4), (1, 3, 2048, 64, 16, 8)]
BIG = (1, 1, 8192, 2064, 8, 6)
PITCHES = ["tight", "pad64", "odd"]
MODES = ["linear", "area"]
CASES = [(s, m) for s in SHAPES for m in MODES if (m == "linear" and s != BIG) or (m == "area" and s[4] <= s[2] and s[5] <= s[3])]
TAIL = 96          # bytes of the allocation behind the last image row: the guard region
_id = lambda v: v if isinstance(v, str) else "x".join(map(str, v))


# ------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------
def px_u8(v):
    """SpinToImage_C's rule on float32 values: NaN -> 0, clamp to 0..255, halves away from zero; floor(t + 0.5) in float64 is exact for |t| < 2^24"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = np.minimum(np.floor(v.astype(np.float64) + 0.5), 255.0)
        return np.where(v > 0, r, 0.0).astype(np.uint8)


def expected_image(px_frames, size, mode):
    """px_frames uint8 [B][D][Nx][Ny] -> the image [B][H][W][D]: the oracle on the frames' pixels in image order, its frames transposed back"""
    src = np.ascontiguousarray(px_frames.transpose(0, 3, 2, 1))                  # p[b][y][x][d] = frames[b][d][x][y]
    return np.ascontiguousarray(oracle(src, size, mode)[0].transpose(0, 3, 2, 1))


@functools.lru_cache(maxsize=None)
def _frames(shape):
    """(8-bit frames, float frames with the same pixels: +-0.25 around them)"""
    B, D, Nx, Ny = shape[:4]
    rng = np.random.default_rng(sum(shape))
    f8 = rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8)
    f32 = f8.astype(np.float32) + np.where(rng.integers(0, 2, f8.shape) == 1, np.float32(0.25), np.float32(-0.25))
    assert np.array_equal(px_u8(f32), f8)
    f8.setflags(write=False); f32.setflags(write=False)
    return f8, f32


@functools.lru_cache(maxsize=None)
def _want(shape, mode):
    """computed once per (shape, mode), shared by the pitches and the frame types, and left unchanged"""
    w = expected_image(_frames(shape)[0], shape[4:], mode)
    w.setflags(write=False)
    return w


def overlay_ref(m, img, lut, lo, hi, alpha, smooth):
    """the definition of include/aefft.h, step by step: m float32 [B][Mx][My], img uint8 [B][H][W][D], lut uint8 [256][D]"""
    B, H, W, D = img.shape
    Mx, My = m.shape[1:]
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        inv = np.float32(255.0) / np.float32(hi - lo)                                # 1.
        t = (m.astype(np.float32) - lo).astype(np.float32)                           # 2. the subtraction, rounded ...
        k0 = px_u8((t * inv).astype(np.float32)).astype(np.int64)                    # ... the product, rounded; px_u8
    if not smooth:                                                                   # 3.
        xi, yj = np.arange(W, dtype=np.int64) * Mx // W, np.arange(H, dtype=np.int64) * My // H
        k = k0[:, xi][:, :, yj].transpose(0, 2, 1)                                   # [B][H][W]
    else:                                                                            # 4.
        x0, x1, wx = _linear_axis(Mx, W)
        y0, y1, wy = _linear_axis(My, H)
        wx, wy = wx[None, :, None], wy[None, None, :]
        top = (2048 - wx) * k0[:, x0][:, :, y0] + wx * k0[:, x1][:, :, y0]           # [B][W][H]
        bot = (2048 - wx) * k0[:, x0][:, :, y1] + wx * k0[:, x1][:, :, y1]
        k = (((2048 - wy) * top + wy * bot + 2 ** 21) >> 22).transpose(0, 2, 1)
    assert k.min() >= 0 and k.max() <= 255
    col = lut.astype(np.int64)[k]                                                    # [B][H][W][D]
    return ((alpha * col + (256 - alpha) * img.astype(np.int64) + 128) >> 8).astype(np.uint8), k


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")          # (a copy: cached arrays stay read-only)


def _layout(B, D, W, H, kind):
    """(pitch, offset of the first image in its allocation, bytes of the allocation: the images and TAIL bytes behind them)"""
    pitch = {"tight": W * D, "pad64": (W * D + 63) // 64 * 64, "odd": W * D + 5}[kind]
    off = 1 if kind == "odd" else 0
    return pitch, off, off + B * H * pitch + TAIL


def _alloc(B, D, W, H, kind, ctx, seed, content=None):
    """an allocation of random bytes (pad bytes, tail and guard included), optionally with `content` [B][H][W][D] in its live bytes:
    (host copy, host view of the live bytes, the device allocation, the device view [B][H][W][D])"""
    pitch, off, n = _layout(B, D, W, H, kind)
    flat = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    live = np.lib.stride_tricks.as_strided(flat[off:], (B, H, W, D), (H * pitch, pitch, D, 1))
    if content is not None:
        live[...] = content
    d = _dev(flat, ctx)
    return flat, live, d, torch.as_strided(d, (B, H, W, D), (H * pitch, pitch, D, 1), off)


def _check_whole_allocation(flat, live, d, want, tag):
    """the live bytes are `want`; every pad byte, the tail and the guard behind it are as they were"""
    got = host(d)
    live[...] = want
    print(tag, "bytes that differ:", int((got != flat).sum()))
    assert np.array_equal(got, flat), tag


# ------------------------------------------------------------------------------------------
# 1. call 1 against the integer formulas: every shape, pitch, mode and frame type
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("shape,mode", CASES, ids=_id)
def test_frames_resize_equals_the_integer_formulas(ctx, shape, mode, kind):
    B, D, Nx, Ny, W, H = shape
    want = _want(shape, mode)
    for which, frames in zip(("8-bit", "float"), _frames(shape)):
        flat, live, d, view = _alloc(B, D, W, H, kind, ctx, seed=len(kind) + len(mode) + len(which))
        assert ctx.frames_resize_to_image(_dev(frames, ctx), (W, H), mode, out=view) is view
        ctx.sync()
        _check_whole_allocation(flat, live, d, want, (shape, mode, kind, which))


def test_fresh_output_and_area_at_an_integer_ratio_is_the_rounded_block_mean(ctx):
    shape = (2, 4, 64, 64, 32, 32)
    B, D, Nx, Ny, W, H = shape
    f8 = _frames(shape)[0]
    blocks = f8.astype(np.int64).reshape(B, D, W, 2, H, 2).sum(axis=(3, 5))                          # [B][D][W][H]
    want = np.ascontiguousarray(((2 * blocks + 4) // 8).transpose(0, 3, 2, 1)).astype(np.uint8)     # floor(mean + 1/2)
    got = ctx.frames_resize_to_image(_dev(f8, ctx), (W, H), "area")
    ctx.sync()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, D) and got.is_contiguous() and np.array_equal(host(got), want)
    assert np.array_equal(want, _want(shape, "area"))


# ------------------------------------------------------------------------------------------
# 2. float frames: px_u8's special values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", [((2, 3, 16, 12, 37, 29), "linear"), ((2, 3, 66, 34, 20, 11), "linear"), ((2, 3, 66, 34, 20, 11), "area")], ids=_id)
def test_float_frames_are_turned_into_pixels_first(ctx, shape, mode):
    B, D, Nx, Ny, W, H = shape
    rng = np.random.default_rng(11)
    f = rng.uniform(-40, 300, (B, D, Nx, Ny)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 300.0, 0.5, 1.5, 254.5, 255.5, 2.5, 0.49999997, -0.5, 255.0, 0.0], dtype=np.float32)
    f.reshape(-1)[rng.choice(f.size, 20 * special.size, replace=False)] = np.tile(special, 20)
    p = px_u8(f)
    assert set(np.unique(px_u8(special))) == {0, 1, 2, 3, 255}
    a = ctx.frames_resize_to_image(_dev(f, ctx), (W, H), mode)
    b = ctx.frames_resize_to_image(_dev(p, ctx), (W, H), mode)
    ctx.sync()
    assert np.array_equal(host(a), expected_image(p, (W, H), mode)) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# 3. a region of interest of a larger batch as destination
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 3, 66, 34, 50, 30), (2, 4, 64, 64, 32, 32)], ids=_id)
def test_region_of_interest_of_a_larger_batch(ctx, shape, mode):
    """big[:, 3:3+H, 5:5+W]: the parent's pitch, and a batch stride that is not H * pitch; everything outside the region stays"""
    B, D, Nx, Ny, W, H = shape
    rng = np.random.default_rng(5)
    f8 = rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8)
    want = expected_image(f8, (W, H), mode)
    for frames in (f8, f8.astype(np.float32)):
        big_h = rng.integers(0, 256, (B, H + 11, W + 9, D), dtype=np.uint8)
        big = _dev(big_h, ctx)
        roi = big[:, 3:3 + H, 5:5 + W]
        assert roi.stride(0) != H * roi.stride(1) and not roi.is_contiguous()
        assert ctx.frames_resize_to_image(_dev(frames, ctx), (W, H), mode, out=roi) is roi
        ctx.sync()
        big_h[:, 3:3 + H, 5:5 + W] = want
        assert np.array_equal(host(big), big_h), (shape, mode, frames.dtype)


# ------------------------------------------------------------------------------------------
# 4. consequences of the definition
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 3, 11, 9), (2, 4, 64, 64), (1, 3, 130, 70)], ids=_id)
def test_same_size_is_frames_to_image(ctx, shape, mode):
    B, D, Nx, Ny = shape
    rng = np.random.default_rng(Nx + Ny)
    for frames in (rng.integers(0, 256, shape, dtype=np.uint8), rng.uniform(-20, 280, shape).astype(np.float32)):
        f = _dev(frames, ctx)
        a = ctx.frames_resize_to_image(f, (Nx, Ny), mode)
        b = ctx.frames_to_image(f)
        ctx.sync()
        assert tuple(a.shape) == tuple(b.shape) == (B, Ny, Nx, D) and torch.equal(a, b), (shape, mode, frames.dtype)


@pytest.mark.parametrize("mode", MODES)
def test_a_constant_frame_stays_constant(ctx, mode):
    for value, (Nx, Ny, W, H) in ((0, (16, 12, 37, 29)), (77, (66, 34, 130, 70)), (255, (16, 8, 41, 23)), (0, (37, 29, 16, 12)), (77, (130, 70, 66, 34)), (255, (200, 150, 10, 12))):
        if mode == "area" and (W > Nx or H > Ny):
            continue
        for dtype in (torch.uint8, torch.float32):
            f = torch.full((2, 3, Nx, Ny), value, dtype=dtype, device=f"cuda:{ctx.device}")
            a = ctx.frames_resize_to_image(f, (W, H), mode)
            ctx.sync()
            assert (host(a) == value).all(), (mode, value, Nx, Ny, W, H, dtype)


# ------------------------------------------------------------------------------------------
# 5. the composition identity, on the device
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", [(s, m) for s in [(2, 3, 8, 8, 11, 9), (1, 3, 66, 34, 130, 70), (1, 2, 200, 150, 10, 12), (2, 4, 64, 64, 32, 32)]
                                        for m in MODES if m == "linear" or (s[4] <= s[2] and s[5] <= s[3])], ids=_id)
def test_the_call_is_the_composition_of_three_existing_calls(ctx, shape, mode):
    """frames_to_image(F) -> image_resize_to_frames(.., (W, H), mode, 8-bit) -> frames_to_image, bit for bit"""
    B, D, Nx, Ny, W, H = shape
    rng = np.random.default_rng(W)
    for frames in (rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8), rng.uniform(-20, 280, (B, D, Nx, Ny)).astype(np.float32)):
        f = _dev(frames, ctx)
        one = ctx.frames_resize_to_image(f, (W, H), mode)
        three = ctx.frames_to_image(ctx.image_resize_to_frames(ctx.frames_to_image(f), (W, H), mode, dtype=torch.uint8))
        ctx.sync()
        assert torch.equal(one, three), (shape, mode, frames.dtype)


# ------------------------------------------------------------------------------------------
# 6., 8. end to end on a small net: camera image -> frames -> net -> camera-sized image, and its score map onto the camera image
# ------------------------------------------------------------------------------------------
def _small_net(ctx, D, N, B):
    net = aefft.Net(ctx, D, N, N, [2], 3, 1, batch=B)
    for l, w in enumerate(_weights(np.random.default_rng(3), D, [2], 3, 3)):
        net.set_pair(l, *[0.25 * a for a in w])
    return net


def test_a_reconstruction_goes_back_to_the_camera_size(ctx):
    D, N, B, W, H = 3, 16, 2, 37, 29
    cam = _dev(np.random.default_rng(8).integers(0, 256, (B, H, W, D), dtype=np.uint8), ctx)
    net = _small_net(ctx, D, N, B)
    try:
        frames = ctx.image_resize_to_frames(cam, (N, N), "linear")
        recon = ctx.empty(B, D, N, N, dtype=torch.uint8)
        net.infer(frames, recon)
        back = ctx.frames_resize_to_image(recon, (W, H), "linear")               # (queued behind the net: nothing waits in between)
        ctx.sync()
        r = host(recon)
        assert len(np.unique(r)) > 2
        assert np.array_equal(host(back), expected_image(r, (W, H), "linear"))
    finally:
        net.close()


@pytest.mark.parametrize("smooth", [False, True])
def test_a_score_map_of_the_library_goes_onto_the_camera_image(ctx, smooth):
    D, N, B, W, H = 3, 16, 2, 37, 29
    cam_h = np.random.default_rng(9).integers(0, 256, (B, H, W, D), dtype=np.uint8)
    cam = _dev(cam_h, ctx)
    lut_h = aefft.heat_lut(D)
    net = _small_net(ctx, D, N, B)
    try:
        frames = ctx.image_resize_to_frames(cam, (N, N), "linear")
        m, _, _ = net.score_map(frames, 8)
        ctx.sync()
        m_h = host(m).copy()
        assert m_h.shape == (B, 2, 2) and np.isfinite(m_h).all() and m_h.max() > m_h.min()
        lo, hi = float(m_h.min()), float(m_h.max())
        assert ctx.map_overlay(m, cam, _dev(lut_h, ctx), lo, hi, alpha=160, smooth=smooth) is cam
        ctx.sync()
        want, k = overlay_ref(m_h, cam_h, lut_h, lo, hi, 160, smooth)
        assert k.min() == 0 and k.max() == 255
        assert np.array_equal(host(cam), want)
    finally:
        net.close()


# ------------------------------------------------------------------------------------------
# 7. call 2 against the numpy restatement
# ------------------------------------------------------------------------------------------
MAPS = [(1, 1, 1, 1, 8, 8), (2, 3, 4, 4, 11, 9), (1, 3, 8, 6, 130, 70), (2, 4, 32, 32, 64, 64), (1, 3, 32, 32, 640, 480)]     # (B, D, Mx, My, W, H)
SCALES = [(0.0, 510.0), (510.0, 0.0), (0.25, 7.5)]      # inv = +-1/2 exactly: odd entries fall on rounding halves; an inexact inv
ALPHAS = [0, 1, 128, 255, 256]


@functools.lru_cache(maxsize=None)
def _map(shape, lo, hi):
    B, D, Mx, My, W, H = shape
    rng = np.random.default_rng(Mx + W)
    span = hi - lo
    m = (lo + span * rng.uniform(-0.15, 1.15, (B, Mx, My))).astype(np.float32)           # below lo and above hi included
    flat = m.reshape(-1)
    if abs(span) == 510.0:
        flat[::3] = 2 * rng.integers(-3, 260, flat[::3].size) + 1                       # exactly on rounding halves
    if flat.size >= 16:
        flat[[1, 5, 7, 10, 11]] = [np.nan, np.inf, -np.inf, lo, hi]
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("lo,hi", SCALES, ids=["up", "down", "inexact"])
@pytest.mark.parametrize("smooth", [False, True], ids=["tile", "smooth"])
@pytest.mark.parametrize("shape", MAPS, ids=_id)
def test_map_overlay_equals_the_restatement(ctx, shape, smooth, lo, hi, kind):
    B, D, Mx, My, W, H = shape
    m_h = _map(shape, lo, hi)
    rng = np.random.default_rng(W + D)
    lut_h = rng.integers(0, 256, (256, D), dtype=np.uint8)
    img_h = rng.integers(0, 256, (B, H, W, D), dtype=np.uint8)
    m = _dev(m_h, ctx)
    lut = _dev(np.concatenate([[0], lut_h.reshape(-1)]).astype(np.uint8), ctx)[1:].view(256, D)      # (the table at an odd address)
    for alpha in ALPHAS:
        flat, live, d, view = _alloc(B, D, W, H, kind, ctx, seed=alpha + len(kind), content=img_h)
        assert ctx.map_overlay(m, view, lut, lo, hi, alpha=alpha, smooth=smooth) is view
        ctx.sync()
        want, k = overlay_ref(m_h, img_h, lut_h, lo, hi, alpha, smooth)
        if alpha == 0:
            assert np.array_equal(want, img_h)                                       # every byte as it was
        if alpha == 256:
            assert np.array_equal(want, lut_h[k])                                    # the table's colour exactly
        _check_whole_allocation(flat, live, d, want, (shape, smooth, lo, hi, kind, alpha))


def test_map_overlay_takes_one_image_and_one_map_without_the_batch_axes(ctx):
    shape = (1, 3, 8, 6, 130, 70)
    m_h, lut_h = _map(shape, 0.25, 7.5), aefft.heat_lut(3)
    img_h = np.random.default_rng(1).integers(0, 256, (70, 130, 3), dtype=np.uint8)
    img = _dev(img_h, ctx)
    assert ctx.map_overlay(_dev(m_h[0], ctx), img, _dev(lut_h, ctx), 0.25, 7.5) is img       # alpha = 128, smooth
    ctx.sync()
    assert np.array_equal(host(img), overlay_ref(m_h, img_h[None], lut_h, 0.25, 7.5, 128, True)[0][0])


# ------------------------------------------------------------------------------------------
# 9. each call captured once and replayed
# ------------------------------------------------------------------------------------------
def test_both_calls_are_captured_once_and_replayed():
    """one launch each, no allocation, no synchronisation: two kernel nodes of one graph; a replay on new inputs gives their bytes"""
    shape = (2, 3, 66, 34, 130, 70)
    B, D, Nx, Ny, W, H = shape
    f8 = _frames((2, 3, 66, 34, 130, 70))[0]
    mshape = (2, 3, 8, 6, 130, 70)
    m_h, lut_h = _map(mshape, 0.25, 7.5), aefft.heat_lut(3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        frames = torch.zeros(B, D, Nx, Ny, dtype=torch.uint8, device=dev)
        m = torch.zeros(B, 8, 6, dtype=torch.float32, device=dev)
        lut = _dev(lut_h, c)
        out = torch.full((B, H, W, D), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.frames_resize_to_image(frames, (W, H), "linear", out=out)
            c.map_overlay(m, out, lut, 0.25, 7.5, alpha=100)
        torch.cuda.synchronize()
        frames.copy_(_dev(f8, c)); m.copy_(_dev(m_h, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        resized = _want(shape, "linear")
        assert np.array_equal(host(out), overlay_ref(m_h, resized, lut_h, 0.25, 7.5, 100, True)[0])
        direct = c.map_overlay(m, c.frames_resize_to_image(frames, (W, H), "linear"), lut, 0.25, 7.5, alpha=100)
        c.sync()
        assert torch.equal(direct, out)
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 10. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    B, D, Nx, Ny, W, H = 2, 3, 8, 8, 11, 9
    pitch, stride = W * D, H * W * D
    dev = f"cuda:{ctx.device}"
    img = torch.full((B * stride + 64,), 0x3C, dtype=torch.uint8, device=dev)
    frm = torch.full((4 * B * D * Nx * Ny + 64,), 0xC3, dtype=torch.uint8, device=dev)
    ip, fp = img.data_ptr(), frm.data_ptr()
    assert fp % 16 == 0
    LIN, AREA = 0, 1
    # (frames, u8, Nx, Ny, mode, image, pitch, stride, W, H, B, D), the whole message behind the call's name
    # the rules' full texts, as the library words them
    NULL, DIM, RANGE, FRANGE = "null context, image or frames", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and W, H in 1..8192", "Nx, Ny must be in 1..8192"
    MODE, AREA_RULE = "mode must be AEFFT_RESIZE_LINEAR or AEFFT_RESIZE_AREA", "AEFFT_RESIZE_AREA does not enlarge: it needs W <= Nx and H <= Ny"
    PITCH, STRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ROWS_FIT, BATCH_FIT = "H * pitch does not fit the address space", "B * image_stride does not fit the address space"
    ALIGN, OVERLAP = "frames_d must be 16-byte aligned", "the frame and image ranges overlap (the op is out-of-place)"
    cases = [
        ("null image", (fp, 1, Nx, Ny, LIN, None, pitch, stride, W, H, B, D), NULL),
        ("null frames", (None, 1, Nx, Ny, LIN, ip, pitch, stride, W, H, B, D), NULL),
        ("D = 0", (fp, 1, Nx, Ny, LIN, ip, pitch, stride, W, H, B, 0), DIM),
        ("D = 5", (fp, 1, Nx, Ny, LIN, ip, 5 * W, 5 * W * H, W, H, B, 5), DIM),
        ("B = 0", (fp, 1, Nx, Ny, LIN, ip, pitch, stride, W, H, 0, D), RANGE),
        ("W = 0", (fp, 1, Nx, Ny, LIN, ip, pitch, stride, 0, H, B, D), RANGE),
        ("H = 8193", (fp, 1, Nx, Ny, LIN, ip, pitch, stride, W, 8193, 1, D), RANGE),
        ("Nx = 0", (fp, 1, 0, Ny, LIN, ip, pitch, stride, W, H, B, D), FRANGE),
        ("Ny = 8193", (fp, 1, Nx, 8193, LIN, ip, pitch, stride, W, H, B, D), FRANGE),
        ("mode = 2", (fp, 1, Nx, Ny, 2, ip, pitch, stride, W, H, B, D), MODE),
        ("mode = -1", (fp, 1, Nx, Ny, -1, ip, pitch, stride, W, H, B, D), MODE),
        ("AREA enlarging x", (fp, 1, Nx, Ny, AREA, ip, pitch, stride, Nx + 1, Ny, B, D), AREA_RULE),
        ("AREA enlarging y", (fp, 1, Nx, Ny, AREA, ip, Nx * D, (Ny + 1) * Nx * D, Nx, Ny + 1, B, D), AREA_RULE),
        ("pitch = W D - 1", (fp, 1, Nx, Ny, LIN, ip, pitch - 1, stride, W, H, B, D), PITCH),
        ("stride too small", (fp, 1, Nx, Ny, LIN, ip, pitch, (H - 1) * pitch + W * D - 1, W, H, B, D), STRIDE),
        ("stride = 0", (fp, 1, Nx, Ny, LIN, ip, pitch, 0, W, H, B, D), STRIDE),
        ("pitch overflows", (fp, 1, Nx, Ny, LIN, ip, 2 ** 62, stride, W, H, 1, D), ROWS_FIT),
        ("stride overflows", (fp, 1, Nx, Ny, LIN, ip, pitch, 2 ** 62, W, H, 3, D), BATCH_FIT),
        ("frames off by 4", (fp + 4, 0, Nx, Ny, LIN, ip, pitch, stride, W, H, B, D), ALIGN),
        ("overlap: frames inside the image", (ip + 16, 1, Nx, Ny, LIN, ip, pitch, stride, W, H, B, D), OVERLAP),
        ("overlap: image inside the float frames", (fp, 0, Nx, Ny, LIN, fp + 64, pitch, stride, W, H, B, D), OVERLAP),
        ("overlap: the second image only", (fp, 0, Nx, Ny, LIN, fp + 4 * B * D * Nx * Ny - stride - 32, pitch, stride, W, H, B, D), OVERLAP),
    ]
    for what, args, rule in cases:
        assert L.aefft_frames_resize_to_image(ctx.h, *args) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_frames_resize_to_image: " + rule, (what, msg)
    mp = torch.full((1024,), 0x40, dtype=torch.uint8, device=dev)                    # floats 3.0039...: a map in its first 128 bytes
    lt = torch.full((256 * D + 64,), 0x77, dtype=torch.uint8, device=dev)
    m, l = mp.data_ptr(), lt.data_ptr()
    assert m % 16 == 0
    inf, nan = float("inf"), float("nan")
    # (map, Mx, My, lo, hi, smooth, lut, alpha, image, pitch, stride, W, H, B, D)
    NULL, MRANGE, ALPHA = "null context, map, lut or image", "Mx, My must be in 1..1024", "alpha must be 0..256"
    LOHI, ALIGN = "lo and hi must be finite and different (255 / (hi - lo) finite)", "map_d must be 16-byte aligned"
    MAP_OVERLAP, LUT_OVERLAP = "the map and image ranges overlap", "the lut and image ranges overlap"
    cases = [
        ("null map", (None, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, B, D), NULL),
        ("null lut", (m, 4, 4, 0.0, 1.0, 1, None, 128, ip, pitch, stride, W, H, B, D), NULL),
        ("null image", (m, 4, 4, 0.0, 1.0, 1, l, 128, None, pitch, stride, W, H, B, D), NULL),
        ("Mx = 0", (m, 0, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, B, D), MRANGE),
        ("My = 1025", (m, 4, 1025, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, 1, D), MRANGE),
        ("D = 5", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, 5 * W, 5 * W * H, W, H, B, 5), DIM),
        ("B = 0", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, 0, D), RANGE),
        ("W = 8193", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, 8193 * D, stride, 8193, H, 1, D), RANGE),
        ("H = 0", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, 0, B, D), RANGE),
        ("alpha = 257", (m, 4, 4, 0.0, 1.0, 1, l, 257, ip, pitch, stride, W, H, B, D), ALPHA),
        ("alpha = -1", (m, 4, 4, 0.0, 1.0, 1, l, -1, ip, pitch, stride, W, H, B, D), ALPHA),
        ("lo == hi", (m, 4, 4, 2.0, 2.0, 1, l, 128, ip, pitch, stride, W, H, B, D), LOHI),
        ("lo = nan", (m, 4, 4, nan, 1.0, 1, l, 128, ip, pitch, stride, W, H, B, D), LOHI),
        ("hi = inf", (m, 4, 4, 0.0, inf, 1, l, 128, ip, pitch, stride, W, H, B, D), LOHI),
        ("hi = -inf", (m, 4, 4, 0.0, -inf, 1, l, 128, ip, pitch, stride, W, H, B, D), LOHI),
        ("map off by 4", (m + 4, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, B, D), ALIGN),
        ("pitch = W D - 1", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch - 1, stride, W, H, B, D), PITCH),
        ("stride too small", (m, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, (H - 1) * pitch + W * D - 1, W, H, B, D), STRIDE),
        ("overlap: the map inside the image", (ip + 16, 4, 4, 0.0, 1.0, 1, l, 128, ip, pitch, stride, W, H, B, D), MAP_OVERLAP),
        ("overlap: the image inside the map", (m, 4, 4, 0.0, 1.0, 1, l, 128, m + 4 * B * 16 - 8, pitch, stride, W, H, B, D), MAP_OVERLAP),
        ("overlap: the table inside the image", (m, 4, 4, 0.0, 1.0, 1, ip + stride + 5, 128, ip, pitch, stride, W, H, B, D), LUT_OVERLAP),
        ("overlap: the image begins in the table", (m, 4, 4, 0.0, 1.0, 1, l, 128, l + 256 * D - 1, pitch, stride, W, H, B, D), LUT_OVERLAP),
    ]
    for what, args, rule in cases:
        assert L.aefft_map_overlay_image(ctx.h, *args) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_map_overlay_image: " + rule, (what, msg)
    ctx.sync()
    assert (host(img) == 0x3C).all() and (host(frm) == 0xC3).all() and (host(mp) == 0x40).all() and (host(lt) == 0x77).all()
    # what is NOT an error: a stride of any value for one image; the smallest legal stride (a constant source: every pixel 0xC3)
    one = torch.full(((H - 1) * pitch + W * D,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_frames_resize_to_image(ctx.h, fp, 1, Nx, Ny, LIN, one.data_ptr(), pitch, 0, W, H, 1, D) == aefft.OK
    small = (H - 1) * pitch + W * D
    two = torch.full((B * small,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_frames_resize_to_image(ctx.h, fp, 1, Nx, Ny, LIN, two.data_ptr(), pitch, small, W, H, B, D) == aefft.OK
    ctx.sync()
    assert (host(one) == 0xC3).all() and (host(two) == 0xC3).all()
    # alpha = 256 with a constant table: the same two layouts come back as the table's byte
    assert L.aefft_map_overlay_image(ctx.h, m, 4, 4, 0.0, 1.0, 1, l, 256, one.data_ptr(), pitch, 0, W, H, 1, D) == aefft.OK
    assert L.aefft_map_overlay_image(ctx.h, m, 4, 4, 1.0, 0.0, 0, l, 256, two.data_ptr(), pitch, small, W, H, B, D) == aefft.OK
    ctx.sync()
    assert (host(one) == 0x77).all() and (host(two) == 0x77).all()
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    f = frm[:B * D * Nx * Ny].view(B, D, Nx, Ny)
    v = img[:B * stride].view(B, H, W, D)
    with pytest.raises(ValueError):
        ctx.frames_resize_to_image(f, (W, H), out=v.permute(0, 2, 1, 3))
    with pytest.raises(ValueError):
        ctx.frames_resize_to_image(f, (W, H), out=torch.empty(B, H, 2 * W, D, dtype=torch.uint8, device=dev)[:, :, ::2])
    with pytest.raises(ValueError):
        ctx.frames_resize_to_image(f, (W, H), mode="cubic")
    with pytest.raises(ValueError):
        ctx.frames_resize_to_image(f.permute(0, 1, 3, 2), (W, H))
    with pytest.raises(aefft.AefftError, match="AEFFT_RESIZE_AREA"):
        ctx.frames_resize_to_image(f, (W, H), mode="area")
    lut3 = lt[:256 * D].view(256, D)
    mm = mp[:4 * B * 16].view(torch.float32).view(B, 4, 4)
    with pytest.raises(ValueError):
        ctx.map_overlay(mm, v.permute(0, 2, 1, 3), lut3, 0.0, 1.0)
    with pytest.raises(ValueError):
        ctx.map_overlay(mm[:1], v, lut3, 0.0, 1.0)
    with pytest.raises(ValueError):
        ctx.map_overlay(mm, v, lut3, 1.0, 1.0)
    with pytest.raises(ValueError):
        ctx.map_overlay(mm, v, lut3, 0.0, 1.0, alpha=300)
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.map_overlay(mm, mp[64:64 + B * stride].view(B, H, W, D), lut3, 0.0, 1.0)
    ctx.sync()
    assert (host(img) == 0x3C).all() and (host(frm) == 0xC3).all() and (host(mp) == 0x40).all() and (host(lt) == 0x77).all()


# ------------------------------------------------------------------------------------------
# 11. profile accounting
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_one_call_is_one_image_launch_with_its_bytes(ctx, f32):
    B, D, Nx, Ny, W, H, Mx, My = 2, 3, 66, 34, 130, 70, 8, 6
    dev = f"cuda:{ctx.device}"
    frames = torch.zeros(B, D, Nx, Ny, dtype=torch.float32 if f32 else torch.uint8, device=dev)
    img = torch.zeros(B, H, W, D, dtype=torch.uint8, device=dev)
    small = torch.zeros(B, 20, 40, D, dtype=torch.uint8, device=dev)
    m, lut = torch.zeros(B, Mx, My, device=dev), _dev(aefft.heat_lut(D), ctx)
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.frames_resize_to_image(frames, (W, H), "linear", out=img)
        one = ctx.prof_read()
        ctx.frames_resize_to_image(frames, (40, 20), "area", out=small)
        two = ctx.prof_read()
        ctx.map_overlay(m, img, lut, 0.0, 1.0)
        three = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    es = 4 if f32 else 1
    n1, n2, n3 = B * D * (Nx * Ny * es + W * H), B * D * (Nx * Ny * es + 40 * 20), B * (4 * Mx * My + 2 * W * H * D) + 256 * D
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == n1
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == n1 + n2
    assert three["image"]["launches"] == 3 and three["image"]["bytes"] == n1 + n2 + n3
    assert sum(v["launches"] for v in three.values()) == 3
