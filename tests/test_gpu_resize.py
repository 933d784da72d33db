"""aefft_image_resize_to_frames (Context.image_resize_to_frames): resize + ImageToSpin_C in one launch, against a numpy int64 restatement of
include/aefft.h's formulas written here -- EXACT equality for 8-bit and float frames, both modes, every shape with a tight, a 64-aligned and
an unaligned pitch (the last from a base off by one byte), a region of interest whose batch stride is not H * pitch, the output pre-filled
and a guard region behind it, random pad bytes, the identity against image_to_frames, a constant image, a net fed from the call, one graph
capture and replay, every AEFFT_EINVAL rule, and the profile entry."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_fft_path import host
from test_gpu_sizes import _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (B, D, W, H, Nx, Ny): identity; odd source with W D no dword multiple; enlarging (edge clamps at both ends, w reaching 2048); exact 2x (AREA = the
# block mean); more than one tile with remainders and Ny % 4 == 2; ratios 20 and 12.5 (the footprint that needs bands of source rows); the
# reference's own case; AREA with ~30 x 17 source pixels per cell (the 64-bit sum); ONE tile whose rows are so wide that a band holds 5 of the 50
# (LINEAR) or 64 (AREA) source rows it needs (rz_geometry: P = 1465 / 1537, RB = 5): every sum runs across ten bands or more
SHAPES = [(1, 1, 8, 8, 8, 8), (2, 3, 11, 9, 8, 8), (1, 3, 7, 5, 16, 8), (2, 4, 64, 64, 32, 32), (1, 3, 130, 70, 66, 34), (1, 2, 200, 150, 10, 12),
          (2, 3, 640, 480, 256, 256), (1, 3, 1920, 1080, 64, 64), (1, 3, 2048, 64, 21, 4)]
PITCHES = ["tight", "pad64", "odd"]
MODES = ["linear", "area"]
CASES = [(s, m) for s in SHAPES for m in MODES if m == "linear" or (s[4] <= s[2] and s[5] <= s[3])]
GUARD = 64         # bytes behind the frames that must stay as they were
TAIL = 96          # bytes of the allocation behind the last image row


# ------------------------------------------------------------------------------------------
# the oracle: include/aefft.h's formulas in numpy int64
# ------------------------------------------------------------------------------------------
def _linear_axis(S, N):
    i = np.arange(N, dtype=np.int64)
    n, den = (2 * i + 1) * S - N, 2 * N
    s = np.floor_divide(n, den)
    r = n - s * den
    w = (4096 * r + den) // (2 * den)
    w[s < 0] = 0; s[s < 0] = 0
    w[s >= S - 1] = 0; s[s >= S - 1] = S - 1
    return s, np.minimum(s + 1, S - 1), w


def _overlaps(S, N):
    """o[i][k] = max(0, min((i+1) S, (k+1) N) - max(i S, k N)), [N][S]"""
    i, k = np.arange(N, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * S, (k + 1) * N) - np.maximum(i * S, k * N))


def oracle(px, size, mode):
    """px uint8 [B][H][W][D] -> (8-bit frames, float frames), both [B][D][Nx][Ny]"""
    B, H, W, D = px.shape
    Nx, Ny = size
    p = px.astype(np.int64)
    if mode == "linear":
        x0, x1, wx = _linear_axis(W, Nx)
        y0, y1, wy = _linear_axis(H, Ny)
        wx, wy = wx[None, None, :, None], wy[None, :, None, None]
        top = (2048 - wx) * p[:, y0][:, :, x0] + wx * p[:, y0][:, :, x1]
        bot = (2048 - wx) * p[:, y1][:, :, x0] + wx * p[:, y1][:, :, x1]
        v = (2048 - wy) * top + wy * bot                                        # [B][Ny][Nx][D]
        assert v.max() < 2 ** 30
        u8, q = (v + 2 ** 21) >> 22, (v + 32) >> 6
    else:
        ox, oy = _overlaps(W, Nx), _overlaps(H, Ny)
        assert (ox.sum(1) == W).all() and (oy.sum(1) == H).all()
        rows = np.tensordot(p, ox, axes=([2], [1]))                              # [B][H][D][Nx]
        num = np.tensordot(oy, rows, axes=([1], [1])).transpose(1, 0, 3, 2)      # [Ny][B][D][Nx] -> [B][Ny][Nx][D]
        wh = W * H
        u8, q = (2 * num + wh) // (2 * wh), (65536 * num + wh // 2) // wh
    assert u8.min() >= 0 and u8.max() <= 255 and q.max() < 2 ** 24
    f32 = q.astype(np.float32) * np.float32(2.0 ** -16)
    assert np.array_equal(f32.astype(np.float64) * 65536, q)                     # (the float is exact)
    tr = lambda a: np.ascontiguousarray(a.transpose(0, 3, 2, 1))
    return tr(u8.astype(np.uint8)), tr(f32)


@functools.lru_cache(maxsize=None)
def _pixels(shape):
    B, D, W, H, Nx, Ny = shape
    px = np.random.default_rng(sum(shape)).integers(0, 256, (B, H, W, D), dtype=np.uint8)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _want(shape, mode):
    """computed once per (shape, mode), shared by the pitches and left unchanged"""
    w8, w32 = oracle(_pixels(shape), shape[4:], mode)
    w8.setflags(write=False); w32.setflags(write=False)
    return w8, w32


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")          # (a copy: the cached pixels stay read-only)


def _layout(shape, kind):
    """(pitch, offset of the first image in its allocation, bytes of the allocation)"""
    B, D, W, H = shape[:4]
    pitch = {"tight": W * D, "pad64": (W * D + 63) // 64 * 64, "odd": W * D + 5}[kind]
    off = 1 if kind == "odd" else 0
    return pitch, off, off + B * H * pitch + TAIL


def _pitched(px, shape, kind, ctx, seed):
    """the pixels inside a flat allocation of random bytes (pad bytes and tail included), as a device view [B][H][W][D]"""
    B, D, W, H = shape[:4]
    pitch, off, n = _layout(shape, kind)
    flat = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(flat[off:], (B, H, W, D), (H * pitch, pitch, D, 1))[...] = px
    return torch.as_strided(_dev(flat, ctx), (B, H, W, D), (H * pitch, pitch, D, 1), off)


def _guarded(ctx, shape, dtype, fill):
    """(out [B][D][Nx][Ny] pre-filled, the whole allocation as bytes, bytes of the frames): GUARD bytes of 0x5A behind the frames"""
    B, D, W, H, Nx, Ny = shape
    nbytes = B * D * Nx * Ny * (4 if dtype == torch.float32 else 1)
    raw = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    assert raw.data_ptr() % 16 == 0
    out = raw[:nbytes].view(dtype).view(B, D, Nx, Ny)
    out.fill_(fill)
    return out, raw, nbytes


def _run_and_check(ctx, img, shape, mode, want8, want32, tag):
    out8, raw8, n8 = _guarded(ctx, shape, torch.uint8, 0xEE)
    out32, raw32, n32 = _guarded(ctx, shape, torch.float32, float("nan"))
    size = shape[4:]
    assert ctx.image_resize_to_frames(img, size, mode, out=out8) is out8
    assert ctx.image_resize_to_frames(img, size, mode, out=out32) is out32
    ctx.sync()
    g8, g32 = host(out8), host(out32)
    print(tag, "8-bit mismatches", int((g8 != want8).sum()), "float mismatches", int((g32.view(np.uint32) != want32.view(np.uint32)).sum()))
    assert g8.dtype == np.uint8 and np.array_equal(g8, want8), tag
    assert g32.dtype == np.float32 and not np.isnan(g32).any() and np.array_equal(g32.view(np.uint32), want32.view(np.uint32)), tag
    assert (host(raw8)[n8:] == 0x5A).all() and (host(raw32)[n32:] == 0x5A).all(), (tag, "guard")
    # 0xEE is a legal pixel: the same again over the complement
    out8.fill_(0x11)
    ctx.image_resize_to_frames(img, size, mode, out=out8)
    ctx.sync()
    assert np.array_equal(host(out8), want8), tag


# ------------------------------------------------------------------------------------------
# 1. every shape, pitch and mode; a region of interest
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("shape,mode", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_resize_equals_the_integer_formulas(ctx, shape, mode, kind):
    want8, want32 = _want(shape, mode)
    img = _pitched(_pixels(shape), shape, kind, ctx, seed=len(kind) + len(mode))      # (the pad bytes are random: none of them may show)
    _run_and_check(ctx, img, shape, mode, want8, want32, (shape, mode, kind))


@pytest.mark.parametrize("mode", MODES)
def test_fresh_outputs_and_one_image_without_the_batch_axis(ctx, mode):
    shape = (2, 3, 11, 9, 8, 8)
    want8, want32 = _want(shape, mode)
    img = _dev(_pixels(shape), ctx)
    new8, new32 = ctx.image_resize_to_frames(img, (8, 8), mode), ctx.image_resize_to_frames(img, (8, 8), mode, dtype=torch.float32)
    one = ctx.image_resize_to_frames(img[1], (8, 8), mode)
    ctx.sync()
    assert new8.dtype == torch.uint8 and np.array_equal(host(new8), want8)
    assert new32.dtype == torch.float32 and np.array_equal(host(new32), want32)
    assert tuple(one.shape) == (1, 3, 8, 8) and np.array_equal(host(one), want8[1:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 3, 130, 70, 66, 34), (2, 4, 64, 64, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_region_of_interest_of_a_larger_batch(ctx, shape, mode):
    """big[:, 3:3+H, 5:5+W]: the parent's pitch, and a batch stride that is not H * pitch"""
    B, D, W, H, Nx, Ny = shape
    big_h = np.random.default_rng(5).integers(0, 256, (B, H + 11, W + 9, D), dtype=np.uint8)
    roi_h = big_h[:, 3:3 + H, 5:5 + W]
    want8, want32 = oracle(roi_h, (Nx, Ny), mode)
    roi = _dev(big_h, ctx)[:, 3:3 + H, 5:5 + W]
    assert roi.stride(0) != H * roi.stride(1) and not roi.is_contiguous()
    _run_and_check(ctx, roi, shape, mode, want8, want32, (shape, mode, "roi"))


# ------------------------------------------------------------------------------------------
# 2. consequences of the definition
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 3, 11, 9), (2, 4, 64, 64), (1, 3, 130, 70)], ids=lambda s: "x".join(map(str, s)))
def test_same_size_is_image_to_frames(ctx, shape, mode):
    B, D, W, H = shape
    img = _dev(np.random.default_rng(W + H).integers(0, 256, (B, H, W, D), dtype=np.uint8), ctx)
    for dtype in (torch.uint8, torch.float32):
        a = ctx.image_resize_to_frames(img, (W, H), mode, dtype=dtype)
        b = ctx.image_to_frames(img, dtype=dtype)
        ctx.sync()
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), (shape, mode, dtype)


@pytest.mark.parametrize("mode", MODES)
def test_a_constant_image_stays_constant(ctx, mode):
    for value, (W, H, Nx, Ny) in ((0, (37, 29, 16, 12)), (255, (200, 150, 10, 12)), (77, (130, 70, 66, 34)), (255, (7, 5, 16, 8) if mode == "linear" else (64, 64, 32, 32))):
        img = torch.full((2, H, W, 3), value, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        a8 = ctx.image_resize_to_frames(img, (Nx, Ny), mode)
        a32 = ctx.image_resize_to_frames(img, (Nx, Ny), mode, dtype=torch.float32)
        ctx.sync()
        assert (host(a8) == value).all() and (host(a32) == np.float32(value)).all(), (mode, value, W, H)


def test_area_at_integer_ratios_is_the_rounded_block_mean(ctx):
    B, D, W, H, Nx, Ny = 2, 4, 64, 64, 32, 32
    px = _pixels((B, D, W, H, Nx, Ny))
    blocks = px.astype(np.int64).reshape(B, Ny, 2, Nx, 2, D).sum(axis=(2, 4))                 # [B][Ny][Nx][D]
    want = np.ascontiguousarray(((2 * blocks + 4) // 8).transpose(0, 3, 2, 1)).astype(np.uint8)   # floor(mean + 1/2)
    got = ctx.image_resize_to_frames(_dev(px, ctx), (Nx, Ny), "area")
    ctx.sync()
    assert np.array_equal(host(got), want)


# ------------------------------------------------------------------------------------------
# 3. a net fed from the call; a captured call
# ------------------------------------------------------------------------------------------
def test_step_grad_u8_on_resized_frames_is_bit_for_bit(ctx):
    D, Nx, Ny, B = 3, 16, 16, 2
    shape = (B, D, 37, 29, Nx, Ny)
    want8, _ = _want(shape, "linear")
    img_d, planar_d = _dev(_pixels(shape), ctx), _dev(want8, ctx)
    outs = []
    for frames in (lambda: ctx.image_resize_to_frames(img_d, (Nx, Ny), "linear", dtype=torch.uint8), lambda: planar_d):
        net = aefft.Net(ctx, D, Nx, Ny, [2], 3, 1, batch=B)
        try:
            for l, w in enumerate(_weights(np.random.default_rng(3), D, [2], 3, 3)):
                net.set_pair(l, *w)
            recon = ctx.empty(B, D, Nx, Ny)
            gbuf = net.grad_buffer(); grads = torch.empty_like(gbuf)
            net.step_grad(frames(), recon)                                       # (queued behind the resize: nothing waits in between)
            grads.copy_(gbuf)
            ctx.sync()
            outs.append((host(recon).copy(), host(grads).copy()))
        finally:
            net.close()
    assert np.isfinite(outs[0][1]).all() and np.abs(outs[0][1]).max() > 0
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


def test_the_call_is_captured_once_and_replayed():
    """one launch, no allocation, no synchronisation: the call is a single kernel node of a graph; a replay on new pixels gives their bytes"""
    shape = (2, 3, 130, 70, 66, 34)
    B, D, W, H, Nx, Ny = shape
    want8, _ = _want(shape, "area")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        img = torch.zeros(B, H, W, D, dtype=torch.uint8, device=f"cuda:{c.device}")
        out = torch.full((B, D, Nx, Ny), 0xEE, dtype=torch.uint8, device=f"cuda:{c.device}")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.image_resize_to_frames(img, (Nx, Ny), "area", out=out)
        torch.cuda.synchronize()
        img.copy_(_dev(_pixels(shape), c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), want8)
        direct = c.image_resize_to_frames(img, (Nx, Ny), "area")
        c.sync()
        assert torch.equal(direct, out)
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(ctx):
    L = ctx.L
    B, D, W, H, Nx, Ny = 2, 3, 11, 9, 8, 8
    pitch, stride = W * D, H * W * D
    dev = f"cuda:{ctx.device}"
    img = torch.full((B * stride + 64,), 0x3C, dtype=torch.uint8, device=dev)
    frm = torch.full((4 * B * D * Nx * Ny + 64,), 0xC3, dtype=torch.uint8, device=dev)
    ip, fp = img.data_ptr(), frm.data_ptr()
    assert fp % 16 == 0
    LIN, AREA = 0, 1
    # the rules' full texts, as the library words them
    NULL, DIM, RANGE = "null context, image or frames", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and W, H, Nx, Ny in 1..8192"
    MODE, AREA_RULE = "mode must be AEFFT_RESIZE_LINEAR or AEFFT_RESIZE_AREA", "AEFFT_RESIZE_AREA does not enlarge: it needs Nx <= W and Ny <= H"
    PITCH, STRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ALIGN, OVERLAP = "frames_d must be 16-byte aligned", "the frame and image ranges overlap (the op is out-of-place)"
    # (image, pitch, stride, W, H, mode, frames, u8, B, D, Nx, Ny), the whole message behind the call's name
    cases = [
        ("null image", (None, pitch, stride, W, H, LIN, fp, 1, B, D, Nx, Ny), NULL),
        ("null frames", (ip, pitch, stride, W, H, LIN, None, 1, B, D, Nx, Ny), NULL),
        ("D = 0", (ip, pitch, stride, W, H, LIN, fp, 1, B, 0, Nx, Ny), DIM),
        ("D = 5", (ip, 5 * W, 5 * W * H, W, H, LIN, fp, 1, B, 5, Nx, Ny), DIM),
        ("B = 0", (ip, pitch, stride, W, H, LIN, fp, 1, 0, D, Nx, Ny), RANGE),
        ("W = 0", (ip, pitch, stride, 0, H, LIN, fp, 1, B, D, Nx, Ny), RANGE),
        ("H = 8193", (ip, pitch, stride, W, 8193, LIN, fp, 1, 1, D, Nx, Ny), RANGE),
        ("Nx = 0", (ip, pitch, stride, W, H, LIN, fp, 1, B, D, 0, Ny), RANGE),
        ("Ny = 8193", (ip, pitch, stride, W, H, LIN, fp, 1, B, D, Nx, 8193), RANGE),
        ("mode = 2", (ip, pitch, stride, W, H, 2, fp, 1, B, D, Nx, Ny), MODE),
        ("mode = -1", (ip, pitch, stride, W, H, -1, fp, 1, B, D, Nx, Ny), MODE),
        ("AREA enlarging x", (ip, pitch, stride, W, H, AREA, fp, 1, B, D, W + 1, Ny), AREA_RULE),
        ("AREA enlarging y", (ip, pitch, stride, W, H, AREA, fp, 1, B, D, Nx, H + 1), AREA_RULE),
        ("pitch = W D - 1", (ip, pitch - 1, stride, W, H, LIN, fp, 1, B, D, Nx, Ny), PITCH),
        ("stride too small", (ip, pitch, (H - 1) * pitch + W * D - 1, W, H, LIN, fp, 1, B, D, Nx, Ny), STRIDE),
        ("stride = 0", (ip, pitch, 0, W, H, LIN, fp, 1, B, D, Nx, Ny), STRIDE),
        ("frames off by 4", (ip, pitch, stride, W, H, LIN, fp + 4, 0, B, D, Nx, Ny), ALIGN),
        ("overlap: frames inside the image", (ip, pitch, stride, W, H, LIN, ip + 16, 1, B, D, Nx, Ny), OVERLAP),
        ("overlap: image inside the float frames", (fp + 64, pitch, stride, W, H, LIN, fp, 0, B, D, Nx, Ny), OVERLAP),
        ("overlap: the second image only", (fp + 4 * B * D * Nx * Ny - stride - 32, pitch, stride, W, H, LIN, fp, 0, B, D, Nx, Ny), OVERLAP),
    ]
    for what, args, rule in cases:
        assert L.aefft_image_resize_to_frames(ctx.h, *args) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_image_resize_to_frames: " + rule, (what, msg)
    # what is NOT an error: a stride of any value for one image; the smallest legal stride
    one = torch.full((D * Nx * Ny,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_image_resize_to_frames(ctx.h, ip, pitch, 0, W, H, LIN, one.data_ptr(), 1, 1, D, Nx, Ny) == aefft.OK
    two = torch.full((B * D * Nx * Ny,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_image_resize_to_frames(ctx.h, ip, pitch, (H - 1) * pitch + W * D, W, H, LIN, two.data_ptr(), 1, B, D, Nx, Ny) == aefft.OK
    ctx.sync()
    assert (host(img) == 0x3C).all() and (host(frm) == 0xC3).all()
    assert (host(one) == 0x3C).all() and (host(two) == 0x3C).all()                 # (a constant source: every pixel 0x3C)
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    v = img[:B * stride].view(B, H, W, D)
    with pytest.raises(ValueError):
        ctx.image_resize_to_frames(v.permute(0, 2, 1, 3), (Nx, Ny))
    with pytest.raises(ValueError):
        ctx.image_resize_to_frames(v[:, :, ::2], (Nx, Ny))
    with pytest.raises(ValueError):
        ctx.image_resize_to_frames(v, (Nx, Ny), mode="cubic")
    with pytest.raises(ValueError):
        ctx.image_resize_to_frames(v, (Nx, Ny), out=ctx.empty(B, D, Ny, Nx + 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ctx.image_resize_to_frames(v, (Nx, Ny), out=ctx.empty(B, D, Nx, Ny, dtype=torch.float64))
    with pytest.raises(aefft.AefftError, match="AEFFT_RESIZE_AREA"):
        ctx.image_resize_to_frames(v, (W + 1, Ny), mode="area")


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_one_call_is_one_image_launch_with_its_bytes(ctx, f32):
    B, D, W, H, Nx, Ny = 2, 3, 130, 70, 66, 34
    img = torch.zeros(B, H, W, D, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    frames = ctx.empty(B, D, Nx, Ny, dtype=torch.float32 if f32 else torch.uint8)
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.image_resize_to_frames(img, (Nx, Ny), "linear", out=frames)
        one = ctx.prof_read()
        ctx.image_resize_to_frames(img, (Nx, Ny), "area", out=frames)
        two = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    n = B * D * (W * H + Nx * Ny * (4 if f32 else 1))
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == n
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == 2 * n
    assert sum(v["launches"] for v in two.values()) == 2
