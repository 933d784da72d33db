"""aefft_image_to_yuv and aefft_frames_resize_to_yuv (Context.image_to_yuv, Context.frames_resize_to_yuv) on the device -- EXACT equality
everywhere: the conversion against the numpy restatement of yuv_out_ref.py (every format and matrix; tight / 64-aligned / odd-based planes with a
batch stride that is not the plane's size, pre-filled with two complementary fills, pad bytes and a guard region unchanged; tight, padded and
odd-based source images; odd sizes that reach chroma blocks of 2 and 1 live pixels; all 65536 (R, B) pairs at the G values that reach every clamp),
the fused call against test_gpu_present's oracle followed by that restatement (both modes, both frame types), the composition identity on the
device, the loop decoder surface -> frames -> net -> encoder surface, one graph capture and replay, every AEFFT_EINVAL rule, and the profile
entry."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import yuv_out_ref as R
from test_gpu_fft_path import host
from test_gpu_present import _small_net, expected_image, px_u8

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

FORMATS, MATRICES = R.FORMATS, R.MATRICES
KINDS = ["tight", "pad64", "odd"]
MODES = ["linear", "area"]
GUARD = 64         # bytes behind a plane's allocation that must stay as they were
# (W, H) of the plain call: one block; odd sizes (NV12, I420: the last chroma column and row average 2 and 1 live pixels) / an odd height (YUYV);
# several blocks with a group that crosses the row's end
IMAGE_SHAPES = {"nv12": [(8, 8), (11, 9), (130, 70)], "i420": [(8, 8), (11, 9), (130, 70)], "yuyv": [(8, 8), (12, 9), (130, 70)]}
# (B, Nx, Ny, W, H) of the fused call: identity; enlarging to odd; reduction; enlarging; several tiles; strong reduction; a y-reduction of 43 (the
# present kernel's tile would be one row high); the camera case; 1080p; an x-reduction of 128 whose tiles need more source columns than a band
# holds, so that the sums run across bands (fy_geometry: to 16 x 4 AREA needs 512 columns with XB = 322, LINEAR needs 386 and XB is 386 -- one
# band --; to 16 x 8 LINEAR needs 386 with XB = 322 too)
RESIZE_SHAPES = [(1, 8, 8, 8, 8), (2, 8, 8, 11, 9), (1, 16, 8, 6, 4), (2, 32, 32, 64, 64), (1, 66, 34, 130, 70), (1, 64, 64, 10, 12), (1, 64, 512, 10, 12),
                 (2, 256, 256, 640, 480), (1, 64, 64, 1920, 1080), (1, 2048, 64, 16, 4), (1, 2048, 64, 16, 8)]
RESIZE_CASES = [(s, f, m) for s in RESIZE_SHAPES for f in FORMATS for m in MODES
                if (f != "yuyv" or s[3] % 2 == 0) and (m == "linear" or (s[3] <= s[1] and s[4] <= s[2]))]


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _ids(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")


@functools.lru_cache(maxsize=None)
def _image(B, W, H, D):
    img = np.random.default_rng(B + 3 * W + 7 * H + D).integers(0, 256, (B, H, W, D), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _planes(B, W, H, fmt, matrix, order):
    """the restatement's planes of _image: computed once, shared and left unchanged"""
    p = R.image_to_yuv(_image(B, W, H, 1 if order == "gray" else 3), fmt, matrix, order)
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _frames(shape, D=3):
    """(8-bit frames, float frames with the same pixels: +-0.25 around them)"""
    B, Nx, Ny = shape[:3]
    rng = np.random.default_rng(sum(shape) + D)
    f8 = rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8)
    f32 = f8.astype(np.float32) + np.where(rng.integers(0, 2, f8.shape) == 1, np.float32(0.25), np.float32(-0.25))
    assert np.array_equal(px_u8(f32), f8)
    f8.setflags(write=False); f32.setflags(write=False)
    return f8, f32


@functools.lru_cache(maxsize=None)
def _resized(shape, mode, D=3):
    """the oracle's image [B][H][W][D] of _frames(shape): once per (shape, mode), shared by the formats, layouts and frame types"""
    img = expected_image(_frames(shape, D)[0], shape[3:], mode)
    img.setflags(write=False)
    return img


def _strided(a, kind, ctx, seed=None, fill=None):
    """an array [B][rows][...] inside a flat device allocation, as (the device view of a's shape, the flat tensor, what the flat tensor holds with
    a's bytes in place): pitch tight, rounded up to 64, or live + 5 from a base off by one byte (the byte route); a batch stride that is not
    rows * pitch; GUARD bytes behind.  seed: random pad bytes and a's bytes in place (a source); fill: every byte `fill` (a destination)"""
    B, rows = a.shape[:2]
    live = int(np.prod(a.shape[2:]))
    pitch = {"tight": live, "pad64": (live + 63) // 64 * 64, "odd": live + 5}[kind]
    off = 1 if kind == "odd" else 0
    stride = rows * pitch + (7 if kind == "odd" else 32)
    n = off + B * stride + GUARD
    flat = np.full(n, fill, dtype=np.uint8) if seed is None else np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    inner = tuple(int(np.prod(a.shape[k + 1:])) for k in range(2, a.ndim))
    want = flat.copy()
    np.lib.stride_tricks.as_strided(want[off:], a.shape, (stride, pitch) + inner)[...] = a
    dflat = _dev(want if seed is not None else flat, ctx)
    return torch.as_strided(dflat, a.shape, (stride, pitch) + inner, off), dflat, want


def _dest(want_planes, kind, ctx, fill):
    """pre-filled destination planes: tight and pad64 every plane alike (pad64: the dword route whatever W is); odd: the planes alternate between
    the odd base and pad64, so that one call mixes pitches (the byte route)"""
    return [_strided(a, "pad64" if kind == "odd" and k % 2 else kind, ctx, fill=fill) for k, a in enumerate(want_planes)]


def _check_dest(dest, tag):
    for k, (_, dflat, want) in enumerate(dest):
        got = host(dflat)
        assert np.array_equal(got, want), (tag, "plane", k, "mismatches", int((got != want).sum()), "of", got.size)


# ------------------------------------------------------------------------------------------
# 1. image_to_yuv
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt,size", [(f, s) for f in FORMATS for s in IMAGE_SHAPES[f]], ids=_ids)
def test_planes_equal_the_integer_formula(ctx, fmt, size, kind):
    B, (W, H) = 2, size
    for m, matrix in enumerate(MATRICES):
        src, _, _ = _strided(_image(B, W, H, 3), KINDS[(KINDS.index(kind) + m) % 3], ctx, seed=5)      # (tight, padded and odd-based sources over the matrices)
        want = _planes(B, W, H, fmt, matrix, "bgr")
        for fill in (0xEE, 0x11):                                               # (either is a legal sample: the same again over the complement)
            dest = _dest(want, kind, ctx, fill)
            out = tuple(v for v, _, _ in dest)
            assert ctx.image_to_yuv(src, fmt, matrix, "bgr", out=out) is out
            ctx.sync()
            print(fmt, size, kind, matrix, hex(fill), "mismatches", [int((host(d) != w).sum()) for _, d, w in dest])
            _check_dest(dest, (fmt, size, kind, matrix, fill))                   # live bytes converted; pad bytes, batch gaps and the guard as they were


@pytest.mark.parametrize("fmt", FORMATS)
def test_orders_fresh_planes_and_one_image_without_the_batch_axis(ctx, fmt):
    B, W, H = 2, 130, 70
    for matrix, order in (("bt709", "rgb"), ("bt601", "gray"), ("jpeg", "gray")):
        D = 1 if order == "gray" else 3
        src, _, _ = _strided(_image(B, W, H, D), "odd", ctx, seed=6)
        want = _planes(B, W, H, fmt, matrix, order)
        dest = _dest(want, "odd", ctx, 0x5A)
        ctx.image_to_yuv(src, fmt, matrix, order, out=tuple(v for v, _, _ in dest))
        ctx.sync()
        _check_dest(dest, (fmt, matrix, order))
        if order == "gray":                                                      # every chroma sample is 128, and was written
            chroma = host(dest[0][0])[..., 1::2] if fmt == "yuyv" else np.concatenate([host(v).ravel() for v, _, _ in dest[1:]])
            assert (chroma == 128).all()
    img = _image(B, W, H, 3)
    fresh = ctx.image_to_yuv(_dev(img[1], ctx), fmt)                             # [H][W][D]: one image
    ctx.sync()
    want = _planes(B, W, H, fmt, "bt601", "bgr")
    assert len(fresh) == len(want)
    for f, w in zip(fresh, want):
        assert f.dtype == torch.uint8 and f.is_contiguous() and tuple(f.shape) == (1,) + w.shape[1:] and np.array_equal(host(f), w[1:])
    # a grey image in three channels gives the planes of the GRAY order
    g = _image(B, W, H, 1)
    a = ctx.image_to_yuv(_dev(np.repeat(g, 3, axis=-1), ctx), fmt, "bt709", "rgb")
    b = ctx.image_to_yuv(_dev(g, ctx), fmt, "bt709", "gray")
    ctx.sync()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    if fmt == "i420":                                                            # YV12: the same call with the two pointers swapped
        y, u, v = (torch.zeros(w.shape, dtype=torch.uint8, device=f"cuda:{ctx.device}") for w in want)
        ctx.image_to_yuv(_dev(img, ctx), fmt, out=(y, v, u))
        ctx.sync()
        assert np.array_equal(host(u), want[2]) and np.array_equal(host(v), want[1]) and np.array_equal(host(y), want[0])


@pytest.mark.parametrize("matrix", MATRICES)
def test_every_red_blue_pair_with_the_green_values_that_reach_every_clamp(ctx, matrix):
    """four 512 x 512 images, G = 0, 1, 254, 255: each 2 x 2 block holds one (R, B) pair four times, so the chroma planes enumerate all 65536 pairs
    (U ends at R = G = 255, B = 0 and R = G = 0, B = 255; V at R = 0, G = B = 255 and R = 255, G = B = 0)"""
    r, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rb = np.repeat(np.repeat(np.stack([r, b], axis=-1), 2, axis=0), 2, axis=1)
    img = np.stack([np.stack([rb[..., 0], np.full((512, 512), g, np.uint8), rb[..., 1]], axis=-1) for g in (0, 1, 254, 255)])
    for fmt in ("nv12", "yuyv"):
        want = R.image_to_yuv(img, fmt, matrix, "rgb")
        if fmt == "nv12":
            Y, U, V = R.pixel_yuv(r, np.zeros_like(r), b, matrix)
            assert np.array_equal(want[1][0, ..., 0], U) and np.array_equal(want[1][0, ..., 1], V) and np.array_equal(want[0][0, ::2, ::2], Y)      # four equal pixels: one pixel's
            lo, hi = (1, 255) if matrix == "jpeg" else (16, 240)
            assert want[1].min() == lo and want[1].max() == hi and want[1][..., 0].max() == hi and want[1][..., 1].max() == hi
        got = ctx.image_to_yuv(_dev(img, ctx), fmt, matrix, "rgb")
        ctx.sync()
        print(matrix, fmt, "mismatches", [int((host(g) != w).sum()) for g, w in zip(got, want)])
        assert all(np.array_equal(host(g), w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------
# 2. frames_resize_to_yuv
# ------------------------------------------------------------------------------------------
def _run_fused(ctx, shape, fmt, mode, matrix, order, kind, tag):
    B, Nx, Ny, W, H = shape
    D = 1 if order == "gray" else 3
    want = R.image_to_yuv(_resized(shape, mode, D), fmt, matrix, order)
    f8, f32 = _frames(shape, D)
    for frames, fill in ((_dev(f8, ctx), 0xEE), (_dev(f32, ctx), 0x11)):         # (8-bit over one fill, float over the complement)
        dest = _dest(want, kind, ctx, fill)
        out = tuple(v for v, _, _ in dest)
        assert ctx.frames_resize_to_yuv(frames, (W, H), fmt, matrix, order, mode, out=out) is out
        ctx.sync()
        print(tag, str(frames.dtype), "mismatches", [int((host(d) != w).sum()) for _, d, w in dest])
        _check_dest(dest, (tag, frames.dtype))


@pytest.mark.parametrize("shape,fmt,mode", RESIZE_CASES, ids=_ids)
def test_fused_equals_the_resize_then_the_conversion_formulas(ctx, shape, fmt, mode):
    B, Nx, Ny, W, H = shape
    kinds = KINDS if W * H < 100000 else [KINDS[(W + len(fmt) + len(mode)) % 3]]      # (the large destinations: one layout each, all three over the cases)
    for kind in kinds:
        _run_fused(ctx, shape, fmt, mode, "bt601", "bgr", kind, (shape, fmt, mode, kind))


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_other_matrices_and_orders(ctx, fmt):
    shape = (1, 130, 70, 66, 34)
    for matrix, order, mode in (("bt709", "bgr", "linear"), ("jpeg", "bgr", "area"), ("bt601", "rgb", "area"), ("bt709", "gray", "linear"), ("jpeg", "gray", "area")):
        _run_fused(ctx, shape, fmt, mode, matrix, order, "pad64", (fmt, matrix, order, mode))


@pytest.mark.parametrize("fmt", FORMATS)
def test_composition_identity_on_the_device(ctx, fmt):
    """fused == frames_resize_to_image -> image_to_yuv; at equal sizes == frames_to_image -> image_to_yuv (both modes)"""
    for shape in ((2, 16, 12, 12, 10), (1, 66, 34, 130, 70), (2, 64, 64, 32, 32), (1, 64, 512, 10, 12), (2, 12, 10, 12, 10), (1, 130, 70, 130, 70)):
        B, Nx, Ny, W, H = shape
        for (matrix, order), D in ((("bt601", "bgr"), 3), (("bt709", "gray"), 1)):
            for frames in (_dev(a, ctx) for a in _frames(shape, D)):
                for mode in MODES:
                    if mode == "area" and (W > Nx or H > Ny):
                        continue
                    fused = ctx.frames_resize_to_yuv(frames, (W, H), fmt, matrix, order, mode)
                    two = ctx.image_to_yuv(ctx.frames_resize_to_image(frames, (W, H), mode), fmt, matrix, order)
                    ctx.sync()
                    assert all(torch.equal(p, q) for p, q in zip(fused, two)), (fmt, shape, matrix, order, mode, frames.dtype)
                    if (Nx, Ny) == (W, H):
                        plain = ctx.image_to_yuv(ctx.frames_to_image(frames), fmt, matrix, order)
                        ctx.sync()
                        assert all(torch.equal(p, q) for p, q in zip(fused, plain)), (fmt, shape, matrix, order, mode, frames.dtype)


# ------------------------------------------------------------------------------------------
# 3. the loop; a captured call
# ------------------------------------------------------------------------------------------
def test_decoder_surface_to_frames_to_net_to_encoder_surface(ctx):
    """yuv_resize_to_frames -> a small net's infer -> frames_resize_to_yuv, both ends views into one NV12 surface each, of the same pitch"""
    D, N, B, W, H = 3, 16, 2, 38, 30
    pitch, rows = 64, 32 + 16                                                    # luma rows padded to 32, chroma behind them
    rng = np.random.default_rng(9)
    surf_in = _dev(rng.integers(0, 256, (B, rows, pitch), dtype=np.uint8), ctx)
    surf_out = torch.full((B, rows, pitch), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    views = lambda s: (s[:, :H, :W], s[:, 32:32 + H // 2, :W].unflatten(-1, (W // 2, 2)))
    net = _small_net(ctx, D, N, B)
    try:
        frames = ctx.yuv_resize_to_frames(views(surf_in), "nv12", (N, N), mode="area")
        recon = ctx.empty(B, D, N, N, dtype=torch.uint8)
        net.infer(frames, recon)
        out = views(surf_out)
        assert ctx.frames_resize_to_yuv(recon, (W, H), "nv12", out=out) is out   # (queued behind the net: nothing waits in between)
        ctx.sync()
        r = host(recon)
        assert len(np.unique(r)) > 2
        want = R.image_to_yuv(expected_image(r, (W, H), "linear"), "nv12")
        assert np.array_equal(host(out[0]), want[0]) and np.array_equal(host(out[1]), want[1])
        rest = host(surf_out).copy()
        rest[:, :H, :W] = 0x5A; rest[:, 32:32 + H // 2, :W] = 0x5A
        assert (rest == 0x5A).all(), "bytes of the surface outside the planes were written"
    finally:
        net.close()


def test_the_calls_are_captured_once_and_replayed():
    """one launch each, no allocation, no synchronisation: a graph of the two calls replayed on new samples gives their bytes"""
    fmt, shape = "nv12", (2, 66, 34, 130, 70)
    B, Nx, Ny, W, H = shape
    f8 = _frames(shape)[0]
    img = _image(B, W, H, 3)
    want_f = R.image_to_yuv(_resized(shape, "linear"), fmt)
    want_i = _planes(B, W, H, "yuyv", "bt601", "bgr")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        frames = torch.zeros(f8.shape, dtype=torch.uint8, device=dev)
        image = torch.zeros(img.shape, dtype=torch.uint8, device=dev)
        out_f = tuple(torch.full(w.shape, 0xEE, dtype=torch.uint8, device=dev) for w in want_f)
        out_i = tuple(torch.full(w.shape, 0xEE, dtype=torch.uint8, device=dev) for w in want_i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.frames_resize_to_yuv(frames, (W, H), fmt, out=out_f)
            c.image_to_yuv(image, "yuyv", out=out_i)
        torch.cuda.synchronize()
        frames.copy_(_dev(f8, c)); image.copy_(_dev(img, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(host(o), w) for o, w in zip(out_f, want_f)) and all(np.array_equal(host(o), w) for o, w in zip(out_i, want_i))
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def _dst(fmt, matrix, W, H, planes, pitches, strides):
    d = aefft.YuvDst()
    d.format, d.matrix, d.W, d.H = fmt, matrix, W, H
    for k in range(3):
        d.plane[k], d.pitch[k], d.stride[k] = planes[k], pitches[k], strides[k]
    return d


def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    B, W, H, Nx, Ny = 2, 12, 10, 16, 12
    Wc, Hc = 6, 5
    dev = f"cuda:{ctx.device}"
    ybuf = torch.full((B * W * H * 2 + 64,), 0x3C, dtype=torch.uint8, device=dev)           # (room for YUYV rows too)
    cbuf = torch.full((2 * B * Wc * Hc * 2 + 64,), 0x3C, dtype=torch.uint8, device=dev)
    frm = torch.full((4 * B * 3 * Nx * Ny + 64,), 0xC3, dtype=torch.uint8, device=dev)
    img = torch.full((B * H * W * 3 + 64,), 0xC3, dtype=torch.uint8, device=dev)
    yp, cp, fp, ip = ybuf.data_ptr(), cbuf.data_ptr(), frm.data_ptr(), img.data_ptr()
    vp = cp + B * Wc * Hc * 2
    assert fp % 16 == 0
    NV12, I420, YUYV, LIN, AREA = 0, 1, 2, 0, 1
    nv = dict(fmt=NV12, matrix=0, W=W, H=H, planes=[yp, cp, None], pitches=[W, 2 * Wc, 0], strides=[W * H, 2 * Wc * Hc, 0])
    i4 = dict(fmt=I420, matrix=0, W=W, H=H, planes=[yp, cp, vp], pitches=[W, Wc, Wc], strides=[W * H, Wc * Hc, Wc * Hc])
    yu = dict(fmt=YUYV, matrix=0, W=W, H=H, planes=[yp, None, None], pitches=[2 * W, 0, 0], strides=[2 * W * H, 0, 0])

    def var(base, **kw):
        d = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        for k, v in kw.items():
            if isinstance(v, dict):
                for i, x in v.items():
                    d[k][i] = x
            else:
                d[k] = v
        return _dst(**d)

    # (frames, u8, Nx, Ny, mode, order, descriptor, B | image, pitch, stride, order, descriptor, B); None for the descriptor: a null one
    rf = lambda d, order=0, mode=LIN, f=fp, u8=1, b=B, nx=Nx, ny=Ny: ("r", d, lambda ref: (f, u8, nx, ny, mode, order, ref, b))
    im = lambda d, order=0, i=ip, pitch=W * 3, stride=W * H * 3, b=B: ("i", d, lambda ref: (i, pitch, stride, order, ref, b))
    NULL_R, NULL_I = "null context, descriptor or frames", "null context, descriptor or image"
    PLANE = "null plane (NV12 needs plane[0..1], I420 plane[0..2], YUYV plane[0])"
    FORMAT, MATRIX = "format must be AEFFT_YUV_NV12, AEFFT_YUV_I420 or AEFFT_YUV_YUYV", "matrix must be AEFFT_YUV_BT601, AEFFT_YUV_BT709 or AEFFT_YUV_JPEG"
    ORDER, EVEN = "order must be AEFFT_YUV_BGR, AEFFT_YUV_RGB or AEFFT_YUV_GRAY", "YUYV needs an even W"
    RANGE, FRANGE = "B must be >= 1 and W, H in 1..8192", "Nx, Ny must be in 1..8192"
    MODE, AREA_RULE = "mode must be AEFFT_RESIZE_LINEAR or AEFFT_RESIZE_AREA", "AEFFT_RESIZE_AREA does not enlarge: it needs W <= Nx and H <= Ny"
    PPITCH = "pitch too small: pitch[0] >= W (YUYV 2 W), NV12 pitch[1] >= 2 ceil(W / 2), I420 pitch[1], pitch[2] >= ceil(W / 2)"
    PSTRIDE = "stride too small: each used stride[k] must be at least (rows - 1) * pitch[k] + the live bytes of a row for B > 1"
    ROWS_FIT, BATCH_FIT = "rows * pitch does not fit the address space", "B * stride does not fit the address space"
    IPITCH, ISTRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ALIGN = "frames_d must be 16-byte aligned"
    PLANES, SOURCE = "two destination planes' byte ranges overlap", "a destination plane and the source range overlap (the op is out-of-place)"
    cases = [
        ("null descriptor", rf(None), NULL_R), ("null descriptor", im(None), NULL_I),
        ("null frames", rf(var(nv), f=None), NULL_R), ("null image", im(var(nv), i=None), NULL_I),
        ("null luma", rf(var(nv, planes={0: None})), PLANE), ("null chroma", im(var(nv, planes={1: None})), PLANE),
        ("null chroma with GRAY", im(var(nv, planes={1: None}), order=2, pitch=W, stride=W * H), PLANE), ("null V", rf(var(i4, planes={2: None})), PLANE),
        ("format = 3", rf(var(nv, fmt=3)), FORMAT), ("format = -1", im(var(nv, fmt=-1)), FORMAT),
        ("matrix = 3", rf(var(nv, matrix=3)), MATRIX), ("order = 3", rf(var(nv), order=3), ORDER), ("order = -1", im(var(nv), order=-1), ORDER),
        ("mode = 2", rf(var(nv), mode=2), MODE),
        ("B = 0", rf(var(nv), b=0), RANGE), ("W = 0", im(var(nv, W=0)), RANGE), ("H = 8193", rf(var(nv, H=8193), b=1), RANGE),
        ("Nx = 0", rf(var(nv), nx=0), FRANGE), ("Ny = 8193", rf(var(nv), ny=8193), FRANGE),
        ("YUYV odd W", rf(var(yu, W=W - 1)), EVEN), ("YUYV odd W", im(var(yu, W=W - 1)), EVEN),
        ("luma pitch", rf(var(nv, pitches={0: W - 1})), PPITCH), ("NV12 chroma pitch", im(var(nv, pitches={1: 2 * Wc - 1})), PPITCH),
        ("I420 V pitch", rf(var(i4, pitches={2: Wc - 1})), PPITCH), ("YUYV pitch", rf(var(yu, pitches={0: 2 * W - 1})), PPITCH),
        ("luma stride", rf(var(nv, strides={0: W * H - 1})), PSTRIDE), ("chroma stride", im(var(nv, strides={1: 0})), PSTRIDE),
        ("image pitch", im(var(nv), pitch=W * 3 - 1), IPITCH), ("image stride", im(var(nv), stride=W * H * 3 - 1), ISTRIDE),
        ("AREA enlarging x", rf(var(nv), mode=AREA, nx=W - 1), AREA_RULE), ("AREA enlarging y", rf(var(nv), mode=AREA, ny=H - 1), AREA_RULE),
        ("frames off by 4", rf(var(nv), f=fp + 4, u8=0), ALIGN),
        ("planes: chroma inside the luma plane", rf(var(nv, planes={1: yp + 16})), PLANES),
        ("planes: V over U's second image only", im(var(i4, planes={2: cp + Wc * Hc + 3})), PLANES),
        ("planes: V is U", rf(var(i4, planes={2: cp})), PLANES),
        ("source: the luma plane inside the frames", rf(var(nv, planes={0: fp + 16})), SOURCE),
        ("source: the chroma plane inside the float frames", rf(var(nv, planes={1: fp + 4 * 3 * Nx * Ny + 64}), u8=0), SOURCE),
        ("source: the second image's V plane only", rf(var(i4, planes={2: fp - Wc * Hc - 2})), SOURCE),
        ("source: the image inside the luma plane", im(var(nv), i=yp + 8, pitch=W, stride=W * H, order=2), SOURCE),
        ("rows * pitch overflows", rf(var(nv, pitches={0: 2 ** 62}), b=1), ROWS_FIT),
        ("B * stride overflows", rf(var(nv, strides={0: 2 ** 63 + 8})), BATCH_FIT),
    ]
    for what, (kind, d, args), rule in cases:
        ref = None if d is None else C.byref(d)
        name, rc = ("aefft_frames_resize_to_yuv", L.aefft_frames_resize_to_yuv(ctx.h, *args(ref))) if kind == "r" else ("aefft_image_to_yuv", L.aefft_image_to_yuv(ctx.h, *args(ref)))
        assert rc == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == name + ": " + rule, (what, msg)
    ctx.sync()
    assert (host(ybuf) == 0x3C).all() and (host(cbuf) == 0x3C).all() and (host(frm) == 0xC3).all() and (host(img) == 0xC3).all()
    # what is NOT an error: strides of any value for one image; the smallest legal strides; a batch of NV12 surfaces, each chroma plane between two lumas
    surf = torch.full((B * (H + Hc) * W + 64,), 0x3C, dtype=torch.uint8, device=dev)
    assert L.aefft_frames_resize_to_yuv(ctx.h, fp, 1, Nx, Ny, LIN, 0, C.byref(var(nv, planes={0: surf.data_ptr(), 1: surf.data_ptr() + H * W}, strides={0: 0, 1: 0})), 1) == aefft.OK
    one = var(nv, planes={0: surf.data_ptr(), 1: surf.data_ptr() + H * W}, strides={0: (H + Hc) * W, 1: (H + Hc) * W})
    assert L.aefft_frames_resize_to_yuv(ctx.h, fp, 1, Nx, Ny, AREA, 0, C.byref(one), B) == aefft.OK
    assert L.aefft_image_to_yuv(ctx.h, ip, W * 3, W * H * 3, 0, C.byref(one), B) == aefft.OK
    ctx.sync()
    px = np.full((B, H, W, 3), 0xC3, np.uint8)                                                                       # (a constant source: constant planes)
    y, uv = R.image_to_yuv(px, "nv12")
    s = host(surf)[:B * (H + Hc) * W].reshape(B, H + Hc, W)
    assert np.array_equal(s[:, :H], y) and np.array_equal(s[:, H:].reshape(B, Hc, Wc, 2), uv) and (host(surf)[B * (H + Hc) * W:] == 0x3C).all()
    assert len(np.unique(y)) == 1 and len(np.unique(uv)) == 1
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    yv = ybuf[:B * H * W].view(B, H, W)
    uvv = cbuf[:B * Hc * Wc * 2].view(B, Hc, Wc, 2)
    image = img[:B * H * W * 3].view(B, H, W, 3)
    frames = frm[:B * 3 * Nx * Ny].view(B, 3, Nx, Ny)
    with pytest.raises(ValueError):
        ctx.image_to_yuv(image, "nv12", out=(yv.permute(0, 2, 1), uvv))
    with pytest.raises(ValueError):
        ctx.image_to_yuv(image, "nv12", out=(yv, uvv[:, :, :, :1]))
    with pytest.raises(ValueError):
        ctx.image_to_yuv(image, "nv12", order="gray")
    with pytest.raises(ValueError):
        ctx.image_to_yuv(image[:, :, :11], "yuyv")
    with pytest.raises(ValueError):
        ctx.frames_resize_to_yuv(frames, (W, H), "nv12", mode="cubic")
    with pytest.raises(ValueError):
        ctx.frames_resize_to_yuv(frames, (W, H), "nv12", matrix="bt2020")
    with pytest.raises(ValueError):
        ctx.frames_resize_to_yuv(frames, (W + 2, H), "nv12", out=(yv, uvv))
    with pytest.raises(aefft.AefftError, match="AEFFT_RESIZE_AREA"):
        ctx.frames_resize_to_yuv(frames, (Nx + 2, H), "nv12", mode="area")
    ctx.sync()
    assert (host(ybuf) == 0x3C).all() and (host(cbuf) == 0x3C).all()


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
def test_each_call_is_one_image_launch_with_its_bytes(ctx):
    B, W, H, Nx, Ny = 2, 131, 71, 66, 34
    Wc, Hc = 66, 36
    f8, f32 = ctx.empty(B, 3, Nx, Ny, dtype=torch.uint8), ctx.empty(B, 3, Nx, Ny, dtype=torch.float32)
    g8 = ctx.empty(B, 1, Nx, Ny, dtype=torch.uint8)
    img = ctx.empty(B, H, W, 3, dtype=torch.uint8)
    calls = [
        (lambda: ctx.frames_resize_to_yuv(f8, (W, H), "nv12"), B * (3 * Nx * Ny + W * H + 2 * Wc * Hc)),
        (lambda: ctx.frames_resize_to_yuv(f32, (Nx, Ny), "i420", mode="area"), B * (12 * Nx * Ny + Nx * Ny + 2 * (Nx // 2) * (Ny // 2))),
        (lambda: ctx.frames_resize_to_yuv(g8, (W, H), "nv12", order="gray"), B * (Nx * Ny + W * H + 2 * Wc * Hc)),
        (lambda: ctx.frames_resize_to_yuv(f8, (W + 1, H), "yuyv"), B * (3 * Nx * Ny + 2 * (W + 1) * H)),
        (lambda: ctx.image_to_yuv(img, "nv12"), B * (3 * W * H + W * H + 2 * Wc * Hc)),
    ]
    ctx.prof_enable(); ctx.prof_reset()
    try:
        total = 0
        for k, (call, n) in enumerate(calls):
            call()
            got = ctx.prof_read()
            total += n
            assert got["image"]["launches"] == k + 1 and got["image"]["bytes"] == total, (k, got["image"], total)
            assert sum(v["launches"] for v in got.values()) == k + 1
    finally:
        ctx.prof_enable(False)
