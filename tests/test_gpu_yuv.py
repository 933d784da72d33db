"""aefft_yuv_to_image and aefft_yuv_resize_to_frames (Context.yuv_to_image, Context.yuv_resize_to_frames) on the device -- EXACT equality
everywhere: the conversion against the numpy restatement of yuv_ref.py (every format and matrix, tight / 64-aligned / odd-based planes with a batch
stride that is not the plane's size, pre-filled outputs with a guard region, random pad bytes, all 65536 chroma pairs with the four luma values
that reach every clamp), the fused call against that restatement followed by test_gpu_resize's oracle (both modes, both frame types), the
composition identity on the device, a net fed from the call, one graph capture and replay, every AEFFT_EINVAL rule, and the profile entry."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import yuv_ref as R
from test_gpu_fft_path import host
from test_gpu_resize import oracle
from test_gpu_sizes import _weights

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

FORMATS, MATRICES = R.FORMATS, R.MATRICES
KINDS = ["tight", "pad64", "odd"]
MODES = ["linear", "area"]
GUARD = 64         # bytes behind an output that must stay as they were
# (W, H) of the plain call: one tile; odd sizes (NV12, I420: the last chroma column and row serve one pixel) / an odd height (YUYV); several blocks
IMAGE_SHAPES = {"nv12": [(8, 8), (11, 9), (130, 70)], "i420": [(8, 8), (11, 9), (130, 70)], "yuyv": [(8, 8), (12, 9), (130, 70)]}
# (B, W, H, Nx, Ny) of the fused call: identity; odd source; enlarging; exact 2x; several tiles with remainders and Ny % 4 == 2; bands of source rows;
# the camera case; a thumbnail of 1080p (AREA's 64-bit sum, many bands); ONE tile whose rows are so wide that a band holds 5 of the 50 (LINEAR) or
# 64 (AREA) source rows it needs (yv_geometry: P = 1465 / 1537, RB = 5): every sum runs across ten bands or more
RESIZE_SHAPES = [(1, 8, 8, 8, 8), (2, 11, 9, 8, 8), (1, 6, 4, 16, 8), (2, 64, 64, 32, 32), (1, 130, 70, 66, 34), (1, 200, 150, 10, 12), (2, 640, 480, 256, 256),
                 (1, 1920, 1080, 64, 64), (1, 2048, 64, 21, 4)]
RESIZE_CASES = [(s, f, m) for s in RESIZE_SHAPES for f in FORMATS for m in MODES
                if (f != "yuyv" or s[1] % 2 == 0) and (m == "linear" or (s[3] <= s[1] and s[4] <= s[2]))]


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _ids(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def _planes(fmt, B, W, H):
    p = R.random_planes(np.random.default_rng(B + 3 * W + 7 * H + len(fmt)), fmt, B, W, H)
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _image(fmt, B, W, H, matrix, order):
    """the restatement's pixels [B][H][W][D]: computed once, shared and left unchanged"""
    img = R.yuv_to_image(_planes(fmt, B, W, H), fmt, matrix, order)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _frames(fmt, shape, mode, matrix="bt601", order="bgr"):
    B, W, H, Nx, Ny = shape
    w8, w32 = oracle(_image(fmt, B, W, H, matrix, order), (Nx, Ny), mode)
    w8.setflags(write=False); w32.setflags(write=False)
    return w8, w32


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")


def _plane_view(a, kind, ctx, seed):
    """the plane [B][rows][...] inside a flat allocation of random bytes, as a device view of the plane's shape: pitch tight, rounded up to 64, or
    live + 5 from a base off by one byte (the byte route); a batch stride that is not rows * pitch; pad bytes and tail random"""
    B, rows = a.shape[:2]
    live = int(np.prod(a.shape[2:]))
    pitch = {"tight": live, "pad64": (live + 63) // 64 * 64, "odd": live + 5}[kind]
    off = 1 if kind == "odd" else 0
    stride = rows * pitch + (7 if kind == "odd" else 32)
    flat = np.random.default_rng(seed).integers(0, 256, off + B * stride + 32, dtype=np.uint8)
    inner = tuple(int(np.prod(a.shape[k + 1:])) for k in range(2, a.ndim))
    np.lib.stride_tricks.as_strided(flat[off:], a.shape, (stride, pitch) + inner)[...] = a
    return torch.as_strided(_dev(flat, ctx), a.shape, (stride, pitch) + inner, off)


def _views(planes, kind, ctx):
    """the planes' device views.  tight and pad64: every plane alike (pad64: the dword route whatever W is); odd: the planes alternate between
    the odd base and pad64, so that one call mixes pitches (the byte route)"""
    return tuple(_plane_view(a, "pad64" if kind == "odd" and k % 2 else kind, ctx, seed=11 + k) for k, a in enumerate(planes))


def _guarded(ctx, shape, dtype, fill):
    """(out of `shape` pre-filled, the whole allocation as bytes, bytes of out): GUARD bytes of 0x5A behind it"""
    nbytes = int(np.prod(shape)) * (4 if dtype == torch.float32 else 1)
    raw = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    assert raw.data_ptr() % 16 == 0
    out = raw[:nbytes].view(dtype).view(*shape)
    out.fill_(fill)
    return out, raw, nbytes


# ------------------------------------------------------------------------------------------
# 1. yuv_to_image
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt,size", [(f, s) for f in FORMATS for s in IMAGE_SHAPES[f]], ids=_ids)
def test_image_equals_the_integer_formula(ctx, fmt, size, kind):
    B, (W, H) = 2, size
    src = _views(_planes(fmt, B, W, H), kind, ctx)
    if kind != "tight":
        assert any(v.stride(0) != v.shape[1] * v.stride(1) for v in src) and not src[0].is_contiguous()
    for matrix in MATRICES:
        want = _image(fmt, B, W, H, matrix, "bgr")
        for fill in (0xEE, 0x11):                                               # (either is a legal pixel: the same again over the complement)
            out, raw, n = _guarded(ctx, (B, H, W, 3), torch.uint8, fill)
            assert ctx.yuv_to_image(src, fmt, matrix, "bgr", out=out) is out
            ctx.sync()
            got = host(out)
            print(fmt, size, kind, matrix, "mismatches", int((got != want).sum()))
            assert np.array_equal(got, want), (fmt, size, kind, matrix)
            assert (host(raw)[n:] == 0x5A).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_image_orders_a_padded_destination_and_one_image_without_the_batch_axis(ctx, fmt):
    B, W, H = 2, 130, 70
    planes = _planes(fmt, B, W, H)
    src = _views(planes, "odd", ctx)
    for matrix, order in (("bt709", "rgb"), ("bt601", "gray"), ("jpeg", "gray")):
        want = _image(fmt, B, W, H, matrix, order)
        D = want.shape[-1]
        # a destination with a pitch of W D + 5 from an odd base and a batch stride beyond the image: bytes outside the pixels stay
        pitch, stride = W * D + 5, H * (W * D + 5) + 3
        raw = torch.full((1 + B * stride + GUARD,), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        out = torch.as_strided(raw, (B, H, W, D), (stride, pitch, D, 1), 1)
        use = src[:1] if order == "gray" and fmt != "yuyv" else src             # (gray: the luma plane alone is enough)
        ctx.yuv_to_image(use, fmt, matrix, order, out=out)
        ctx.sync()
        assert np.array_equal(host(out), want), (fmt, matrix, order)
        touched = host(raw).copy()
        np.lib.stride_tricks.as_strided(touched[1:], (B, H, W, D), (stride, pitch, D, 1))[...] = 0x5A
        assert (touched == 0x5A).all(), (fmt, matrix, order, "bytes outside the pixels were written")
    fresh = ctx.yuv_to_image(tuple(_dev(a[1], ctx) for a in planes), fmt)
    ctx.sync()
    assert tuple(fresh.shape) == (1, H, W, 3) and fresh.dtype == torch.uint8 and np.array_equal(host(fresh), _image(fmt, B, W, H, "bt601", "bgr")[1:])
    if fmt == "i420":                                                            # YV12: the same call with the two pointers swapped
        yv12 = ctx.yuv_to_image((src[0], src[2], src[1]), fmt, "bt601", "rgb")
        ctx.sync()
        assert np.array_equal(host(yv12), R.yuv_to_image((planes[0], planes[2], planes[1]), fmt, "bt601", "rgb"))


@pytest.mark.parametrize("matrix", MATRICES)
def test_every_chroma_pair_with_the_luma_values_that_reach_every_clamp(ctx, matrix):
    """512 x 512 NV12: the chroma plane enumerates all 65536 (U, V); each 2 x 2 luma block carries 0, 16, 235, 255"""
    u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    uv = np.ascontiguousarray(np.stack([u, v], axis=-1))[None]
    y = np.tile(np.array([[0, 16], [235, 255]], dtype=np.uint8), (256, 256))[None]
    want = R.yuv_to_image((y, uv), "nv12", matrix, "bgr")
    assert want.min() == 0 and want.max() == 255
    got = ctx.yuv_to_image((_dev(y, ctx), _dev(uv, ctx)), "nv12", matrix, "bgr")
    ctx.sync()
    print(matrix, "mismatches", int((host(got) != want).sum()))
    assert np.array_equal(host(got), want)


# ------------------------------------------------------------------------------------------
# 2. yuv_resize_to_frames
# ------------------------------------------------------------------------------------------
def _run_fused(ctx, src, fmt, shape, mode, matrix, order, want8, want32, tag):
    B, W, H, Nx, Ny = shape
    D = want8.shape[1]
    out8, raw8, n8 = _guarded(ctx, (B, D, Nx, Ny), torch.uint8, 0xEE)
    out32, raw32, n32 = _guarded(ctx, (B, D, Nx, Ny), torch.float32, float("nan"))
    assert ctx.yuv_resize_to_frames(src, fmt, (Nx, Ny), matrix, order, mode, out=out8) is out8
    assert ctx.yuv_resize_to_frames(src, fmt, (Nx, Ny), matrix, order, mode, out=out32) is out32
    ctx.sync()
    g8, g32 = host(out8), host(out32)
    print(tag, "8-bit mismatches", int((g8 != want8).sum()), "float mismatches", int((g32.view(np.uint32) != want32.view(np.uint32)).sum()))
    assert g8.dtype == np.uint8 and np.array_equal(g8, want8), tag
    assert g32.dtype == np.float32 and not np.isnan(g32).any() and np.array_equal(g32.view(np.uint32), want32.view(np.uint32)), tag
    assert (host(raw8)[n8:] == 0x5A).all() and (host(raw32)[n32:] == 0x5A).all(), (tag, "guard")
    out8.fill_(0x11)                                                             # 0xEE is a legal pixel: the same again over the complement
    ctx.yuv_resize_to_frames(src, fmt, (Nx, Ny), matrix, order, mode, out=out8)
    ctx.sync()
    assert np.array_equal(host(out8), want8), tag


@pytest.mark.parametrize("shape,fmt,mode", RESIZE_CASES, ids=_ids)
def test_fused_equals_the_conversion_then_the_resize_formulas(ctx, shape, fmt, mode):
    B, W, H, Nx, Ny = shape
    want8, want32 = _frames(fmt, shape, mode)
    kinds = KINDS if W * H < 100000 else [KINDS[(W + len(fmt) + len(mode)) % 3]]      # (the large sources: one layout each, all three over the cases)
    for kind in kinds:
        src = _views(_planes(fmt, B, W, H), kind, ctx)
        _run_fused(ctx, src, fmt, shape, mode, "bt601", "bgr", want8, want32, (shape, fmt, mode, kind))


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_other_matrices_and_orders(ctx, fmt):
    shape = (1, 130, 70, 66, 34)
    B, W, H, Nx, Ny = shape
    planes = _planes(fmt, B, W, H)
    src = _views(planes, "pad64", ctx)
    for matrix, order, mode in (("bt709", "bgr", "linear"), ("jpeg", "bgr", "area"), ("bt601", "rgb", "area"), ("bt709", "gray", "linear"), ("jpeg", "gray", "area")):
        want8, want32 = _frames(fmt, shape, mode, matrix, order)
        use = src[:1] if order == "gray" and fmt != "yuyv" else src
        _run_fused(ctx, use, fmt, shape, mode, matrix, order, want8, want32, (fmt, matrix, order, mode))


@pytest.mark.parametrize("fmt", FORMATS)
def test_composition_identity_on_the_device(ctx, fmt):
    """fused == yuv_to_image -> image_resize_to_frames; at equal sizes == yuv_to_image -> image_to_frames (both modes)"""
    for (B, W, H, Nx, Ny) in ((2, 12, 10, 8, 8), (1, 130, 70, 66, 34), (2, 64, 64, 32, 32), (2, 12, 10, 12, 10), (1, 130, 70, 130, 70)):
        src = tuple(_dev(a, ctx) for a in _planes(fmt, B, W, H))
        for matrix, order in (("bt601", "bgr"), ("bt709", "gray")):
            img = ctx.yuv_to_image(src, fmt, matrix, order)
            for mode in MODES:
                for dtype in (torch.uint8, torch.float32):
                    fused = ctx.yuv_resize_to_frames(src, fmt, (Nx, Ny), matrix, order, mode, dtype=dtype)
                    two = ctx.image_resize_to_frames(img, (Nx, Ny), mode, dtype=dtype)
                    ctx.sync()
                    assert fused.dtype == two.dtype and torch.equal(fused.view(torch.uint8), two.contiguous().view(torch.uint8)), (fmt, W, H, Nx, Ny, matrix, order, mode, dtype)
                    if (Nx, Ny) == (W, H):
                        plain = ctx.image_to_frames(img, dtype=dtype)
                        ctx.sync()
                        assert torch.equal(fused.view(torch.uint8), plain.view(torch.uint8)), (fmt, W, H, matrix, order, mode, dtype)


# ------------------------------------------------------------------------------------------
# 3. a net fed from the call; a captured call
# ------------------------------------------------------------------------------------------
def test_step_grad_u8_on_the_calls_frames_is_bit_for_bit(ctx):
    D, N, B = 3, 64, 2
    W, H = 130, 70
    src = tuple(_dev(a, ctx) for a in _planes("nv12", B, W, H))
    outs = []
    for frames in (lambda: ctx.yuv_resize_to_frames(src, "nv12", (N, N), mode="area"),
                   lambda: ctx.image_resize_to_frames(ctx.yuv_to_image(src, "nv12"), (N, N), "area")):
        net = aefft.Net(ctx, D, N, N, [2], 3, 1, batch=B)
        try:
            for l, w in enumerate(_weights(np.random.default_rng(3), D, [2], 3, 3)):
                net.set_pair(l, *w)
            recon = ctx.empty(B, D, N, N)
            gbuf = net.grad_buffer(); grads = torch.empty_like(gbuf)
            f = frames()
            assert f.dtype == torch.uint8
            net.step_grad(f, recon)                                              # (step_grad_u8, queued behind the call: nothing waits in between)
            grads.copy_(gbuf)
            ctx.sync()
            outs.append((host(recon).copy(), host(grads).copy()))
        finally:
            net.close()
    assert np.isfinite(outs[0][1]).all() and np.abs(outs[0][1]).max() > 0
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


def test_the_calls_are_captured_once_and_replayed():
    """one launch each, no allocation, no synchronisation: a graph of the two calls replayed on new samples gives their bytes"""
    fmt, shape = "nv12", (2, 130, 70, 66, 34)
    B, W, H, Nx, Ny = shape
    planes = _planes(fmt, B, W, H)
    want8, _ = _frames(fmt, shape, "area")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        src = tuple(torch.zeros(a.shape, dtype=torch.uint8, device=f"cuda:{c.device}") for a in planes)
        out = torch.full((B, 3, Nx, Ny), 0xEE, dtype=torch.uint8, device=f"cuda:{c.device}")
        img = torch.full((B, H, W, 3), 0xEE, dtype=torch.uint8, device=f"cuda:{c.device}")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.yuv_resize_to_frames(src, fmt, (Nx, Ny), mode="area", out=out)
            c.yuv_to_image(src, fmt, out=img)
        torch.cuda.synchronize()
        for s, a in zip(src, planes):
            s.copy_(_dev(a, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), want8) and np.array_equal(host(img), _image(fmt, B, W, H, "bt601", "bgr"))
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def _desc(fmt, matrix, W, H, planes, pitches, strides):
    d = aefft.YuvDesc()
    d.format, d.matrix, d.W, d.H = fmt, matrix, W, H
    for k in range(3):
        d.plane[k], d.pitch[k], d.stride[k] = planes[k], pitches[k], strides[k]
    return d


def test_argument_errors_leave_the_outputs_untouched(ctx):
    L = ctx.L
    B, W, H, Nx, Ny = 2, 12, 10, 8, 8
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
        return _desc(**d)

    # (descriptor, order, mode, frames, u8, B, Nx, Ny | image, pitch, stride), the whole message behind the call's name; None for the descriptor: a null one
    rf = lambda d, order=0, mode=LIN, f=fp, u8=1, b=B, nx=Nx, ny=Ny: ("r", d, (order, mode, f, u8, b, nx, ny))
    im = lambda d, order=0, i=ip, pitch=W * 3, stride=W * H * 3, b=B: ("i", d, (order, i, pitch, stride, b))
    # the rules' full texts, as the library words them
    NULL_R, NULL_I = "null context, descriptor or frames", "null context, descriptor or image"
    PLANE = "null plane (NV12 needs plane[0..1], I420 plane[0..2], YUYV and AEFFT_YUV_GRAY plane[0])"
    FORMAT, MATRIX = "format must be AEFFT_YUV_NV12, AEFFT_YUV_I420 or AEFFT_YUV_YUYV", "matrix must be AEFFT_YUV_BT601, AEFFT_YUV_BT709 or AEFFT_YUV_JPEG"
    ORDER, EVEN = "order must be AEFFT_YUV_BGR, AEFFT_YUV_RGB or AEFFT_YUV_GRAY", "YUYV needs an even W"
    RANGE, FRANGE = "B must be >= 1 and W, H in 1..8192", "Nx, Ny must be in 1..8192"
    MODE, AREA_RULE = "mode must be AEFFT_RESIZE_LINEAR or AEFFT_RESIZE_AREA", "AEFFT_RESIZE_AREA does not enlarge: it needs Nx <= W and Ny <= H"
    PPITCH = "pitch too small: pitch[0] >= W (YUYV 2 W), NV12 pitch[1] >= 2 ceil(W / 2), I420 pitch[1], pitch[2] >= ceil(W / 2)"
    PSTRIDE = "stride too small: each used stride[k] must be at least (rows - 1) * pitch[k] + the live bytes of a row for B > 1"
    ROWS_FIT, BATCH_FIT = "rows * pitch does not fit the address space", "B * stride does not fit the address space"
    IPITCH, ISTRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ALIGN = "frames_d must be 16-byte aligned"
    OVERLAP_R, OVERLAP_I = "a source plane and the frame range overlap (the op is out-of-place)", "a source plane and the image range overlap (the op is out-of-place)"
    cases = [
        ("null descriptor", rf(None), NULL_R), ("null descriptor", im(None), NULL_I),
        ("null frames", rf(var(nv), f=None), NULL_R), ("null image", im(var(nv), i=None), NULL_I),
        ("null luma", rf(var(nv, planes={0: None})), PLANE), ("null chroma", im(var(nv, planes={1: None})), PLANE),
        ("null V", rf(var(i4, planes={2: None})), PLANE),
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
        ("AREA enlarging x", rf(var(nv), mode=AREA, nx=W + 1), AREA_RULE), ("AREA enlarging y", rf(var(nv), mode=AREA, ny=H + 1), AREA_RULE),
        ("frames off by 4", rf(var(nv), f=fp + 4, u8=0), ALIGN),
        ("overlap: frames inside the luma plane", rf(var(nv), f=yp + 16), OVERLAP_R),
        ("overlap: the chroma plane inside the float frames", rf(var(nv, planes={1: fp + 64}), u8=0), OVERLAP_R),
        ("overlap: the second image's V plane only", rf(var(i4, planes={2: fp - Wc * Hc - 2})), OVERLAP_R),
        ("overlap: image inside the luma plane", im(var(nv), i=yp + 8, pitch=W, stride=W * H, order=2), OVERLAP_I),
        ("rows * pitch overflows", rf(var(nv, pitches={0: 2 ** 62}), b=1), ROWS_FIT),
        ("B * stride overflows", rf(var(nv, strides={0: 2 ** 63 + 8})), BATCH_FIT),
    ]
    for what, (kind, d, args), rule in cases:
        ref = None if d is None else C.byref(d)
        name, rc = ("aefft_yuv_resize_to_frames", L.aefft_yuv_resize_to_frames(ctx.h, ref, *args)) if kind == "r" else ("aefft_yuv_to_image", L.aefft_yuv_to_image(ctx.h, ref, *args))
        assert rc == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == name + ": " + rule, (what, msg)
    # what is NOT an error: strides of any value for one image; the smallest legal strides; null chroma planes with GRAY
    one = torch.full((3 * Nx * Ny,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_yuv_resize_to_frames(ctx.h, C.byref(var(nv, strides={0: 0, 1: 0})), 0, LIN, one.data_ptr(), 1, 1, Nx, Ny) == aefft.OK
    two = torch.full((B * Nx * Ny,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_yuv_resize_to_frames(ctx.h, C.byref(var(nv, planes={1: None})), 2, AREA, two.data_ptr(), 1, B, Nx, Ny) == aefft.OK
    ctx.sync()
    assert (host(ybuf) == 0x3C).all() and (host(cbuf) == 0x3C).all() and (host(frm) == 0xC3).all() and (host(img) == 0xC3).all()
    px = R.convert(np.array([0x3C]), np.array([0x3C]), np.array([0x3C]), "bt601", "bgr")[0]                          # (a constant source)
    assert (host(one).reshape(3, -1) == px[:, None]).all()
    assert (host(two) == R.convert(np.array([0x3C]), np.array([128]), np.array([128]), "bt601", "gray")[0, 0]).all()
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    y = ybuf[:B * H * W].view(B, H, W)
    uv = cbuf[:B * Hc * Wc * 2].view(B, Hc, Wc, 2)
    with pytest.raises(ValueError):
        ctx.yuv_to_image((y.permute(0, 2, 1), uv), "nv12")
    with pytest.raises(ValueError):
        ctx.yuv_to_image((y, uv[:, :, :, :1]), "nv12")
    with pytest.raises(ValueError):
        ctx.yuv_resize_to_frames((y, uv), "nv12", (Nx, Ny), mode="cubic")
    with pytest.raises(ValueError):
        ctx.yuv_resize_to_frames((y, uv), "nv12", (Nx, Ny), matrix="bt2020")
    with pytest.raises(ValueError):
        ctx.yuv_resize_to_frames((y, uv), "nv12", (Nx, Ny), out=ctx.empty(B, 3, Ny, Nx + 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ctx.yuv_to_image((y, uv), "nv12", out=ctx.empty(B, H, W, 1, dtype=torch.uint8))
    with pytest.raises(aefft.AefftError, match="AEFFT_RESIZE_AREA"):
        ctx.yuv_resize_to_frames((y, uv), "nv12", (W + 1, Ny), mode="area")


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
def test_each_call_is_one_image_launch_with_its_bytes(ctx):
    B, W, H, Nx, Ny = 2, 131, 71, 66, 34
    Wc, Hc = 66, 36
    dev = f"cuda:{ctx.device}"
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)
    nv12, i420, yuyv = (z(B, H, W), z(B, Hc, Wc, 2)), (z(B, H, W), z(B, Hc, Wc), z(B, Hc, Wc)), (z(B, H, W // 2 + 1, 4),)
    f8, f32 = ctx.empty(B, 3, Nx, Ny, dtype=torch.uint8), ctx.empty(B, 3, Nx, Ny, dtype=torch.float32)
    g8 = ctx.empty(B, 1, Nx, Ny, dtype=torch.uint8)
    img = ctx.empty(B, H, W, 3, dtype=torch.uint8)
    calls = [
        (lambda: ctx.yuv_resize_to_frames(nv12, "nv12", (Nx, Ny), out=f8), B * (W * H + 2 * Wc * Hc + 3 * Nx * Ny)),
        (lambda: ctx.yuv_resize_to_frames(i420, "i420", (Nx, Ny), mode="area", out=f32), B * (W * H + 2 * Wc * Hc + 12 * Nx * Ny)),
        (lambda: ctx.yuv_resize_to_frames(nv12, "nv12", (Nx, Ny), order="gray", out=g8), B * (W * H + Nx * Ny)),
        (lambda: ctx.yuv_resize_to_frames(yuyv, "yuyv", (Nx, Ny), out=f8), B * (2 * (W + 1) * H + 3 * Nx * Ny)),
        (lambda: ctx.yuv_to_image(nv12, "nv12", out=img), B * (W * H + 2 * Wc * Hc + 3 * W * H)),
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
