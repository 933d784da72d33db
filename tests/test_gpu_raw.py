"""aefft_raw_to_image (Context.raw_to_image) on the device -- EXACT equality with the numpy restatement of bayer_ref.py everywhere: every pattern,
method and container over the sizes at which the kernel can go wrong (the smallest, odd ones, a tile plus two each way, several tiles with
remainders), one and three images in padded layouts with canary bytes; the word and the byte route; levels and gains that reach both clamps; a
colour matrix with negative entries and the null one against the identity; the table route; PACKED against U16; the call's image fed to
image_resize_to_frames; one graph capture and replay; every AEFFT_EINVAL rule; the profile entry."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import bayer_ref as R
from test_gpu_fft_path import host
from test_gpu_resize import oracle

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16                                  # bayer_kernels.hip BA_TW, BA_TH
SIZES = [(4, 4), (5, 7), (TILE_W + 2, TILE_H + 2), (131, 37)]
CONTAINERS = [("u8", 8), ("u16", 10), ("u16", 12), ("u16", 16), ("packed", 10), ("packed", 12)]
CASES = [(p, m) for p in R.PATTERNS for m in R.METHODS if p != "mono" or m == "mhc"]
CCM = [1.6, -0.45, -0.15, -0.3, 1.55, -0.25, 0.05, -0.7, 1.65]      # a camera's matrix: rows sum to 1, negative entries
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _levels(bits, k):
    """k = 0 the plain levels; 1 a black level, a white below the top and gains; 2 a narrow window with gains 64 (MONO's too) and 0: both clamps everywhere"""
    top = (1 << bits) - 1
    return [(0, top, (1.0, 1.0, 1.0)), (top // 16, top - top // 8, (1.9, 1.0, 1.4)), (top // 3, top // 3 + 3, (64.0, 0.0, 0.37))][k]


@functools.lru_cache(maxsize=None)
def _samples(bits, B, W, H):
    s = np.random.default_rng(bits + 3 * B + 7 * W + 11 * H).integers(0, 1 << bits, (B, H, W))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _want(bits, B, W, H, pattern, method, levels=0, order="bgr", ccm=False, lut=None):
    """the restatement's pixels [B][H][W][D]: computed once, shared and left unchanged"""
    black, white, gains = _levels(bits, levels)
    table = None if lut is None else (R.srgb_lut() if lut == "srgb" else R.gamma_lut(lut))
    img = R.raw_to_image(_samples(bits, B, W, H), pattern, black, white, gains, method, order, CCM if ccm else None, table)
    img.setflags(write=False)
    return img


def _row_bytes(samples, container, bits):
    """the rows [B][H][live bytes] as the container holds them"""
    if container == "u8":
        return samples.astype(np.uint8)
    if container == "u16":
        return np.ascontiguousarray(samples.astype("<u2")).view(np.uint8).reshape(samples.shape[:2] + (-1,))
    return R.pack(samples, bits)


def _source(ctx, samples, container, bits, kind="pad"):
    """the device tensor Context.raw_to_image takes, a view into a flat allocation of random bytes: kind "pad" a pitch rounded up to 64 and a batch
    stride beyond the image from an aligned base (the word route); "odd" pitch live + 5 (U16: + 6) from a base off by one byte (U16: two): the
    byte route"""
    rows = _row_bytes(samples, container, bits)
    B, H, live = rows.shape
    two = container == "u16"
    pitch = (live + 63) // 64 * 64 if kind == "pad" else live + (6 if two else 5)
    off = 0 if kind == "pad" else (2 if two else 1)
    stride = H * pitch + (32 if kind == "pad" else (6 if two else 7))
    flat = np.random.default_rng(live + H).integers(0, 256, (off + B * stride + 33) // 2 * 2, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(flat[off:], rows.shape, (stride, pitch, 1))[...] = rows
    dev = torch.as_tensor(flat, device=f"cuda:{ctx.device}")
    if two:
        return torch.as_strided(dev.view(torch.int16), (B, H, live // 2), (stride // 2, pitch // 2, 1), off // 2)
    return torch.as_strided(dev, (B, H, live), (stride, pitch, 1), off)


def _dest(ctx, B, W, H, D, kind="pad"):
    """(out [B][H][W][D] as a view, the whole allocation, (off, stride, pitch)): canary bytes 0x5A beyond W * D of each row, between the images and
    around the destination; "pad": everything a multiple of 4 (dword stores), "odd": a base off by one byte and an odd pitch (byte stores)"""
    pitch = (W * D + 3) // 4 * 4 + 8 if kind == "pad" else (W * D + 5) | 1
    off = 16 if kind == "pad" else 1
    stride = H * pitch + (16 if kind == "pad" else 3)
    raw = torch.full((off + B * stride + GUARD,), 0x5A, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    return torch.as_strided(raw, (B, H, W, D), (stride, pitch, D, 1), off), raw, (off, stride, pitch)


def _check(out, raw, lay, want, tag):
    off, stride, pitch = lay
    got = host(out)
    print(tag, "mismatches", int((got != want).sum()))
    assert np.array_equal(got, want), tag
    touched = host(raw).copy()
    np.lib.stride_tricks.as_strided(touched[off:], want.shape, (stride, pitch, want.shape[-1], 1))[...] = 0x5A
    assert (touched == 0x5A).all(), (tag, "bytes outside the pixels were written")


def _kw(container, bits, levels=0):
    black, white, gains = _levels(bits, levels)
    return dict(bits=bits, packed=container == "packed", black=black, white=white, gains=gains)


# ------------------------------------------------------------------------------------------
# 1. the sweep
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,method", CASES, ids=lambda v: v)
def test_device_bytes_equal_the_restatement(ctx, pattern, method):
    D = 1 if pattern == "mono" else 3
    n = 0
    for container, bits in CONTAINERS:
        for (W, H) in SIZES:
            for B in (1, 3):
                n += 1
                levels = n % 3
                src = _source(ctx, _samples(bits, B, W, H), container, bits)
                assert not src.is_contiguous()
                out, raw, lay = _dest(ctx, B, W, H, D)
                assert ctx.raw_to_image(src, pattern, method=method, out=out, **_kw(container, bits, levels)) is out
                ctx.sync()
                _check(out, raw, lay, _want(bits, B, W, H, pattern, method, levels), (pattern, method, container, bits, W, H, B, levels))


# ------------------------------------------------------------------------------------------
# 2. the two routes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container,bits", CONTAINERS, ids=lambda v: str(v))
def test_word_and_byte_routes_give_the_same_bytes(ctx, container, bits):
    B, W, H = 3, 131, 37
    for pattern, method in (("grbg", "mhc"), ("gbrg", "bilinear"), ("mono", "mhc")):
        D = 1 if pattern == "mono" else 3
        want = _want(bits, B, W, H, pattern, method, 1)
        got = {}
        for skind, dkind in (("pad", "pad"), ("odd", "odd"), ("pad", "odd"), ("odd", "pad")):
            src = _source(ctx, _samples(bits, B, W, H), container, bits, skind)
            es = src.element_size()
            aligned = src.data_ptr() % 4 == 0 and (src.stride(1) * es) % 4 == 0 and (src.stride(0) * es) % 4 == 0
            assert aligned == (skind == "pad")
            out, raw, lay = _dest(ctx, B, W, H, D, dkind)
            assert (out.data_ptr() % 4 == 0 and out.stride(1) % 4 == 0 and out.stride(0) % 4 == 0) == (dkind == "pad")
            ctx.raw_to_image(src, pattern, method=method, out=out, **_kw(container, bits, 1))
            ctx.sync()
            _check(out, raw, lay, want, (pattern, method, container, bits, skind, dkind))
            got[skind, dkind] = host(out)
        assert all(np.array_equal(g, got["pad", "pad"]) for g in got.values())


# ------------------------------------------------------------------------------------------
# 3. levels, matrix, table, PACKED == U16
# ------------------------------------------------------------------------------------------
def test_levels_and_gains_that_reach_both_clamps(ctx):
    B, W, H = 1, 131, 37
    for container, bits in (("u8", 8), ("u16", 12), ("packed", 10)):
        for pattern in ("rggb", "mono"):
            want = _want(bits, B, W, H, pattern, "mhc", 2)
            assert want.min() == 0 and want.max() == 255
            got = ctx.raw_to_image(_source(ctx, _samples(bits, B, W, H), container, bits), pattern, **_kw(container, bits, 2))
            ctx.sync()
            assert np.array_equal(host(got), want), (container, bits, pattern)
    # the identity of the 8-bit case: every pixel's native channel is its raw byte
    s = _samples(8, 1, 131, 37)
    dev = ctx.raw_to_image(_source(ctx, s, "u8", 8), "bggr", order="rgb")
    ctx.sync()
    got = host(dev)
    assert np.array_equal(np.take_along_axis(got, np.broadcast_to(R.colour_map("bggr", 131, 37), s.shape)[..., None], axis=-1)[..., 0], s)


def test_colour_matrix_with_negative_entries_and_the_null_one(ctx):
    B, W, H, bits = 3, 66, 18, 12
    src = _source(ctx, _samples(bits, B, W, H), "u16", bits)
    for method in R.METHODS:
        for order in ("bgr", "rgb"):
            want = _want(bits, B, W, H, "gbrg", method, 1, order, True)
            got = ctx.raw_to_image(src, "gbrg", method=method, order=order, ccm=CCM, **_kw("u16", bits, 1))
            ctx.sync()
            assert np.array_equal(host(got), want), (method, order)
        assert not np.array_equal(_want(bits, B, W, H, "gbrg", method, 1, "bgr", True), _want(bits, B, W, H, "gbrg", method, 1))
        none = ctx.raw_to_image(src, "gbrg", method=method, **_kw("u16", bits, 1))
        eye = ctx.raw_to_image(src, "gbrg", method=method, ccm=np.eye(3), **_kw("u16", bits, 1))
        ctx.sync()
        assert torch.equal(none, eye) and np.array_equal(host(none), _want(bits, B, W, H, "gbrg", method, 1))


def test_table_route(ctx):
    B, W, H, bits = 3, 131, 37, 12
    src = _source(ctx, _samples(bits, B, W, H), "packed", bits)
    for pattern in ("rggb", "mono"):
        for name, table in (("srgb", aefft.srgb_lut()), (2.2, aefft.gamma_lut())):
            want = _want(bits, B, W, H, pattern, "mhc", 1, "bgr", pattern != "mono", name)
            got = ctx.raw_to_image(src, pattern, ccm=CCM, lut=table, **_kw("packed", bits, 1))
            ctx.sync()
            assert np.array_equal(host(got), want), (pattern, name)
    # a table on the device at an odd address, shorter than 4096 entries would be refused: exactly 4096 bytes, the last 15 never read
    flat = torch.zeros(4097, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    flat[1:] = torch.as_tensor(aefft.srgb_lut(), device=flat.device)
    flat[4082:] = 7                                                              # entries above 4080: whatever they hold
    got = ctx.raw_to_image(src, "rggb", ccm=CCM, lut=flat[1:], **_kw("packed", bits, 1))
    ctx.sync()
    assert flat[1:].data_ptr() % 2 == 1 and np.array_equal(host(got), _want(bits, B, W, H, "rggb", "mhc", 1, "bgr", True, "srgb"))


def test_packed_equals_u16_on_the_device(ctx):
    B, W, H = 3, 131, 37
    for bits in (10, 12):
        s = _samples(bits, B, W, H)
        for pattern, method in (("rggb", "mhc"), ("bggr", "bilinear"), ("mono", "mhc")):
            a = ctx.raw_to_image(_source(ctx, s, "packed", bits), pattern, method=method, **_kw("packed", bits, 1))
            b = ctx.raw_to_image(_source(ctx, s, "u16", bits, "odd"), pattern, method=method, **_kw("u16", bits, 1))
            ctx.sync()
            assert torch.equal(a, b), (bits, pattern, method)


# ------------------------------------------------------------------------------------------
# 4. into the resize; a captured call
# ------------------------------------------------------------------------------------------
def test_the_image_feeds_image_resize_to_frames(ctx):
    B, W, H, bits, Nx, Ny = 3, 131, 37, 12, 40, 12
    img = ctx.raw_to_image(_source(ctx, _samples(bits, B, W, H), "packed", bits), "grbg", **_kw("packed", bits, 1))
    for mode in ("linear", "area"):
        w8, _ = oracle(_want(bits, B, W, H, "grbg", "mhc", 1), (Nx, Ny), mode)
        frames = ctx.image_resize_to_frames(img, (Nx, Ny), mode)
        ctx.sync()
        assert frames.dtype == torch.uint8 and np.array_equal(host(frames), w8), mode


def test_the_call_is_captured_once_and_replayed():
    """one launch, no allocation, no synchronisation: a graph of the call on a side stream, a single branch, replayed on new samples gives their bytes"""
    B, W, H, bits = 3, 131, 37, 12
    rows = _row_bytes(_samples(bits, B, W, H), "packed", bits)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        src = torch.zeros(rows.shape, dtype=torch.uint8, device=dev)
        lut = torch.as_tensor(aefft.srgb_lut(), device=dev)
        img = torch.full((B, H, W, 3), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.raw_to_image(src, "rggb", ccm=CCM, lut=lut, out=img, **_kw("packed", bits, 1))
        torch.cuda.synchronize()
        src.copy_(torch.as_tensor(rows, device=dev))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(img), _want(bits, B, W, H, "rggb", "mhc", 1, "bgr", True, "srgb"))
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 5. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(ctx):
    L = ctx.L
    B, W, H = 2, 12, 10
    dev = f"cuda:{ctx.device}"
    sbuf = torch.full((B * 2 * W * H + 64,), 0x3C, dtype=torch.uint8, device=dev)
    img = torch.full((B * H * W * 3 + 64,), 0xC3, dtype=torch.uint8, device=dev)
    lut = torch.full((4096,), 0x77, dtype=torch.uint8, device=dev)
    sp, ip, lp = sbuf.data_ptr(), img.data_ptr(), lut.data_ptr()
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    keep = []

    def desc(pattern=0, container=0, bits=8, W=W, H=H, data=sp, pitch=None, stride=None, black=0, white=None, gain=(1.0, 1.0, 1.0), method=1, ccm=None, lut=None):
        d = aefft.RawDesc()
        live = {0: W, 1: 2 * W, 2: (W * bits + 7) // 8}.get(container, W)
        d.pattern, d.container, d.bits, d.W, d.H, d.data = pattern, container, bits, W, H, data
        d.pitch = live if pitch is None else pitch
        d.stride = d.pitch * H if stride is None else stride
        d.black, d.white, d.method, d.lut_d = black, (1 << bits) - 1 if white is None else white, method, lut
        for k in range(3):
            d.gain[k] = gain[k]
        if ccm is not None:
            arr = (C.c_float * 9)(*ccm)
            keep.append(arr)
            d.ccm = C.cast(arr, C.POINTER(C.c_float))
        return d

    call = lambda d, order=0, i=ip, pitch=W * 3, stride=W * H * 3, b=B: (d, (order, i, pitch, stride, b))
    NULL = "null context, descriptor, data or image"
    PATTERN, CONT = "pattern must be AEFFT_RAW_RGGB, _GRBG, _GBRG, _BGGR or _MONO", "container must be AEFFT_RAW_U8, AEFFT_RAW_U16 or AEFFT_RAW_PACKED"
    METHOD, ORDER = "method must be AEFFT_DEMOSAIC_BILINEAR or AEFFT_DEMOSAIC_MHC", "order must be AEFFT_YUV_BGR or AEFFT_YUV_RGB"
    BITS = "bits must be 8 for AEFFT_RAW_U8, 9..16 for AEFFT_RAW_U16 and 10 or 12 for AEFFT_RAW_PACKED"
    RANGE, EVEN = "B must be >= 1 and W, H in 4..8192", "AEFFT_RAW_U16 needs data, pitch and stride to be multiples of 2"
    PITCH = "pitch too small: U8 pitch >= W, U16 pitch >= 2 W, PACKED pitch >= ceil(W * bits / 8)"
    STRIDE = "stride must be at least (H - 1) * pitch + the live bytes of a row for B > 1"
    ROWS_FIT, BATCH_FIT = "H * pitch does not fit the address space", "B * stride does not fit the address space"
    IPITCH, ISTRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    LEVELS, GAIN = "black and white must satisfy 0 <= black < white <= 2^bits - 1", "every gain must be finite and in 0..64"
    CCM_RULE = "every ccm entry must be finite and below 4 in magnitude"
    OVER_S, OVER_T = "the source and image ranges overlap (the op is out-of-place)", "the table and image ranges overlap"
    cases = [
        ("null descriptor", call(None), NULL), ("null data", call(desc(data=None)), NULL), ("null image", call(desc(), i=None), NULL),
        ("pattern = 5", call(desc(pattern=5)), PATTERN), ("pattern = -1", call(desc(pattern=-1)), PATTERN), ("container = 3", call(desc(container=3)), CONT),
        ("method = 2", call(desc(method=2)), METHOD), ("mono, method = -1", call(desc(pattern=4, method=-1), pitch=W, stride=W * H), METHOD),
        ("order = 2", call(desc(), order=2), ORDER), ("order = -1", call(desc(), order=-1), ORDER),
        ("U8 bits 10", call(desc(bits=10)), BITS), ("U16 bits 8", call(desc(container=1, bits=8)), BITS), ("U16 bits 17", call(desc(container=1, bits=17)), BITS),
        ("PACKED bits 8", call(desc(container=2, bits=8)), BITS), ("PACKED bits 14", call(desc(container=2, bits=14)), BITS),
        ("B = 0", call(desc(), b=0), RANGE), ("W = 3", call(desc(W=3)), RANGE), ("H = 8193", call(desc(H=8193), b=1), RANGE),
        ("U16 odd pointer", call(desc(container=1, bits=12, data=sp + 1)), EVEN), ("U16 odd pitch", call(desc(container=1, bits=12, pitch=2 * W + 1)), EVEN),
        ("U16 odd stride", call(desc(container=1, bits=12, stride=2 * W * H + 1)), EVEN),
        ("U8 pitch", call(desc(pitch=W - 1)), PITCH), ("U16 pitch", call(desc(container=1, bits=12, pitch=2 * W - 2)), PITCH),
        ("PACKED pitch", call(desc(container=2, bits=10, pitch=14)), PITCH), ("stride", call(desc(stride=W * H - 1)), STRIDE),
        ("rows * pitch overflows", call(desc(pitch=2 ** 62), b=1), ROWS_FIT), ("B * stride overflows", call(desc(stride=2 ** 63 + 8)), BATCH_FIT),
        ("image pitch", call(desc(), pitch=W * 3 - 1), IPITCH), ("image stride", call(desc(), stride=W * H * 3 - 1), ISTRIDE),
        ("mono image pitch", call(desc(pattern=4), pitch=W - 1, stride=W * H), IPITCH),
        ("black = white", call(desc(black=7, white=7)), LEVELS), ("black < 0", call(desc(black=-1)), LEVELS), ("white = 2^bits", call(desc(white=256)), LEVELS),
        ("white beyond 10 bits", call(desc(container=2, bits=10, white=1024)), LEVELS),
        ("gain nan", call(desc(gain=(1.0, nan, 1.0))), GAIN), ("gain < 0", call(desc(gain=(-0.5, 1.0, 1.0))), GAIN), ("gain 65", call(desc(gain=(1.0, 1.0, 65.0))), GAIN),
        ("gain inf", call(desc(gain=(inf, 1.0, 1.0))), GAIN),
        ("ccm nan", call(desc(ccm=eye[:4] + [nan] + eye[5:])), CCM_RULE), ("ccm = 4", call(desc(ccm=eye[:8] + [4.0])), CCM_RULE),
        ("ccm = -4", call(desc(ccm=[-4.0] + eye[1:])), CCM_RULE),
        ("overlap: image inside the source", call(desc(), i=sp + 8, pitch=W * 3, stride=W * H * 3), OVER_S),
        ("overlap: source behind the image's start", call(desc(data=ip + 16)), OVER_S),
        ("overlap: the table inside the image", call(desc(lut=ip + 32)), OVER_T),
    ]
    for what, (d, args), rule in cases:
        rc = L.aefft_raw_to_image(ctx.h, None if d is None else C.byref(d), *args)
        assert rc == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_raw_to_image: " + rule, (what, msg)
    # what is NOT an error: any stride for one image; the smallest legal stride; a mono source with gains and a matrix that a Bayer call would refuse
    one = torch.full((H * W * 3,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_raw_to_image(ctx.h, C.byref(desc(stride=1)), 0, one.data_ptr(), W * 3, 0, 1) == aefft.OK
    two = torch.full((B * H * W,), 0xEE, dtype=torch.uint8, device=dev)
    assert L.aefft_raw_to_image(ctx.h, C.byref(desc(pattern=4, stride=(H - 1) * W + W, gain=(1.0, nan, 99.0), ccm=[9.0] * 9)), 7, two.data_ptr(), W, W * H, B) == aefft.OK
    ctx.sync()
    assert (host(sbuf) == 0x3C).all() and (host(img) == 0xC3).all() and (host(lut) == 0x77).all()
    assert (host(one) == 0x3C).all() and (host(two) == 0x3C).all()                # (a constant mosaic gives a constant image; 8-bit identity)
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    s = sbuf[:B * H * W].view(B, H, W)
    with pytest.raises(ValueError):
        ctx.raw_to_image(s.permute(0, 2, 1), "rggb")
    with pytest.raises(ValueError):
        ctx.raw_to_image(s, "rggb", out=ctx.empty(B, H, W, 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ctx.raw_to_image(s, "rggb", lut=np.zeros(256, dtype=np.uint8))
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.raw_to_image(s, "mono", out=s.unsqueeze(-1))


# ------------------------------------------------------------------------------------------
# 6. profile accounting
# ------------------------------------------------------------------------------------------
def test_the_call_is_one_image_launch_with_its_bytes(ctx):
    B, W, H = 2, 131, 71
    dev = f"cuda:{ctx.device}"
    u8 = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
    u16 = torch.zeros(B, H, W, dtype=torch.int16, device=dev)
    p12 = torch.zeros(B, H, (W * 12 + 7) // 8, dtype=torch.uint8, device=dev)
    p10 = torch.zeros(B, H, (W * 10 + 7) // 8, dtype=torch.uint8, device=dev)
    lut = torch.as_tensor(aefft.gamma_lut(), device=dev)
    img, grey = ctx.empty(B, H, W, 3, dtype=torch.uint8), ctx.empty(B, H, W, 1, dtype=torch.uint8)
    calls = [
        (lambda: ctx.raw_to_image(u8, "rggb", out=img), B * H * (W + 3 * W)),
        (lambda: ctx.raw_to_image(u16, "grbg", bits=12, method="bilinear", out=img), B * H * (2 * W + 3 * W)),
        (lambda: ctx.raw_to_image(p12, "bggr", bits=12, packed=True, lut=lut, out=img), B * H * ((W * 12 + 7) // 8 + 3 * W) + 4096),
        (lambda: ctx.raw_to_image(p10, "mono", bits=10, packed=True, out=grey), B * H * ((W * 10 + 7) // 8 + W)),
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
