"""aefft_image_to_frames / aefft_frames_to_image (Context.image_to_frames / frames_to_image): ImageToSpin_C and SpinToImage_C on the device,
byte-exact against numpy -- every shape with a tight, an aligned padded and an unaligned pitch (the last from a base off by one byte), 8-bit
and float frames, pad bytes and the bytes behind the last row untouched, the float rule on its edge values and against the inverse row
pass's own 8-bit output, the net calls fed from image_to_frames bit for bit and without synchronisation, errors, and the profile entry."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from frozen_cases import _rule, _weights, host, track
from frozen_cases import ctx, _close_nets  # noqa: F401  (fixtures: the module's context, and every tracked net closed behind each test)

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (B, D, Nx, Ny): the smallest case; the smallest smooth net grid (Nx D = 30: rows that are no dword multiples); one tile + a remainder on both
# axes with Ny % 4 = 2; two tiles + remainders; exact tiles, BGRA; odd sizes; a camera frame
SHAPES = [(1, 1, 8, 8), (2, 3, 10, 12), (3, 3, 66, 34), (1, 3, 130, 70), (2, 4, 64, 64), (1, 2, 7, 5), (2, 3, 640, 480)]
PITCHES = ["tight", "pad64", "odd"]
TAIL = 96          # bytes of the allocation behind the last image row
PAD = 0xA5


def _layout(shape, kind):
    """(pitch, offset of the first image in its allocation, bytes of the allocation)"""
    B, D, Nx, Ny = shape
    pitch = {"tight": Nx * D, "pad64": (Nx * D + 63) // 64 * 64, "odd": Nx * D + 5}[kind]
    off = 1 if kind == "odd" else 0
    return pitch, off, off + B * Ny * pitch + TAIL


def _view(flat, shape, kind):
    """the images inside the flat allocation: uint8 [B][Ny][Nx][D] with the row pitch of `kind`"""
    B, D, Nx, Ny = shape
    pitch, off, _ = _layout(shape, kind)
    return torch.as_strided(flat, (B, Ny, Nx, D), (Ny * pitch, pitch, D, 1), off)


def _np_view(flat, shape, kind):
    B, D, Nx, Ny = shape
    pitch, off, _ = _layout(shape, kind)
    return np.lib.stride_tricks.as_strided(flat[off:], (B, Ny, Nx, D), (Ny * pitch, pitch, D, 1))


def _to_frames(px):
    """numpy's ImageToSpin_C: [B][Ny][Nx][D] -> [B][D][Nx][Ny]"""
    return np.ascontiguousarray(px.transpose(0, 3, 2, 1))


def _dev(a, ctx):
    return torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{ctx.device}")


# ------------------------------------------------------------------------------------------
# 1. unpack
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_unpack_equals_the_numpy_transpose(ctx, shape, kind):
    B, D, Nx, Ny = shape
    rng = np.random.default_rng(sum(shape) + len(kind))
    flat_h = rng.integers(0, 256, _layout(shape, kind)[2], dtype=np.uint8)          # (the pad bytes are random too: none of them may show)
    want = _to_frames(_np_view(flat_h, shape, kind))
    img = _view(_dev(flat_h, ctx), shape, kind)
    out8 = ctx.empty(B, D, Nx, Ny, dtype=torch.uint8); out8.fill_(0xEE)
    out32 = ctx.empty(B, D, Nx, Ny); out32.fill_(float("nan"))
    assert ctx.image_to_frames(img, out=out8) is out8
    assert ctx.image_to_frames(img, out=out32) is out32
    new8, new32 = ctx.image_to_frames(img), ctx.image_to_frames(img, dtype=torch.float32)
    ctx.sync()
    assert np.array_equal(host(out8), want), (shape, kind)
    assert host(out32).dtype == np.float32 and np.array_equal(host(out32), want.astype(np.float32)), (shape, kind)
    assert new8.dtype == torch.uint8 and np.array_equal(host(new8), want)
    assert new32.dtype == torch.float32 and np.array_equal(host(new32), want.astype(np.float32))
    # fewer pixels than the sentinel would hide: 0xEE is a legal pixel, so the same again with the complement
    out8.fill_(0x11)
    ctx.image_to_frames(img, out=out8)
    ctx.sync()
    assert np.array_equal(host(out8), want)


def test_unpack_takes_one_image_without_the_batch_axis(ctx):
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)
    out = ctx.image_to_frames(_dev(px, ctx))
    ctx.sync()
    assert np.array_equal(host(out), _to_frames(px[None]))


# ------------------------------------------------------------------------------------------
# 2. / 3. pack
# ------------------------------------------------------------------------------------------
def _pack_and_check(ctx, frames_h, want_px, shape, kind):
    """frames_to_image into a PAD-filled allocation: the pixels are want_px, every other byte of the allocation is still PAD"""
    n = _layout(shape, kind)[2]
    flat = torch.full((n,), PAD, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    img = _view(flat, shape, kind)
    assert ctx.frames_to_image(_dev(frames_h, ctx), out=img) is img
    ctx.sync()
    want = np.full(n, PAD, np.uint8)
    _np_view(want, shape, kind)[...] = want_px
    got = host(flat)
    assert np.array_equal(_np_view(got, shape, kind), want_px), (shape, kind, "pixels")
    assert np.array_equal(got[-TAIL:], want[-TAIL:]), (shape, kind, "bytes behind the last row")
    assert np.array_equal(got, want), (shape, kind, "pad bytes")
    return img


@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pack_of_8bit_frames_is_the_inverse_and_leaves_the_pad_alone(ctx, shape, kind):
    B, D, Nx, Ny = shape
    rng = np.random.default_rng(sum(shape) + 7 * len(kind))
    frames_h = rng.integers(0, 256, (B, D, Nx, Ny), dtype=np.uint8)
    want_px = np.ascontiguousarray(frames_h.transpose(0, 3, 2, 1))
    _pack_and_check(ctx, frames_h, want_px, shape, kind)
    # a fresh contiguous image when none is given
    img = ctx.frames_to_image(_dev(frames_h, ctx))
    ctx.sync()
    assert tuple(img.shape) == (B, Ny, Nx, D) and np.array_equal(host(img), want_px)
    # frames_to_image(image_to_frames(x)) == x, from and into the pitched layout
    flat_h = rng.integers(0, 256, _layout(shape, kind)[2], dtype=np.uint8)
    x = _view(_dev(flat_h, ctx), shape, kind)
    back = torch.full((len(flat_h),), PAD, dtype=torch.uint8, device=x.device)
    ctx.frames_to_image(ctx.image_to_frames(x), out=_view(back, shape, kind))
    ctx.sync()
    assert np.array_equal(_np_view(host(back), shape, kind), _np_view(flat_h, shape, kind)), (shape, kind)


def _edge_values(rng, n):
    """n float32 values: the rule's edges -- k + 0.5 and k + 0.49999997 for k in 0..255, negatives, -0.0, 255.4, 255.5, 1e9, NaN, +-inf --
    scattered over random values in -50..300 (a shape with fewer elements than edges takes a random choice of both)"""
    k = np.arange(256, dtype=np.float64)
    edges = np.concatenate([k + 0.5, (k + np.float64(np.float32(0.49999997))), [-0.5, -0.49999997, -1.5, -7.25, -300.0, -1e9, -0.0, 0.0, 255.4, 255.5, 255.49998,
                                                                                  256.0, 1e9, np.nan, np.inf, -np.inf]]).astype(np.float32)
    v = rng.uniform(-50, 300, n).astype(np.float32)
    if n >= 2 * len(edges):
        v[rng.choice(n, len(edges), replace=False)] = edges
    else:
        pick = rng.random(n) < 0.7
        v[pick] = rng.choice(edges, int(pick.sum()))
    return v


@pytest.mark.parametrize("kind", PITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pack_of_float_frames_applies_spin_to_image(ctx, shape, kind):
    B, D, Nx, Ny = shape
    rng = np.random.default_rng(sum(shape) + 13 * len(kind))
    with np.errstate(invalid="ignore"):
        frames_h = _edge_values(rng, B * D * Nx * Ny).reshape(B, D, Nx, Ny)
        want_px = np.ascontiguousarray(_rule(frames_h).transpose(0, 3, 2, 1))
        if B * D * Nx * Ny >= 2000:
            assert np.isnan(frames_h).any() and np.isinf(frames_h).any() and (frames_h % 1 == 0.5).sum() >= 250
    _pack_and_check(ctx, frames_h, want_px, shape, kind)


# ------------------------------------------------------------------------------------------
# 4. the rule is the row pass's;  5. composition without synchronisation
# ------------------------------------------------------------------------------------------
NETS = {"16x16": (3, 16, 16, False), "10x12": (3, 10, 12, True)}       # D, Nx, Ny, AEFFT_NET_SMOOTH_SIZES
B_NET = 2


def _small_net(ctx, name, seed=3):
    D, Nx, Ny, smooth = NETS[name]
    net = track(aefft.Net(ctx, D, Nx, Ny, [2], 3, 1, batch=B_NET, smooth_sizes=smooth))
    for l, w in enumerate(_weights(np.random.default_rng(seed), D, [2], 3, 3)):
        net.set_pair(l, *w)
    return net


def test_the_float_rule_is_the_inverse_row_passes(ctx):
    """frames_to_image of infer's float reconstruction == the transpose of infer's own 8-bit reconstruction, byte for byte.  The decoder is
    scaled so that the image spills over both ends of 0..255."""
    D, Nx, Ny, _ = NETS["16x16"]
    rng = np.random.default_rng(11)
    net = _small_net(ctx, "16x16")
    c, b, f, p = net.get_pair(0)
    net.set_pair(0, c, b, 40.0 * f, p + 100.0)
    frames = _dev(rng.integers(0, 256, (B_NET, D, Nx, Ny), dtype=np.uint8), ctx)
    rec32 = ctx.empty(B_NET, D, Nx, Ny); rec8 = ctx.empty(B_NET, D, Nx, Ny, dtype=torch.uint8)
    net.infer(frames, rec32)
    net.infer(frames, rec8)
    img = ctx.frames_to_image(rec32)
    ctx.sync()
    r = host(rec32)
    assert (r < 0).any() and (r > 255).any() and ((r > 1) & (r < 254)).any(), (r.min(), r.max())
    assert np.array_equal(host(img), host(rec8).transpose(0, 3, 2, 1))


def _net_calls(ctx, name, frames):
    """infer (8-bit in and out + the hidden layer), score and step_grad queued back to back on `frames`; the results, read afterwards"""
    D, Nx, Ny, _ = NETS[name]
    net = _small_net(ctx, name)
    g = net.dims[0]
    rec8 = ctx.empty(B_NET, D, Nx, Ny, dtype=torch.uint8); hid = ctx.empty(B_NET, g["dM"], g["Nx"], g["Ny"])
    score = ctx.empty(B_NET); recon = ctx.empty(B_NET, D, Nx, Ny)
    gbuf = net.grad_buffer(); grads = torch.empty_like(gbuf)
    fr = frames()                                  # (image_to_frames, or the planar bytes: queued, not waited for)
    net.infer(fr, rec8, 0, hid)
    net.score(fr, score)
    net.step_grad(fr, recon)
    grads.copy_(gbuf)
    img = ctx.frames_to_image(rec8)
    ctx.sync()
    out = [host(t).copy() for t in (fr, rec8, hid, score, recon, grads, img)]
    net.close()
    return out


@pytest.mark.parametrize("name", list(NETS))
def test_net_calls_on_unpacked_frames_are_bit_for_bit(ctx, name):
    D, Nx, Ny, _ = NETS[name]
    rng = np.random.default_rng(Nx + Ny)
    px = rng.integers(0, 256, (B_NET, Ny, Nx, D), dtype=np.uint8)
    img_d, planar_d = _dev(px, ctx), _dev(_to_frames(px), ctx)
    ctx.sync()
    a = _net_calls(ctx, name, lambda: ctx.image_to_frames(img_d))
    b = _net_calls(ctx, name, lambda: planar_d)
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (name, k)
    assert np.isfinite(a[3]).all() and np.isfinite(a[5]).all()
    assert np.array_equal(a[6], a[1].transpose(0, 3, 2, 1))


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(ctx):
    L = ctx.L
    B, D, Nx, Ny = 2, 3, 10, 12
    pitch = Nx * D
    dev = f"cuda:{ctx.device}"
    img = torch.full((B * Ny * pitch + 64,), 0x3C, dtype=torch.uint8, device=dev)
    frm = torch.full((B * D * Nx * Ny + 64,), 0xC3, dtype=torch.uint8, device=dev)
    ip, fp = img.data_ptr(), frm.data_ptr()
    assert fp % 16 == 0
    n_f = B * D * Nx * Ny
    # the rules' full texts, as the library words them
    NULL, DIM, RANGE = "null context, image or frames", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and Nx, Ny in 1..8192"
    PITCH, ALIGN, OVERLAP = "pitch must be at least Nx * D bytes", "frames_d must be 16-byte aligned", "the frame and image ranges overlap (the op is out-of-place)"
    cases = [
        ("D = 0", (ip, pitch, fp, 1, B, 0, Nx, Ny), DIM), ("D = 5", (ip, 5 * Nx, fp, 1, B, 5, Nx, Ny), DIM),
        ("Nx = 0", (ip, pitch, fp, 1, B, D, 0, Ny), RANGE), ("Ny = 8193", (ip, pitch, fp, 1, B, D, Nx, 8193), RANGE), ("B = 0", (ip, pitch, fp, 1, 0, D, Nx, Ny), RANGE),
        ("pitch = Nx D - 1", (ip, pitch - 1, fp, 1, B, D, Nx, Ny), PITCH),
        ("null image", (None, pitch, fp, 1, B, D, Nx, Ny), NULL), ("null frames", (ip, pitch, None, 1, B, D, Nx, Ny), NULL),
        ("frames off by 4", (ip, pitch, fp + 4, 0, 1, 1, 2, 2), ALIGN),
        ("overlap: frames inside the image", (ip, pitch, ip + 16, 1, B, D, Nx, Ny), OVERLAP),
        ("overlap: image inside the float frames", (fp + n_f, pitch, fp, 0, 1, D, Nx, Ny), OVERLAP),
    ]
    for what, (i_p, pt, f_p, u8, b, d, nx, ny), rule in cases:
        for name, args in (("aefft_image_to_frames", (ctx.h, i_p, pt, f_p, u8, b, d, nx, ny)), ("aefft_frames_to_image", (ctx.h, f_p, u8, i_p, pt, b, d, nx, ny))):
            assert getattr(L, name)(*args) == aefft.EINVAL, what
            msg = L.aefft_last_error(ctx.h).decode()
            assert msg == name + ": " + rule, (what, msg)
    ctx.sync()
    assert (host(img) == 0x3C).all() and (host(frm) == 0xC3).all()
    # layouts the C call cannot describe are refused by the binding; a library error surfaces with its message
    with pytest.raises(ValueError):
        ctx.image_to_frames(img[:B * Ny * pitch].view(B, Ny, Nx, D).permute(0, 2, 1, 3))
    with pytest.raises(ValueError):
        ctx.frames_to_image(frm[:n_f].view(B, D, Nx, Ny), out=img[:n_f].view(B, Nx, Ny, D))
    with pytest.raises(aefft.AefftError, match="pitch"):
        ctx.check(L.aefft_image_to_frames(ctx.h, ip, pitch - 1, fp, 1, B, D, Nx, Ny))


# ------------------------------------------------------------------------------------------
# 7. profile accounting
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_one_call_is_one_image_launch_with_its_bytes(ctx, f32):
    B, D, Nx, Ny = 2, 3, 66, 34
    img = torch.zeros(B, Ny, Nx, D, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    frames = ctx.empty(B, D, Nx, Ny, dtype=torch.float32 if f32 else torch.uint8)
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.image_to_frames(img, out=frames)
        one = ctx.prof_read()
        ctx.frames_to_image(frames, out=img)
        two = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    n = B * D * Nx * Ny * (5 if f32 else 2)
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == n
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == 2 * n
    assert sum(v["launches"] for v in two.values()) == 2
