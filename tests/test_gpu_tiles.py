"""aefft_image_tiles_to_frames / aefft_frames_tiles_to_image (Context.image_tiles_to_frames, Context.frames_tiles_to_image) and Net.infer_tiled on
the device against the numpy restatement of tiles_ref.py -- EXACT equality everywhere: every shape with 8-bit and float frames in both
directions, B = 2 with a stride larger than the image, an unaligned image pointer and an odd pitch next to the aligned dword route, destination
allocations pre-filled with random bytes whose row padding and tail must come back unchanged.  Then the round trip, the identities with
image_to_frames / frames_to_image, one graph capture and replay, every AEFFT_EINVAL rule, the profile entry, and tiled inference of a small net."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import tiles_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (W, H, Nx, Ny, V, M, the D values): odd sizes with reflection on all four sides and three tiles per axis; an image smaller than a tile (iterated
# reflection); R = 0, hard seams; a plain partition; the identity with image_to_frames; a non-square tile with per-axis parameters; Ny % 4 == 2 (the
# element route; overlap 4 on both axes would break 2 V <= N for Ny = 6, so the rows take 3: rim 1, ramp 1); several LDS blocks per tile and remainders;
# the smallest of everything
SHAPES = [(13, 9, 8, 8, 4, 1, (3,)), (5, 3, 8, 8, 4, 1, (3,)), (9, 9, 8, 8, 4, 2, (3,)), (16, 8, 8, 8, 0, 0, (3,)), (8, 8, 8, 8, 0, 0, (1, 2, 3, 4)),
          (37, 29, 16, 8, (6, 4), (1, 2), (3,)), (23, 17, 10, 6, (4, 3), 1, (3,)), (130, 70, 32, 32, 8, 2, (4,)), (1, 1, 2, 2, 0, 0, (3,))]
CASES = [s[:6] + (d,) for s in SHAPES for d in s[6]]
B = 2
TAIL = 96                                                                        # bytes of an allocation behind its live bytes: the guard region
NP = {torch.uint8: np.uint8, torch.float32: np.float32}
_id = lambda v: "-".join(str(q).replace(" ", "") for q in v) if isinstance(v, tuple) else str(v)
# image layouts (pad bytes behind a row, gap bytes behind an image, bytes the image pointer is off 16): tight at an aligned pointer -- the dword
# route wherever W D is a multiple of 4; pitch and stride multiples of 4 whatever W D is -- the dword route with dwords that cross the row's end; an
# odd pitch; an unaligned pointer
LAYOUTS = ["tight", "words", "odd", "skewed"]


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")          # (a copy: cached arrays stay read-only)


def _layout(W, H, D, layout):
    fill = -W * D % 4
    pad, gap, skew = {"tight": (0, 0, 0), "words": (fill + 4, fill + 8, 0), "odd": (1 + W * D % 2, 5, 0), "skewed": (fill, fill + 4, 1)}[layout]
    pitch = W * D + pad
    stride = (H - 1) * pitch + W * D + gap
    return pitch, stride, skew, skew + (B - 1) * stride + (H - 1) * pitch + W * D      # the last: bytes up to the last live byte


def _image_view(flat, W, H, D, layout):
    """the [B][H][W][D] view of a flat uint8 tensor (device or numpy) under `layout`"""
    pitch, stride, skew, _ = _layout(W, H, D, layout)
    if isinstance(flat, np.ndarray):
        return np.lib.stride_tricks.as_strided(flat[skew:], (B, H, W, D), (stride, pitch, D, 1), writeable=False)
    return flat[skew:].as_strided((B, H, W, D), (stride, pitch, D, 1))


@functools.lru_cache(maxsize=None)
def _image(W, H, D):
    img = np.random.default_rng(W * 131 + H * 7 + D).integers(0, 256, (B, H, W, D), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _tiles(case):
    """(random 8-bit tiles, float tiles of their own with NaN, +-inf, negatives, values above 255 and exact halves among them, the restated blend
    of each), computed once and read-only"""
    W, H, Nx, Ny, V, M, D = case
    ntx, nty = R.plan(W, H, Nx, Ny, V, M)[:2]
    shape = (B * ntx * nty, D, Nx, Ny)
    rng = np.random.default_rng(sum(shape) + W)
    t8 = rng.integers(0, 256, shape, dtype=np.uint8)
    t32 = rng.uniform(-40, 300, shape).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 300.0, 0.5, 1.5, 254.5, 255.5, 2.5, 0.49999997, -0.5, 255.0, 0.0], dtype=np.float32)
    flat = t32.reshape(-1)
    reps = max(1, flat.size // (8 * special.size))
    pick = rng.choice(flat.size, min(flat.size, reps * special.size), replace=False)
    flat[pick] = np.tile(special, reps)[:pick.size]
    out = (t8, t32, R.blend(t8, W, H, V, M), R.blend(t32, W, H, V, M))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _gathered(case):
    W, H, Nx, Ny, V, M, D = case
    g = R.gather(_image(W, H, D), Nx, Ny, V, M)
    g.setflags(write=False)
    return g


# ------------------------------------------------------------------------------------------
# 1. exact equality with the restatement, both directions, every layout and both frame types
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gather_equals_the_restatement(ctx, case, layout):
    W, H, Nx, Ny, V, M, D = case
    pitch, stride, skew, live = _layout(W, H, D, layout)
    flat = np.random.default_rng(3).integers(0, 256, live + TAIL, dtype=np.uint8)
    view = _image_view(flat, W, H, D, layout)
    np.lib.stride_tricks.as_strided(flat[skew:], (B, H, W, D), (stride, pitch, D, 1))[...] = _image(W, H, D)
    src = _image_view(_dev(flat, ctx), W, H, D, layout)
    assert np.array_equal(view, _image(W, H, D)) and (src.data_ptr() % 4 != 0) == (layout == "skewed")
    want = _gathered(case)
    for dtype in (torch.uint8, torch.float32):
        n = want.size * (1 if dtype == torch.uint8 else 4)
        guard = np.random.default_rng(9).integers(0, 256, n + TAIL, dtype=np.uint8)
        d = _dev(guard, ctx)
        out = d[:n].view(dtype).view(*want.shape)
        assert ctx.image_tiles_to_frames(src, (Nx, Ny), V, M, out=out) is out
        ctx.sync()
        got = host(d)
        bad = int((got[:n] != want.astype(NP[dtype]).reshape(-1).view(np.uint8)).sum())
        print(case, layout, dtype, "bytes that differ:", bad)
        assert bad == 0, (case, layout, dtype)
        assert np.array_equal(got[n:], guard[n:]), "the bytes behind the frames changed"
    fresh = ctx.image_tiles_to_frames(src, (Nx, Ny), V, M)
    assert fresh.dtype == torch.uint8 and np.array_equal(host(fresh), want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_blend_equals_the_restatement(ctx, case, layout):
    W, H, Nx, Ny, V, M, D = case
    pitch, stride, skew, live = _layout(W, H, D, layout)
    t8, t32, want8, want32 = _tiles(case)
    for tiles, want in ((t8, want8), (t32, want32), (_gathered(case), _image(W, H, D)), (_gathered(case).astype(np.float32), _image(W, H, D))):
        guard = np.random.default_rng(11).integers(0, 256, live + TAIL, dtype=np.uint8)
        d = _dev(guard, ctx)
        out = _image_view(d, W, H, D, layout)
        assert ctx.frames_tiles_to_image(_dev(tiles, ctx), (W, H), V, M, out=out) is out
        ctx.sync()
        got = host(d)
        expect = guard.copy()
        np.lib.stride_tricks.as_strided(expect[skew:], (B, H, W, D), (stride, pitch, D, 1))[...] = want       # everything else: as it was
        bad = int((got != expect).sum())
        print(case, layout, tiles.dtype, "bytes that differ (row padding, gaps and tail included):", bad)
        assert bad == 0, (case, layout, tiles.dtype)
    fresh = ctx.frames_tiles_to_image(_dev(t8, ctx), (W, H), V, M)
    assert tuple(fresh.shape) == (B, H, W, D) and np.array_equal(host(fresh), want8)


def test_the_float_tiles_hold_the_special_values():
    t32 = _tiles(CASES[0])[1]
    assert np.isnan(t32).any() and np.isposinf(t32).any() and np.isneginf(t32).any() and (t32 < 0).any() and (t32 > 255).any()
    fin = t32[np.isfinite(t32)]
    assert ((fin % 1 == 0.5) & (fin > 0) & (fin < 255)).any()


# ------------------------------------------------------------------------------------------
# 2. the consequences of the definition on the device
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_blend_of_gather_is_the_image_and_constant_tiles_give_a_constant_image(ctx, case):
    W, H, Nx, Ny, V, M, D = case
    img = _dev(_image(W, H, D), ctx)
    for dtype in (torch.uint8, torch.float32):
        tiles = ctx.image_tiles_to_frames(img, (Nx, Ny), V, M, dtype=dtype)
        back = ctx.frames_tiles_to_image(tiles, (W, H), V, M)
        const = ctx.frames_tiles_to_image(torch.full_like(tiles, 77), (W, H), V, M)
        ctx.sync()
        assert torch.equal(back, img), (case, dtype)
        assert (host(const) == 77).all(), (case, dtype)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_one_tile_without_overlap_is_image_to_frames(ctx, D):
    img = _dev(_image(8, 8, D), ctx)
    for dtype in (torch.uint8, torch.float32):
        tiles = ctx.image_tiles_to_frames(img, (8, 8), 0, dtype=dtype)
        plain = ctx.image_to_frames(img, dtype=dtype)
        assert torch.equal(tiles, plain)
        assert torch.equal(ctx.frames_tiles_to_image(tiles, (8, 8), 0), ctx.frames_to_image(plain))
    # a plain partition: the tiles are image_to_frames of the blocks
    img = _dev(_image(16, 8, 3), ctx)
    tiles = ctx.image_tiles_to_frames(img, (8, 8), 0)
    for b in range(B):
        for tx in range(2):
            assert torch.equal(tiles[2 * b + tx], ctx.image_to_frames(img[b, :, 8 * tx:8 * tx + 8].contiguous())[0])


# ------------------------------------------------------------------------------------------
# 3. captured once and replayed
# ------------------------------------------------------------------------------------------
def test_both_calls_are_captured_once_and_replayed():
    W, H, Nx, Ny, V, M, D = 130, 70, 32, 32, 8, 2, 3
    image = _image(W, H, D)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        img = torch.zeros(image.shape, dtype=torch.uint8, device=dev)
        ntx, nty = R.plan(W, H, Nx, Ny, V, M)[:2]
        tiles = torch.full((B * ntx * nty, D, Nx, Ny), 0xEE, dtype=torch.uint8, device=dev)
        back = torch.full(image.shape, 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.image_tiles_to_frames(img, (Nx, Ny), V, M, out=tiles)
            c.frames_tiles_to_image(tiles, (W, H), V, M, out=back)
        torch.cuda.synchronize()
        img.copy_(_dev(image, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(tiles), R.gather(image, Nx, Ny, V, M)) and np.array_equal(host(back), image)
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    W, H, Nx, Ny, V, M, D = 13, 9, 8, 8, 4, 1, 3
    pitch, stride = W * D, H * W * D
    dev = f"cuda:{ctx.device}"
    a = torch.full((8192,), 0x3C, dtype=torch.uint8, device=dev)                 # the images
    f = torch.full((8192,), 0xC3, dtype=torch.uint8, device=dev)                 # the frames: 2 x 6 tiles x 3 x 8 x 8 floats fit
    ap, fp = a.data_ptr(), f.data_ptr()
    assert ap % 16 == 0 and fp % 16 == 0
    good = aefft.TileDesc(W, H, Nx, Ny, V, V, M, M)
    desc = lambda **kw: aefft.TileDesc(*[kw.get(k, getattr(good, k)) for k, _ in aefft.TileDesc._fields_])
    # (image, pitch, stride, description, frames, frames_u8, B, D), the whole message behind the call's name
    # the rules' full texts, as the library words them
    NULL, DIM, RANGE = "null context, image, frames or description", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and W, H in 1..8192"
    PLAN = "the description is not one aefft_tile_plan_make takes (W, H in 1..8192; Nx, Ny in 2..2048; 0 <= 2 overlap <= N; 0 <= 2 rim <= overlap)"
    PITCH, STRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ROWS_FIT, BATCH_FIT = "H * pitch does not fit the address space", "B * image_stride does not fit the address space"
    ALIGN, OVERLAP, COUNT = "frames_d must be 16-byte aligned", "the frame and image ranges overlap (the op is out-of-place)", "B * ntx * nty tiles do not fit an int"
    cases = [
        ("null image", (None, pitch, stride, good, fp, 1, 2, D), NULL),
        ("null frames", (ap, pitch, stride, good, None, 1, 2, D), NULL),
        ("null description", (ap, pitch, stride, None, fp, 1, 2, D), NULL),
        ("W = 0", (ap, pitch, stride, desc(W=0), fp, 1, 2, D), PLAN),
        ("H = 8193", (ap, pitch, stride, desc(H=8193), fp, 1, 2, D), PLAN),
        ("Nx = 1", (ap, pitch, stride, desc(Nx=1), fp, 1, 2, D), PLAN),
        ("Ny = 2049", (ap, pitch, stride, desc(Ny=2049), fp, 1, 2, D), PLAN),
        ("2 V > N", (ap, pitch, stride, desc(overlap_x=5), fp, 1, 2, D), PLAN),
        ("V < 0", (ap, pitch, stride, desc(overlap_y=-1), fp, 1, 2, D), PLAN),
        ("2 M > V", (ap, pitch, stride, desc(rim_x=3), fp, 1, 2, D), PLAN),
        ("M < 0", (ap, pitch, stride, desc(rim_y=-1), fp, 1, 2, D), PLAN),
        ("D = 0", (ap, pitch, stride, good, fp, 1, 2, 0), DIM),
        ("D = 5", (ap, 5 * W, 5 * W * H, good, fp, 1, 1, 5), DIM),
        ("B = 0", (ap, pitch, stride, good, fp, 1, 0, D), RANGE),
        ("pitch too small", (ap, pitch - 1, stride, good, fp, 1, 2, D), PITCH),
        ("stride too small", (ap, pitch, stride - 1, good, fp, 1, 2, D), STRIDE),
        ("stride that overflows", (ap, pitch, 2 ** 63, good, fp, 1, 3, D), BATCH_FIT),
        ("pitch that overflows", (ap, 2 ** 62, stride, good, fp, 1, 1, D), ROWS_FIT),
        ("frames off by 4", (ap, pitch, stride, good, fp + 4, 1, 2, D), ALIGN),
        ("frames off by 8, float", (ap, pitch, stride, good, fp + 8, 0, 2, D), ALIGN),
        ("overlap: the frames begin in the images", (ap, pitch, stride, good, ap + 16, 1, 2, D), OVERLAP),
        ("overlap: the images begin in the float frames", (fp + 2 * 6 * 3 * 64 * 4 - 16, pitch, stride, good, fp, 0, 2, D), OVERLAP),
        ("a tile count beyond an int", (ap, 8192, 8192 * 8192, desc(W=8192, H=8192, Nx=2, Ny=2, overlap_x=1, overlap_y=1, rim_x=0, rim_y=0), fp, 1, 64, 1), COUNT),
    ]
    for what, (im, pi, st, de, fr, u8, b, d), rule in cases:
        de = None if de is None else C.byref(de)
        assert L.aefft_image_tiles_to_frames(ctx.h, im, pi, st, de, fr, u8, b, d) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_image_tiles_to_frames: " + rule, (what, msg)
        assert L.aefft_frames_tiles_to_image(ctx.h, fr, u8, de, im, pi, st, b, d) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_frames_tiles_to_image: " + rule, (what, msg)
    ctx.sync()
    assert (host(a) == 0x3C).all() and (host(f) == 0xC3).all()
    # what is NOT an error: neighbouring ranges, a stride that is ignored for B == 1
    n = 2 * 6 * D * Nx * Ny
    assert L.aefft_image_tiles_to_frames(ctx.h, ap, pitch, stride, C.byref(good), ap + 1024, 1, 2, D) == aefft.OK
    assert L.aefft_frames_tiles_to_image(ctx.h, fp, 1, C.byref(good), fp + 2048, pitch, 0, 1, D) == aefft.OK
    ctx.sync()
    got = host(a)
    assert (got[:1024] == 0x3C).all() and (got[1024:1024 + n] == 0x3C).all() and (got[1024 + n:] == 0x3C).all()      # (tiles of a constant image)
    got = host(f)
    assert (got == 0xC3).all()                                                                                     # (the blend of constant tiles)
    # the binding refuses what the C call would, before it reaches the library; a library error surfaces with its message
    img = a[:2 * stride].view(2, H, W, D)
    for kw in (dict(tile=(8, 1)), dict(overlap=5), dict(rim=3), dict(dtype=torch.float64), dict(out=torch.empty(11, D, Nx, Ny, dtype=torch.uint8, device=dev))):
        with pytest.raises(ValueError):
            ctx.image_tiles_to_frames(img, **dict(dict(tile=(Nx, Ny), overlap=V, rim=M), **kw))
    with pytest.raises(ValueError):
        ctx.frames_tiles_to_image(f[:5 * D * Nx * Ny].view(5, D, Nx, Ny), (W, H), V, M)
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.image_tiles_to_frames(img, (Nx, Ny), V, M, out=a[16:16 + n].view(12, D, Nx, Ny))


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
def test_each_call_is_one_image_launch_with_its_bytes(ctx):
    W, H, Nx, Ny, V, M, D = 130, 70, 32, 32, 8, 2, 3
    ntx, nty = R.plan(W, H, Nx, Ny, V, M)[:2]
    ni, nf = B * W * H * D, B * ntx * nty * D * Nx * Ny
    img = _dev(_image(W, H, D), ctx)
    ctx.prof_enable(); ctx.prof_reset()
    try:
        t8 = ctx.image_tiles_to_frames(img, (Nx, Ny), V, M)
        one = ctx.prof_read()
        t32 = ctx.image_tiles_to_frames(img, (Nx, Ny), V, M, dtype=torch.float32)
        two = ctx.prof_read()
        ctx.frames_tiles_to_image(t8, (W, H), V, M)
        three = ctx.prof_read()
        ctx.frames_tiles_to_image(t32, (W, H), V, M)
        four = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == ni + nf
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == 2 * ni + 5 * nf
    assert three["image"]["launches"] == 3 and three["image"]["bytes"] == 3 * ni + 6 * nf
    assert four["image"]["launches"] == 4 and four["image"]["bytes"] == 4 * ni + 10 * nf
    assert sum(v["launches"] for v in four.values()) == 4


# ------------------------------------------------------------------------------------------
# 6. tiled inference of a small net
# ------------------------------------------------------------------------------------------
def _small_net(ctx, rng_seed=21):
    D, N, Bn, dM, Nk = 3, 16, 4, 8, 3
    rng = np.random.default_rng(rng_seed)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    c, f = q32(0.3 * rng.uniform(-1, 1, (dM, D, Nk, Nk))), q32(0.3 * rng.uniform(-1, 1, (D, dM, Nk, Nk)))
    bias, p = q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, D))
    net = aefft.Net(ctx, D, N, N, [dM], Nk, 1, batch=Bn)
    net.set_pair(0, c, bias, f, p)
    return net


def test_infer_tiled_is_gather_infer_blend_and_leaves_the_net_as_it_was(ctx):
    """a 3 -> 8 net with a 3 x 3 kernel, scale 1, 16 x 16 frames, batch 4, on a 37 x 29 x 3 image with overlap 4 and rim 1: 9 tiles, three chunks, the last
    one padded.  The output equals, byte for byte, the restated blend of the 8-bit reconstructions net.infer returns for the gathered tiles chunk
    by chunk; a training step afterwards gives the same bits as on a net that never made the call."""
    W, H, D, N, Bn, V, M = 37, 29, 3, 16, 4, 4, 1
    image = np.random.default_rng(8).integers(0, 256, (1, H, W, D), dtype=np.uint8)
    assert R.plan(W, H, N, N, V, M)[:2] == (3, 3)
    tiles = R.gather(image, N, N, V, M)
    padded = np.concatenate([tiles, np.zeros((3, D, N, N), np.uint8)])
    frames = _dev(np.random.default_rng(9).integers(0, 256, (Bn, D, N, N), dtype=np.uint8), ctx)
    net, other = _small_net(ctx), _small_net(ctx)
    try:
        recon = np.empty_like(padded)
        for k in range(0, 12, Bn):
            r, _ = net.infer(_dev(padded[k:k + Bn], ctx), torch.empty(Bn, D, N, N, dtype=torch.uint8, device=frames.device))
            ctx.sync()
            recon[k:k + Bn] = host(r)
        want = R.blend(recon[:9], W, H, V, M)
        assert not np.array_equal(want, image) and want.std() > 0
        img = _dev(image, ctx)
        out = net.infer_tiled(img, V, M)
        ctx.sync()
        assert out.dtype == torch.uint8 and tuple(out.shape) == (1, H, W, D)
        assert np.array_equal(host(out), want)
        given = torch.full((1, H, W, D), 0xEE, dtype=torch.uint8, device=img.device)
        assert net.infer_tiled(img, V, M, out=given) is given
        ctx.sync()
        assert np.array_equal(host(given), want)
        # the net is as it was: the same gradient bits and the same weights after a step as a net that never made the call
        for n_ in (net, other):
            n_.step_grad(frames, None)
            n_.step_apply(0.05)
        ctx.sync()
        assert np.array_equal(host(net.grad_buffer()).view(np.uint32), host(other.grad_buffer()).view(np.uint32))
        for a_, b_ in zip(net.get_pair(0), other.get_pair(0)):
            assert np.array_equal(a_.view(np.uint32), b_.view(np.uint32))
        with pytest.raises(ValueError):
            net.infer_tiled(img, 9, M)
        with pytest.raises(ValueError):
            net.infer_tiled(img[..., :2], V, M)
        with pytest.raises(ValueError):
            net.infer_tiled(img, V, M, out=torch.empty(1, H, W + 1, D, dtype=torch.uint8, device=img.device))
    finally:
        net.close(); other.close()
    spatial = aefft.Net(ctx, D, N, N, [8], 3, 1, batch=Bn, spatial=True)
    try:
        with pytest.raises(ValueError, match="spatial"):
            spatial.infer_tiled(_dev(image, ctx), V, M)
    finally:
        spatial.close()
