"""aefft_frames_degrade (Context.frames_degrade) on the device against the numpy restatement of degrade_ref.py -- EXACT equality, bit for bit:
every blur with every noise setting, both source and both destination types, on shapes that take the dword and the element route, one tile and
several, with the destination allocation pre-filled with random bytes that must come back unchanged behind the live frames.  Then the
identities of the definition on the device, one graph capture and replay, every AEFFT_EINVAL rule, the profile entry, and the call feeding
step_grad_target and score_target of a small net."""
import functools
import importlib

import numpy as np
import pytest
import torch

import degrade_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (B, D, Nx, Ny): one tile on the dword route; Ny a multiple of 4 with B = 2 (the carry of first_frame into the counter's fourth word); Ny % 4 == 2;
# odd sizes (pairs straddle rows); one element; a whole tile row, two tile rows; several tiles with remainders and halos across tile edges
SHAPES = [(1, 1, 8, 8), (2, 3, 16, 12), (1, 3, 10, 6), (1, 2, 9, 7), (1, 1, 1, 1), (2, 4, 64, 64), (1, 3, 130, 70)]
BIG = (2, 3, 256, 256)
NOISE = [(0.0, 0.0), (1.5, 0.0), (25.0, 0.02), (255.0, 0.0), (0.0, 1.0)]          # (sigma, impulse)
BLURS = [0, 1, 2, 3, 4]
SEED = 0x9E3779B97F4A7C15                                                        # a non-zero high word
FIRST = 2 ** 32 - 1                                                              # B = 2: frame 1 is frame 2^32
TAIL = 96                                                                        # bytes of the allocation behind the last frame: the guard region
NP = {torch.uint8: np.uint8, torch.float32: np.float32}
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")          # (a copy: cached arrays stay read-only)


@functools.lru_cache(maxsize=None)
def _sources(shape):
    """(8-bit frames, float frames of their own: NaN, +-inf, negatives, values above 255 and exact halves among them), computed once and read-only"""
    rng = np.random.default_rng(sum(shape))
    f8 = rng.integers(0, 256, shape, dtype=np.uint8)
    f32 = rng.uniform(-40, 300, shape).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 300.0, 0.5, 1.5, 254.5, 255.5, 2.5, 0.49999997, -0.5, 255.0, 0.0], dtype=np.float32)
    flat = f32.reshape(-1)
    if flat.size >= special.size:
        reps = max(1, flat.size // (8 * special.size))
        flat[rng.choice(flat.size, reps * special.size, replace=False)] = np.tile(special, reps)
    else:
        flat[:] = special[:flat.size]
    f8.setflags(write=False); f32.setflags(write=False)
    return f8, f32


@functools.lru_cache(maxsize=None)
def _want(shape, f32_src, blur, sigma, impulse, dst):
    w = R.degrade(_sources(shape)[1 if f32_src else 0], blur, sigma, impulse, SEED, FIRST, dtype=dst)
    w.setflags(write=False)
    return w


def _guarded(shape, dtype, ctx, seed):
    """a destination inside an allocation of random bytes with TAIL bytes behind it: (host copy of the bytes, the allocation, the frames' view)"""
    n = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 4)
    flat = np.random.default_rng(seed).integers(0, 256, n + TAIL, dtype=np.uint8)
    d = _dev(flat, ctx)
    return flat, d, d[:n].view(dtype).view(*shape)


def _check(ctx, shape, blur, cases):
    """every (sigma, impulse, float source, destination type) of `cases` at this shape and blur: the live bytes are the restatement's, the tail is
    as it was"""
    src = [_dev(a, ctx) for a in _sources(shape)]
    for k, (sigma, impulse, f32_src, dst) in enumerate(cases):
        flat, d, view = _guarded(shape, dst, ctx, seed=k + blur)
        assert ctx.frames_degrade(src[1 if f32_src else 0], blur, sigma, impulse, SEED, FIRST, out=view) is view
        ctx.sync()
        want = _want(shape, f32_src, blur, sigma, impulse, NP[dst])
        got = host(d)
        live = want.size * want.itemsize
        differ = got[:live] != want.reshape(-1).view(np.uint8)
        bad = int(differ.sum())
        print(shape, "blur", blur, "sigma", sigma, "impulse", impulse, "float source" if f32_src else "8-bit source", dst, "bytes that differ:", bad,
              "by position in the dword:", np.bincount(np.nonzero(differ)[0] % 4, minlength=4).tolist())
        assert bad == 0, (shape, blur, sigma, impulse, f32_src, dst)
        assert np.array_equal(got[live:], flat[live:]), "the bytes behind the live frames changed"


# ------------------------------------------------------------------------------------------
# 1. exact equality with the restatement.  The small shapes take the WHOLE product blur x noise x source type x destination type (700 calls in
#    35 tests); the 256^2 shape runs once.  Nothing is left out.
# ------------------------------------------------------------------------------------------
ALL = [(s, i, f, d) for (s, i) in NOISE for f in (False, True) for d in (torch.uint8, torch.float32)]


@pytest.mark.parametrize("blur", BLURS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_degrade_equals_the_restatement(ctx, shape, blur):
    _check(ctx, shape, blur, ALL)


def test_degrade_equals_the_restatement_at_256_squared(ctx):
    _check(ctx, BIG, 2, [(25.0, 0.02, False, torch.uint8)])


def test_the_float_sources_hold_the_special_values():
    for shape in SHAPES + [BIG]:
        f = _sources(shape)[1]
        if f.size >= 14:
            assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and (f < 0).any() and (f[np.isfinite(f)] > 255).any()
            assert (f == np.float32(254.5)).any() and (f == np.float32(0.49999997)).any()


# ------------------------------------------------------------------------------------------
# 2. identities of the definition, on the device
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 12), (1, 2, 9, 7), (1, 3, 130, 70)], ids=_id)
def test_all_zero_parameters_copy_convert_or_round(ctx, shape):
    f8, f32 = _sources(shape)
    a, b = _dev(f8, ctx), _dev(f32, ctx)
    same = ctx.frames_degrade(a)
    up = ctx.frames_degrade(a, dtype=torch.float32)
    px = ctx.frames_degrade(b, dtype=torch.uint8)
    ctx.sync()
    assert same.dtype == torch.uint8 and torch.equal(same, a)
    assert up.dtype == torch.float32 and np.array_equal(host(up), f8.astype(np.float32))
    assert px.dtype == torch.uint8 and np.array_equal(host(px), R.px_u8(f32))
    assert ctx.frames_degrade(b).dtype == torch.float32                           # dtype defaults to the source's


@pytest.mark.parametrize("blur", [0, 3])
@pytest.mark.parametrize("shape", [(2, 3, 16, 12), (2, 2, 9, 7)], ids=_id)
def test_a_batch_split_gives_the_same_frames(ctx, shape, blur):
    """degrade(B = 2, first_frame = f)[1] == degrade(B = 1, first_frame = f + 1)[0]: what a data-parallel rank relies on"""
    src = _dev(_sources(shape)[0], ctx)
    for first in (0, FIRST, 2 ** 64 - 2):
        both = ctx.frames_degrade(src, blur, 25.0, 0.02, SEED, first)
        one = ctx.frames_degrade(src[1:].clone(), blur, 25.0, 0.02, SEED, first + 1)
        zero = ctx.frames_degrade(src[:1].clone(), blur, 25.0, 0.02, SEED, first)
        ctx.sync()
        assert torch.equal(both[1:], one) and torch.equal(both[:1], zero) and not torch.equal(both[:1], both[1:])
    again = ctx.frames_degrade(src, blur, 25.0, 0.02, SEED, 0)                    # the same arguments: the same bytes
    other = ctx.frames_degrade(src, blur, 25.0, 0.02, SEED + 1, 0)
    ctx.sync()
    assert torch.equal(again, ctx.frames_degrade(src, blur, 25.0, 0.02, SEED, 0)) and not torch.equal(again, other)


@pytest.mark.parametrize("blur", [0, 1])
def test_element_offsets_beyond_2_to_the_31(ctx, blur):
    """33 frames of 4 x 4096 x 4096: frame 32 starts at element 2^31 of the batch.  By the batch-split identity it equals the same frame degraded
    alone with its own number (whose offsets are small), and so does frame 31, which ends there; on the device, no host reference of 2^31 elements"""
    B, D, N = 33, 4, 4096
    src = torch.randint(0, 256, (B, D, N, N), dtype=torch.uint8, device=f"cuda:{ctx.device}")
    assert src.numel() > 2 ** 31
    out = ctx.frames_degrade(src, blur, 25.0, 0.02, SEED, FIRST)
    for b in (31, 32):
        alone = ctx.frames_degrade(src[b:b + 1], blur, 25.0, 0.02, SEED, FIRST + b)
        ctx.sync()
        assert torch.equal(out[b:b + 1], alone) and not torch.equal(alone, src[b:b + 1]), (blur, b)
    del src, out, alone
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(2, 3, 16, 12), (1, 2, 9, 7)], ids=_id)
def test_in_place_equals_out_of_place(ctx, shape):
    for k, dtype in enumerate((torch.uint8, torch.float32)):
        src = _dev(_sources(shape)[k], ctx)
        apart = ctx.frames_degrade(src, 0, 25.0, 0.02, SEED, FIRST)
        work = src.clone()
        assert ctx.frames_degrade(work, 0, 25.0, 0.02, SEED, FIRST, out=work) is work
        ctx.sync()
        assert apart.dtype == dtype and work.dtype == dtype
        assert np.array_equal(host(apart).view(np.uint8), host(work).view(np.uint8)) and not np.array_equal(host(work).view(np.uint8), host(src).view(np.uint8))


@pytest.mark.parametrize("blur", BLURS)
def test_a_constant_frame_stays_constant(ctx, blur):
    for value, shape in ((0, (1, 2, 9, 7)), (77, (2, 3, 130, 70)), (255, (1, 1, 64, 64))):
        for dtype in (torch.uint8, torch.float32):
            f = torch.full(shape, value, dtype=dtype, device=f"cuda:{ctx.device}")
            for out in (torch.uint8, torch.float32):
                got = ctx.frames_degrade(f, blur, dtype=out)
                ctx.sync()
                assert (host(got) == value).all(), (blur, value, shape, dtype, out)


@pytest.mark.parametrize("Ny", [40, 41])
def test_a_delta_under_blur_4_is_the_outer_product_of_the_weights(ctx, Ny):
    delta = np.zeros((1, 1, 37, Ny), np.uint8)
    delta[0, 0, 30, 33] = 255                                                    # (its footprint crosses the tile edge at row 32)
    w = R.weights(4).astype(np.float64)
    want = np.zeros((37, Ny))
    want[26:35, 29:38] = 255 * np.outer(w, w) / 65536
    got = ctx.frames_degrade(_dev(delta, ctx), 4, dtype=torch.float32)
    ctx.sync()
    assert np.array_equal(host(got)[0, 0], want.astype(np.float32)) and want.sum() == 255.0


# ------------------------------------------------------------------------------------------
# 3. captured once and replayed
# ------------------------------------------------------------------------------------------
def test_the_call_is_captured_once_and_replayed():
    shape = (2, 3, 130, 70)
    f8 = np.random.default_rng(4).integers(0, 256, shape, dtype=np.uint8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        frames = torch.zeros(shape, dtype=torch.uint8, device=dev)
        out8 = torch.full(shape, 0xEE, dtype=torch.uint8, device=dev)
        out32 = torch.zeros(shape, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.frames_degrade(frames, 2, 25.0, 0.02, SEED, FIRST, out=out8)
            c.frames_degrade(frames, 0, 1.5, 0.0, SEED, FIRST, out=out32)
        torch.cuda.synchronize()
        frames.copy_(_dev(f8, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager8 = c.frames_degrade(frames, 2, 25.0, 0.02, SEED, FIRST)
        eager32 = c.frames_degrade(frames, 0, 1.5, 0.0, SEED, FIRST, dtype=torch.float32)
        c.sync()
        assert torch.equal(out8, eager8) and torch.equal(out32, eager32)
        assert np.array_equal(host(out8), R.degrade(f8, 2, 25.0, 0.02, SEED, FIRST))
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    B, D, Nx, Ny = 2, 3, 8, 8
    n = B * D * Nx * Ny
    dev = f"cuda:{ctx.device}"
    a = torch.full((4 * n + 64,), 0x3C, dtype=torch.uint8, device=dev)
    b = torch.full((4 * n + 64,), 0xC3, dtype=torch.uint8, device=dev)
    ap, bp = a.data_ptr(), b.data_ptr()
    assert ap % 16 == 0 and bp % 16 == 0
    inf, nan = float("inf"), float("nan")
    # (src, src_u8, dst, dst_u8, B, D, Nx, Ny, blur, sigma, impulse, seed, first_frame), the whole message behind the call's name
    # the rules' full texts, as the library words them
    NULL, DIM, RANGE = "null context, source or destination", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and Nx, Ny in 1..8192"
    BLUR, SIGMA, IMPULSE = "blur must be 0..4", "sigma must be finite and in 0..255", "impulse must be finite and in 0..1"
    ALIGN = "src_d and dst_d must be 16-byte aligned"
    OVERLAP = "the source and destination ranges overlap (in place needs dst_d == src_d, blur == 0 and src_u8 == dst_u8)"
    cases = [
        ("null source", (None, 1, bp, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), NULL),
        ("null destination", (ap, 1, None, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), NULL),
        ("D = 0", (ap, 1, bp, 1, B, 0, Nx, Ny, 0, 1.0, 0.0, 1, 0), DIM),
        ("D = 5", (ap, 1, bp, 1, 1, 5, Nx, Ny, 0, 1.0, 0.0, 1, 0), DIM),
        ("B = 0", (ap, 1, bp, 1, 0, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), RANGE),
        ("Nx = 0", (ap, 1, bp, 1, B, D, 0, Ny, 0, 1.0, 0.0, 1, 0), RANGE),
        ("Ny = 8193", (ap, 1, bp, 1, B, D, Nx, 8193, 0, 1.0, 0.0, 1, 0), RANGE),
        ("blur = 5", (ap, 1, bp, 1, B, D, Nx, Ny, 5, 1.0, 0.0, 1, 0), BLUR),
        ("blur = -1", (ap, 1, bp, 1, B, D, Nx, Ny, -1, 1.0, 0.0, 1, 0), BLUR),
        ("sigma = -1", (ap, 1, bp, 1, B, D, Nx, Ny, 0, -1.0, 0.0, 1, 0), SIGMA),
        ("sigma = 255.5", (ap, 1, bp, 1, B, D, Nx, Ny, 0, 255.5, 0.0, 1, 0), SIGMA),
        ("sigma = nan", (ap, 1, bp, 1, B, D, Nx, Ny, 0, nan, 0.0, 1, 0), SIGMA),
        ("sigma = inf", (ap, 1, bp, 1, B, D, Nx, Ny, 0, inf, 0.0, 1, 0), SIGMA),
        ("impulse = -0.5", (ap, 1, bp, 1, B, D, Nx, Ny, 0, 1.0, -0.5, 1, 0), IMPULSE),
        ("impulse = 1.5", (ap, 1, bp, 1, B, D, Nx, Ny, 0, 1.0, 1.5, 1, 0), IMPULSE),
        ("impulse = nan", (ap, 1, bp, 1, B, D, Nx, Ny, 0, 1.0, nan, 1, 0), IMPULSE),
        ("source off by 4", (ap + 4, 0, bp, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), ALIGN),
        ("destination off by 8", (ap, 1, bp + 8, 0, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), ALIGN),
        ("in place with a blur", (ap, 1, ap, 1, B, D, Nx, Ny, 1, 1.0, 0.0, 1, 0), OVERLAP),
        ("in place with another type", (ap, 1, ap, 0, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), OVERLAP),
        ("in place with another type, float source", (ap, 0, ap, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), OVERLAP),
        ("overlap: shifted by 16", (ap, 1, ap + 16, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), OVERLAP),
        ("overlap: the destination ends in the source", (ap + n - 16, 1, ap, 1, B, D, Nx, Ny, 0, 1.0, 0.0, 1, 0), OVERLAP),
        ("overlap: the float destination reaches the source", (ap + 4 * n - 16, 1, ap, 0, B, D, Nx, Ny, 2, 1.0, 0.0, 1, 0), OVERLAP),
    ]
    # (sizes that overflow the address space cannot be reached through int arguments where size_t has 64 bits: B D Nx Ny 4 <= 2^61)
    for what, args, rule in cases:
        assert L.aefft_frames_degrade(ctx.h, *args) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_frames_degrade: " + rule, (what, msg)
    ctx.sync()
    assert (host(a) == 0x3C).all() and (host(b) == 0xC3).all()
    # what is NOT an error: the limits of sigma and impulse, neighbouring ranges, the in-place form
    assert L.aefft_frames_degrade(ctx.h, ap, 1, ap + n, 1, B, D, Nx, Ny, 4, 255.0, 1.0, 2 ** 64 - 1, 2 ** 64 - 1) == aefft.OK
    assert L.aefft_frames_degrade(ctx.h, bp, 1, bp, 1, 4 * B, D, Nx, Ny, 0, 0.0, 0.0, 0, 0) == aefft.OK        # (in place, all zero: a copy)
    ctx.sync()
    got = host(a)
    assert (got[:n] == 0x3C).all() and set(np.unique(got[n:2 * n])) <= {0, 255} and (got[2 * n:] == 0x3C).all() and (host(b) == 0xC3).all()
    # the binding refuses what the C call would, before it reaches the library; a library error surfaces with its message
    f = a[:n].view(B, D, Nx, Ny)
    for kw in (dict(blur=5), dict(sigma=-1.0), dict(impulse=2.0), dict(seed=-1), dict(dtype=torch.float64), dict(blur=1, out=f),
               dict(out=torch.empty(B, D, Nx, Ny + 1, dtype=torch.uint8, device=dev))):
        with pytest.raises(ValueError):
            ctx.frames_degrade(f, **kw)
    with pytest.raises(ValueError):
        ctx.frames_degrade(f.permute(0, 1, 3, 2))
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.frames_degrade(f, 1, out=a[16:16 + n].view(B, D, Nx, Ny))


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
PROFILE_NAMES = ["r2c_rows", "r2c_cols", "c2r_cols", "c2r_rows", "contract", "resize", "diff_mse", "bias_grad", "pad", "shrink", "update", "gradient_diff",
                 "spatial", "kspec", "kgrad", "weight_taps", "moment", "chain", "sgrad", "opmse", "score", "score_map", "image", "target", "ssim"]


def test_one_call_is_one_image_launch_with_its_bytes(ctx):
    shape = (2, 3, 66, 34)
    n = int(np.prod(shape))
    dev = f"cuda:{ctx.device}"
    f8 = torch.zeros(shape, dtype=torch.uint8, device=dev)
    f32 = torch.zeros(shape, dtype=torch.float32, device=dev)
    assert [ctx.L.aefft_prof_name(k).decode() for k in range(ctx.L.aefft_prof_count())] == PROFILE_NAMES
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.frames_degrade(f8, 2, 25.0, 0.02)
        one = ctx.prof_read()
        ctx.frames_degrade(f8, 0, 25.0, out=f32)
        two = ctx.prof_read()
        ctx.frames_degrade(f32, 1, out=f8)
        three = ctx.prof_read()
        ctx.frames_degrade(f32, 0, 1.0, out=f32)
        four = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert list(four) == PROFILE_NAMES
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == 2 * n
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == 7 * n
    assert three["image"]["launches"] == 3 and three["image"]["bytes"] == 12 * n
    assert four["image"]["launches"] == 4 and four["image"]["bytes"] == 20 * n
    assert sum(v["launches"] for v in four.values()) == 4


# ------------------------------------------------------------------------------------------
# 6. the call in front of the target step and the target score of a small net
# ------------------------------------------------------------------------------------------
def test_degraded_frames_feed_the_target_step_and_score(ctx):
    """a 64^2 net of one pair: frames_degrade's 8-bit and float outputs go straight into step_grad_target and score_target; the packed gradient
    buffer and the scores equal, bit for bit, those from the same arrays uploaded from the restatement"""
    D, N, B, dM, Nk = 3, 64, 2, 4, 5
    rng = np.random.default_rng(12)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    c, f = q32(0.1 * rng.uniform(-1, 1, (dM, D, Nk, Nk))), q32(0.1 * rng.uniform(-1, 1, (D, dM, Nk, Nk)))
    bias, p = q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, D))
    clean_h = rng.integers(0, 256, (B, D, N, N), dtype=np.uint8)
    clean = _dev(clean_h, ctx)
    net = aefft.Net(ctx, D, N, N, [dM], Nk, 2, batch=B)
    try:
        net.set_pair(0, c, bias, f, p)
        for dtype in (torch.uint8, torch.float32):
            ours = ctx.frames_degrade(clean, 2, 25.0, 0.02, SEED, 5, dtype=dtype)            # (queued in front of the net: nothing waits in between)
            net.step_grad_target(ours, clean, None)
            s_ours, _ = net.score_target(ours, clean)
            ctx.sync()
            g_ours, s_ours = host(net.grad_buffer()).copy(), host(s_ours).copy()
            theirs_h = R.degrade(clean_h, 2, 25.0, 0.02, SEED, 5, dtype=NP[dtype])
            assert np.array_equal(host(ours), theirs_h) and not np.array_equal(theirs_h.astype(np.float32), clean_h.astype(np.float32))
            theirs = _dev(theirs_h, ctx)
            net.step_grad_target(theirs, clean, None)
            s_theirs, _ = net.score_target(theirs, clean)
            ctx.sync()
            g_theirs = host(net.grad_buffer())
            assert np.isfinite(g_ours).all() and np.abs(g_ours).max() > 0 and (s_ours > 0).all()
            assert np.array_equal(g_ours.view(np.uint32), g_theirs.view(np.uint32)), dtype
            assert np.array_equal(s_ours.view(np.uint32), host(s_theirs).view(np.uint32)), dtype
    finally:
        net.close()
