"""aefft_image_compare_map (Context.image_compare_map) and Net.score_tiled on the device against the numpy restatement of compare_ref.py -- EXACT
equality of the float bits everywhere, map and score, both metrics: the shapes at which each mechanism of the kernel can go wrong, B = 1 and 3,
the four image layouts applied to a and b independently (every pairing of the dword and the byte route), a region of interest, a_d == b_d, a
skipped score, the bytes behind the map, one graph capture and replay, the cell rule against aefft_map_overlay_image, tiled scoring of a small net, every AEFFT_EINVAL rule
and the profile entry."""
import functools
import importlib

import numpy as np
import pytest
import torch

import compare_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

# (W, H, Mx, My, D), B: cells of 3 and 4 pixels with a dword straddling two cells and three channels; one-pixel cells; a all 0 against b all 255, the
# largest sums (64 x 64 x 4); cells of 43 / 44 x 35; odd everything at D = 2; a span of cells wider than one workgroup's; a plain grid of 8 x 8 cells;
# sensor resolution with rows in cells of 15 and 16
SHAPES = [((13, 9, 4, 3, 3), 1), ((5, 5, 5, 5, 1), 1), ((128, 64, 2, 1, 4), 1), ((130, 70, 3, 2, 3), 1), ((65, 67, 5, 7, 2), 1), ((641, 37, 11, 1, 3), 1),
          ((256, 256, 32, 32, 3), 1), ((1920, 1080, 120, 68, 3), 2)]
EXTREME = (128, 64, 2, 1, 4)
METRICS = ("mse", "ssim")
TAIL = 24                                                                        # floats of the map's allocation behind its live entries: the guard
LAYOUTS = ["tight", "words", "odd", "skewed"]                                    # as test_gpu_tiles.py: the first two take the dword route (tight: where W D % 4 == 0)
_id = lambda v: "-".join(str(q) for q in v) if isinstance(v, tuple) else str(v)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")


@functools.lru_cache(maxsize=None)
def _pair(shape, B):
    """(a, b, {metric: (map, score) of the restatement}), computed once and read-only: b is a with noise on it, so that the SSIM is not trivial"""
    W, H, Mx, My, D = shape
    rng = np.random.default_rng(W * 131 + H * 7 + D + B)
    a = rng.integers(0, 256, (B, H, W, D), dtype=np.uint8)
    b = (a.astype(np.int64) + rng.integers(-40, 41, a.shape)).clip(0, 255).astype(np.uint8)
    b[:, : H // 2, : W // 3] = rng.integers(0, 256, b[:, : H // 2, : W // 3].shape, dtype=np.uint8)      # ... and one unrelated corner
    if shape == EXTREME:
        a[...], b[...] = 0, 255
    want = {m: R.compare(a, b, (Mx, My), m) for m in METRICS}
    for v in (a, b) + tuple(x for w in want.values() for x in w):
        v.setflags(write=False)
    return a, b, want


def _layout(W, H, D, B, layout):
    fill = -W * D % 4
    pad, gap, skew = {"tight": (0, 0, 0), "words": (fill + 4, fill + 8, 0), "odd": (1 + W * D % 2, 5, 0), "skewed": (fill, fill + 4, 1)}[layout]
    pitch = W * D + pad
    stride = (H - 1) * pitch + W * D + gap
    return pitch, stride, skew, skew + (B - 1) * stride + (H - 1) * pitch + W * D      # the last: bytes up to the last live byte


def _laid_out(img, layout, ctx):
    """the device view [B][H][W][D] of `img` under `layout`, in an allocation that ends with the image's last live byte"""
    B, H, W, D = img.shape
    pitch, stride, skew, live = _layout(W, H, D, B, layout)
    flat = np.random.default_rng(3).integers(0, 256, live, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(flat[skew:], (B, H, W, D), (stride, pitch, D, 1))[...] = img
    return _dev(flat, ctx)[skew:].as_strided((B, H, W, D), (stride, pitch, D, 1))


def _words(t):
    """does the library take this image by aligned dwords?"""
    B, H = t.shape[:2]
    return (t.data_ptr() | (t.stride(1) if H > 1 else 0) | (t.stride(0) if B > 1 else 0)) % 4 == 0


def _check(ctx, a, b, shape, want, what):
    W, H, Mx, My, D = shape
    B = a.shape[0]
    n = B * Mx * My
    for metric in METRICS:
        guard = np.random.default_rng(9).uniform(-5, 5, n + TAIL).astype(np.float32)
        buf = _dev(guard, ctx)
        m, s = ctx.image_compare_map(a, b, (Mx, My), metric, map=buf[:n].view(B, Mx, My))
        ctx.sync()
        got = host(buf)
        bad = int((bits(got[:n]) != bits(want[metric][0]).reshape(-1)).sum())
        print(what, metric, "map entries whose bits differ:", bad, "score:", host(s), "want:", want[metric][1])
        assert m.data_ptr() == buf.data_ptr() and bad == 0, (what, metric)
        assert np.array_equal(bits(got[n:]), bits(guard[n:])), "the floats behind the map changed"
        assert s.dtype == torch.float32 and tuple(s.shape) == (B,) and np.array_equal(bits(host(s)), bits(want[metric][1])), (what, metric)


# ------------------------------------------------------------------------------------------
# 1. exact equality with the restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", SHAPES, ids=_id)
def test_map_and_score_equal_the_restatement(ctx, shape, B):
    a, b, want = _pair(shape, B)
    _check(ctx, _dev(a, ctx), _dev(b, ctx), shape, want, (shape, B))
    if shape == EXTREME:
        assert (want["mse"][0] == 65025.0).all() and (want["mse"][1] == 65025.0).all()


@pytest.mark.parametrize("shape", [(13, 9, 4, 3, 3), (130, 70, 3, 2, 3), (65, 67, 5, 7, 2), (5, 5, 5, 5, 1)], ids=_id)
def test_a_batch_of_three(ctx, shape):
    a, b, want = _pair(shape, 3)
    _check(ctx, _dev(a, ctx), _dev(b, ctx), shape, want, (shape, 3))


@pytest.mark.parametrize("lb", LAYOUTS)
@pytest.mark.parametrize("la", LAYOUTS)
def test_each_image_takes_its_own_layout(ctx, la, lb):
    """the four layouts for a and b independently, B = 3: the same bits whatever route either side takes"""
    for shape in ((13, 9, 4, 3, 3), (65, 67, 5, 7, 2)):
        a, b, want = _pair(shape, 3)
        da, db = _laid_out(a, la, ctx), _laid_out(b, lb, ctx)
        W, D = shape[0], shape[4]
        assert _words(da) == (la == "words" or (la == "tight" and W * D % 4 == 0)) and _words(db) == (lb == "words" or (lb == "tight" and W * D % 4 == 0))
        _check(ctx, da, db, shape, want, (shape, la, lb))


def test_the_layouts_pair_the_dword_route_with_the_byte_route_both_ways(ctx):
    a, b, _ = _pair((13, 9, 4, 3, 3), 3)
    routes = {(la, lb): (_words(_laid_out(a, la, ctx)), _words(_laid_out(b, lb, ctx))) for la in LAYOUTS for lb in LAYOUTS}
    assert routes["words", "odd"] == (True, False) and routes["skewed", "words"] == (False, True)
    assert set(routes.values()) == {(True, True), (True, False), (False, True), (False, False)}


def test_a_region_of_interest_and_one_buffer_for_both(ctx):
    shape = (13, 9, 4, 3, 3)
    a, b, want = _pair(shape, 3)
    big = _dev(np.random.default_rng(4).integers(0, 256, (3, 20, 30, 3), dtype=np.uint8), ctx)
    roi = big[:, 3:12, 5:18]
    roi[...] = _dev(a, ctx)
    before = host(big)
    _check(ctx, roi, _dev(b, ctx), shape, want, "a is a region of interest")
    swapped = {m: R.compare(b, a, shape[2:4], m) for m in METRICS}
    _check(ctx, _dev(b, ctx), roi, shape, swapped, "b is a region of interest")
    assert np.array_equal(host(big), before)
    for m in METRICS:                                                             # (the definition is symmetric)
        assert np.array_equal(bits(swapped[m][0]), bits(want[m][0]))
    # a_d == b_d: exactly 0.0 and exactly 1.0
    for src in (roi, _dev(a, ctx)):
        m, s = ctx.image_compare_map(src, src, (4, 3), "mse")
        ctx.sync()
        assert (bits(host(m)) == 0).all() and (bits(host(s)) == 0).all()
        m, s = ctx.image_compare_map(src, src, (4, 3), "ssim")
        ctx.sync()
        assert (host(m) == np.float32(1.0)).all() and (host(s) == np.float32(1.0)).all()


def test_a_null_score_is_left_alone(ctx):
    shape = (130, 70, 3, 2, 3)
    a, b, want = _pair(shape, 1)
    L = ctx.L
    da, db = _dev(a, ctx), _dev(b, ctx)
    for k, metric in enumerate(METRICS):
        m, s = ctx.image_compare_map(da, db, (3, 2), metric, score=False)
        ctx.sync()
        assert s is None and np.array_equal(bits(host(m)), bits(want[metric][0]))
        # the map in front of a buffer of -7.0, where a score would most likely be written by mistake: six entries, then floats that stay
        buf = torch.full((6 + TAIL,), -7.0, device=da.device)
        assert L.aefft_image_compare_map(ctx.h, da.data_ptr(), 390, 0, db.data_ptr(), 390, 0, 130, 70, 1, 3, k, 3, 2, buf.data_ptr(), None) == aefft.OK
        ctx.sync()
        assert np.array_equal(bits(host(buf)[:6]), bits(want[metric][0]).reshape(-1)) and (host(buf)[6:] == -7.0).all()


def test_both_launches_are_captured_once_and_replayed():
    shape = (130, 70, 3, 2, 3)
    a, b, want = _pair(shape, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        da, db = torch.zeros(a.shape, dtype=torch.uint8, device=dev), torch.zeros(a.shape, dtype=torch.uint8, device=dev)
        m, s = torch.full((3, 3, 2), -1.0, device=dev), torch.full((3,), -1.0, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.image_compare_map(da, db, (3, 2), "ssim", map=m, score=s)
        torch.cuda.synchronize()
        da.copy_(_dev(a, c)); db.copy_(_dev(b, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(host(m)), bits(want["ssim"][0])) and np.array_equal(bits(host(s)), bits(want["ssim"][1]))
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 2. the cell rule is the overlay's
# ------------------------------------------------------------------------------------------
def test_the_overlay_paints_exactly_the_pixels_an_entry_was_computed_from(ctx):
    W, H, Mx, My, D = 13, 9, 4, 3, 3
    a = _pair((W, H, Mx, My, D), 1)[0]
    ex, ey = R.edges(W, Mx), R.edges(H, My)
    lut = np.full((256, D), 200, np.uint8)
    lut[0] = 10                                                                   # two colours: entry 0, and everything above
    for I in range(Mx):
        for J in range(My):
            b = a.copy()
            b[:, ey[J]:ey[J + 1], ex[I]:ex[I + 1]] ^= 0x55                         # every pixel of cell (I, J), nothing else
            m, _ = ctx.image_compare_map(_dev(a, ctx), _dev(b, ctx), (Mx, My), "mse", score=False)
            canvas = torch.zeros(1, H, W, D, dtype=torch.uint8, device=m.device)
            ctx.map_overlay(m, canvas, _dev(lut, ctx), 0.0, 1.0, alpha=256, smooth=False)
            ctx.sync()
            got = host(m)[0]
            assert got[I, J] > 0 and (np.delete(got.reshape(-1), I * My + J) == 0).all(), (I, J)
            painted = (host(canvas) == 200).all(axis=3)
            assert np.array_equal(painted, (a != b).any(axis=3)) and ((host(canvas) == 200) | (host(canvas) == 10)).all(), (I, J)


# ------------------------------------------------------------------------------------------
# 3. tiled scoring of a small net
# ------------------------------------------------------------------------------------------
def test_score_tiled_is_infer_tiled_then_compare(ctx):
    """a 3 -> 4 -> 3 net with 5 x 5 kernels, scale 2, 64 x 64 tiles, batch 2, on two 130 x 70 x 3 images with overlap 16, rim 4 and cells of about 16
    pixels: `out` holds Net.infer_tiled's bytes, map and score equal the restatement of (image, out) -- and of (target, out) -- bit for bit"""
    D, N, Bn, dM, Nk, W, H, V, M = 3, 64, 2, 4, 5, 130, 70, 16, 4
    rng = np.random.default_rng(21)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    c, f = q32(0.1 * rng.uniform(-1, 1, (dM, D, Nk, Nk))), q32(0.1 * rng.uniform(-1, 1, (D, dM, Nk, Nk)))
    bias, p = q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, D))
    image = rng.integers(0, 256, (2, H, W, D), dtype=np.uint8)
    target = rng.integers(0, 256, (2, H, W, D), dtype=np.uint8)
    cells = aefft.cells_for_tile(W, H, 16)
    assert cells == (9, 5)
    net = aefft.Net(ctx, D, N, N, [dM], Nk, 2, batch=Bn)
    try:
        net.set_pair(0, c, bias, f, p)
        img, tgt = _dev(image, ctx), _dev(target, ctx)
        plain = net.infer_tiled(img, V, M)
        ctx.sync()
        recon = host(plain)
        assert recon.std() > 0 and not np.array_equal(recon, image)
        for metric in METRICS:
            m, s, out = net.score_tiled(img, V, M, tile=16, metric=metric)
            ctx.sync()
            want = R.compare(image, recon, cells, metric)
            assert np.array_equal(host(out), recon) and tuple(m.shape) == (2, 9, 5)
            assert np.array_equal(bits(host(m)), bits(want[0])) and np.array_equal(bits(host(s)), bits(want[1])), metric
            given = torch.full((2, H, W, D), 0xEE, dtype=torch.uint8, device=img.device)
            m, s, out = net.score_tiled(img, V, M, tile=16, metric=metric, target=tgt, out=given)
            ctx.sync()
            want = R.compare(target, recon, cells, metric)
            assert out is given and np.array_equal(host(given), recon)
            assert np.array_equal(bits(host(m)), bits(want[0])) and np.array_equal(bits(host(s)), bits(want[1])), (metric, "target")
        m, s, _ = net.score_tiled(img, V, M, tile=(32, 35), score=False)
        assert s is None and tuple(m.shape) == (2, 5, 2)
        with pytest.raises(ValueError):
            net.score_tiled(img, V, M, tile=65)
        with pytest.raises(ValueError):
            net.score_tiled(img, V, M, target=tgt[:, :, :100])
    finally:
        net.close()
    spatial = aefft.Net(ctx, D, 16, 16, [8], 3, 1, batch=Bn, spatial=True)
    try:
        with pytest.raises(ValueError, match="spatial"):
            spatial.score_tiled(_dev(image, ctx), V, M)
    finally:
        spatial.close()


# ------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    W, H, D, Mx, My = 13, 9, 3, 4, 3
    pitch, stride = W * D, H * W * D
    dev = f"cuda:{ctx.device}"
    a = torch.full((8192,), 0x3C, dtype=torch.uint8, device=dev)                  # both images
    o = torch.full((2048,), -3.0, device=dev)                                     # the map and the score
    ap, op = a.data_ptr(), o.data_ptr()
    bp, mp, sp = ap + 2048, op, op + 4096
    assert ap % 16 == 0 and op % 16 == 0
    good = dict(a=ap, apitch=pitch, astride=stride, b=bp, bpitch=pitch, bstride=stride, W=W, H=H, B=2, D=D, metric=0, Mx=Mx, My=My, map=mp, score=sp)
    call = lambda **kw: L.aefft_image_compare_map(ctx.h, *dict(good, **kw).values())
    NULL, DIM, RANGE = "null context, image or map", "D must be 1..4 (grey, BGR, BGRA)", "B must be >= 1 and W, H in 1..8192"
    CELLS, SIDE = "Mx must be in 1..min(W, 1024) and My in 1..min(H, 1024)", "a cell side above 64: ceil(W / Mx) and ceil(H / My) must be at most 64"
    METRIC, ALIGN = "metric must be AEFFT_COMPARE_MSE or AEFFT_COMPARE_SSIM", "map_d and score_d must be 16-byte aligned"
    PITCH, STRIDE = "pitch must be at least W * D bytes", "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"
    ROWS_FIT, BATCH_FIT = "H * pitch does not fit the address space", "B * image_stride does not fit the address space"
    FIT = "B * Mx * My does not fit the address space or B * My an int"
    cases = [
        ("null a", dict(a=None), NULL), ("null b", dict(b=None), NULL), ("null map", dict(map=None), NULL),
        ("W = 0", dict(W=0), RANGE), ("W = 8193", dict(W=8193), RANGE), ("H = 0", dict(H=0), RANGE), ("H = 8193", dict(H=8193), RANGE), ("B = 0", dict(B=0), RANGE),
        ("D = 0", dict(D=0), DIM), ("D = 5", dict(D=5), DIM),
        ("Mx = 0", dict(Mx=0), CELLS), ("Mx > W", dict(Mx=14), CELLS), ("My = 0", dict(My=0), CELLS), ("My > H", dict(My=10), CELLS),
        ("Mx > 1024", dict(W=2000, Mx=1025), CELLS), ("My < 0", dict(My=-1), CELLS),
        ("cells of 65 columns", dict(W=130, Mx=2), SIDE), ("cells of 65 rows", dict(H=65, My=1), SIDE),
        ("metric 2", dict(metric=2), METRIC), ("metric -1", dict(metric=-1), METRIC),
        ("a's pitch too small", dict(apitch=pitch - 1), "a_d: " + PITCH), ("b's pitch too small", dict(bpitch=pitch - 1), "b_d: " + PITCH),
        ("a's stride too small", dict(astride=stride - 1), "a_d: " + STRIDE), ("b's stride too small", dict(bstride=stride - 1), "b_d: " + STRIDE),
        ("a pitch that overflows", dict(apitch=2 ** 62), "a_d: " + ROWS_FIT), ("a stride that overflows", dict(bstride=2 ** 63, B=3), "b_d: " + BATCH_FIT),
        ("map off by 4", dict(map=mp + 4), ALIGN), ("score off by 8", dict(score=sp + 8), ALIGN),
        ("the map begins in a", dict(map=ap + 16), "the map and image ranges overlap"),
        ("b begins in the map", dict(b=mp + 2 * Mx * My * 4 - 1), "the map and image ranges overlap"),
        ("the score lies in b", dict(score=bp + 32), "the score and image ranges overlap"),
        ("the score lies in the map", dict(score=mp + 16), "the score and map ranges overlap"),
        ("cell rows beyond an int", dict(B=2 ** 31 - 1), FIT),
    ]
    for what, kw, rule in cases:
        assert call(**kw) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_image_compare_map: " + rule, (what, msg)
        assert call(**dict(kw, metric=kw.get("metric", 1))) == aefft.EINVAL, what
    ctx.sync()
    assert (host(a) == 0x3C).all() and (host(o) == -3.0).all()
    # what is NOT an error: neighbouring ranges, strides that are ignored for B == 1, a == b, no score; and the call is right afterwards
    assert call(B=1, astride=0, bstride=1, b=ap, map=mp, score=mp + Mx * My * 4) == aefft.OK
    ctx.sync()
    got = host(o)
    assert (got[:Mx * My] == 0.0).all() and got[Mx * My] == 0.0 and (got[Mx * My + 1:] == -3.0).all()
    A, Bv, want = _pair((W, H, Mx, My, D), 3)
    a[:A.size] = _dev(A, ctx).reshape(-1)
    a[2048:2048 + Bv.size] = _dev(Bv, ctx).reshape(-1)
    for k, metric in enumerate(METRICS):
        assert call(B=3, metric=k) == aefft.OK
        ctx.sync()
        got = host(o)
        assert np.array_equal(bits(got[:3 * Mx * My]), bits(want[metric][0]).reshape(-1)) and np.array_equal(bits(got[1024:1027]), bits(want[metric][1]))
    # the binding refuses what the C call would, before it reaches the library; a library error surfaces with its message
    img = a[:2 * stride].view(2, H, W, D)
    for kw in (dict(cells=(14, 3)), dict(metric="psnr"), dict(map=torch.empty(2, 3, 4, device=dev)), dict(score=torch.empty(3, device=dev))):
        with pytest.raises(ValueError):
            ctx.image_compare_map(img, img, **dict(dict(cells=(Mx, My)), **kw))
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.image_compare_map(img, img, (Mx, My), map=a[:2 * Mx * My * 4].view(torch.float32).view(2, Mx, My))


# ------------------------------------------------------------------------------------------
# 5. profile accounting
# ------------------------------------------------------------------------------------------
def test_the_call_is_accounted_as_image_launches_with_its_bytes(ctx):
    shape = (130, 70, 3, 2, 3)
    W, H, Mx, My, D = shape
    a, b, _ = _pair(shape, 3)
    da, db = _dev(a, ctx), _dev(b, ctx)
    n = 2 * 3 * W * H * D + 4 * 3 * Mx * My
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.image_compare_map(da, db, (Mx, My), "mse")
        one = ctx.prof_read()
        ctx.image_compare_map(da, db, (Mx, My), "ssim", score=False)
        two = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert one["image"]["launches"] == 2 and one["image"]["bytes"] == n
    assert two["image"]["launches"] == 3 and two["image"]["bytes"] == 2 * n
    assert sum(v["launches"] for v in two.values()) == 3
