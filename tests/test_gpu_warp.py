"""aefft_image_warp_affine and aefft_image_remap (Context.image_warp, Context.image_remap) on the device against warp_ref.py -- EXACT byte equality of
every destination byte, the bytes between the rows, between the images and around the buffers included: destinations of 1 x 1, 17 x 5, 65 x 33 and
130 x 67 (odd, and crossing the 32 x 32 tile and a lane's four pixels in both directions) from sources of other sizes, D = 1..4, B = 1 and 3 with one
affine and with three, the byte route (pointer offset 1, pitch W D + 5) beside the dword route, the affines at which it goes wrong (identity,
translation, both quarter turns, a mirror, a rotation, a minification, entirely outside, the limits of aefft_affine_make, bit patterns beyond them),
both interpolations and the three borders with a constant that differs per channel, the tables (identity, random, INT32_MIN / INT32_MAX / just outside
each edge, an affine's), one graph capture and replay, the profile entries, every AEFFT_EINVAL rule and the chain into aefft_image_compare_map."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import warp_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

SENTINEL = 0x7B
GUARD = 16                                                                       # guard bytes in front of and behind every buffer
# (source W x H, destination W x H): the tile is 32 x 32 and a lane owns four pixels of a row
SHAPES = [((1, 1), (1, 1)), ((1, 9), (17, 5)), ((53, 37), (65, 33)), ((96, 64), (130, 67))]
INTERPS, BORDERS = list(R.INTERP), list(R.BORDER)
COMBOS = [(i, b) for i in INTERPS for b in BORDERS]
VALUE = (200, 100, 50, 25)                                                       # the constant, different in every channel
C30, S30 = 0.8 * np.cos(np.pi / 6), 0.8 * np.sin(np.pi / 6)
Q = 1 << 24
# name -> the six Q24 coefficients for a source of Ws x Hs (floats go through aefft_affine_make's rule; "beyond" are bit patterns it never gives)
AFFINES = {
    "identity": lambda Ws, Hs: R.affine_make([1, 0, 0, 0, 1, 0]),
    "translation": lambda Ws, Hs: R.affine_make([1, 0, -3, 0, 1, 2]),
    "turn_cw": lambda Ws, Hs: R.affine_make([0, 1, 0, -1, 0, Hs - 1]),
    "turn_ccw": lambda Ws, Hs: R.affine_make([0, -1, Ws - 1, 1, 0, 0]),
    "mirror": lambda Ws, Hs: R.affine_make([-1, 0, Ws - 1, 0, 1, 0]),
    "rotation30": lambda Ws, Hs: R.affine_make([C30, -S30, 0.31 * Ws, S30, C30, -0.2 * Hs]),
    "minify3.7": lambda Ws, Hs: R.affine_make([3.7, 0, 0.4, 0, 3.7, -0.3]),
    "half_pixel": lambda Ws, Hs: R.affine_make([1, 0, 0.5, 0, 1, 0.5]),
    "outside": lambda Ws, Hs: R.affine_make([1, 0, 20000, 0, 1, -20000]),
    "limits": lambda Ws, Hs: [R.LIN_LIMIT, -R.LIN_LIMIT, R.OFF_LIMIT, -R.LIN_LIMIT, R.LIN_LIMIT, -R.OFF_LIMIT],
    "beyond": lambda Ws, Hs: [2 ** 62 + 12345, -2 ** 61, 2 ** 63 - 1, 3 ** 39, -2 ** 63, 7 * Ws << 30],
    "beyond2": lambda Ws, Hs: [(Q << 20) + Q, 5, -3 * Q, 2 ** 63 - 1, Q, 2 ** 63 - 4096],
}
NAMES = list(AFFINES)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def source(size, B, D):
    """B random source images of one size, once"""
    W, H = size
    a = np.random.default_rng(W * 131 + H * 7 + B * 3 + D).integers(0, 256, (B, H, W, D), dtype=np.uint8)
    a.setflags(write=False)
    return a


class Buf:
    """B images of W x H x D inside a flat device buffer with guard bytes all round: words=True puts everything on multiples of 4 (the dword route),
    False the pointer at offset 1 with pitch W D + 5 and a stride that is no multiple of 4 (the byte route)"""

    def __init__(self, ctx, B, W, H, D, words, fill):
        self.fill = fill
        self.off = GUARD if words else GUARD + 1
        self.pitch = (W * D + 3) // 4 * 4 + 4 if words else W * D + 5
        one = (H - 1) * self.pitch + W * D
        self.stride = (one + 3) // 4 * 4 + 8 if words else one + 3 + ((one + 3) % 4 == 0)      # (never a multiple of 4)
        self.extent = (B - 1) * self.stride + one
        self.shape = (B, H, W, D)
        self.flat = torch.full((self.off + self.extent + GUARD,), fill, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        self.view = self.flat.as_strided(self.shape, (self.stride, self.pitch, D, 1), self.off)
        assert (self.view.data_ptr() % 4 == 0) == words and (B == 1 or (self.stride % 4 == 0) == words)

    def put(self, a):
        self.view.copy_(torch.as_tensor(np.array(a), device=self.flat.device))
        return self

    def expect(self, a):
        """the whole flat buffer when the images hold `a` and nothing else was written"""
        B, H, W, D = self.shape
        want = np.full(self.flat.numel(), self.fill, np.uint8)
        v = np.lib.stride_tricks.as_strided(want[self.off:], self.shape, (self.stride, self.pitch, D, 1), writeable=True)
        v[...] = a
        return want


def check(buf, want, what):
    got = host(buf.flat)
    exp = buf.expect(want)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at flat offset {bad[0]} (images start at {buf.off}, pitch {buf.pitch}, stride {buf.stride}): "
                             f"got {got[bad[0]]}, want {exp[bad[0]]}")


def _cases():
    """every (shape, affine) once; D, B, the route, one affine or three and the (interp, border) pairs rotate so that each value meets each shape:
    two pairs a case, all six where the case index is a multiple of 5"""
    out = []
    for si in range(len(SHAPES)):
        for ai, name in enumerate(NAMES):
            k = si * len(NAMES) + ai
            combos = COMBOS if k % 5 == 0 else [COMBOS[k % 6], COMBOS[(k + 3 + k // 6) % 6]]
            out.append(pytest.param(si, name, 1 + (si + ai) % 4, 3 if (k // 2) % 2 else 1, bool((k + k // 4) % 2), bool((k // 3) % 2), combos, id=f"{si}-{name}"))
    return out


@pytest.mark.parametrize("si,name,D,B,words,per_image,combos", _cases())
def test_warp_affine_is_the_restatement_byte_for_byte(ctx, si, name, D, B, words, per_image, combos):
    (Ws, Hs), (Wd, Hd) = SHAPES[si]
    src = source((Ws, Hs), B, D)
    nm = B if per_image else 1
    rows = [AFFINES[NAMES[(NAMES.index(name) + b) % len(NAMES)]](Ws, Hs) for b in range(nm)]      # nm == B: three different affines
    q = torch.tensor([[v - 2 ** 64 if v >= 2 ** 63 else v for v in r] for r in rows], dtype=torch.int64, device=f"cuda:{ctx.device}")
    s = Buf(ctx, B, Ws, Hs, D, words, 0xA5).put(src)
    word = R.border_word(VALUE, D)
    for interp, border in combos:
        d = Buf(ctx, B, Wd, Hd, D, words, SENTINEL)
        out = ctx.image_warp(s.view, q, (Wd, Hd), interp, border, VALUE[:D], out=d.view)
        assert out is d.view
        want = R.warp_affine(src, rows[0] if nm == 1 else rows, (Wd, Hd), interp, border, word)
        check(d, want, f"{name} {interp} {border} D {D} B {B} nm {nm} words {words}")
    check(s, src, "the source")                                                  # (only read)


def test_float_matrices_are_quantised_as_affine_make_does_and_the_consequences_hold(ctx):
    """the float path of Context.image_warp (affine_q + upload), the default size and a fresh destination; the header's consequences on the device"""
    src = source((53, 37), 3, 3)
    dev = torch.as_tensor(np.array(src), device=f"cuda:{ctx.device}")
    for interp in INTERPS:
        for border in BORDERS:
            kw = dict(interp=interp, border=border, value=VALUE[:3])
            assert np.array_equal(host(ctx.image_warp(dev, [[1, 0, 0], [0, 1, 0]], **kw)), src)
            assert np.array_equal(host(ctx.image_warp(dev, [[0, 1, 0], [-1, 0, 36]], (37, 53), **kw)), np.rot90(src, -1, axes=(1, 2)))
            assert np.array_equal(host(ctx.image_warp(dev, [[0, -1, 52], [1, 0, 0]], (37, 53), **kw)), np.rot90(src, 1, axes=(1, 2)))
            out = host(ctx.image_warp(dev, [[1, 0, 2], [0, 1, -1]], **kw))
            assert np.array_equal(out[:, 1:, :51], src[:, :36, 2:]) and np.array_equal(out, R.warp_affine(src, R.affine_make([1, 0, 2, 0, 1, -1]), (53, 37), interp, border,
                                                                                                         R.border_word(VALUE, 3)))
        out = host(ctx.image_warp(dev, [[1, 0, 500], [0, 1, 0]], interp=interp, value=VALUE[:3]))
        assert (out == np.array(VALUE[:3], np.uint8)).all()
    ms = [[[C30, -S30, 9.5], [S30, C30, -4.25]], [[1.01, 0.02, -0.3], [-0.015, 0.99, 0.7]], [[-1, 0, 52], [0, -1, 36]]]
    assert np.array_equal(aefft.affine_q(ms), np.array([R.affine_make(m) for m in ms]))
    got = host(ctx.image_warp(dev, ms, border="reflect"))
    assert np.array_equal(got, R.warp_affine(src, [R.affine_make(m) for m in ms], (53, 37), "linear", "reflect"))
    line = torch.tensor([[[10], [20]]], dtype=torch.uint8, device=dev.device)
    assert host(ctx.image_warp(line, [[1, 0, 0.5], [0, 1, 0]], (1, 1))).item() == 15 and host(ctx.image_warp(line, [[1, 0, 0.5], [0, 1, 0]], (1, 1), "nearest")).item() == 20


def _table(kind, src_size, dst_size, rng):
    (Ws, Hs), (Wd, Hd) = src_size, dst_size
    if kind == "identity":
        y, x = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
        return np.stack([2048 * x, 2048 * y], -1).astype(np.int32)
    if kind == "inside":
        return np.stack([rng.integers(0, 2048 * (Ws - 1) + 1, (Hd, Wd)), rng.integers(0, 2048 * (Hs - 1) + 1, (Hd, Wd))], -1).astype(np.int32)
    if kind == "any":
        return rng.integers(-2 ** 31, 2 ** 31, (Hd, Wd, 2)).astype(np.int32)
    xs = np.array([-2 ** 31, 2 ** 31 - 1, -1, -1024, -1025, 2048 * (Ws - 1) + 1, 2048 * Ws - 1024, 2048 * Ws - 1025, 2048 * Ws, 1024], np.int64)
    ys = np.array([-2 ** 31, 2 ** 31 - 1, -1, -1024, -1025, 2048 * (Hs - 1) + 1, 2048 * Hs - 1024, 2048 * Hs - 1025, 2048 * Hs, 1024], np.int64)
    t = np.stack([rng.choice(xs, (Hd, Wd)), rng.choice(ys, (Hd, Wd))], -1)
    inside = rng.random((Hd, Wd)) < 0.3                                          # one coordinate at an extreme, the other inside the image
    t[..., 1] = np.where(inside, rng.integers(0, 2048 * (Hs - 1) + 1, (Hd, Wd)), t[..., 1])
    return t.astype(np.int32)


@pytest.mark.parametrize("si", range(len(SHAPES)))
@pytest.mark.parametrize("kind", ["identity", "inside", "any", "edges"])
def test_remap_is_the_restatement_byte_for_byte(ctx, si, kind):
    src_size, dst_size = SHAPES[si]
    k = si * 4 + ["identity", "inside", "any", "edges"].index(kind)
    D, B, words = 1 + (k + si) % 4, 3 if k % 2 else 1, bool((k // 2) % 2)        # (B = 3: one table for the three images)
    rng = np.random.default_rng(100 + k)
    src = source(src_size, B, D)
    table = _table(kind, src_size, dst_size, rng)
    tab = torch.as_tensor(table, device=f"cuda:{ctx.device}")
    s = Buf(ctx, B, *src_size, D, words, 0xA5).put(src)
    word = R.border_word(VALUE, D)
    for interp, border in (COMBOS if kind == "edges" else [COMBOS[k % 6], COMBOS[(k + 3 + k // 6) % 6]]):
        d = Buf(ctx, B, *dst_size, D, words, SENTINEL)
        ctx.image_remap(s.view, tab, interp, border, VALUE[:D], out=d.view)
        check(d, R.remap(src, table, interp, border, word), f"{kind} {interp} {border} D {D} B {B} words {words}")
    assert np.array_equal(host(tab), table)
    check(s, src, "the source")


def test_remap_with_an_affines_table_is_warp_affine(ctx):
    src = source((96, 64), 3, 3)
    dev = torch.as_tensor(np.array(src), device=f"cuda:{ctx.device}")
    for m in ([[C30, -S30, 20.3], [S30, C30, -11.7]], [[3.7, 0, 0.4], [0, 3.7, -0.3]], [[1, 0, 0.5], [0, 1, 0.5]]):
        table = aefft.affine_table(m, (130, 67))
        tx, ty = R.affine_txty(R.affine_make(m), 130, 67)
        assert np.array_equal(table[..., 0], tx) and np.array_equal(table[..., 1], ty)
        tab = torch.as_tensor(table, device=dev.device)
        for interp, border in COMBOS:
            a = host(ctx.image_warp(dev, m, (130, 67), interp, border, VALUE[:3]))
            b = host(ctx.image_remap(dev, tab, interp, border, VALUE[:3]))
            assert np.array_equal(a, b), (m, interp, border)
    assert np.array_equal(a, R.warp_affine(src, R.affine_make(m), (130, 67), interp, border, R.border_word(VALUE, 3)))


def test_graph_capture_and_replay_of_remap_then_warp():
    src = source((53, 37), 3, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        table = _table("inside", (53, 37), (65, 33), np.random.default_rng(9))
        m = [[C30, -S30, 9.5], [S30, C30, -4.25]]
        tab = torch.as_tensor(table, device=dev)
        q = torch.as_tensor(aefft.affine_q(m), device=dev)
        dsrc = torch.zeros(src.shape, dtype=torch.uint8, device=dev)
        mid = torch.full((3, 33, 65, 3), SENTINEL, dtype=torch.uint8, device=dev)
        out = torch.full((3, 67, 130, 3), SENTINEL, dtype=torch.uint8, device=dev)

        def chain():                                                             # a single chain: no parallel branches
            c.image_remap(dsrc, tab, "linear", "reflect", out=mid)
            c.image_warp(mid, q, (130, 67), "linear", "constant", VALUE[:3], out=out)
        with torch.cuda.stream(side):
            chain()
        torch.cuda.synchronize()
        mid.fill_(SENTINEL); out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain()
        torch.cuda.synchronize()
        assert (host(out) == SENTINEL).all() and (host(mid) == SENTINEL).all()    # nothing ran during the capture
        dsrc.copy_(torch.as_tensor(np.array(src), device=dev))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        wmid = R.remap(src, table, "linear", "reflect")
        assert np.array_equal(host(mid), wmid)
        assert np.array_equal(host(out), R.warp_affine(wmid, R.affine_make(m), (130, 67), "linear", "constant", R.border_word(VALUE, 3)))
        del g
    finally:
        c.close()


def test_the_calls_are_accounted_as_image_entries_with_their_bytes(ctx):
    B, D, (Ws, Hs), (Wd, Hd) = 3, 3, (53, 37), (65, 33)
    dev = torch.as_tensor(np.array(source((Ws, Hs), B, D)), device=f"cuda:{ctx.device}")
    tab = torch.zeros(Hd, Wd, 2, dtype=torch.int32, device=dev.device)
    pix = B * D * (Ws * Hs + Wd * Hd)
    want = [pix + 48, pix + 48 * B, pix + 8 * Wd * Hd]
    eye = [[1, 0, 0], [0, 1, 0]]
    ctx.prof_enable(); ctx.prof_reset()
    try:
        reads = []
        for call in (lambda: ctx.image_warp(dev, eye, (Wd, Hd)), lambda: ctx.image_warp(dev, [eye] * B, (Wd, Hd)), lambda: ctx.image_remap(dev, tab)):
            call()
            ctx.sync()
            reads.append(ctx.prof_read())
    finally:
        ctx.prof_enable(False)
    for k, read in enumerate(reads):
        assert read["image"]["launches"] == k + 1 and read["image"]["bytes"] == sum(want[:k + 1]), (k, read["image"])
        assert sum(v["launches"] for v in read.values()) == k + 1                # one launch each


def test_every_einval_rule_leaves_the_destination_untouched(ctx):
    L = aefft.lib()
    dev = f"cuda:{ctx.device}"
    B, D, Ws, Hs, Wd, Hd = 2, 3, 7, 5, 8, 6
    buf = torch.full((8192,), SENTINEL, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    assert base % 16 == 0
    src, dst, m, tab = base, base + 2048, base + 4096, base + 6144
    sp, ss, dp, ds = Ws * D, Ws * D * Hs, Wd * D, Wd * D * Hd
    warp = dict(src=src, sp=sp, ss=ss, Ws=Ws, Hs=Hs, m=m, nm=1, interp=1, border=0, value=0, dst=dst, dp=dp, ds=ds, Wd=Wd, Hd=Hd, B=B, D=D)
    remap = {k: v for k, v in warp.items() if k != "nm"}
    remap["m"] = tab
    dims, big, huge = "B must be >= 1 and Ws, Hs, Wd, Hd in 1..8192", 1 << 62, 1 << 63      # H * big and (B - 1) * huge pass half the address space
    shared = [("src null", dict(src=None), None), ("dst null", dict(dst=None), None), ("m null", dict(m=None), None),
              ("D 0", dict(D=0), "D must be 1..4 (grey, BGR, BGRA)"), ("D 5", dict(D=5), "D must be 1..4 (grey, BGR, BGRA)"), ("B 0", dict(B=0), dims),
              ("Ws 0", dict(Ws=0), dims), ("Hs 8193", dict(Hs=8193), dims), ("Wd 0", dict(Wd=0), dims), ("Hd 8193", dict(Hd=8193), dims), ("Wd -1", dict(Wd=-1), dims),
              ("interp 2", dict(interp=2), "interp must be AEFFT_WARP_NEAREST or AEFFT_WARP_LINEAR"), ("interp -1", dict(interp=-1), "interp must be AEFFT_WARP_NEAREST or AEFFT_WARP_LINEAR"),
              ("border 3", dict(border=3), "border must be AEFFT_BORDER_CONSTANT, AEFFT_BORDER_REPLICATE or AEFFT_BORDER_REFLECT"),
              ("border -1", dict(border=-1), "border must be AEFFT_BORDER_CONSTANT, AEFFT_BORDER_REPLICATE or AEFFT_BORDER_REFLECT"),
              ("src pitch", dict(sp=sp - 1), "src_d: pitch must be at least W * D bytes"), ("dst pitch", dict(dp=dp - 1), "dst_d: pitch must be at least W * D bytes"),
              ("src stride", dict(ss=ss - 1), "src_d: image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"),
              ("dst stride", dict(ds=ds - 1), "dst_d: image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1"),
              ("src rows overflow", dict(sp=big), "src_d: H * pitch does not fit the address space"), ("dst rows overflow", dict(dp=big), "dst_d: H * pitch does not fit the address space"),
              ("src batch overflow", dict(ss=huge), "src_d: B * image_stride does not fit the address space"),
              ("dst batch overflow", dict(ds=huge), "dst_d: B * image_stride does not fit the address space"),
              ("dst on src", dict(dst=src + ss * B - 1), "the source and destination ranges overlap (the op is out-of-place)"),
              ("dst in src", dict(dst=src), "the source and destination ranges overlap (the op is out-of-place)")]
    cases = {"aefft_image_warp_affine": (L.aefft_image_warp_affine, warp, "null context, source, affines or destination", shared + [
                 ("nm 0", dict(nm=0), "nm must be 1 (one affine for the batch) or B (one per image)"), ("nm 3", dict(nm=3), "nm must be 1 (one affine for the batch) or B (one per image)"),
                 ("m unaligned", dict(m=m + 8), "m_d must be 16-byte aligned"), ("dst on m", dict(m=dst + 16), "the affines and the destination range overlap"),
                 ("dst on the second m", dict(m=dst - 48, nm=2), "the affines and the destination range overlap")]),
             "aefft_image_remap": (L.aefft_image_remap, remap, "null context, source, table or destination", shared + [
                 ("tab unaligned", dict(m=tab + 4), "map_d must be 16-byte aligned"), ("dst on tab", dict(m=dst + 32), "the table and the destination range overlap"),
                 ("dst on the table's end", dict(m=dst - 8 * Wd * Hd + 16), "the table and the destination range overlap")])}
    for name, (fn, good, null, rules) in cases.items():
        assert fn(ctx.h, *good.values()) == 0, L.aefft_last_error(ctx.h).decode()
        ctx.sync()
        buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        for what, kw, rule in rules:
            assert fn(ctx.h, *dict(good, **kw).values()) == aefft.EINVAL, (name, what)
            msg = L.aefft_last_error(ctx.h).decode()
            assert msg == name + ": " + (rule or null), (name, what, msg)
        assert fn(None, *good.values()) == aefft.EINVAL
        ctx.sync()
        assert (host(buf) == SENTINEL).all(), name                                # nothing was enqueued: every byte as it was
    # B == 1: the strides are ignored
    assert L.aefft_image_remap(ctx.h, *dict(remap, B=1, ss=0, ds=0).values()) == 0 and L.aefft_image_warp_affine(ctx.h, *dict(warp, B=1, ss=0, ds=0).values()) == 0
    ctx.sync()
    # the Python wrappers raise with the library's sentence
    img = torch.zeros(1, 4, 4, 1, dtype=torch.uint8, device=dev)
    with pytest.raises(aefft.AefftError, match="aefft_image_warp_affine: the source and destination ranges overlap"):
        ctx.image_warp(img, [[1, 0, 0], [0, 1, 0]], out=img)
    with pytest.raises(aefft.AefftError, match="aefft_image_remap: the source and destination ranges overlap"):
        ctx.image_remap(img, torch.zeros(4, 4, 2, dtype=torch.int32, device=dev), out=img)


def test_chain_undistort_pose_correct_and_compare(ctx):
    """an image that an ideal lens delivered shifted by (+5, -3) pixels against the reference: the lens table (zero distortion: the identity, exactly)
    and the inverse integer translation put every pixel back, and aefft_image_compare_map against the reference is exactly zero away from the strip
    the shift left uncovered"""
    W, H, D, dx, dy = 96, 64, 3, 5, -3
    ref = source((W, H), 1, D)[0]
    shifted = np.zeros_like(ref)
    shifted[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = ref[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]     # shifted(x, y) = ref(x - dx, y - dy)
    dev = f"cuda:{ctx.device}"
    K = [[700.0, 0, 47.5], [0, 700.0, 31.5], [0, 0, 1]]
    table = aefft.undistort_table(K, (0, 0, 0, 0, 0), (W, H))
    ideal = ctx.image_remap(torch.as_tensor(shifted, device=dev), torch.as_tensor(table, device=dev))
    assert np.array_equal(host(ideal)[0], shifted)
    back = ctx.image_warp(ideal, [[1, 0, dx], [0, 1, dy]])                       # destination (x, y) samples (x + dx, y + dy)
    cells = aefft.cells_for_tile(W, H, 8)
    mp, score = ctx.image_compare_map(back, torch.as_tensor(np.array(ref[None]), device=dev), cells)
    mp = host(mp)[0]                                                             # [Mx][My]: 12 x 8 cells of 8 x 8 pixels
    assert mp.shape == (12, 8) and (mp[:11, 1:] == 0).all()                      # the uncovered strip: the last 5 columns, the first 3 rows
    assert (mp[11, :] > 0).all() and (mp[:, 0] > 0).all()
    assert np.array_equal(host(back)[0, 3:, :W - 5], ref[3:, :W - 5])
