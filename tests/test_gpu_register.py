"""aefft_frames_register_ref and aefft_frames_register (Context.frames_register_ref, Context.frames_register, Context.image_align) on the device
against register_ref.py, the definition in double: grids 16 x 16, 32 x 8 (a swapped axis shows), 64 x 64 and the smooth 48 x 40 (the mixed-radix
route), B = 1 and 3, D = 1 and 3, 8-bit and float frames, one reference and one per image.  The exact case (NOWINDOW, cutoff 1, circular rolls of
random bytes), the general case (HANN, cutoffs 1.0 and 0.5, textures cropped from a 2 x canvas) within 2^-11 of the restatement, the affine bytes
from the device's own shift, the chain through Context.image_align into aefft_image_compare_map, one graph capture and replay, run-to-run
identity, every AEFFT_EINVAL rule and the profile entries."""
import ctypes as C
import functools
import importlib
import itertools

import numpy as np
import pytest
import torch

import register_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (32, 8), (64, 64), (48, 40)]
COMBOS = list(itertools.product((1, 3), (1, 3), (True, False)))                  # B, D, 8-bit
ROLLS = [(3, -2), (-5, 3), (-7, -3)]                                             # one per image; |dy| < 4 for Ny = 8
TOL = 2.0 ** -11                                                                 # the position quantum of the warp that consumes the result
SENTINEL = 0x7B
SEEDS = {(48, 40): 1003}                                                            # moved where a seed gave two surface values closer than GAP
GAP = 1e-3                                                                       # the least distance between the two largest surface values of a case


def host(t):
    return t.detach().cpu().numpy()


def shifts_of(t):
    return host(t).view(aefft.SHIFT).ravel()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def as_frames(a, u8):
    """the test's frames from bytes: as they are, or floats that are no whole numbers (exact in float32)"""
    return a if u8 else a.astype(np.float32) * 0.5 + 3.25


@functools.lru_cache(maxsize=None)
def exact_case(shape, B, D, u8, nref):
    """(ref frames [nref][D][Nx][Ny], frames [B][D][Nx][Ny], the restatement's results)"""
    Nx, Ny = shape
    rng = np.random.default_rng(Nx * 1000 + Ny * 10 + B + D + nref)
    ref = as_frames(rng.integers(0, 256, (nref, D, Nx, Ny), dtype=np.uint8), u8)
    img = np.stack([np.roll(ref[b % nref], ROLLS[b], (1, 2)) for b in range(B)])
    want, _ = R.register(img, ref, "nowindow", 1.0)
    return ref, img, want


def general_shift(shape, b):
    Nx, Ny = shape
    return ((-1) ** b * (Nx / 8.0 + 0.37 * b + 0.25), -(Ny / 8.0) + 0.6 * b - 0.4)


@functools.lru_cache(maxsize=None)
def general_case(shape, cutoff, B, D, u8, nref):
    """textures cropped from a 2 x canvas, each image its reference moved by general_shift: (ref, frames, the restatement's results, the surfaces)"""
    Nx, Ny = shape
    seed = Nx * 7 + Ny + 31 * D + SEEDS.get(shape, 0)
    canv = [R.canvas(Nx, Ny, seed + k, D) for k in range(nref)]
    ref = as_frames(np.stack([R.crop(c, Nx, Ny) for c in canv]), u8)
    img = as_frames(np.stack([R.crop(canv[b % nref], Nx, Ny, *general_shift(shape, b)) for b in range(B)]), u8)
    want, s = R.register(img, ref, "hann", cutoff)
    return ref, img, want, s


def run(ctx, ref, img, window, cutoff, **kw):
    dev = f"cuda:{ctx.device}"
    r = ctx.frames_register_ref(torch.as_tensor(np.ascontiguousarray(ref), device=dev), window)
    return ctx.frames_register(torch.as_tensor(np.ascontiguousarray(img), device=dev), r, cutoff=cutoff, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_case_circular_rolls_of_random_bytes(ctx, shape):
    """NOWINDOW, cutoff 1: cell equal to the restatement's, |dx - roll| and |dy - roll| <= 1e-4, |response - 1| <= 1e-3"""
    worst = [0.0, 0.0]
    for (B, D, u8), nref in itertools.product(COMBOS, (1, 3)):
        if nref > B:
            continue
        ref, img, want = exact_case(shape, B, D, u8, nref)
        got = shifts_of(run(ctx, ref, img, "nowindow", 1.0))
        for b in range(B):
            dx, dy, resp, cell = want[b]
            assert (dx, dy) == ROLLS[b] and abs(resp - 1) <= 1e-9                 # (the restatement itself)
            assert got["cell"][b] == cell, (shape, B, D, u8, nref, b)
            worst[0] = max(worst[0], abs(got["dx"][b] - dx), abs(got["dy"][b] - dy))
            worst[1] = max(worst[1], abs(got["response"][b] - 1.0))
    print("exact %s: largest |shift - truth| %.3g, |response - 1| %.3g" % (shape, *worst))
    assert worst[0] <= 1e-4 and worst[1] <= 1e-3


@pytest.mark.parametrize("cutoff", [1.0, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_general_case_textures_within_the_warps_quantum(ctx, shape, cutoff):
    """HANN: cell equal to the restatement's; dx, dy and response within 2^-11 of it.  Asserted first, on the restatement alone: the two largest
    surface values of every case lie at least 1e-3 apart (or the peak cell would hang on float rounding)."""
    cases = [(B, D, u8, nref) for (B, D, u8), nref in itertools.product(COMBOS, (1, 3)) if nref <= B]
    for c in cases:
        for s in general_case(shape, cutoff, *c)[3]:
            assert R.peak_gap(s) >= GAP, (shape, cutoff, c, R.peak_gap(s))
    worst = 0.0
    for c in cases:
        ref, img, want, _ = general_case(shape, cutoff, *c)
        got = shifts_of(run(ctx, ref, img, "hann", cutoff))
        for b in range(c[0]):
            assert got["cell"][b] == want[b][3], (shape, cutoff, c, b)
            worst = max(worst, *(abs(float(got[k][b]) - want[b][i]) for i, k in enumerate(("dx", "dy", "response"))))
    print("general %s cutoff %.1f: largest |device - restatement| %.3g" % (shape, cutoff, worst))
    assert worst <= TOL


@pytest.mark.parametrize("shape", [(16, 16), (32, 8)])
def test_affine_bytes_follow_the_devices_own_shift(ctx, shape):
    ref, img, want = exact_case(shape, 3, 1, True, 1)
    plain = host(run(ctx, ref, img, "nowindow", 1.0))
    for scale in ((1.0, 1.0), (2.0, 1.5)):
        sh, aff = run(ctx, ref, img, "nowindow", 1.0, scale=scale, affine=True)
        assert np.array_equal(host(sh), plain)                                   # affine_d = NULL changes nothing else
        got = shifts_of(sh)
        for b in range(3):
            assert host(aff)[b].tolist() == R.affine(got["dx"][b], got["dy"][b], got["response"][b], 0.0, scale), (shape, scale, b)
            assert host(aff)[b, [0, 1, 3, 4]].tolist() == [R.Q, 0, 0, R.Q]
        assert [host(aff)[b, 2] for b in range(3)] != [0, 0, 0]
    # a general case: fractional shifts through rint
    ref, img, want, _ = general_case(shape, 1.0, 3, 1, True, 1)
    sh, aff = run(ctx, ref, img, "hann", 1.0, scale=(2.0, 1.5), affine=True)
    got = shifts_of(sh)
    for b in range(3):
        assert host(aff)[b].tolist() == R.affine(got["dx"][b], got["dy"][b], got["response"][b], 0.0, (2.0, 1.5))
    # an unrelated random image: the response stays below min_response, the affine is the identity and the shift is still written
    noise = np.random.default_rng(99).integers(0, 256, img.shape, dtype=np.uint8)
    free = shifts_of(run(ctx, ref, noise, "hann", 1.0))
    assert (free["response"] < 0.9).all()
    sh, aff = run(ctx, ref, noise, "hann", 1.0, min_response=0.9, affine=True)
    assert np.array_equal(shifts_of(sh), free) and host(aff).tolist() == [[R.Q, 0, 0, 0, R.Q, 0]] * 3


def test_chain_align_and_compare(ctx):
    """a 64 x 64 x 3 image and its copy moved by (+5, -3) with replicated border: Context.image_align at frame size 64 x 64, nearest, puts it back, and
    aefft_image_compare_map against the reference is exactly zero away from the strip the shift left uncovered"""
    W = H = 64
    dx, dy = 5, -3
    tex = R.crop(R.canvas(W, H, 2024, 3), W, H)                                  # [D][Nx][Ny]
    ref = np.ascontiguousarray(tex.transpose(2, 1, 0))                           # image[y][x][d] = frames[d][x][y]
    ys, xs = np.clip(np.arange(H) - dy, 0, H - 1), np.clip(np.arange(W) - dx, 0, W - 1)
    moved = np.ascontiguousarray(ref[ys][:, xs])                                 # moved(x, y) = ref(x - dx, y - dy)
    frames = lambda im: np.ascontiguousarray(im.transpose(2, 1, 0))[None]
    (est,), _ = R.register(frames(moved), frames(ref), "hann", 0.5)
    assert abs(est[0] - dx) < 0.4 and abs(est[1] - dy) < 0.4, est                 # the condition, on the restatement
    dev = f"cuda:{ctx.device}"
    r = ctx.frames_register_ref(ctx.image_resize_to_frames(torch.as_tensor(ref, device=dev), (64, 64)), "hann")
    back, sh, aff = ctx.image_align(torch.as_tensor(moved, device=dev), r, (64, 64), interp="nearest")
    got = shifts_of(sh)
    assert abs(got["dx"][0] - est[0]) <= TOL and abs(got["dy"][0] - est[1]) <= TOL
    mp, _ = ctx.image_compare_map(back, torch.as_tensor(ref[None], device=dev), aefft.cells_for_tile(W, H, 8))
    mp = host(mp)[0]                                                             # [Mx][My]: 8 x 8 cells of 8 x 8 pixels
    assert mp.shape == (8, 8) and (mp[:7, 1:] == 0).all()                        # the uncovered strip: the last 5 columns, the first 3 rows
    assert (mp[7, :] > 0).any() and (mp[:, 0] > 0).any()


def _raw_call(c, L, frames, spec, shifts, aff, work, B, D, Nx, Ny, window=0, nref=1, cutoff=0.5):
    return L.aefft_frames_register(c.h, frames.data_ptr(), 1, B, D, Nx, Ny, window, spec.data_ptr(), nref, cutoff, 0.0, 1.0, 1.0, shifts.data_ptr(),
                                   aff.data_ptr(), work.data_ptr(), work.numel())


def test_graph_capture_and_replay_of_register_then_warp():
    shape, B, D = (64, 64), 3, 3
    ref, img, want, _ = general_case(shape, 0.5, B, D, True, 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        L, dev = aefft.lib(), f"cuda:{c.device}"
        with torch.cuda.stream(side):
            r = c.frames_register_ref(torch.as_tensor(ref, device=dev), "hann")
        frames = torch.zeros(img.shape, dtype=torch.uint8, device=dev)
        image = torch.as_tensor(np.ascontiguousarray(img.transpose(0, 3, 2, 1)), device=dev)      # [B][Ny][Nx][D]
        shifts = torch.full((B, 16), SENTINEL, dtype=torch.uint8, device=dev)
        aff = torch.zeros(B, 6, dtype=torch.int64, device=dev)
        out = torch.full(image.shape, SENTINEL, dtype=torch.uint8, device=dev)
        work = torch.zeros(L.aefft_register_workspace(64, 64, B), dtype=torch.uint8, device=dev)

        def chain():                                                             # a single chain: no parallel branches
            assert _raw_call(c, L, frames, r.spec, shifts, aff, work, B, D, 64, 64) == 0, L.aefft_last_error(c.h).decode()
            c.image_warp(image, aff, interp="linear", border="replicate", out=out)
        with torch.cuda.stream(side):
            frames.copy_(torch.as_tensor(img, device=dev))
            chain()                                                              # the warm call: the transform workspace is taken here
        torch.cuda.synchronize()
        eager = [host(shifts).copy(), host(aff).copy(), host(out).copy()]
        assert shifts_of(shifts)["cell"].tolist() == [w[3] for w in want]
        shifts.fill_(SENTINEL); aff.zero_(); out.fill_(SENTINEL); frames.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain()
        torch.cuda.synchronize()
        assert (host(out) == SENTINEL).all() and (host(shifts) == SENTINEL).all()  # nothing ran during the capture
        frames.copy_(torch.as_tensor(img, device=dev))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, (shifts, aff, out)):
            assert np.array_equal(a, host(b))
        del g
    finally:
        c.close()


def test_two_runs_give_identical_bytes(ctx):
    for shape, window, cutoff in (((64, 64), "hann", 0.5), ((48, 40), "hann", 1.0)):
        ref, img, _, _ = general_case(shape, cutoff, 3, 3, False, 3)
        a = [host(t).copy() for t in run(ctx, ref, img, window, cutoff, scale=(2.0, 1.5), affine=True)]
        b = [host(t) for t in run(ctx, ref, img, window, cutoff, scale=(2.0, 1.5), affine=True)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_every_einval_rule_leaves_the_outputs_untouched(ctx):
    L = aefft.lib()
    dev = f"cuda:{ctx.device}"
    B, D, Nx, Ny = 2, 3, 16, 32
    need = L.aefft_register_workspace(Nx, Ny, B)
    fb, sb = B * D * Nx * Ny, B * Nx * (Ny // 2 + 1) * 8
    buf = torch.full((4 * 16384 + need,), SENTINEL, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    assert base % 16 == 0 and fb <= 16384 and sb <= 16384
    frames, spec, shift, aff, work = base, base + 16384, base + 32768, base + 32768 + 1024, base + 65536
    good = dict(frames=frames, u8=1, B=B, D=D, Nx=Nx, Ny=Ny, window=0, spec=spec, nref=1, cutoff=C.c_float(0.5), minr=C.c_float(0.0), sx=C.c_double(1.0), sy=C.c_double(2.0),
                shift=shift, aff=aff, work=work, wb=need)
    sizes = "Nx, Ny must be powers of two in 8..2048, or even sizes in 10..2048 with no prime factor above 5"
    align = "frames_d, the spectra, the outputs and work_d must be 16-byte aligned"
    scale = "scale_x and scale_y must be in (0, 32]"
    over = "the shifts, the affines and the workspace overlap an input or each other"
    nan = float("nan")
    rules = [("frames null", dict(frames=None), None), ("spec null", dict(spec=None), None), ("shift null", dict(shift=None), None), ("work null", dict(work=None), None),
             ("D 0", dict(D=0), "D must be 1..4"), ("D 5", dict(D=5), "D must be 1..4"), ("B 0", dict(B=0), "B must be >= 1 and B * Nx * Ny below 2^29"),
             ("Nx 14", dict(Nx=14), sizes), ("Ny 6", dict(Ny=6), sizes), ("Nx 4096", dict(Nx=4096), sizes), ("Ny 31", dict(Ny=31), sizes),
             ("window 2", dict(window=2), "window must be AEFFT_REGISTER_HANN or AEFFT_REGISTER_NOWINDOW"), ("window -1", dict(window=-1), "window must be AEFFT_REGISTER_HANN or AEFFT_REGISTER_NOWINDOW"),
             ("nref 0", dict(nref=0), "nref must be 1 (one reference for the batch) or B (one per image)"), ("nref 3", dict(nref=3), "nref must be 1 (one reference for the batch) or B (one per image)"),
             ("cutoff 0", dict(cutoff=C.c_float(0.0)), "cutoff must be in (0, 1]"), ("cutoff 1.01", dict(cutoff=C.c_float(1.01)), "cutoff must be in (0, 1]"),
             ("cutoff nan", dict(cutoff=C.c_float(nan)), "cutoff must be in (0, 1]"), ("cutoff -1", dict(cutoff=C.c_float(-1.0)), "cutoff must be in (0, 1]"),
             ("K 0", dict(cutoff=C.c_float(0.05)), "the cutoff keeps no bin (K = 0)"),
             ("sx 0", dict(sx=C.c_double(0.0)), scale), ("sy 32.5", dict(sy=C.c_double(32.5)), scale), ("sx nan", dict(sx=C.c_double(nan)), scale), ("sy inf", dict(sy=C.c_double(float("inf"))), scale),
             ("frames unaligned", dict(frames=frames + 4), align), ("spec unaligned", dict(spec=spec + 8), align), ("shift unaligned", dict(shift=shift + 8), align),
             ("aff unaligned", dict(aff=aff + 8), align), ("work unaligned", dict(work=work + 8), align),
             ("work short", dict(wb=need - 1), "work_bytes is below aefft_register_workspace(Nx, Ny, B) (nref for B in aefft_frames_register_ref)"),
             ("shift on frames", dict(shift=frames + fb - 16), over), ("shift on spec", dict(shift=spec), over), ("aff on shift", dict(aff=shift + 16), over),
             ("work on frames", dict(work=frames), over), ("aff in work", dict(aff=work + need - 16), over), ("shift in work", dict(shift=work + 32), over)]
    fn = L.aefft_frames_register
    # a good call first (its spectra are the sentinel's bytes: any finite numbers do), then the buffer back to the sentinel
    assert fn(ctx.h, *good.values()) == 0, L.aefft_last_error(ctx.h).decode()
    assert fn(ctx.h, *dict(good, aff=None).values()) == 0
    ctx.sync()
    buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    for what, kw, rule in rules:
        assert fn(ctx.h, *dict(good, **kw).values()) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_frames_register: " + (rule or "null context, frames, reference spectra, shifts or workspace"), (what, msg)
    assert fn(None, *good.values()) == aefft.EINVAL
    ref_good = dict(frames=frames, u8=1, nref=B, D=D, Nx=Nx, Ny=Ny, window=1, spec=spec, work=work, wb=need)
    ref_rules = [("frames null", dict(frames=None), "null context, frames, spectra or workspace"), ("spec null", dict(spec=None), "null context, frames, spectra or workspace"),
                 ("D 5", dict(D=5), "D must be 1..4"), ("nref 0", dict(nref=0), "nref must be >= 1 and nref * Nx * Ny below 2^29"), ("Nx 14", dict(Nx=14), sizes),
                 ("window 2", dict(window=2), "window must be AEFFT_REGISTER_HANN or AEFFT_REGISTER_NOWINDOW"), ("spec unaligned", dict(spec=spec + 8), align),
                 ("work short", dict(wb=need - 1), "work_bytes is below aefft_register_workspace(Nx, Ny, B) (nref for B in aefft_frames_register_ref)"),
                 ("spec on frames", dict(spec=frames + fb - 16), "the spectra and the workspace overlap the frames or each other"),
                 ("work on spec", dict(work=spec), "the spectra and the workspace overlap the frames or each other")]
    for what, kw, rule in ref_rules:
        assert L.aefft_frames_register_ref(ctx.h, *dict(ref_good, **kw).values()) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_frames_register_ref: " + rule, (what, msg)
    ctx.sync()
    assert (host(buf) == SENTINEL).all()                                         # nothing was enqueued: every byte as it was
    # the Python wrapper raises with the library's sentence
    f = torch.zeros(1, 1, 12, 14, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="Nx, Ny must be powers of two"):
        ctx.frames_register_ref(f)


def test_the_calls_are_accounted_as_image_entries_beside_the_transforms(ctx):
    shape, B, D = (64, 64), 3, 3
    Nx, Ny = shape
    ref, img, _, _ = general_case(shape, 0.5, B, D, True, 1)
    dev = f"cuda:{ctx.device}"
    dref, dimg = torch.as_tensor(ref, device=dev), torch.as_tensor(img, device=dev)
    r = ctx.frames_register_ref(dref, "hann")                                    # (the warm call)
    n, sb = Nx * Ny, Nx * (Ny // 2 + 1) * 8
    ctx.prof_enable(); ctx.prof_reset()
    try:
        r = ctx.frames_register_ref(dref, "hann")
        ctx.sync()
        first = ctx.prof_read()
        ctx.frames_register(dimg, r, affine=True)
        ctx.sync()
        second = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert first["image"]["launches"] == 1 and first["image"]["bytes"] == D * n + 4 * n
    assert first["r2c_rows"]["launches"] == 1 and first["r2c_cols"]["launches"] == 1 and sum(v["launches"] for v in first.values()) == 3
    want = B * D * n + 4 * B * n + sb * (2 * B + 1) + 4 * B * n + B * 64
    assert second["image"]["launches"] == 4 and second["image"]["bytes"] == first["image"]["bytes"] + want
    for k, count in (("r2c_rows", 2), ("r2c_cols", 2), ("c2r_cols", 1), ("c2r_rows", 1)):
        assert second[k]["launches"] == count, k
    assert sum(v["launches"] for v in second.values()) == 10
