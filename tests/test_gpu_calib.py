"""aefft_map_stats_update / _merge / _finish and aefft_map_peak (Context.map_stats*, Context.map_peak, Net.calibrate_tiled) on the device against
calib_ref.py -- EXACT byte equality of every state, baseline, peak and cell: the shapes around the kernels' 256-lane block at B = 1, 3, 5 and 9 in two
and three updates in a row, the values at which it goes wrong (0..65025, -1..1, a grid of 1/32 where ties are common, NaN, infinities and zeros of both
signs planted, a cell that is never finite, a constant cell), the order independence of the extremes, a split and its merge, every finish (both modes,
ranks 1..4 with counts below the rank, both senses, k 0, 3 and -2.5, empty inf and 0; the SIGMA baseline's bits include the device's double division
and square root), the peak (both senses, with and without a baseline, ties, an image of NaN only, two runs byte for byte), one graph capture and replay
of update -> finish -> peak, the profile entries, the chain into aefft_map_regions, every AEFFT_EINVAL rule and Net.calibrate_tiled."""
import functools
import importlib

import numpy as np
import pytest
import torch

import calib_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

LANES, PEAK_LANES = 256, 1024                                                    # the kernels' blocks (csrc/calib_kernels.hip CB_LANES, CB_PEAK_LANES)
SHAPES = [(1, 1), (1, 7), (15, 17), (16, 16), (1, 257), (3, 1024), (240, 135)]  # 15 x 17 = 255 cells, 16 x 16 = 256, 1 x 257: a block and a cell
KINDS = ["wide", "unit", "grid"]
UPDATES = [(1, 3), (5, 9), (3, 1, 5)]                                            # B of the updates in a row: 1, 3, 5, 9; above 4 so that slots are evicted
SENTINEL = 0x7B
_id = lambda v: "x".join(str(q) for q in v) if isinstance(v, tuple) else str(v)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")


def footage(shape, B, kind, rng, specials=True):
    """B maps: random float32 in 0..65025 ("wide"), in -1..1 ("unit") or on a grid of 1/32 ("grid"); with `specials` NaN, +-inf and +-0 planted
    in about a tenth of the entries, cell 0 never finite and the last cell constant"""
    Mx, My = shape
    if kind == "wide":
        m = (rng.random((B, Mx, My)) * 65025).astype(np.float32)
    elif kind == "unit":
        m = (rng.random((B, Mx, My)) * 2 - 1).astype(np.float32)
    else:
        m = (rng.integers(-4, 12, (B, Mx, My)) / 32.0).astype(np.float32)
    if specials:
        pick = rng.random(m.shape) < 0.1
        vals = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32), m.shape)
        m = np.where(pick, vals, m).astype(np.float32)
        flat = m.reshape(B, -1)
        flat[:, 0] = np.where(rng.random(B) < 0.5, np.float32(np.nan), np.float32(np.inf))
        if Mx * My > 1:
            flat[:, -1] = np.float32(0.1)
    return m


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(the maps of each update, the restated state after each update), once; the updates in a row depend on the case, so that every shape meets each"""
    rng = np.random.default_rng(shape[0] * 1031 + shape[1] * 7 + KINDS.index(kind))
    Bs = UPDATES[(SHAPES.index(shape) + KINDS.index(kind)) % len(UPDATES)]
    maps, states = [], []
    st = R.empty(*shape)
    for B in Bs:
        m = footage(shape, B, kind, rng)
        m.setflags(write=False)
        st = R.update(st, m)
        maps.append(m)
        states.append(st)
    return maps, states


def state_bytes(state):
    return host(state).tobytes()


def run_updates(ctx, shape, maps):
    state = ctx.map_stats(*shape)
    for m in maps:
        ctx.map_stats_update(state, _dev(m, ctx))
    return state


# ------------------------------------------------------------------------------------------
# 1. update, finish and peak on every shape and kind of value
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_update_finish_and_peak_are_the_restatement(ctx, shape, kind):
    maps, states = _case(shape, kind)
    Mx, My = shape
    state = ctx.map_stats(Mx, My)
    assert state.numel() == R.stats_bytes(Mx, My) and not host(state).any() and state.cells == shape
    for m, want in zip(maps, states):
        assert ctx.map_stats_update(state, _dev(m, ctx)) is state
        ctx.sync()
        got = R.from_bytes(host(state), Mx, My)
        for plane in ("c", "hi", "lo", "S1", "S2"):
            assert got[plane].tobytes() == want[plane].tobytes(), (shape, kind, plane)
        assert state_bytes(state) == R.to_bytes(want, Mx, My).tobytes()            # (the padding too)
    want = states[-1]
    assert want["c"][0] == 0                                                     # the cell that is never finite
    # finish: RANK at every rank (cells with fewer values than the rank among them), SIGMA at every k, both senses, both `empty`
    for sense in ("above", "below"):
        for rank, empty in ((1, np.inf), (2, 0.0), (3, np.inf), (4, 0.0)):
            ref = ctx.map_stats_finish(state, shape, "rank", sense, rank=rank, empty=empty)
            assert bits(host(ref)).tobytes() == bits(R.finish(want, Mx, My, "rank", sense, rank=rank, empty=empty)).tobytes(), (shape, kind, sense, rank)
        for k, empty in ((0.0, 0.0), (3.0, np.inf), (-2.5, 0.0)):
            ref = ctx.map_stats_finish(state, shape, "sigma", sense, k=k, rank=1 + int(abs(k)), empty=empty)
            w = R.finish(want, Mx, My, "sigma", sense, k=k, empty=empty)
            differ = np.flatnonzero(bits(host(ref)).reshape(-1) != bits(w).reshape(-1))
            print(shape, kind, sense, k, "SIGMA cells that differ:", differ.size)
            assert differ.size == 0, (shape, kind, sense, k, differ[:8], host(ref).reshape(-1)[differ[:8]], w.reshape(-1)[differ[:8]])
    assert state_bytes(state) == R.to_bytes(want, Mx, My).tobytes()                # the finish only reads the state
    # peak of the last maps: both senses, with and without the baseline
    m = maps[-1]
    dm = _dev(m, ctx)
    for sense in ("above", "below"):
        base = R.finish(want, Mx, My, "rank", sense, rank=2, empty=-np.inf)
        for ref in (None, base):
            pk, cell = ctx.map_peak(dm, None if ref is None else _dev(ref, ctx), sense)
            wp, wc = R.peak(m, ref, sense)
            assert np.array_equal(host(cell), wc) and bits(host(pk)).tobytes() == bits(wp).tobytes(), (shape, kind, sense, ref is not None, host(cell), wc)


def test_counts_below_the_rank_are_met():
    """(what the sweep above relies on: its cases hold cells with 0, 1, 2 and 3 counted values as well as full ones)"""
    seen = set()
    for shape in SHAPES[2:]:
        for kind in KINDS:
            seen |= set(np.unique(_case(shape, kind)[1][-1]["c"]).tolist())
    assert {0, 1, 2, 3, 4, 5} <= seen


# ------------------------------------------------------------------------------------------
# 2. the extremes and the counts do not depend on the order; a split and its merge
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_orders_of_the_same_frames_give_the_same_extremes(ctx, kind):
    shape = (15, 17)
    rng = np.random.default_rng(5 + KINDS.index(kind))
    m = footage(shape, 9, kind, rng)
    perm = rng.permutation(9)
    a = run_updates(ctx, shape, [m])
    b = run_updates(ctx, shape, [m[perm][:4], m[perm][4:]])
    ctx.sync()
    n = shape[0] * shape[1]
    ha, hb = host(a), host(b)
    assert ha[16 * n:52 * n].tobytes() == hb[16 * n:52 * n].tobytes()              # hi, lo and c
    assert ha[16 * n:52 * n].tobytes() == R.to_bytes(R.update(R.empty(*shape), m), *shape)[16 * n:52 * n].tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1), (15, 17), (1, 257), (240, 135)], ids=_id)
def test_a_split_and_its_merge(ctx, shape, kind):
    maps, states = _case(shape, kind)
    Mx, My = shape
    n = Mx * My
    first, second = run_updates(ctx, shape, maps[:1]), run_updates(ctx, shape, maps[1:])
    keep = second.clone()
    assert ctx.map_stats_merge(first, second) is first
    ctx.sync()
    r1, r2 = states[0], R.update(R.empty(Mx, My), np.concatenate(maps[1:]))
    if len(maps) > 2:
        r2 = R.update(R.update(R.empty(Mx, My), maps[1]), maps[2])
    assert state_bytes(first) == R.to_bytes(R.merge(r1, r2), Mx, My).tobytes()     # the restatement of that same split
    assert state_bytes(second) == state_bytes(keep)                                # src is only read
    assert host(first)[16 * n:52 * n].tobytes() == R.to_bytes(states[-1], Mx, My)[16 * n:52 * n].tobytes()      # hi, lo, c of the unsplit run
    # an empty state merges to the other one, either way round
    e = ctx.map_stats(Mx, My)
    ctx.map_stats_merge(e, second)
    ctx.map_stats_merge(second, ctx.map_stats(Mx, My), cells=shape)
    ctx.sync()
    assert state_bytes(e) == state_bytes(keep) == state_bytes(second)


# ------------------------------------------------------------------------------------------
# 3. the peak: ties, an image of NaN only, two runs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(1, 7), (15, 17), (1, 257), (32, 33), (91, 91), (240, 135)], ids=_id)      # 1056 = PEAK_LANES + 32 cells; 8281: a round of 8 x 1024 and 89
def test_peak_ties_go_to_the_smallest_index_and_nan_images_give_nan(ctx, shape, B):
    Mx, My = shape
    n = Mx * My
    rng = np.random.default_rng(n + B)
    m = (rng.integers(-3, 4, (B, Mx, My)) / 32.0).astype(np.float32)              # seven values only: the peak is attained many times
    m[rng.random(m.shape) < 0.2] = np.nan
    m.reshape(B, -1)[:, n // 2] = -0.0
    m[B - 1] = np.nan                                                            # the last image: NaN only
    if B > 1:
        m[0].reshape(-1)[:] = np.where(np.arange(n) % 2 == 1, np.float32(0.0), np.float32(-0.0))      # zeros of both signs: all equal
    ref = (rng.integers(-2, 3, (Mx, My)) / 32.0).astype(np.float32)
    dm, dr = _dev(m, ctx), _dev(ref, ctx)
    for sense in ("above", "below"):
        for r, d in ((None, None), (ref, dr)):
            runs = []
            for junk in (0x11, 0xFF):
                pk = torch.full((B,), float(junk), device=dm.device)
                cell = torch.full((B,), junk, dtype=torch.int32, device=dm.device)
                got = ctx.map_peak(dm, d, sense, peak=pk, cell=cell)
                assert got[0] is pk and got[1] is cell
                ctx.sync()
                runs.append((host(pk).tobytes(), host(cell).tobytes()))
            wp, wc = R.peak(m, r, sense)
            assert runs[0] == runs[1] == (wp.tobytes(), wc.tobytes()), (shape, B, sense, r is not None)
            assert wc[B - 1] == -1 and bits(wp)[B - 1] == 0x7FC00000
            if B > 1 and r is None:
                assert wc[0] == 0 and bits(wp)[0] == 0


# ------------------------------------------------------------------------------------------
# 4. capture and replay; the profile entries
# ------------------------------------------------------------------------------------------
def test_update_finish_and_peak_are_captured_once_and_replayed():
    shape, B = (15, 17), 5
    rng = np.random.default_rng(77)
    m = footage(shape, B, "wide", rng)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        dm = torch.zeros(m.shape, device=dev)
        state = c.map_stats(*shape)
        ref = torch.full(shape, 7.0, device=dev)
        pk = torch.full((B,), 7.0, device=dev)
        cell = torch.full((B,), 7, dtype=torch.int32, device=dev)

        def chain():                                                             # a single chain: no parallel branches
            c.map_stats_update(state, dm)
            c.map_stats_finish(state, shape, "sigma", k=3.0, ref=ref)
            c.map_peak(dm, ref, peak=pk, cell=cell)
        with torch.cuda.stream(side):
            chain()
        torch.cuda.synchronize()
        state.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain()
        torch.cuda.synchronize()
        assert not host(state).any()                                             # nothing ran during the capture
        dm.copy_(_dev(m, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = R.update(R.empty(*shape), m)
        wref = R.finish(want, *shape, "sigma", k=3.0)
        wp, wc = R.peak(m, wref)
        assert state_bytes(state) == R.to_bytes(want, *shape).tobytes() and bits(host(ref)).tobytes() == bits(wref).tobytes()
        assert bits(host(pk)).tobytes() == bits(wp).tobytes() and np.array_equal(host(cell), wc)
        del g
    finally:
        c.close()


def test_the_calls_are_accounted_as_image_entries_with_their_bytes(ctx):
    shape, B = (50, 67), 3
    n = 50 * 67
    rng = np.random.default_rng(3)
    m = _dev(footage(shape, B, "unit", rng), ctx)
    state, other = ctx.map_stats(*shape), ctx.map_stats(*shape)
    ref = ctx.empty(*shape)
    ctx.map_stats_update(other, m)
    want = [4 * B * n + 104 * n, 156 * n, 56 * n, 4 * B * n + 4 * n + 8 * B, 4 * B * n + 8 * B]
    ctx.prof_enable(); ctx.prof_reset()
    try:
        reads = []
        for call in (lambda: ctx.map_stats_update(state, m), lambda: ctx.map_stats_merge(state, other), lambda: ctx.map_stats_finish(state, shape, ref=ref),
                     lambda: ctx.map_peak(m, ref), lambda: ctx.map_peak(m)):
            call()
            reads.append(ctx.prof_read())
    finally:
        ctx.prof_enable(False)
    for k, read in enumerate(reads):
        assert read["image"]["launches"] == k + 1 and read["image"]["bytes"] == sum(want[:k + 1]), (k, read["image"])
        assert sum(v["launches"] for v in read.values()) == k + 1


# ------------------------------------------------------------------------------------------
# 5. end to end: a baseline from nominal maps, detections against it
# ------------------------------------------------------------------------------------------
def test_a_rank_baseline_silences_the_nominal_maps_and_finds_the_planted_block(ctx):
    shape = (40, 30)
    Mx, My = shape
    rng = np.random.default_rng(11)
    scene = (rng.random(shape) * 900 + 50).astype(np.float32)                     # reconstruction error is never uniform over a scene
    nominal = (scene[None] * (0.8 + 0.4 * rng.random((6, Mx, My)))).astype(np.float32)
    dn = _dev(nominal, ctx)
    state = ctx.map_stats(Mx, My)
    ctx.map_stats_update(state, dn[:4])
    ctx.map_stats_update(state, dn[4:])
    ref = ctx.map_stats_finish(state, shape, "rank", "above", rank=1)
    ctx.sync()
    assert np.array_equal(host(ref), nominal.max(0))
    t = 2.0 ** -20
    labels, regions, count = ctx.map_regions(dn, t, t, ref=ref)
    pk, cell = ctx.map_peak(dn, ref)
    ctx.sync()
    assert host(count).tolist() == [0] * 6 and not host(labels).any() and (host(pk) <= 0).all()
    seventh = nominal[2:3].copy()
    seventh[0, 17:20, 11:13] = host(ref)[17:20, 11:13] + np.float32(100.0)
    seventh[0, 18, 12] += np.float32(50.0)
    d7 = _dev(seventh, ctx)
    labels, regions, count = ctx.map_regions(d7, t, t, ref=ref)
    pk, cell = ctx.map_peak(d7, ref)
    ctx.sync()
    r = host(regions).view(aefft.REGION)[..., 0][0, 0]
    assert host(count).tolist() == [1] and (r["i0"], r["j0"], r["i1"], r["j1"], r["area"]) == (17, 11, 19, 12, 6)
    lab = host(labels)[0]
    assert lab[17:20, 11:13].all() and lab.sum() == 6
    assert host(cell).tolist() == [18 * My + 12] == [r["peak_i"] * My + r["peak_j"]] and host(pk)[0] == r["peak"] > 100


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    Mx, My, B = 5, 7, 2
    n = Mx * My
    dev = f"cuda:{ctx.device}"
    buf = torch.full((16384,), SENTINEL, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    assert base % 16 == 0
    mp, rp, sp, s2p, op, pp, cp = base, base + 512, base + 1024, base + 3072, base + 5120, base + 5632, base + 5648      # map, ref, two states, ref out, peak, cell
    need = L.aefft_map_stats_bytes(Mx, My)
    assert need == 1824 and 4 * B * n <= 512 and 4 * n <= 512 and need <= 2048
    SIZE, BATCH, INT = "Mx, My must be in 1..1024", "B must be >= 1", "B * Mx * My does not fit an int"
    BYTES, SENSE = "stats_bytes is below aefft_map_stats_bytes(Mx, My)", "sense must be AEFFT_REGIONS_ABOVE or AEFFT_REGIONS_BELOW"
    sizes = [("Mx = 0", dict(Mx=0), SIZE), ("Mx = 1025", dict(Mx=1025), SIZE), ("My = 0", dict(My=0), SIZE), ("My = 1025", dict(My=1025), SIZE), ("My < 0", dict(My=-3), SIZE)]
    batch = [("B = 0", dict(B=0), BATCH), ("B < 0", dict(B=-1), BATCH), ("cells beyond an int", dict(B=2 ** 31 - 1), INT), ("cells just beyond an int", dict(Mx=1024, My=1024, B=2048), INT)]
    short = [("a state one byte short", dict(stats_bytes=need - 1), BYTES), ("no state bytes", dict(stats_bytes=0), BYTES)]

    def sweep(name, fn, good, cases):
        for what, kw, rule in cases:
            assert fn(ctx.h, *dict(good, **kw).values()) == aefft.EINVAL, (name, what)
            msg = L.aefft_last_error(ctx.h).decode()
            assert msg == name + ": " + rule, (name, what, msg)

    NULL, ALIGN, OVER = "null context, map or state", "map_d and stats_d must be 16-byte aligned", "the map and state ranges overlap"
    up = dict(map=mp, Mx=Mx, My=My, B=B, stats=sp, stats_bytes=need)
    sweep("aefft_map_stats_update", L.aefft_map_stats_update, up, [("null map", dict(map=None), NULL), ("null state", dict(stats=None), NULL)] + sizes + batch + short + [
        ("map off by 4", dict(map=mp + 4), ALIGN), ("state off by 8", dict(stats=sp + 8), ALIGN), ("the state in the map", dict(stats=mp + 16), OVER),
        ("the map in the state", dict(map=sp + 1808), OVER), ("the map ends in the state", dict(map=sp - 272), OVER)])
    NULL, ALIGN, OVER = "null context, dst or src state", "dst_d and src_d must be 16-byte aligned", "the dst and src state ranges overlap"
    mg = dict(dst=sp, src=s2p, Mx=Mx, My=My, stats_bytes=need)
    sweep("aefft_map_stats_merge", L.aefft_map_stats_merge, mg, [("null dst", dict(dst=None), NULL), ("null src", dict(src=None), NULL)] + sizes + short + [
        ("dst off by 4", dict(dst=sp + 4), ALIGN), ("src off by 8", dict(src=s2p + 8), ALIGN), ("src is dst", dict(src=sp), OVER), ("src in dst", dict(src=sp + 1808), OVER),
        ("dst in src", dict(dst=s2p - 1808), OVER)])
    NULL, ALIGN, OVER = "null context, state or ref", "stats_d and ref_d must be 16-byte aligned", "the state and ref ranges overlap"
    fi = dict(stats=sp, stats_bytes=need, Mx=Mx, My=My, mode=1, sense=0, k=3.0, rank=1, empty=0.0, ref=op)
    sweep("aefft_map_stats_finish", L.aefft_map_stats_finish, fi, [("null state", dict(stats=None), NULL), ("null ref", dict(ref=None), NULL)] + sizes + short + [
        ("mode 2", dict(mode=2), "mode must be AEFFT_CALIB_SIGMA or AEFFT_CALIB_RANK"), ("mode -1", dict(mode=-1), "mode must be AEFFT_CALIB_SIGMA or AEFFT_CALIB_RANK"),
        ("sense 2", dict(sense=2), SENSE), ("sense -1 under SIGMA", dict(mode=0, sense=-1), SENSE), ("rank 0", dict(rank=0), "rank must be in 1..4"),
        ("rank 5 under SIGMA", dict(mode=0, rank=5), "rank must be in 1..4"), ("k NaN", dict(mode=0, k=float("nan")), "k must be finite"),
        ("k inf", dict(mode=0, k=float("inf")), "k must be finite"), ("k -inf under RANK", dict(k=float("-inf")), "k must be finite"),
        ("state off by 4", dict(stats=sp + 4), ALIGN), ("ref off by 8", dict(ref=op + 8), ALIGN), ("ref in the state", dict(ref=sp + 16), OVER),
        ("ref over the state's end", dict(ref=sp + 1808), OVER), ("ref ends in the state", dict(ref=sp - 128), OVER)])
    NULL, ALIGN, OVER = "null context, map, peak or cell", "map_d, ref_d, peak_d and cell_d must be 16-byte aligned", "the peak and cell ranges overlap an input or each other"
    pe = dict(map=mp, ref=rp, Mx=Mx, My=My, B=B, sense=0, peak=pp, cell=cp)
    sweep("aefft_map_peak", L.aefft_map_peak, pe, [("null map", dict(map=None), NULL), ("null peak", dict(peak=None), NULL), ("null cell", dict(cell=None), NULL)] + sizes + batch + [
        ("sense 2", dict(sense=2), SENSE), ("sense -1", dict(sense=-1), SENSE), ("map off by 4", dict(map=mp + 4), ALIGN), ("ref off by 8", dict(ref=rp + 8), ALIGN),
        ("peak off by 4", dict(peak=pp + 4), ALIGN), ("cell off by 8", dict(cell=cp + 8), ALIGN), ("cell is peak", dict(cell=pp), OVER), ("peak in the map", dict(peak=mp + 16), OVER),
        ("cell in the map", dict(cell=mp + 272), OVER), ("peak in the baseline", dict(peak=rp + 128), OVER), ("cell in the baseline", dict(cell=rp), OVER)])
    ctx.sync()
    assert (host(buf) == SENTINEL).all()
    # what is NOT an error: neighbouring ranges, a larger state, no baseline; and the calls are right afterwards
    rng = np.random.default_rng(9)
    m = footage((Mx, My), B, "grid", rng)
    buf[:4 * B * n] = _dev(m, ctx).reshape(-1).view(torch.uint8)
    buf[1024:1024 + need] = 0
    buf[3072:3072 + need] = 0
    assert L.aefft_map_stats_update(ctx.h, mp, Mx, My, B, sp, need + 64) == aefft.OK
    assert L.aefft_map_stats_update(ctx.h, mp, Mx, My, B, s2p, need) == aefft.OK
    assert L.aefft_map_stats_merge(ctx.h, sp, s2p, Mx, My, need) == aefft.OK
    assert L.aefft_map_stats_finish(ctx.h, sp, need, Mx, My, 1, 0, 3.0, 2, 0.0, rp) == aefft.OK      # (ref_d right behind the map)
    assert L.aefft_map_peak(ctx.h, mp, rp, Mx, My, B, 0, pp, pp + 16) == aefft.OK                   # (cell_d right behind peak_d)
    assert L.aefft_map_peak(ctx.h, mp, None, Mx, My, B, 1, op, op + 16) == aefft.OK
    ctx.sync()
    one = R.update(R.empty(Mx, My), m)
    want = R.merge(one, one)
    got = host(buf)
    assert got[1024:1024 + need].tobytes() == R.to_bytes(want, Mx, My).tobytes() and got[3072:3072 + need].tobytes() == R.to_bytes(one, Mx, My).tobytes()
    wref = R.finish(want, Mx, My, "rank", "above", rank=2, empty=0.0)
    assert got[512:512 + 4 * n].tobytes() == wref.tobytes()
    wp, wc = R.peak(m, wref, "above")
    assert got[5632:5640].tobytes() == wp.tobytes() and got[5648:5656].tobytes() == wc.tobytes()
    wp, wc = R.peak(m, None, "below")
    assert got[5120:5128].tobytes() == wp.tobytes() and got[5136:5144].tobytes() == wc.tobytes()
    assert (got[1024 + need:3072] == SENTINEL).all() and (got[5656:] == SENTINEL).all()
    # the binding refuses what the C call would, before it reaches the library; a library error surfaces with its message
    dm = buf[:4 * B * n].view(torch.float32).view(B, Mx, My)
    state = ctx.map_stats(Mx, My)
    for bad in (lambda: ctx.map_stats_update(state[:-16], dm), lambda: ctx.map_stats_update(state, dm.double()), lambda: ctx.map_stats_finish(state, (Mx, My), mode="mean"),
                lambda: ctx.map_stats_finish(state, (Mx, My), rank=5), lambda: ctx.map_stats_finish(state, (Mx, My), "sigma", k=float("nan")),
                lambda: ctx.map_stats_merge(state, state), lambda: ctx.map_peak(dm, sense="up"), lambda: ctx.map_peak(dm, peak=torch.empty(3, device=dev)),
                lambda: ctx.map_stats(0, 3), lambda: ctx.map_stats(3, 1025)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(aefft.AefftError, match="aefft_map_stats_update: the map and state ranges overlap"):
        ctx.map_stats_update(buf[:2048], dm)


# ------------------------------------------------------------------------------------------
# 7. Net.calibrate_tiled
# ------------------------------------------------------------------------------------------
def test_calibrate_tiled_is_score_tiled_then_map_stats_update(ctx):
    """a 3 -> 4 -> 3 net with 5 x 5 kernels on one 96 x 80 x 3 image: calibrate_tiled's map is score_tiled's, its state map_stats_update's of that map
    -- and the restatement's --; a second call goes on with the state"""
    D, N, Bn, dM, Nk, W, H, V, M = 3, 64, 2, 4, 5, 96, 80, 16, 4
    rng = np.random.default_rng(23)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    c, f = q32(0.1 * rng.uniform(-1, 1, (dM, D, Nk, Nk))), q32(0.1 * rng.uniform(-1, 1, (D, dM, Nk, Nk)))
    bias, p = q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, D))
    image = rng.integers(0, 256, (1, H, W, D), dtype=np.uint8)
    cells = aefft.cells_for_tile(W, H, 16)
    net = aefft.Net(ctx, D, N, N, [dM], Nk, 2, batch=Bn)
    try:
        net.set_pair(0, c, bias, f, p)
        img = _dev(image, ctx)
        for metric in ("mse", "ssim"):
            m, _, _ = net.score_tiled(img, V, M, tile=16, metric=metric, score=False)
            sep = ctx.map_stats_update(ctx.map_stats(*cells), m)
            state, m2 = net.calibrate_tiled(img, V, M, tile=16, metric=metric)
            ctx.sync()
            mh = host(m)
            assert tuple(m2.shape) == (1,) + cells and bits(host(m2)).tobytes() == bits(mh).tobytes()
            want = R.update(R.empty(*cells), mh)
            assert state_bytes(state) == state_bytes(sep) == R.to_bytes(want, *cells).tobytes() and (want["c"] == 1).all()
            again, _ = net.calibrate_tiled(img, V, M, tile=16, metric=metric, state=state)
            ctx.sync()
            assert again is state and state_bytes(state) == R.to_bytes(R.update(want, mh), *cells).tobytes()
            S1, S2, hi, lo, cnt = aefft.map_stats_view(state, *cells)
            assert (host(cnt) == 2).all() and np.array_equal(host(hi)[0], mh[0]) and np.array_equal(host(hi)[1], mh[0]) and np.array_equal(host(S1), 2 * mh[0].astype(np.float64))
            ref = ctx.map_stats_finish(state, cells, "rank", "below" if metric == "ssim" else "above")
            labels, regions, count, _, _ = net.detect_tiled(img, V, M, tile=16, metric=metric, lo=-2.0 ** -20 if metric == "ssim" else 2.0 ** -20, ref=ref)
            ctx.sync()
            assert host(count).tolist() == [0]                                   # the calibrated image is nominal
    finally:
        net.close()
