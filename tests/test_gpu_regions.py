"""aefft_map_regions (Context.map_regions), region_pixels and Net.detect_tiled on the device against the flood fill of regions_ref.py -- EXACT
equality of every label, every count and every byte of the regions, the untouched tail included: the shapes around the kernel's 16 x 16 tile at
B = 1 and 3, the patterns at which labelling goes wrong (spiral, U, comb, ring, diagonals, checkerboard, bars across every tile, random maps near
the percolation threshold), the keep rule (hysteresis, min_area, hi == lo), the values (BELOW, a baseline, NaN, infinities, zeros of both signs,
equal peaks), two runs byte for byte, one graph capture and replay, the Python paths, every AEFFT_EINVAL rule and the profile entry."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import regions_ref as R

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

T = 16                                                                           # the kernel's tile side (csrc/regions_kernels.hip RG_T)
SHAPES = [(1, 1), (1, 7), (7, 1), (T, T), (T + 1, T + 1), (2 * T + 1, T - 1), (3, 1024), (1024, 3), (256, 256)]
PATTERNS = ["empty", "full", "spiral", "u", "comb", "ring", "diag", "antidiag", "checker", "bars", "random30", "random50", "random60"]
BIG = ["full", "spiral", "bars", "random60"]                                     # at 256 x 256: what needs the size (the flood fill is plain Python)
BOTH = ("diag", "antidiag", "checker")                                           # the patterns whose answer depends on the connectivity
TAIL = 24                                                                        # ints of the labels' allocation behind its live entries: the guard
SENTINEL = 0x7B7B7B7B
Q = np.float32(1.0 / 32.0)
_id = lambda v: "x".join(str(q) for q in v) if isinstance(v, tuple) else str(v)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = aefft.Context(0)
    yield c
    c.close()


def _dev(a, ctx):
    return torch.as_tensor(np.array(a, order="C"), device=f"cuda:{ctx.device}")


def masks(kind, Mx, My, B, rng):
    """[B][Mx][My]: the pattern, the pattern turned round, the pattern again (random: three draws) -- a full image beside an empty or a full one would
    show a connection across images"""
    m = [R.pattern(kind, Mx, My, rng) for _ in range(B)]
    if B > 1 and not kind.startswith("random"):
        m[1] = m[1][::-1, ::-1]
    return np.stack(m)


def values(mask, rng, sense="above", levels=16):
    """a map on a grid of 1/32 around lo = 0.5 (equal values are common, so peaks tie): foreground 0.5 +- k / 32 with k < levels (strong from k = 8
    on at hi = 0.75 / 0.25), background one to eight steps on the other side"""
    k = rng.integers(0, levels, mask.shape).astype(np.float32)
    away = (rng.integers(1, 9, mask.shape)).astype(np.float32)
    sign = np.float32(1.0 if sense == "above" else -1.0)
    return np.where(mask, np.float32(0.5) + sign * k * Q, np.float32(0.5) - sign * away * Q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, B, kind, sense="above"):
    """(map, {connectivity: (labels, regions, count)} of the restatement at lo 0.5, hi 0.75 / 0.25, min_area 1, 64 regions over the sentinel), once"""
    Mx, My = shape
    rng = np.random.default_rng(Mx * 1031 + My * 7 + B + len(kind) * 13 + PATTERNS.index(kind))
    m = values(masks(kind, Mx, My, B, rng), rng, sense)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(shape, B, kind, conn, sense="above", min_area=1, max_regions=64, plain=False):
    lo, hi = 0.5, (0.5 if plain else 0.75 if sense == "above" else 0.25)
    w = R.regions(_case(shape, B, kind, sense), lo, hi, sense=sense, connectivity=conn, min_area=min_area, max_regions=max_regions, fill=_fill(B, max_regions))
    for a in w:
        a.setflags(write=False)
    return w


def _fill(B, max_regions):
    return np.full((B, max_regions, 8), SENTINEL, np.int32).view(R.REGION)[..., 0]


def _run(ctx, m, lo, hi, want, what, ref=None, sense="above", conn=8, min_area=1, max_regions=64):
    """one call into sentinel-filled outputs; labels, regions (every byte) and counts against `want`; returns the three tensors"""
    B, Mx, My = m.shape
    n = B * Mx * My
    buf = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    regions = torch.full((B, max_regions, 8), SENTINEL, dtype=torch.int32, device=buf.device) if max_regions else None
    count = torch.full((B,), SENTINEL, dtype=torch.int32, device=buf.device)
    labels, regs, cnt = ctx.map_regions(_dev(m, ctx), lo, hi, ref=None if ref is None else _dev(ref, ctx), sense=sense, connectivity=conn, min_area=min_area,
                                        max_regions=max_regions, labels=buf[:n].view(B, Mx, My), regions=regions, count=count)
    ctx.sync()
    got = host(buf)
    bad = int((got[:n] != want[0].reshape(-1)).sum())
    print(what, "labels that differ:", bad, "count:", host(cnt).tolist(), "want:", want[2].tolist())
    assert labels.data_ptr() == buf.data_ptr() and bad == 0, what
    assert (got[n:] == SENTINEL).all(), "the ints behind the labels changed"
    assert np.array_equal(host(cnt), want[2]), what
    if max_regions:
        assert regs is regions and host(regs).tobytes() == np.ascontiguousarray(want[1]).tobytes(), what
    else:
        assert regs is None
    return labels, regs, cnt


# ------------------------------------------------------------------------------------------
# 1. exact equality with the restatement: shapes x batch x patterns x connectivity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_labels_regions_and_counts_equal_the_restatement(ctx, shape, B):
    for k, kind in enumerate(BIG if shape == (256, 256) else PATTERNS):
        for conn in ((4, 8) if kind in BOTH or shape[0] * shape[1] <= 4 * T * T else ((4, 8)[(k + B) % 2],)):
            _run(ctx, _case(shape, B, kind), 0.5, 0.75, _want(shape, B, kind, conn), (shape, B, kind, conn), conn=conn)


def test_the_patterns_are_what_they_are_meant_to_be():
    """the restatement on the patterns: one spiral, one U, one comb, a ring and the dot in its hole, a checkerboard of ceil(cells / 2) components under 4
    and one under 8, a diagonal of single cells under 4 and one line under 8 -- so the device test above checks what its name says"""
    one = lambda kind, Mx, My, conn: len(R.components(R.pattern(kind, Mx, My), conn))
    assert one("spiral", 33, 15, 4) == 1 and R.spiral(33, 15).sum() > 33 * 15 // 3 and one("u", 33, 15, 4) == 1 and one("comb", 33, 15, 4) == 1
    assert one("ring", 17, 17, 8) == 2 and one("bars", 50, 67, 4) == 1
    assert one("checker", 17, 17, 4) == (17 * 17 + 1) // 2 and one("checker", 17, 17, 8) == 1
    assert one("diag", 17, 17, 4) == 17 and one("diag", 17, 17, 8) == 1 and one("antidiag", 17, 17, 4) == 17 and one("antidiag", 17, 17, 8) == 1
    # the spiral's last cell lies a long way from its first: a chain across every tile
    assert R.spiral(256, 256)[::T, :].any(axis=1).all() and R.spiral(256, 256)[:, ::T].any(axis=0).all()


@pytest.mark.parametrize("conn", [4, 8])
def test_a_checkerboard_has_more_components_than_regions(ctx, conn):
    """ceil(cells / 2) components under 4 (about half of them strong), one under 8; max_regions = 5 < n: count is n and the tail keeps the sentinel"""
    shape = (T + 1, T + 1)
    want = _want(shape, 3, "checker", conn, max_regions=5)
    _run(ctx, _case(shape, 3, "checker"), 0.5, 0.75, want, ("checker", conn), conn=conn, max_regions=5)
    plain = _want(shape, 3, "checker", conn, max_regions=5, plain=True)
    _run(ctx, _case(shape, 3, "checker"), 0.5, None, plain, ("checker, plain threshold", conn), conn=conn, max_regions=5)
    if conn == 4:
        assert (plain[2] == (17 * 17 + 1) // 2).all() and (want[2] > 5).all() and (want[2] < plain[2]).all()
    else:
        assert (plain[2] == 1).all() and (want[1][:, 1:].view(np.int32) == SENTINEL).all()
    _run(ctx, _case(shape, 3, "checker"), 0.5, 0.75, _want(shape, 3, "checker", conn, max_regions=0), ("no regions", conn), conn=conn, max_regions=0)


# ------------------------------------------------------------------------------------------
# 2. the keep rule
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2 * T + 1, T - 1), (50, 67)], ids=_id)
def test_hysteresis_and_min_area_drop_components_and_the_numbering_skips_them(ctx, shape):
    m = _case(shape, 3, "random30")
    every = _want(shape, 3, "random30", 4, plain=True, max_regions=1024)
    hyst = _want(shape, 3, "random30", 4, max_regions=1024)
    big = _want(shape, 3, "random30", 4, min_area=3, max_regions=1024)
    assert (hyst[2] > 0).all() and (hyst[2] < every[2]).all() and (big[2] > 0).all() and (big[2] < hyst[2]).all()      # some dropped, some kept, each time
    _run(ctx, m, 0.5, 0.5, every, "hi == lo", conn=4, max_regions=1024)
    _run(ctx, m, 0.5, 0.75, hyst, "hysteresis", conn=4, max_regions=1024)
    _run(ctx, m, 0.5, 0.75, big, "min_area 3", conn=4, min_area=3, max_regions=1024)
    # a dropped component lies before a kept one in index order: the kept one's number is not its place among all components
    assert all((hyst[0][b] != every[0][b])[hyst[0][b] > 0].any() for b in range(3))


# ------------------------------------------------------------------------------------------
# 3. the values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
def test_below_on_an_ssim_like_map(ctx, conn):
    shape = (50, 67)
    for kind in ("random50", "spiral", "checker"):
        _run(ctx, _case(shape, 3, kind, "below"), 0.5, 0.25, _want(shape, 3, kind, conn, "below"), ("below", kind, conn), sense="below", conn=conn)
    rng = np.random.default_rng(5)
    ssim = (1.0 - 0.6 * rng.random((2, 40, 30)) ** 4).astype(np.float32)          # mostly near 1, a few low cells
    want = R.regions(ssim, 0.9, 0.7, sense="below", connectivity=conn, max_regions=64, fill=_fill(2, 64))
    assert (want[2] > 0).all()
    _run(ctx, ssim, 0.9, 0.7, want, ("ssim-like", conn), sense="below", conn=conn)


@pytest.mark.parametrize("sense", ["above", "below"])
def test_a_baseline_is_subtracted_with_one_rounding(ctx, sense):
    """raw random floats minus a random baseline: map - ref rounds, and the rounded value decides on which side of lo a cell falls; the same map
    without the baseline gives another answer"""
    rng = np.random.default_rng(11)
    m = rng.random((3, 2 * T + 1, T + 3)).astype(np.float32)
    ref = (0.4 * rng.random((2 * T + 1, T + 3))).astype(np.float32)
    lo, hi = (0.45, 0.6) if sense == "above" else (0.25, 0.1)
    with_ref = R.regions(m, lo, hi, ref=ref, sense=sense, connectivity=8, max_regions=64, fill=_fill(3, 64))
    without = R.regions(m, lo, hi, sense=sense, connectivity=8, max_regions=64, fill=_fill(3, 64))
    assert not np.array_equal(with_ref[0], without[0])
    _run(ctx, m, lo, hi, with_ref, ("ref", sense), ref=ref, sense=sense)
    _run(ctx, m, lo, hi, without, ("no ref", sense), sense=sense)
    # cells within an ulp of the threshold after the subtraction: v = (lo + ref) - ref may or may not be lo again
    edge = (np.float32(lo) + ref)[None].astype(np.float32).repeat(2, axis=0)
    edge[1] = np.nextafter(edge[1], np.float32(-1.0 if sense == "above" else 2.0))
    want = R.regions(edge, lo, lo, ref=ref, sense=sense, connectivity=4, max_regions=64, fill=_fill(2, 64))
    _run(ctx, edge, lo, lo, want, ("at the threshold", sense), ref=ref, sense=sense, conn=4)


@pytest.mark.parametrize("sense", ["above", "below"])
def test_nan_infinities_and_zeros_of_both_signs(ctx, sense):
    rng = np.random.default_rng(13)
    shape = (3, 2 * T + 1, T + 3)
    m = values(rng.random(shape) < 0.5, rng, sense)
    pick = rng.integers(0, 12, shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        m[pick == k] = np.float32(v)
    lo, hi = (0.5, 0.75) if sense == "above" else (0.5, 0.25)
    want = R.regions(m, lo, hi, sense=sense, connectivity=8, max_regions=64, fill=_fill(3, 64))
    inf = np.float32(np.inf if sense == "above" else -np.inf)
    assert (want[1]["peak"][want[1]["area"] != SENTINEL] == inf).any() and (want[0][np.isnan(m)] == 0).all()
    _run(ctx, m, lo, hi, want, ("specials", sense), sense=sense)
    # zeros of both signs around a threshold at zero: -0 is +0, as a value (foreground at lo = 0 either way), as a peak (+0 is stored) and in a tie
    z = (np.array([-0.0, 0.0, -0.5, -0.125], np.float32) * np.float32(1.0 if sense == "above" else -1.0))[rng.integers(0, 4, shape)]
    lo, hi = (-0.25, 0.0) if sense == "above" else (0.25, 0.0)
    ref = np.zeros(shape[1:], np.float32)
    for r in (None, ref, -ref):                                                    # (x - (+0) keeps x's sign, x - (-0) turns -0 into +0: the same answer)
        want = R.regions(z, lo, hi, ref=r, sense=sense, connectivity=4, max_regions=64, fill=_fill(3, 64))
        live = want[1]["area"] != SENTINEL
        assert live.any() and (want[1]["peak"][live].view(np.uint32) == 0).all()   # every kept peak is +0.0, bit for bit
        _run(ctx, z, lo, hi, want, ("zeros", sense, r is None), ref=r, sense=sense, conn=4)


def test_equal_peaks_go_to_the_smallest_index(ctx):
    """two values only: every component's peak is attained many times, and the first cell in index order is reported -- not the first in any tile"""
    rng = np.random.default_rng(17)
    for shape in ((T + 1, T + 1), (50, 67)):
        mask = R.pattern("bars", *shape)[None].repeat(2, axis=0)
        m = np.where(mask, np.float32(0.5) + 8 * Q * rng.integers(0, 2, mask.shape), np.float32(0.25)).astype(np.float32)
        m[:, : shape[0] // 2] = np.where(mask[:, : shape[0] // 2], np.float32(0.5), np.float32(0.25))      # the peak first appears beyond the first tiles
        want = R.regions(m, 0.5, 0.75, connectivity=4, max_regions=64, fill=_fill(2, 64))
        assert (want[2] == 1).all() and (want[1]["peak_i"][:, 0] >= shape[0] // 2).all()
        _run(ctx, m, 0.5, 0.75, want, ("ties", shape), conn=4)


# ------------------------------------------------------------------------------------------
# 4. run to run, and under capture
# ------------------------------------------------------------------------------------------
def test_two_runs_agree_byte_for_byte(ctx):
    for shape, kind in (((256, 256), "random60"), ((50, 67), "random50"), ((3, 1024), "spiral")):
        m = _dev(_case(shape, 3, kind), ctx)
        runs = []
        for junk in (0x11, 0xFF):
            ctx.__dict__.get("_regions_work", {}).pop((3,) + shape, None)
            work = ctx.empty(ctx.L.aefft_map_regions_workspace(shape[0], shape[1], 3), dtype=torch.uint8).fill_(junk)      # whatever the workspace held
            ctx.__dict__.setdefault("_regions_work", {})[(3,) + shape] = work
            regions = torch.full((3, 4096, 8), SENTINEL, dtype=torch.int32, device=m.device)
            labels, regions, count = ctx.map_regions(m, 0.5, 0.75, connectivity=8, max_regions=4096, regions=regions)
            ctx.sync()
            runs.append((host(labels).tobytes(), host(regions).tobytes(), host(count).tobytes()))
        assert runs[0] == runs[1], (shape, kind)


def test_the_launches_are_captured_once_and_replayed():
    shape, B = (50, 67), 3
    m = _case(shape, B, "random50")
    want = _want(shape, B, "random50", 8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = aefft.Context(0)                                                     # (enqueues on `side`, the stream the capture runs on)
    try:
        dev = f"cuda:{c.device}"
        dm = torch.zeros(m.shape, device=dev)
        labels = torch.full(m.shape, SENTINEL, dtype=torch.int32, device=dev)
        regions = torch.full((B, 64, 8), SENTINEL, dtype=torch.int32, device=dev)
        count = torch.full((B,), SENTINEL, dtype=torch.int32, device=dev)
        with torch.cuda.stream(side):
            c.map_regions(dm, 0.5, 0.75, max_regions=64, labels=labels, regions=regions, count=count)      # (the workspace is allocated before the capture)
        torch.cuda.synchronize()
        regions.fill_(SENTINEL)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.map_regions(dm, 0.5, 0.75, max_regions=64, labels=labels, regions=regions, count=count)
        torch.cuda.synchronize()
        dm.copy_(_dev(m, c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(labels), want[0]) and np.array_equal(host(count), want[2])
        assert host(regions).tobytes() == np.ascontiguousarray(want[1]).tobytes()
        del g
    finally:
        c.close()


# ------------------------------------------------------------------------------------------
# 5. the Python paths
# ------------------------------------------------------------------------------------------
def test_detect_tiled_is_score_tiled_then_map_regions(ctx):
    """a 3 -> 4 -> 3 net with 5 x 5 kernels on two 130 x 70 x 3 images: detect_tiled's map and out are score_tiled's, its labels, regions and counts
    map_regions' of that map -- and the restatement's --, with sense "below" for the SSIM; the boxes in pixels are the C call's"""
    D, N, Bn, dM, Nk, W, H, V, M = 3, 64, 2, 4, 5, 130, 70, 16, 4
    rng = np.random.default_rng(21)
    q32 = lambda v: v.astype(np.float32).astype(np.float64)
    c, f = q32(0.1 * rng.uniform(-1, 1, (dM, D, Nk, Nk))), q32(0.1 * rng.uniform(-1, 1, (D, dM, Nk, Nk)))
    bias, p = q32(rng.uniform(-1, 1, dM)), q32(rng.uniform(-1, 1, D))
    image = rng.integers(0, 256, (2, H, W, D), dtype=np.uint8)
    cells = aefft.cells_for_tile(W, H, 16)
    net = aefft.Net(ctx, D, N, N, [dM], Nk, 2, batch=Bn)
    try:
        net.set_pair(0, c, bias, f, p)
        img = _dev(image, ctx)
        for metric in ("mse", "ssim"):
            m, _, out = net.score_tiled(img, V, M, tile=16, metric=metric, score=False)
            ctx.sync()
            mh = host(m)
            lo, hi = (float(np.median(mh)), float(np.quantile(mh, 0.9))) if metric == "mse" else (float(np.median(mh)), float(np.quantile(mh, 0.1)))
            labels, regions, count, m2, out2 = net.detect_tiled(img, V, M, tile=16, metric=metric, lo=lo, hi=hi, connectivity=4, min_area=2, max_regions=32)
            l1, r1, c1 = ctx.map_regions(m, lo, hi, sense="below" if metric == "ssim" else "above", connectivity=4, min_area=2, max_regions=32)
            ctx.sync()
            assert np.array_equal(host(m2).view(np.uint32), mh.view(np.uint32)) and np.array_equal(host(out2), host(out))
            want = R.regions(mh, lo, hi, sense="below" if metric == "ssim" else "above", connectivity=4, min_area=2, max_regions=32)
            assert (want[2] > 0).all()
            for got in ((labels, regions, count), (l1, r1, c1)):
                assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[2]), want[2]), metric
                assert host(got[1]).tobytes() == want[1].tobytes(), metric
            recs = host(regions).view(aefft.REGION)[..., 0]
            for b in range(2):
                for r in recs[b, :int(want[2][b])]:
                    box = aefft.region_pixels(r, cells, W, H)
                    assert box == R.to_pixels(r, cells[0], cells[1], W, H) and 0 <= box[0] < box[2] <= W and 0 <= box[1] < box[3] <= H
        with pytest.raises(ValueError):
            net.detect_tiled(img, V, M)
    finally:
        net.close()


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(ctx):
    L = ctx.L
    Mx, My, B, MR = 5, 7, 2, 4
    dev = f"cuda:{ctx.device}"
    n = B * Mx * My
    inp = torch.full((1024,), 0.625, device=dev)                                  # the map and the baseline
    o = torch.full((4096,), SENTINEL, dtype=torch.int32, device=dev)              # labels, regions, count and the workspace
    ip, op = inp.data_ptr(), o.data_ptr()
    mp, rp = ip, ip + 2048
    lp, gp, cp, wp = op, op + 1024, op + 2048, op + 4096
    need = L.aefft_map_regions_workspace(Mx, My, B)
    assert ip % 16 == 0 and op % 16 == 0 and need == 16 * n and 4096 + need <= 4 * 4096
    good = dict(map=mp, ref=rp, Mx=Mx, My=My, B=B, sense=0, lo=0.5, hi=0.75, conn=8, min_area=1, labels=lp, regions=gp, max_regions=MR, count=cp, work=wp,
                work_bytes=need)
    call = lambda **kw: L.aefft_map_regions(ctx.h, *dict(good, **kw).values())
    NULL, SIZE, BATCH, INT = "null context, map, labels, count or workspace", "Mx, My must be in 1..1024", "B must be >= 1", "B * Mx * My does not fit an int"
    SENSE, CONN = "sense must be AEFFT_REGIONS_ABOVE or AEFFT_REGIONS_BELOW", "connectivity must be 4 or 8"
    FINITE, ORDER = "lo and hi must be finite", "lo and hi in the wrong order: AEFFT_REGIONS_ABOVE needs lo <= hi, AEFFT_REGIONS_BELOW hi <= lo"
    AREA, MAXR, AGREE = "min_area must be >= 1", "max_regions must be in 0..65536", "regions_d must be NULL exactly when max_regions == 0"
    ALIGN, WORK = "map_d, ref_d, labels_d, regions_d, count_d and work_d must be 16-byte aligned", "work_bytes is below aefft_map_regions_workspace(Mx, My, B)"
    OVER = "the labels, regions, count and workspace ranges overlap an input or each other"
    cases = [
        ("null map", dict(map=None), NULL), ("null labels", dict(labels=None), NULL), ("null count", dict(count=None), NULL), ("null workspace", dict(work=None), NULL),
        ("Mx = 0", dict(Mx=0), SIZE), ("Mx = 1025", dict(Mx=1025), SIZE), ("My = 0", dict(My=0), SIZE), ("My = 1025", dict(My=1025), SIZE), ("My < 0", dict(My=-3), SIZE),
        ("B = 0", dict(B=0), BATCH), ("B < 0", dict(B=-1), BATCH), ("cells beyond an int", dict(B=2 ** 31 - 1), INT), ("cells just beyond an int", dict(Mx=1024, My=1024, B=2048), INT),
        ("sense 2", dict(sense=2), SENSE), ("sense -1", dict(sense=-1), SENSE), ("connectivity 6", dict(conn=6), CONN), ("connectivity 0", dict(conn=0), CONN),
        ("lo NaN", dict(lo=float("nan")), FINITE), ("hi inf", dict(hi=float("inf")), FINITE), ("lo -inf", dict(lo=float("-inf")), FINITE),
        ("above with lo > hi", dict(lo=0.8), ORDER), ("below with hi > lo", dict(sense=1), ORDER),
        ("min_area 0", dict(min_area=0), AREA), ("max_regions -1", dict(max_regions=-1), MAXR), ("max_regions 65537", dict(max_regions=65537), MAXR),
        ("regions without max_regions", dict(max_regions=0), AGREE), ("max_regions without regions", dict(regions=None), AGREE),
        ("map off by 4", dict(map=mp + 4), ALIGN), ("ref off by 8", dict(ref=rp + 8), ALIGN), ("labels off by 4", dict(labels=lp + 4), ALIGN),
        ("regions off by 8", dict(regions=gp + 8), ALIGN), ("count off by 4", dict(count=cp + 4), ALIGN), ("workspace off by 8", dict(work=wp + 8), ALIGN),
        ("a workspace one byte short", dict(work_bytes=need - 1), WORK), ("no workspace bytes", dict(work_bytes=0), WORK),
        ("labels in the map", dict(labels=mp + 16), OVER), ("the map ends in the labels", dict(map=lp - 256), OVER), ("labels in the baseline", dict(labels=rp), OVER),
        ("regions in the labels", dict(regions=lp + 256), OVER), ("count in the regions", dict(count=gp + 32 * B * MR - 16), OVER),
        ("count in the workspace", dict(count=wp + 16), OVER), ("the workspace over the map", dict(work=mp), OVER), ("the workspace over the labels", dict(work=lp + 16), OVER),
    ]
    for what, kw, rule in cases:
        assert call(**kw) == aefft.EINVAL, what
        msg = L.aefft_last_error(ctx.h).decode()
        assert msg == "aefft_map_regions: " + rule, (what, msg)
    ctx.sync()
    assert (host(inp) == 0.625).all() and (host(o) == SENTINEL).all()
    # what is NOT an error: neighbouring ranges, no baseline, no regions, lo == hi, a larger workspace; and the call is right afterwards
    m = _case((Mx, My), B, "random50")
    inp[:n] = _dev(m, ctx).reshape(-1)
    inp[512:512 + Mx * My] = 0.0
    assert call(labels=lp, regions=lp + 4 * n + (-4 * n) % 16, count=cp, work_bytes=need + 64) == aefft.OK
    assert call(ref=None, regions=None, max_regions=0, hi=0.5) == aefft.OK
    assert call() == aefft.OK
    ctx.sync()
    want = R.regions(m, 0.5, 0.75, connectivity=8, max_regions=MR, fill=_fill(B, MR))
    got = host(o)
    assert np.array_equal(got[:n], want[0].reshape(-1)) and np.array_equal(got[512:512 + B], want[2])
    assert got[256:256 + 8 * B * MR].tobytes() == np.ascontiguousarray(want[1]).tobytes()
    # the binding refuses what the C call would, before it reaches the library; a library error surfaces with its message
    dm = inp[:n].view(B, Mx, My)
    for kw in (dict(sense="up"), dict(connectivity=6), dict(lo=0.8, hi=0.5), dict(min_area=0), dict(max_regions=-1), dict(lo=float("nan")),
               dict(labels=torch.empty(B, My, Mx, dtype=torch.int32, device=dev)), dict(regions=torch.empty(B, 256, 4, dtype=torch.int32, device=dev)),
               dict(count=torch.empty(B, device=dev)), dict(ref=torch.empty(My, Mx, device=dev))):
        with pytest.raises(ValueError):
            ctx.map_regions(dm, **dict(dict(lo=0.5), **kw))
    with pytest.raises(ValueError):
        ctx.map_regions(dm.double(), 0.5)
    with pytest.raises(aefft.AefftError, match="overlap"):
        ctx.map_regions(dm, 0.5, labels=inp[:n].view(torch.int32).view(B, Mx, My))


def test_region_pixels_is_the_c_call(ctx):
    L = ctx.L
    for (Mx, My, W, H) in ((4, 3, 13, 9), (9, 5, 130, 70), (120, 68, 1920, 1080)):
        for i0, i1, j0, j1 in ((0, Mx - 1, 0, My - 1), (0, 0, 0, 0), (Mx - 1, Mx - 1, My - 1, My - 1), (Mx // 3, Mx // 2, My // 3, My // 2)):
            r = aefft.Region(i0, j0, i1, j1, 1, i0, j0, 0.0)
            box = [C.c_int() for _ in range(4)]
            assert L.aefft_region_to_pixels(C.byref(r), Mx, My, W, H, *[C.byref(v) for v in box]) == aefft.OK
            assert aefft.region_pixels(r, (Mx, My), W, H) == tuple(v.value for v in box) == R.to_pixels(dict(i0=i0, j0=j0, i1=i1, j1=j1), Mx, My, W, H)


# ------------------------------------------------------------------------------------------
# 7. profile accounting
# ------------------------------------------------------------------------------------------
def test_the_call_is_accounted_as_one_image_entry_with_its_bytes(ctx):
    shape, B = (50, 67), 3
    m = _dev(_case(shape, B, "random50"), ctx)
    ctx.map_regions(m, 0.5, 0.75, max_regions=64)                                # (the zero fill of the allocated regions is torch's)
    n = B * 50 * 67 * 24 + 32 * B * 64
    ctx.prof_enable(); ctx.prof_reset()
    try:
        ctx.map_regions(m, 0.5, 0.75, max_regions=64)
        one = ctx.prof_read()
        ctx.map_regions(m, 0.5, 0.75, max_regions=0)
        two = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    assert one["image"]["launches"] == 1 and one["image"]["bytes"] == n
    assert two["image"]["launches"] == 2 and two["image"]["bytes"] == 2 * n - 32 * B * 64
    assert sum(v["launches"] for v in two.values()) == 2
