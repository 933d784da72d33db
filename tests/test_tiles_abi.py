"""Tiled inference at the boundary (no GPU): aefft_tile_plan_make, aefft_image_tiles_to_frames and aefft_frames_tiles_to_image declared in the
image-boundary block behind aefft_yuv_resize_to_frames, exported and prototyped; the header's statement of the formulas; the plan through ctypes
against the numpy restatement of tiles_ref.py on a sweep; the properties of the definition on the restatement (the weights sum to den, at most
two tiles per axis, the kept areas cover the image, blend(gather(x)) == x); the argument errors that need no device; the Python layout rules;
every instantiation of the kernels in the back end's resource table (no scratch, no spills); the host check program."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
import tiles_ref as R
from abi_checks import CSRC, ROOT, aefft

PLAN, GATHER, BLEND = "aefft_tile_plan_make", "aefft_image_tiles_to_frames", "aefft_frames_tiles_to_image"
PROTOS = {
    PLAN: ["const aefft_tile_desc* desc", "aefft_tile_plan* plan"],
    GATHER: ["aefft_ctx* ctx", "const unsigned char* image_d", "size_t pitch", "size_t image_stride", "const aefft_tile_desc* desc", "void* frames_d",
             "int frames_u8", "int B", "int D"],
    BLEND: ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "const aefft_tile_desc* desc", "unsigned char* image_d", "size_t pitch",
            "size_t image_stride", "int B", "int D"],
}
FIELDS = ["ntx", "nty", "ox0", "oy0", "step_x", "step_y", "ramp_x", "ramp_y"]


def _sweep():
    """(N, V, M): every legal pair for N <= 16, a handful above"""
    out = []
    for N in (2, 3, 8, 9, 16):
        out += [(N, V, M) for V in range(N // 2 + 1) for M in range(V // 2 + 1)]
    out += [(64, 0, 0), (64, 32, 16), (64, 32, 0), (64, 9, 4), (64, 7, 1), (512, 64, 8), (512, 256, 128), (512, 0, 0), (512, 33, 0), (512, 255, 3)]
    return out


WIDTHS = list(range(1, 41)) + [130, 641, 1920]


# 1.
def test_declared_exported_and_prototyped():
    for name, want in PROTOS.items():
        A.check_call(name, want, {"const aefft_tile_desc*": aefft.TileDesc, "aefft_tile_plan*": aefft.TilePlan})
    for struct, fields in (("aefft_tile_desc", ["W", "H", "Nx", "Ny", "overlap_x", "overlap_y", "rim_x", "rim_y"]), ("aefft_tile_plan", FIELDS)):
        decls = A.struct_fields(struct)
        assert all(d.startswith("int ") for d in decls) and [n for d in decls for n in d[len("int "):].split(", ")] == fields
    assert [f[0] for f in aefft.TileDesc._fields_] == ["W", "H", "Nx", "Ny", "overlap_x", "overlap_y", "rim_x", "rim_y"]
    assert [f[0] for f in aefft.TilePlan._fields_] == FIELDS
    assert all(f[1] is C.c_int for f in aefft.TileDesc._fields_ + aefft.TilePlan._fields_)
    p = inspect.signature(aefft.Context.image_tiles_to_frames).parameters
    assert list(p) == ["self", "image", "tile", "overlap", "rim", "out", "dtype"] and [p[n].default for n in list(p)[4:]] == [0, None, torch.uint8]
    p = inspect.signature(aefft.Context.frames_tiles_to_image).parameters
    assert list(p) == ["self", "frames", "size", "overlap", "rim", "out"] and [p[n].default for n in list(p)[4:]] == [0, None]
    p = inspect.signature(aefft.Net.infer_tiled).parameters
    assert list(p) == ["self", "image", "overlap", "rim", "out"] and [p[n].default for n in list(p)[3:]] == [0, None]
    assert list(inspect.signature(aefft.tile_plan).parameters) == ["W", "H", "Nx", "Ny", "overlap", "rim"]


# 2.
def test_the_calls_stand_behind_yuv_resize_in_the_image_boundary_block():
    A.in_order(A.header(), "int aefft_yuv_resize_to_frames(", "/* aefft_tile_plan_make", "} aefft_tile_desc;", "} aefft_tile_plan;", "int %s(" % PLAN,
               "int %s(" % GATHER, "int %s(" % BLEND, "/* ---- network level")


# 3.
def test_header_states_the_formulas():
    doc = A.doc("/* aefft_tile_plan_make", "} aefft_tile_desc;", margin=False)
    for word in ("S = N - V", "R = V - 2M", "n = max(1, ceil((W - N + 2M) / S) + 1)", "[o_t + M, o_t + N - M)", "E = (n-1) S + N - 2M - W >= 0",
                 "o_0 = -M - floor(E / 2)", "o_t = o_0 + t S", "integer arithmetic only", "1..8192", "2..2048", "0 <= 2 V <= N", "0 <= 2 M <= V",
                 "at most two tiles per axis", "(1920, 512, 64, 8) gives n = 5, S = 448, R = 48, o_0 = -192", "(13, 8, 4, 1) gives n = 3, S = 4, R = 2, o_0 = -1",
                 "(5, 8, 4, 1) gives n = 1, o_0 = -1", "(9, 8, 4, 2) gives n = 3, R = 0, o_0 = -3", "writes nothing", "no device, no context",
                 "f = (b * nty + ty) * ntx + tx", "T = B * ntx * nty",
                 "[T][D][Nx][Ny]", "(float)pixel", "16-byte aligned", "any alignment", "pitch >= W * D", "never read",
                 "frames[f][d][i][j] = image[b][ry(oy_ty + j)][rx(ox_tx + i)][d]", "BORDER_REFLECT_101", "for W = 1 the result is 0", "P = 2(W-1)",
                 "m = x mod P taken non-negative", "r = m when m < W, else P - m", "Every element of every tile is written",
                 "px_u8(v)", "first turned into pixels", "k = x - o_t", "0 when k < M or k >= N - M", "2(k - M) + 1 when t > 0 and k < M + R",
                 "2(N - M - 1 - k) + 1 when t < n-1 and k >= N - M - R", "den = 2R for R > 0 and den = 1 for R = 0", "add up to 2R",
                 "sum to den at every x", "no ramp on their outer side", "acc = sum over the (at most four) tiles of wx * wy * p",
                 "image[y][x][d] = floor((2 acc + denx deny) / (2 denx deny))", "acc < 255 * 2^22", "written once", "never written",
                 "blend(gather(image)) returns the image's bytes", "W == Nx, H == Ny, V = 0", "aefft_image_to_frames / aefft_frames_to_image",
                 "Constant tiles give a constant image", "same arguments always give the same bytes",
                 "one launch on the context's stream", "no host synchronisation", "no allocation", "no workspace", "stream capture", "Out-of-place", "profile id `image`",
                 "bytes read plus the bytes written", "AEFFT_EINVAL", '"aefft_image_tiles_to_frames: "', '"aefft_frames_tiles_to_image: "', "nothing enqueued",
                 "outputs untouched", "anything aefft_tile_plan_make refuses", "D outside 1..4", "B < 1", "pitch or stride that is too small",
                 "not 16-byte aligned", "overlapping source and destination ranges", "overflow the address space or an int tile count"):
        assert word in doc, word


# 4.
def _make(L, W, H, Nx, Ny, vx, vy, mx, my):
    d, p = aefft.TileDesc(W, H, Nx, Ny, vx, vy, mx, my), aefft.TilePlan(*([-77] * 8))
    return L.aefft_tile_plan_make(C.byref(d), C.byref(p)), tuple(getattr(p, f) for f in FIELDS)


def test_the_plan_equals_the_restatement_on_a_sweep():
    L = A.lib()
    n = 0
    for k, (N, V, M) in enumerate(_sweep()):
        for W in WIDTHS:
            # the other axis takes another member of the sweep: the two axes are independent
            N2, V2, M2 = _sweep()[(k * 7 + W) % len(_sweep())]
            H = WIDTHS[(W * 5 + k) % len(WIDTHS)]
            rc, got = _make(L, W, H, N, N2, V, V2, M, M2)
            assert rc == aefft.OK and got == R.plan(W, H, N, N2, (V, V2), (M, M2)), (W, H, N, N2, V, V2, M, M2, got)
            n += 1
    assert n == len(_sweep()) * len(WIDTHS) and n > 2000
    for (W, N, V, M), (cnt, S, Rr, o0) in {(1920, 512, 64, 8): (5, 448, 48, -192), (13, 8, 4, 1): (3, 4, 2, -1), (5, 8, 4, 1): (1, 4, 2, -1),
                                           (9, 8, 4, 2): (3, 4, 0, -3)}.items():
        rc, got = _make(L, W, W, N, N, V, V, M, M)
        assert rc == aefft.OK and got == (cnt, cnt, o0, o0, S, S, Rr, Rr)
        desc, plan = aefft.tile_plan(W, W, N, N, V, M)
        assert tuple(getattr(plan, f) for f in FIELDS) == got and (desc.overlap_x, desc.rim_y) == (V, M)
    _, plan = aefft.tile_plan(37, 29, 16, 8, (6, 4), (1, 2))
    assert tuple(getattr(plan, f) for f in FIELDS) == R.plan(37, 29, 16, 8, (6, 4), (1, 2))


# 5.
def test_the_weights_of_the_definition_sum_to_den_with_at_most_two_tiles():
    for N, V, M in _sweep():
        for W in WIDTHS:
            a = R.axis(W, N, V, M)
            w = R.weights(a)
            assert (w.sum(axis=0) == a["den"]).all(), (W, N, V, M)
            nz = (w != 0).sum(axis=0)
            assert nz.min() >= 1 and nz.max() <= 2, (W, N, V, M)
            # the kept areas [o_t + M, o_t + N - M) cover the image, and one tile fewer would not
            o = a["o0"] + a["S"] * np.arange(a["n"])
            assert o[0] + M <= 0 and o[-1] + N - M >= W and (o[1:] + M <= o[:-1] + N - M).all(), (W, N, V, M)
            assert a["n"] == 1 or (a["n"] - 2) * a["S"] + N - 2 * M < W, (W, N, V, M)
            assert (w >= 0).all() and (R.reflect(np.arange(o[0], o[-1] + N), W) < W).all()


# 6.
def test_blend_of_gather_is_the_image_on_the_restatement():
    rng = np.random.default_rng(5)
    for W, H, Nx, Ny, V, M in [(13, 9, 8, 8, 4, 1), (5, 3, 8, 8, 4, 1), (9, 9, 8, 8, 4, 2), (16, 8, 8, 8, 0, 0), (37, 29, 16, 8, (6, 4), (1, 2)),
                               (23, 17, 10, 6, (4, 3), 1), (130, 70, 32, 32, 8, 2), (1, 1, 2, 2, 0, 0), (40, 33, 9, 3, (4, 1), (2, 0)), (7, 50, 64, 16, (32, 8), (16, 4))]:
        for D in (1, 3):
            img = rng.integers(0, 256, (2, H, W, D), dtype=np.uint8)
            tiles = R.gather(img, Nx, Ny, V, M)
            ntx, nty = R.plan(W, H, Nx, Ny, V, M)[:2]
            assert tiles.shape == (2 * ntx * nty, D, Nx, Ny)
            assert np.array_equal(R.blend(tiles, W, H, V, M), img), (W, H, Nx, Ny, V, M)
            assert np.array_equal(R.blend(tiles.astype(np.float32), W, H, V, M), img)
            assert (R.blend(np.full_like(tiles, 77), W, H, V, M) == 77).all()
    # a plain partition is image_to_frames of the blocks, and the reflection is BORDER_REFLECT_101
    img = rng.integers(0, 256, (1, 8, 16, 3), dtype=np.uint8)
    tiles = R.gather(img, 8, 8, 0)
    assert np.array_equal(tiles[1], img[0, :, 8:].transpose(2, 1, 0))
    assert R.reflect(np.arange(-7, 9), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert np.array_equal(R.px_u8(np.array([np.nan, np.inf, -np.inf, -3, 300, 0.5, 1.5, 254.5, 0.49999997, 2.5], np.float32)), [0, 255, 0, 0, 255, 1, 2, 255, 0, 3])


# 7.
def test_every_illegal_description_is_einval_and_leaves_the_plan_untouched():
    L = A.lib()
    good = dict(W=13, H=9, Nx=8, Ny=8, vx=4, vy=4, mx=1, my=1)
    assert _make(L, **good)[0] == aefft.OK
    for bad in (dict(W=0), dict(W=8193), dict(H=0), dict(H=-1), dict(H=8193), dict(Nx=1), dict(Nx=2049), dict(Ny=1), dict(Ny=0), dict(Ny=2049),
                dict(vx=-1), dict(vx=5), dict(vy=-1), dict(vy=5), dict(mx=-1), dict(mx=3), dict(my=-1), dict(my=3), dict(vx=0), dict(vy=1),
                dict(Nx=9, vx=5), dict(vx=2 ** 30), dict(mx=2 ** 30), dict(Nx=-8)):
        rc, plan = _make(L, **dict(good, **bad))
        assert rc == aefft.EINVAL and plan == (-77,) * 8, bad
        with pytest.raises(ValueError):
            R.plan(*(dict(good, **bad)[k] for k in ("W", "H", "Nx", "Ny")), (dict(good, **bad)["vx"], dict(good, **bad)["vy"]),
                   (dict(good, **bad)["mx"], dict(good, **bad)["my"]))
        with pytest.raises(ValueError):
            g = dict(good, **bad)
            aefft.tile_plan(g["W"], g["H"], g["Nx"], g["Ny"], (g["vx"], g["vy"]), (g["mx"], g["my"]))
    d, p = aefft.TileDesc(13, 9, 8, 8, 4, 4, 1, 1), aefft.TilePlan(*([-77] * 8))
    assert L.aefft_tile_plan_make(None, C.byref(p)) == aefft.EINVAL and L.aefft_tile_plan_make(C.byref(d), None) == aefft.EINVAL
    assert tuple(getattr(p, f) for f in FIELDS) == (-77,) * 8
    # (23, 17, 10, 6) with overlap 4 on both axes breaks 2 V <= N along the rows: the device tests take overlap (4, 3) there
    assert _make(L, 23, 17, 10, 6, 4, 4, 1, 1)[0] == aefft.EINVAL and _make(L, 23, 17, 10, 6, 4, 3, 1, 1)[0] == aefft.OK
    # the limits are legal
    assert _make(L, 8192, 1, 2048, 2, 1024, 1, 512, 0) == (aefft.OK, R.plan(8192, 1, 2048, 2, (1024, 1), (512, 0)))
    for bad in ((4, 4, 4), 1.5, True, "4", (4,)):
        with pytest.raises(ValueError):
            aefft.tile_plan(13, 9, 8, 8, bad, 0)


# 8.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    img, frm = C.c_void_p(base), C.c_void_p(base + 1024)
    d = aefft.TileDesc(13, 9, 8, 8, 4, 4, 1, 1)
    for u8 in (1, 0):
        assert L.aefft_image_tiles_to_frames(None, img, 39, 0, C.byref(d), frm, u8, 1, 3) == aefft.EINVAL
        assert L.aefft_frames_tiles_to_image(None, frm, u8, C.byref(d), img, 39, 0, 1, 3) == aefft.EINVAL
    assert L.aefft_image_tiles_to_frames(None, None, 0, 0, None, None, 0, 0, 0) == aefft.EINVAL
    assert L.aefft_frames_tiles_to_image(None, None, 0, None, None, 0, 0, 0, 0) == aefft.EINVAL
    assert bytes(buf) == bytes(4096)


# 9.
def test_python_layout_rules_need_no_device():
    """the checks of Context.image_tiles_to_frames / frames_tiles_to_image run before anything reaches the device: CPU tensors suffice"""
    ga, ba = aefft._image_tiles_args, aefft._frames_tiles_args
    image = torch.zeros(2, 9, 13, 3, dtype=torch.uint8)
    img, pitch, stride, desc, shape, dtype = ga(image, (8, 8), 4, 1, None, torch.uint8)
    assert (pitch, stride, shape, dtype) == (39, 9 * 39, (2 * 3 * 2, 3, 8, 8), torch.uint8)
    assert (desc.W, desc.H, desc.Nx, desc.Ny, desc.overlap_x, desc.overlap_y, desc.rim_x, desc.rim_y) == (13, 9, 8, 8, 4, 4, 1, 1)
    big = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    roi = big[:, 3:12, 5:18]                                                               # a region of interest
    assert ga(roi, (8, 8), 4, 1, None, torch.float32)[1:3] + ga(roi, (8, 8), 4, 1, None, torch.float32)[4:] == (90, 20 * 90, (12, 3, 8, 8), torch.float32)
    assert ga(image[0], (16, 8), (6, 4), (1, 2), torch.zeros(3, 3, 16, 8), None)[4:] == ((3, 3, 16, 8), torch.float32)
    good = dict(image=image, tile=(8, 8), overlap=4, rim=1, out=None, dtype=torch.uint8)
    for bad in (dict(image=image.float()), dict(image=image[0, 0]), dict(image=image.permute(0, 2, 1, 3)), dict(image=torch.zeros(1, 4, 4, 5, dtype=torch.uint8)),
                dict(tile=8), dict(tile=(8, 1)), dict(tile=(4096, 8)), dict(overlap=5), dict(overlap=-1), dict(rim=3), dict(overlap=(4, 4, 4)), dict(rim=0.5),
                dict(dtype=torch.float64), dict(out=torch.zeros(11, 3, 8, 8, dtype=torch.uint8)), dict(out=torch.zeros(12, 3, 8, 8, dtype=torch.int8)),
                dict(out=torch.zeros(12, 3, 8, 8, dtype=torch.uint8).permute(0, 1, 3, 2))):
        with pytest.raises(ValueError):
            ga(**dict(good, **bad))
    frames = torch.zeros(12, 3, 8, 8, dtype=torch.uint8)
    desc, shape = ba(frames, (13, 9), 4, 1, None)
    assert shape == (2, 9, 13, 3) and (desc.W, desc.H, desc.Nx, desc.Ny) == (13, 9, 8, 8)
    assert ba(frames.float(), (13, 9), 4, 1, torch.zeros(2, 9, 13, 3, dtype=torch.uint8))[1] == (2, 9, 13, 3)
    assert ba(frames[:6], (13, 9), (4, 4), (1, 1), None)[1] == (1, 9, 13, 3)
    good = dict(frames=frames, size=(13, 9), overlap=4, rim=1, out=None)
    for bad in (dict(frames=frames.double()), dict(frames=frames[0]), dict(frames=frames.permute(0, 1, 3, 2)), dict(frames=frames[:5]),
                dict(frames=torch.zeros(12, 5, 8, 8, dtype=torch.uint8)), dict(frames=torch.zeros(0, 3, 8, 8, dtype=torch.uint8)), dict(size=13), dict(size=(0, 9)),
                dict(size=(8193, 9)), dict(overlap=5), dict(rim=3), dict(out=torch.zeros(2, 9, 12, 3, dtype=torch.uint8)), dict(out=torch.zeros(9, 13, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            ba(**dict(good, **bad))


# 10.
def test_tile_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/tile_kernels.rsrc: tile_gather_kernel<D, F32> and tile_blend_kernel<D, F32> for D = 1..4 x {8-bit, float} frames -- what the launcher
    selects (the dword and element routes are chosen inside a kernel) -- nothing else, each with zero scratch and zero spills"""
    [got] = A.instantiations("tile_kernels.rsrc", r"\d+tile_(gather|blend)_kernelILi(\d)ELb([01])EEE")
    assert got == {(k, d, f) for k in ("gather", "blend") for d in "1234" for f in "01"}
    assert "tile_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # the launchers are declared with the others, the entry points stand with the image calls and share their helpers
    internal = open(os.path.join(CSRC, "internal.h")).read()
    assert "hipError_t launch_tile_gather(" in internal and "hipError_t launch_tile_blend(" in internal
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    assert ops.index("// image boundary") < ops.index('extern "C" int aefft_yuv_resize_to_frames(') < ops.index('extern "C" int aefft_tile_plan_make(')
    entry = ops[ops.index('extern "C" int aefft_tile_plan_make('):]
    assert "ranges_overlap(" in entry and "aligned16(" in entry and entry.count("KID_IMAGE") == 2 and ops.count("static bool ranges_overlap(") == 1
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_image_" not in rest and "KID_IMAGE" not in rest
    # no code is shared with the other image kernels through a header
    src = open(os.path.join(CSRC, "tile_kernels.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h", "fft_common.h"}


# 11.
def test_the_host_check_program_is_there_and_stands_alone():
    A.host_check_stands_alone("tiles_hostcheck.cpp", "tile_kernels.hip")
    assert os.path.exists(os.path.join(ROOT, "tools", "tiles_bench.py"))
    # the product never imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "tiles_ref" not in open(os.path.join(dirpath, f)).read(), f
