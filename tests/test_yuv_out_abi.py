"""aefft_image_to_yuv and aefft_frames_resize_to_yuv at the boundary (no GPU): declared behind aefft_frames_tiles_to_image, exported and
prototyped; the destination descriptor's ctypes.Structure; the method signatures; the argument error that needs no device; the header's
description (tables, formulas, layouts, writes); the development-switch, net-option and profiler tables unchanged; every instantiation of the two
kernels in the back end's resource table (no scratch, no spills) with resize_kernels.rsrc still at its 16 and yuv_kernels.rsrc at its 25; the
stand-alone host check; the coefficient table re-derived from Kr, Kb with the remainder rule for the G entries; properties of the numpy restatement
(tests/yuv_out_ref.py), among them its distance from the real formula and the round trip through yuv_ref.convert over all 2^24 (R, G, B); the
Python argument checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
import yuv_out_ref as R
import yuv_ref as RI
from abi_checks import CSRC, aefft

PROTOS = {
    "aefft_image_to_yuv": ["aefft_ctx* ctx", "const unsigned char* image_d", "size_t pitch", "size_t image_stride", "int order", "const aefft_yuv_dst* dst", "int B"],
    "aefft_frames_resize_to_yuv": ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "int Nx", "int Ny", "int mode", "int order", "const aefft_yuv_dst* dst", "int B"],
}
DOC_START = "/* aefft_image_to_yuv, aefft_frames_resize_to_yuv"


def _table_ints():
    return [n for yoff, ky, *rows in R.TABLE.values() for n in (ky,) + tuple(v for row in rows for v in row)]


def test_declared_exported_prototyped_and_placed():
    h = A.header()
    for name, want in PROTOS.items():
        A.check_call(name, want, {"const aefft_yuv_dst*": aefft.YuvDst})
    # the block stands behind the tile calls and in front of the network level, the descriptor in front of the two calls
    A.in_order(h, "int aefft_frames_tiles_to_image(", DOC_START, "} aefft_yuv_dst;", "int aefft_image_to_yuv(", "int aefft_frames_resize_to_yuv(", "/* ---- network level")
    # the existing enums serve both directions: none is declared again
    for e in ("enum { AEFFT_YUV_NV12", "enum { AEFFT_YUV_BT601", "enum { AEFFT_YUV_BGR"):
        assert h.count(e) == 1 and h.index(e) < h.index(DOC_START)


def test_descriptor_structure_has_the_headers_fields_in_order():
    assert A.struct_fields("aefft_yuv_dst") == ["int format, matrix", "int W, H", "unsigned char* plane[3]", "size_t pitch[3]", "size_t stride[3]"]
    f = aefft.YuvDst._fields_
    assert [n for n, _ in f] == ["format", "matrix", "W", "H", "plane", "pitch", "stride"]
    assert [t for _, t in f[:4]] == [C.c_int] * 4
    assert f[4][1]._type_ is C.c_void_p and f[4][1]._length_ == 3
    assert all(t._type_ is C.c_size_t and t._length_ == 3 for _, t in f[5:])
    assert C.sizeof(aefft.YuvDst) == 16 + 9 * C.sizeof(C.c_void_p) == C.sizeof(aefft.YuvDesc)


def test_context_method_signatures():
    p = inspect.signature(aefft.Context.image_to_yuv).parameters
    assert list(p) == ["self", "image", "fmt", "matrix", "order", "out"]
    assert (p["matrix"].default, p["order"].default, p["out"].default) == ("bt601", "bgr", None) and p["fmt"].default is inspect.Parameter.empty
    p = inspect.signature(aefft.Context.frames_resize_to_yuv).parameters
    assert list(p) == ["self", "frames", "size", "fmt", "matrix", "order", "mode", "out"]
    assert (p["matrix"].default, p["order"].default, p["mode"].default, p["out"].default) == ("bt601", "bgr", "linear", None)
    assert p["size"].default is inspect.Parameter.empty and p["fmt"].default is inspect.Parameter.empty


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 1024)()
    base = C.addressof(buf)
    d = aefft.YuvDst()
    d.format, d.matrix, d.W, d.H = 0, 0, 8, 8
    d.plane[0], d.plane[1] = base, base + 64
    d.pitch[0], d.pitch[1] = 8, 8
    src = C.c_void_p(base + 512)
    assert L.aefft_image_to_yuv(None, src, 24, 192, 0, C.byref(d), 1) == A.EINVAL
    for mode in (0, 1):
        assert L.aefft_frames_resize_to_yuv(None, src, 1, 8, 8, mode, 0, C.byref(d), 1) == A.EINVAL
    assert L.aefft_image_to_yuv(None, None, 0, 0, 0, None, 0) == A.EINVAL
    assert L.aefft_frames_resize_to_yuv(None, None, 0, 0, 0, 0, 0, None, 0) == A.EINVAL
    assert bytes(buf) == bytes(1024)


def test_header_describes_the_calls():
    doc = A.doc(DOC_START, "} aefft_yuv_dst;", margin=False)
    ints = _table_ints()
    assert len(ints) == 30
    for n in ints:
        assert str(n) in doc, n
    for word in ("autoencoder.cpp:217-223", "Y = yoff + ((yr R + yg G + yb B + 2^19) >> 20)", "16..235 (0..255 for JPEG) without a clamp", "one luma sample per pixel",
                 "U = clamp(128 + ((ur S_R + ug S_G + ub S_B + (n << 19)) >> (20 + log2 n)), 0, 255)", "V likewise with (vr, vg, vb)", "LIVE pixels",
                 "(2x'..2x'+1, 2y'..2y'+1)", "n = 4, 2 at an odd edge, 1 at the odd corner", "the pair (2x', 2x'+1) of one row, n = 2", "arithmetic shifts", "the floor",
                 "rounded box average", "nearest (replicated)", "no interpolation and no siting offset", "below 2^30", "q(k) = round(k 2^20)", "s_y = 219 / 255",
                 "s_c = 224 / 255", "ky = q(s_y)", "yr = q(Kr s_y)", "yb = q(Kb s_y)", "yg = ky - yr - yb", "ub = vr = q(s_c / 2)", "ur = q(-Kr s_c / (2 (1 - Kb)))",
                 "vb = q(-Kb s_c / (2 (1 - Kr)))", "ug = -(ur + ub)", "vg = -(vr + vb)", "remainders", "sum to exactly 0", "within 0.55",
                 "Y = yoff + ((ky g + 2^19) >> 20)", "g itself for JPEG", "written as 128", "always written", "R = G = B gives U = V = 128", "channel rows swapped",
                 "four equal pixels", "constant image gives constant planes", "aefft_frames_resize_to_image into a tight image followed by aefft_image_to_yuv",
                 "no intermediate image", "aefft_frames_to_image -> aefft_image_to_yuv", "y * pitch[0] + x", "y' * pitch[1] + 2 x'", "V one byte behind", "pitch[1] >= 2 Wc",
                 "plane[0] + pitch * surface_height", "pitch[k] >= Wc", "YV12", "W must be even", "y * pitch[0] + 4 (x >> 1) + 1", "pitch[0] >= 2 W", "ANY alignment",
                 "plane[k] + b * stride[k]", "ignored when B == 1", "y * pitch + x * D + d", "image_stride >= (H - 1) * pitch + W * D", "16-byte aligned", "px_u8",
                 "W <= Nx and H <= Ny", "never written", "2 ceil(W / 2) for NV12 chroma", "ceil(W / 2) for I420 chroma", "2 W for YUYV", "nothing is read from the destination",
                 "whole dwords", "multiple of 4", "both routes give the same bytes", "OpenCV", "unmeasured", "one launch", "no host synchronisation", "no allocation",
                 "no workspace", "stream capture", "Out-of-place", "profile id `image`", "bytes read plus the bytes written", "AEFFT_EINVAL", '"aefft_image_to_yuv: "',
                 '"aefft_frames_resize_to_yuv: "', "nothing enqueued", "every output untouched", "odd W", "enlarging axis", "overlapping each other", "overlapping the source",
                 "overflow the address space", "need not outlive"):
        assert word.lower() in doc.lower(), word


def test_flag_option_and_profiler_tables_are_unchanged():
    """the calls add no development switch, no net option and no profiling id (they are accounted under `image`)"""
    names = A.tables_unchanged("YUV", profiler=("yuv",))[1]
    assert names.count("image") == 1


def test_yuv_out_kernels_use_no_scratch_and_cover_what_the_launchers_name():
    """build/yuv_out_kernels.rsrc: image_yuv_kernel<FMT, D> and frames_yuv_kernel<FMT, D, F32, MODE> for exactly the (FMT, D) the two launchers'
    switches name -- every format with D = 3 and with D = 1 (GRAY has kernels of its own for every format: I420 fills two chroma planes where NV12
    fills one) -- each with zero scratch and zero spills; not specialised on matrix or order"""
    src = open(os.path.join(CSRC, "yuv_out_kernels.hip")).read()
    image_named = {(int(f), int(d)) for f, d in re.findall(r"YO_CASE\((\d), (\d)\)", src)}
    frames_named = {(int(f), int(d)) for f, d in re.findall(r"FY_CASES\((\d), (\d)\)", src)}
    assert image_named == frames_named == {(f, d) for f in (0, 1, 2) for d in (1, 3)}
    assert "FY_CASE(FF, DD, 0, 0) FY_CASE(FF, DD, 0, 1) FY_CASE(FF, DD, 1, 0) FY_CASE(FF, DD, 1, 1)" in src
    image, frames = A.instantiations("yuv_out_kernels.rsrc", r"\d+image_yuv_kernelILi(\d)ELi(\d)EEE", r"\d+frames_yuv_kernelILi(\d)ELi(\d)ELb([01])ELi([01])EEE")
    assert image == {(str(f), str(d)) for f, d in image_named}
    assert frames == {(str(f), str(d), t, m) for f, d in frames_named for t in "01" for m in "01"}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "yuv_out_kernels.hip" in mk.split("SRCS =")[1].split("\n")[0]
    internal = open(os.path.join(CSRC, "internal.h")).read()
    assert "hipError_t launch_image_yuv(" in internal and "hipError_t launch_frames_yuv(" in internal
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    # (in the host unit the two calls stand behind their mirrors and in front of the tile section, which tests/test_tiles_abi.py pins as the last)
    at = [ops.index('extern "C" int %s(' % n) for n in ("aefft_yuv_resize_to_frames", "aefft_image_to_yuv", "aefft_frames_resize_to_yuv", "aefft_tile_plan_make")]
    assert at == sorted(at)
    assert "static int chk_yuv_dest(" in ops and ops.count("static int chk_yuv_planes(") == 1 and ops.count("format must be AEFFT_YUV_NV12") == 1


def test_the_pinned_kernel_files_still_hold_their_kernels():
    names = list(A.rsrc("resize_kernels.rsrc"))
    assert len(names) == 16 and all(re.search(r"\d+resize_kernelILi[1-4]ELb[01]ELi[01]EEE", n) for n in names)
    names = list(A.rsrc("yuv_kernels.rsrc"))
    assert len(names) == 25 and all("yuv_image_kernel" in n or "yuv_resize_kernel" in n for n in names)


def test_host_check_source_is_present_and_stands_alone():
    src = A.host_check_stands_alone("yuv_out_hostcheck.cpp", "yuv_out_kernels.hip")
    assert "int main()" in src and "LD_PRELOAD" not in src
    assert src.index('#include "hostlanes.h"') < src.index("yuv_out_kernels.hip\"")
    kern = open(os.path.join(CSRC, "yuv_out_kernels.hip")).read()
    assert "#ifndef AEFFT_HOSTCHECK" in kern
    # its restatement has a table of its own with the header's integers, and takes nothing from the kernels' tap header
    for n in _table_ints():
        assert str(n) in src and str(n) in kern, n
    assert "rz_tap" not in src and "yo_coef(" in src


@pytest.mark.parametrize("matrix", R.MATRICES)
def test_table_is_rederived_from_kr_kb(matrix):
    assert R.derive(matrix) == R.TABLE[matrix]
    yoff, ky, y, u, v = R.TABLE[matrix]
    assert sum(y) == ky and sum(u) == 0 and sum(v) == 0 and u[2] == v[0]                  # the remainder rule
    _, ry, ru, rv = R.real_coefficients(matrix)
    for row, real in ((y, ry), (u, ru), (v, rv)):
        worst = max(abs(k - r * 2.0 ** 20) for k, r in zip(row, real))
        print(matrix, "distance of the row from its own rounding", [round(k - r * 2.0 ** 20, 3) for k, r in zip(row, real)])
        assert abs(row[0] - real[0] * 2.0 ** 20) <= 0.5 and abs(row[2] - real[2] * 2.0 ** 20) <= 0.5 and worst <= 0.55


def test_properties_of_the_restatement():
    rng = np.random.default_rng(2)
    for matrix in R.MATRICES:
        yoff = R.TABLE[matrix][0]
        for fmt in R.FORMATS:
            # R = G = B: U = V = 128 everywhere, and the planes of the GRAY order
            g = rng.integers(0, 256, (2, 9, 12, 1), dtype=np.uint8)
            grey3, grey1 = R.image_to_yuv(np.repeat(g, 3, axis=-1), fmt, matrix, "bgr"), R.image_to_yuv(g, fmt, matrix, "gray")
            assert all(np.array_equal(a, b) for a, b in zip(grey3, grey1))
            if fmt == "yuyv":
                assert (grey1[0][..., 1::2] == 128).all()
                luma = grey1[0][..., 0::2].reshape(2, 9, 12)
            else:
                assert all((p == 128).all() for p in grey1[1:])
                luma = grey1[0]
            assert np.array_equal(luma, g[..., 0]) if matrix == "jpeg" else (luma.min() >= 16 and luma.max() <= 235)
            # RGB is BGR with the channel rows swapped
            img = rng.integers(0, 256, (2, 9, 12, 3), dtype=np.uint8)
            assert all(np.array_equal(a, b) for a, b in zip(R.image_to_yuv(img, fmt, matrix, "rgb"), R.image_to_yuv(np.ascontiguousarray(img[..., ::-1]), fmt, matrix, "bgr")))
            # a block of four equal pixels gives what one pixel would; a constant image gives constant planes
            px = rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8)
            const = R.image_to_yuv(np.broadcast_to(px, (1, 6, 8, 3)), fmt, matrix, "rgb")
            Y1, U1, V1 = R.pixel_yuv(px[..., 0], px[..., 1], px[..., 2], matrix)
            want = {"nv12": (Y1, np.stack([U1, V1], -1)), "i420": (Y1, U1, V1), "yuyv": (np.stack([Y1, U1, Y1, V1], -1),)}[fmt]
            flat =[p.reshape(-1, p.shape[-1]) if p.ndim == 4 else p.reshape(-1, 1) for p in const]
            wflat = [np.asarray(w).reshape(1, -1) for w in want]
            assert all((p == w).all() for p, w in zip(flat, wflat)), (fmt, matrix)
        assert R.pixel_yuv(0, 0, 0, matrix)[0] == yoff and R.pixel_yuv(255, 255, 255, matrix)[0] == (255 if matrix == "jpeg" else 235)
    # the blocks: odd sizes reach n = 2 and n = 1, and the sample is the rounded mean of its live pixels when the channels are equal (JPEG: U = V = 128)
    img = rng.integers(0, 256, (1, 3, 5, 3), dtype=np.uint8)
    y, u, v = R.image_to_yuv(img, "i420", "bt601", "rgb")
    assert y.shape == (1, 3, 5) and u.shape == v.shape == (1, 2, 3)
    assert u[0, 1, 2] == R.pixel_yuv(*img[0, 2, 4], "bt601")[1] and v[0, 1, 2] == R.pixel_yuv(*img[0, 2, 4], "bt601")[2]                 # n = 1: the corner pixel's own
    S = img[0, 0:2, 4].astype(np.int64).sum(axis=0)                                                                                        # n = 2: the last column
    ku = R.TABLE["bt601"][3]
    assert u[0, 0, 2] == np.clip(128 + ((ku[0] * S[0] + ku[1] * S[1] + ku[2] * S[2] + (2 << 19)) >> 21), 0, 255)
    q = R.image_to_yuv(img[:, :, :4], "yuyv", "bt601", "rgb")[0]
    assert q.shape == (1, 3, 2, 4) and q[0, 2, 1, 0] == y[0, 2, 2] and q[0, 2, 1, 2] == y[0, 2, 3]
    nv = R.image_to_yuv(img, "nv12", "bt601", "rgb")
    assert np.array_equal(nv[0], y) and np.array_equal(nv[1][..., 0], u) and np.array_equal(nv[1][..., 1], v)


@pytest.mark.parametrize("matrix", R.MATRICES)
def test_restatement_against_the_real_formula_and_the_round_trip_over_all_triples(matrix):
    """over all 2^24 (R, G, B), chroma of the pixel's own (n = 1): |restatement - clamp(floor(real + 1/2))| <= 1 in float64 for Y, U and V (the
    counts of differing triples are printed -- DESIGN.md section 25 records them --, not asserted), and yuv_ref.convert (the existing inverse) gives
    the pixel back within 2 grey levels for BT601 and BT709 and within 1 for JPEG"""
    yoff, ry, ru, rv = R.real_coefficients(matrix)
    G, B = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    differing, worst, back = [0, 0, 0], [0, 0, 0], 0
    for Rv in range(256):
        Rr = np.full_like(G, Rv)
        got = R.pixel_yuv(Rr, G, B, matrix)
        for k, (row, off, lo, hi) in enumerate(((ry, yoff, 0, 255), (ru, 128, 0, 255), (rv, 128, 0, 255))):
            real = off + row[0] * Rv + row[1] * G.astype(np.float64) + row[2] * B.astype(np.float64)
            d = np.abs(got[k] - np.clip(np.floor(real + 0.5), lo, hi).astype(np.int64))
            differing[k] += int((d > 0).sum()); worst[k] = max(worst[k], int(d.max()))
        rgb = RI.convert(*got, matrix, "rgb").astype(np.int64)
        back = max(back, int(np.abs(rgb - np.stack([Rr, G, B], axis=-1)).max()))
    print(matrix, "triples that differ from the float64 formula (Y, U, V):", differing, "of", 2 ** 24, "worst", worst, "round trip worst", back)
    assert max(worst) <= 1
    assert back <= (1 if matrix == "jpeg" else 2)


def test_python_argument_checks_need_no_device():
    f = aefft._yuv_dest
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    assert aefft.yuv_plane_shapes("nv12", 2, 11, 9) == [(2, 9, 11), (2, 5, 6, 2)]
    assert aefft.yuv_plane_shapes("i420", 2, 11, 9) == [(2, 9, 11), (2, 5, 6), (2, 5, 6)] and aefft.yuv_plane_shapes("yuyv", 1, 12, 9) == [(1, 9, 6, 4)]
    assert f("nv12", "bt601", "bgr", 2, 11, 9, 3, None, "t") == (None, [])
    dst, keep = f("nv12", "bt709", "rgb", 2, 11, 9, 3, (u8(2, 9, 11), u8(2, 5, 6, 2)), "t")
    assert isinstance(dst, aefft.YuvDst) and (dst.format, dst.matrix, dst.W, dst.H) == (0, 1, 11, 9) and len(keep) == 2
    assert list(dst.pitch)[:2] == [11, 12] and list(dst.stride)[:2] == [99, 60]
    dst, _ = f("i420", "jpeg", "gray", 1, 11, 9, 1, (u8(9, 11), u8(5, 6), u8(5, 6)), "t")                  # unbatched; gray still fills every plane
    assert (dst.format, dst.matrix) == (1, 2) and list(dst.pitch) == [11, 6, 6] and all(dst.plane[k] for k in range(3))
    dst, _ = f("yuyv", "bt601", "bgr", 2, 12, 9, 3, (u8(2, 9, 6, 4),), "t")
    assert dst.pitch[0] == 24
    # two views into one encoder surface: the parent's pitch, a batch stride that is not the plane's size
    surf = u8(2, 16 + 8, 64)
    y, uv = surf[:, :9, :11], surf[:, 16:16 + 5, :12].unflatten(-1, (6, 2))
    dst, _ = f("nv12", "bt601", "bgr", 2, 11, 9, 3, (y, uv), "t")
    assert list(dst.pitch)[:2] == [64, 64] and list(dst.stride)[:2] == [24 * 64, 24 * 64] and dst.plane[1] - dst.plane[0] == 16 * 64
    nv = (u8(2, 9, 11), u8(2, 5, 6, 2))
    bad = [("nv21", "bt601", "bgr", 2, 11, 9, 3, nv), ("nv12", "bt2020", "bgr", 2, 11, 9, 3, nv), ("nv12", "bt601", "bgra", 2, 11, 9, 3, nv),
           ("nv12", "bt601", "bgr", 2, 11, 9, 1, nv), ("nv12", "bt601", "gray", 2, 11, 9, 3, nv), ("nv12", "bt601", "bgr", 2, 11, 9, 4, nv),
           ("yuyv", "bt601", "bgr", 2, 11, 9, 3, None), ("nv12", "bt601", "bgr", 1, 8193, 2, 3, None), ("nv12", "bt601", "bgr", 1, 8, 0, 3, None),
           ("nv12", "bt601", "bgr", 2, 11, 9, 3, nv[:1]), ("nv12", "bt601", "gray", 2, 11, 9, 1, nv[:1]), ("nv12", "bt601", "bgr", 2, 12, 9, 3, nv),
           ("nv12", "bt601", "bgr", 1, 11, 9, 3, nv), ("nv12", "bt601", "bgr", 2, 11, 9, 3, (nv[0], u8(2, 5, 6))), ("nv12", "bt601", "bgr", 2, 11, 9, 3, (nv[0].float(), nv[1])),
           ("i420", "bt601", "bgr", 2, 11, 9, 3, (nv[0], u8(2, 5, 6), u8(2, 5, 7))), ("nv12", "bt601", "bgr", 2, 11, 9, 3, (u8(2, 9, 22)[:, :, ::2], nv[1])),
           ("nv12", "bt601", "bgr", 2, 11, 9, 3, (None, nv[1])), ("nv12", "bt601", "bgr", 2, 11, 9, 3, 5)]
    for fmt, matrix, order, B, W, H, D, out in bad:
        with pytest.raises(ValueError):
            f(fmt, matrix, order, B, W, H, D, out, "t")
