"""aefft_yuv_to_image and aefft_yuv_resize_to_frames at the boundary (no GPU): declared behind aefft_frames_degrade, exported and prototyped; the
three enums; the descriptor's ctypes.Structure; the argument error that needs no device; the header's description (table, formula, chroma rule,
layouts); the development-switch, net-option and profiler tables unchanged; every instantiation of the two kernels in the back end's resource table
(no scratch, no spills) and resize_kernels.rsrc still at its 16; the stand-alone host check; the coefficient table re-derived from Kr, Kb; properties
of the numpy restatement (tests/yuv_ref.py), among them its distance from the real formula over all 2^24 triples; the Python argument checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
import yuv_ref as R
from abi_checks import CSRC, aefft

PROTOS = {
    "aefft_yuv_to_image": ["aefft_ctx* ctx", "const aefft_yuv_desc* src", "int order", "unsigned char* image_d", "size_t pitch", "size_t image_stride", "int B"],
    "aefft_yuv_resize_to_frames": ["aefft_ctx* ctx", "const aefft_yuv_desc* src", "int order", "int mode", "void* frames_d", "int frames_u8", "int B", "int Nx", "int Ny"],
}


def test_declared_exported_prototyped_and_placed():
    for name, want in PROTOS.items():
        A.check_call(name, want, {"const aefft_yuv_desc*": aefft.YuvDesc})
    # the block stands behind aefft_frames_degrade and in front of the network level, enums and descriptor in front of the two calls
    A.in_order(A.header(), "int aefft_frames_degrade(", "/* aefft_yuv_to_image, aefft_yuv_resize_to_frames", "enum { AEFFT_YUV_NV12", "enum { AEFFT_YUV_BT601",
               "enum { AEFFT_YUV_BGR", "} aefft_yuv_desc;", "int aefft_yuv_to_image(", "int aefft_yuv_resize_to_frames(", "/* ---- network level")


def test_enum_values_are_pinned():
    h = A.header()
    for names, table in ((("NV12", "I420", "YUYV"), aefft.YUV_FORMATS), (("BT601", "BT709", "JPEG"), aefft.YUV_MATRICES), (("BGR", "RGB", "GRAY"), aefft.YUV_ORDERS)):
        m = re.search(r"enum\s*\{\s*" + r"\s*,\s*".join(r"AEFFT_YUV_%s\s*=\s*(\d+)" % n for n in names) + r"\s*\}", h)
        assert m and [int(v) for v in m.groups()] == [0, 1, 2], names
        assert table == {n.lower(): k for k, n in enumerate(names)}
    assert tuple(aefft.YUV_FORMATS) == R.FORMATS and tuple(aefft.YUV_MATRICES) == R.MATRICES and tuple(aefft.YUV_ORDERS) == R.ORDERS


def test_descriptor_structure_has_the_headers_fields_in_order():
    assert A.struct_fields("aefft_yuv_desc") == ["int format, matrix", "int W, H", "const unsigned char* plane[3]", "size_t pitch[3]", "size_t stride[3]"]
    f = aefft.YuvDesc._fields_
    assert [n for n, _ in f] == ["format", "matrix", "W", "H", "plane", "pitch", "stride"]
    assert [t for _, t in f[:4]] == [C.c_int] * 4
    assert f[4][1]._type_ is C.c_void_p and f[4][1]._length_ == 3
    assert all(t._type_ is C.c_size_t and t._length_ == 3 for _, t in f[5:])
    assert C.sizeof(aefft.YuvDesc) == 16 + 9 * C.sizeof(C.c_void_p)


def test_context_method_signatures():
    p = inspect.signature(aefft.Context.yuv_to_image).parameters
    assert list(p) == ["self", "planes", "fmt", "matrix", "order", "out"]
    assert (p["matrix"].default, p["order"].default, p["out"].default) == ("bt601", "bgr", None)
    p = inspect.signature(aefft.Context.yuv_resize_to_frames).parameters
    assert list(p) == ["self", "planes", "fmt", "size", "matrix", "order", "mode", "out", "dtype"]
    assert (p["matrix"].default, p["order"].default, p["mode"].default, p["out"].default) == ("bt601", "bgr", "linear", None)
    assert p["dtype"].default is torch.uint8 and p["size"].default is inspect.Parameter.empty


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 1024)()
    base = C.addressof(buf)
    d = aefft.YuvDesc()
    d.format, d.matrix, d.W, d.H = 0, 0, 8, 8
    d.plane[0], d.plane[1] = base, base + 64
    d.pitch[0], d.pitch[1] = 8, 8
    dst = C.c_void_p(base + 512)
    assert L.aefft_yuv_to_image(None, C.byref(d), 0, dst, 24, 192, 1) == A.EINVAL
    for mode in (0, 1):
        assert L.aefft_yuv_resize_to_frames(None, C.byref(d), 0, mode, dst, 1, 1, 4, 4) == A.EINVAL
    assert L.aefft_yuv_to_image(None, None, 0, None, 0, 0, 0) == A.EINVAL
    assert L.aefft_yuv_resize_to_frames(None, None, 0, 0, None, 0, 0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(1024)


def test_header_describes_the_calls():
    doc = A.doc("/* aefft_yuv_to_image, aefft_yuv_resize_to_frames", "enum { AEFFT_YUV_NV12")
    ints = [n for _, ky, rows in R.TABLE.values() for n in (ky,) + tuple(v for ab in rows for v in ab if v)]
    assert len(ints) == 15
    for n in ints:
        assert str(n) in doc, n
    for word in ("autoencoder.cpp:123", ">> 20", "arithmetic shift", "2^19", "c = Y - yoff, u = U - 128, v = V - 128", "NEAREST", "replication", "(x >> 1, y >> 1)", "(x >> 1, y)",
                 "no interpolation and no siting offset", "y * pitch[0] + x", "pitch[0] >= W", "y' * pitch[1] + 2 x'", "V one byte behind", "pitch[1] >= 2 Wc",
                 "plane[0] + pitch * surface_height", "pitch[k] >= Wc", "YV12", "W must be even", "y * pitch[0] + 2 x", "y * pitch[0] + 4 (x >> 1) + 1", "two bytes further",
                 "pitch[0] >= 2 W", "ceil(W / 2)", "plane[k] + b * stride[k]", "ignored when B == 1", "never read", "may be NULL", "even x0, y0", "ANY alignment",
                 "Kr = 0.299", "Kb = 0.114", "Kr = 0.2126", "Kb = 0.0722", "255 / 219", "255 / 224", "NOT clamped below zero", "below 2^30", "(B, G, R) at d = 0, 1, 2",
                 "that is Y itself", "OpenCV", "unmeasured", "y * pitch + x * D + d", "image_stride >= (H - 1) * pitch + W * D", "never written", "bit for bit",
                 "no intermediate image", "aefft_yuv_to_image -> aefft_image_to_frames", "Nx <= W and Ny <= H", "16-byte aligned", "one launch", "no allocation", "no workspace",
                 "stream capture", "Out-of-place", "profile id `image`", "bytes read plus the bytes written", "AEFFT_EINVAL", '"aefft_yuv_to_image: "',
                 '"aefft_yuv_resize_to_frames: "', "nothing enqueued", "odd W", "enlarging axis", "overlapping", "overflow the address space", "need not outlive"):
        assert word in doc, word


def test_flag_option_and_profiler_tables_are_unchanged():
    """the calls add no development switch, no net option and no profiling id (they are accounted under `image`)"""
    names = A.tables_unchanged("YUV", profiler=("yuv",))[1]
    assert names.count("image") == 1


def test_yuv_kernels_use_no_scratch_and_cover_what_the_launchers_name():
    """build/yuv_kernels.rsrc: yuv_image_kernel<FMT, D> and yuv_resize_kernel<FMT, D, F32, MODE> for exactly the (FMT, D) the two launchers' switches
    name -- every format with D = 3, NV12 and YUYV with D = 1 (GRAY reads the luma plane only, which I420 lays out as NV12 does) -- each with zero
    scratch and zero spills; not specialised on matrix or order"""
    src = open(os.path.join(CSRC, "yuv_kernels.hip")).read()
    image_named = {(int(f), int(d)) for f, d in re.findall(r"YI_CASE\((\d), (\d)\)", src)}
    resize_named = {(int(f), int(d)) for f, d in re.findall(r"YV_CASES\((\d), (\d)\)", src)}
    assert image_named == resize_named == {(0, 1), (0, 3), (1, 3), (2, 1), (2, 3)}
    assert "YV_CASE(FF, DD, 0, 0) YV_CASE(FF, DD, 0, 1) YV_CASE(FF, DD, 1, 0) YV_CASE(FF, DD, 1, 1)" in src
    image, resize = A.instantiations("yuv_kernels.rsrc", r"\d+yuv_image_kernelILi(\d)ELi(\d)EEE", r"\d+yuv_resize_kernelILi(\d)ELi(\d)ELb([01])ELi([01])EEE")
    assert image == {(str(f), str(d)) for f, d in image_named}
    assert resize == {(str(f), str(d), t, m) for f, d in resize_named for t in "01" for m in "01"}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "yuv_kernels.hip" in mk.split("SRCS =")[1].split("\n")[0]
    assert "hipError_t launch_yuv_image(" in open(os.path.join(CSRC, "internal.h")).read() and "hipError_t launch_yuv_resize(" in open(os.path.join(CSRC, "internal.h")).read()
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    assert ops.index("// image boundary") < ops.index('extern "C" int aefft_frames_degrade(') < ops.index('extern "C" int aefft_yuv_to_image(') < ops.index('extern "C" int aefft_yuv_resize_to_frames(')
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_image_" not in rest and "KID_IMAGE" not in rest


def test_resize_kernels_still_hold_their_sixteen():
    names = list(A.rsrc("resize_kernels.rsrc"))
    assert len(names) == 16 and all(re.search(r"\d+resize_kernelILi[1-4]ELb[01]ELi[01]EEE", n) for n in names)


def test_host_check_source_is_present_and_stands_alone():
    src = A.host_check_stands_alone("yuv_hostcheck.cpp", "yuv_kernels.hip")
    assert "int main()" in src and "LD_PRELOAD" not in src
    kern = open(os.path.join(CSRC, "yuv_kernels.hip")).read()
    assert "#ifndef AEFFT_HOSTCHECK" in kern and "AEFFT_YUV_HOSTCHECK" not in kern
    # its restatement has a table of its own with the header's integers
    for _, ky, rows in R.TABLE.values():
        for n in (ky,) + tuple(v for ab in rows for v in ab if v):
            assert str(n) in src and str(n) in kern, n


@pytest.mark.parametrize("matrix", R.MATRICES)
def test_table_is_rederived_from_kr_kb(matrix):
    assert R.derive(matrix) == R.TABLE[matrix]


def test_properties_of_the_restatement():
    Y = np.arange(256)
    n = np.full(256, 128)
    for matrix in R.MATRICES:
        rgb = R.convert(Y, n, n, matrix, "rgb")
        assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all()              # u = v = 0: R = G = B
        assert np.array_equal(R.convert(Y, n, n, matrix, "gray")[:, 0], rgb[:, 0])
        if matrix == "jpeg":
            assert np.array_equal(rgb[:, 0], Y)
        else:
            assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and rgb[0, 0] == 0 and rgb[255, 0] == 255 and rgb[126, 0] == 128
    rng = np.random.default_rng(1)
    y, u, v = (rng.integers(0, 256, 4096) for _ in range(3))
    for matrix in R.MATRICES:
        assert np.array_equal(R.convert(y, u, v, matrix, "rgb"), R.convert(y, u, v, matrix, "bgr")[:, ::-1])
        assert np.array_equal(R.convert(y, u, v, "jpeg", "gray")[:, 0], y)                    # JPEG GRAY is Y, whatever the chroma
    # the gather: nearest chroma, ceil-sized planes for odd sizes; yuyv pairs
    p = R.random_planes(rng, "nv12", 2, 5, 3)
    Yg, U, V = R.gather(p, "nv12")
    assert Yg.shape == U.shape == V.shape == (2, 3, 5)
    assert U[1, 2, 4] == p[1][1, 1, 2, 0] and V[1, 2, 4] == p[1][1, 1, 2, 1] and U[0, 1, 3] == p[1][0, 0, 1, 0]
    q = R.random_planes(rng, "yuyv", 1, 4, 2)
    Yg, U, V = R.gather(q, "yuyv")
    assert Yg[0, 1, 3] == q[0][0, 1, 1, 2] and U[0, 1, 3] == q[0][0, 1, 1, 1] and V[0, 1, 2] == q[0][0, 1, 1, 3]


@pytest.mark.parametrize("matrix", R.MATRICES)
def test_restatement_is_within_one_grey_level_of_the_real_formula(matrix):
    """over all 2^24 (Y, U, V): |restatement - clamp(floor(real + 1/2))| <= 1 in float64; the count of differing triples is printed (DESIGN.md
    section 23 records it), not asserted"""
    yoff, sy, rows = R.real_coefficients(matrix)
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    differing, worst = 0, 0
    for Yv in range(256):
        Y = np.full_like(U, Yv)
        got = R.convert(Y, U, V, matrix, "rgb").astype(np.int64)
        real = np.stack([sy * (Yv - yoff) + a * (U - 128.0) + b * (V - 128.0) for a, b in rows], axis=-1)
        want = np.clip(np.floor(real + 0.5), 0, 255).astype(np.int64)
        d = np.abs(got - want)
        differing += int((d.max(axis=-1) > 0).sum()); worst = max(worst, int(d.max()))
    print(matrix, "triples that differ from the float64 formula:", differing, "of", 2 ** 24, "worst", worst)
    assert worst <= 1


def test_python_argument_checks_need_no_device():
    f = aefft._yuv_source
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    desc, B, W, H, D, _ = f((u8(2, 9, 11), u8(2, 5, 6, 2)), "nv12", "bt601", "bgr", "t")
    assert (B, W, H, D) == (2, 11, 9, 3) and (desc.format, desc.matrix, desc.W, desc.H) == (0, 0, 11, 9)
    assert list(desc.pitch)[:2] == [11, 12] and list(desc.stride)[:2] == [99, 60]
    desc, B, W, H, D, _ = f((u8(9, 11), u8(5, 6), u8(5, 6)), "i420", "bt709", "rgb", "t")                  # unbatched
    assert (B, W, H, D) == (1, 11, 9, 3) and (desc.format, desc.matrix) == (1, 1) and list(desc.pitch) == [11, 6, 6]
    desc, B, W, H, D, _ = f((u8(2, 9, 6, 4),), "yuyv", "jpeg", "gray", "t")
    assert (B, W, H, D) == (2, 12, 9, 1) and desc.pitch[0] == 24
    assert f((u8(2, 9, 11),), "nv12", "bt601", "gray", "t")[4] == 1                                        # gray: the luma plane alone
    # two views into one decoder surface: the parent's pitch, a batch stride that is not the plane's size
    surf = u8(2, 16 + 8, 64)
    y, uv = surf[:, :9, :11], surf[:, 16:16 + 5, :12].unflatten(-1, (6, 2))
    desc, B, W, H, D, _ = f((y, uv), "nv12", "bt601", "bgr", "t")
    assert list(desc.pitch)[:2] == [64, 64] and list(desc.stride)[:2] == [24 * 64, 24 * 64] and desc.plane[1] - desc.plane[0] == 16 * 64
    bad = [((u8(2, 9, 11),), "nv12", "bt601", "bgr"), ((u8(2, 9, 11), u8(2, 5, 6, 2)), "nv21", "bt601", "bgr"), ((u8(2, 9, 11), u8(2, 5, 6, 2)), "nv12", "bt2020", "bgr"),
           ((u8(2, 9, 11), u8(2, 5, 6, 2)), "nv12", "bt601", "bgra"), ((u8(2, 9, 11), u8(2, 5, 5, 2)), "nv12", "bt601", "bgr"),
           ((u8(2, 9, 11), u8(2, 4, 6, 2)), "nv12", "bt601", "bgr"), ((u8(2, 9, 11), u8(1, 5, 6, 2)), "nv12", "bt601", "bgr"),
           ((u8(2, 9, 11).float(), u8(2, 5, 6, 2)), "nv12", "bt601", "bgr"), ((u8(2, 9, 11), u8(2, 5, 6)), "nv12", "bt601", "bgr"),
           ((u8(2, 9, 11), u8(2, 5, 6), u8(2, 5, 7)), "i420", "bt601", "bgr"), ((u8(2, 9, 6, 2),), "yuyv", "bt601", "bgr"),
           ((u8(2, 9, 22)[:, :, ::2], u8(2, 5, 6, 2)), "nv12", "bt601", "bgr"), ((u8(2, 11, 9).permute(0, 2, 1), u8(2, 5, 6, 2)), "nv12", "bt601", "bgr"),
           ((None, u8(2, 5, 6, 2)), "nv12", "bt601", "bgr"), ((u8(1, 2, 8194),), "nv12", "bt601", "gray")]
    for planes, fmt, matrix, order in bad:
        with pytest.raises(ValueError):
            f(planes, fmt, matrix, order, "t")
