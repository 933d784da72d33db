"""aefft_raw_to_image at the boundary (no GPU): declared behind aefft_region_to_pixels, exported and prototyped; the three enums; the descriptor's
ctypes.Structure; the Python signatures; the argument error that needs no device; the header's description (filters, reflection rule, packed rule);
the development-switch, net-option and profiler tables unchanged; every instantiation of the two kernels in the back end's resource table (no
scratch, no spills); the stand-alone host check built and run in its quick form; properties of the numpy restatement (tests/bayer_ref.py) and of
the two table helpers; the Python argument checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks as A
import bayer_ref as R
from abi_checks import CSRC, ROOT, aefft

PROTO = ["aefft_ctx* ctx", "const aefft_raw_desc* src", "int order", "unsigned char* image_d", "size_t pitch", "size_t image_stride", "int B"]
DOC = ("/* aefft_raw_to_image: sensor data as delivered", "enum { AEFFT_RAW_RGGB")


def test_declared_exported_prototyped_and_placed():
    A.check_call("aefft_raw_to_image", PROTO, {"const aefft_raw_desc*": aefft.RawDesc})
    A.in_order(A.header(), "int aefft_region_to_pixels(", DOC[0], "enum { AEFFT_RAW_RGGB", "enum { AEFFT_RAW_U8", "enum { AEFFT_DEMOSAIC_BILINEAR",
               "} aefft_raw_desc;", "int aefft_raw_to_image(", "/* ---- network level")
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    # (in the host unit the call stands behind the regions calls, as in the header, and in front of the compare and tile sections, which their
    # own tests pin as the last two)
    A.in_order(ops, "// image boundary", 'extern "C" int aefft_region_to_pixels(', 'extern "C" int aefft_raw_to_image(', 'extern "C" int aefft_image_compare_map(')
    entry = ops[ops.index('extern "C" int aefft_raw_to_image('):ops.index('extern "C" int aefft_image_compare_map(')]
    assert "ranges_overlap(" in entry and entry.count("chk_rows(") == 2 and "IMAGE_WORDS" in entry and "join_recon(ctx)" in entry and entry.count("KID_IMAGE") == 1
    assert "hipMalloc" not in entry and "Synchronize" not in entry and "ws_get" not in entry
    assert "hipError_t launch_raw_image(" in open(os.path.join(CSRC, "internal.h")).read()
    assert "bayer_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read().split("SRCS =")[1].split("\n")[0]


def test_enum_values_are_pinned():
    h = A.header()
    for prefix, names, table in (("AEFFT_RAW_", ("RGGB", "GRBG", "GBRG", "BGGR", "MONO"), aefft.RAW_PATTERNS), ("AEFFT_RAW_", ("U8", "U16", "PACKED"), aefft.RAW_CONTAINERS),
                                 ("AEFFT_DEMOSAIC_", ("BILINEAR", "MHC"), aefft.DEMOSAIC_METHODS)):
        m = re.search(r"enum\s*\{\s*" + r"\s*,\s*".join(prefix + r"%s\s*=\s*(\d+)" % n for n in names) + r"\s*\}", h)
        assert m and [int(v) for v in m.groups()] == list(range(len(names))), names
        assert table == {n.lower(): k for k, n in enumerate(names)}
    assert tuple(aefft.RAW_PATTERNS) == R.PATTERNS and tuple(aefft.RAW_CONTAINERS) == R.CONTAINERS and tuple(aefft.DEMOSAIC_METHODS) == R.METHODS


def test_descriptor_structure_has_the_headers_fields_in_order():
    assert A.struct_fields("aefft_raw_desc") == ["int pattern, container, bits", "int W, H", "const void* data", "size_t pitch, stride", "int black, white", "float gain[3]",
                                                 "int method", "const float* ccm", "const unsigned char* lut_d"]
    f = aefft.RawDesc._fields_
    assert [n for n, _ in f] == ["pattern", "container", "bits", "W", "H", "data", "pitch", "stride", "black", "white", "gain", "method", "ccm", "lut_d"]
    assert [t for _, t in f[:5]] == [C.c_int] * 5 and f[5][1] is C.c_void_p and [t for _, t in f[6:10]] == [C.c_size_t, C.c_size_t, C.c_int, C.c_int]
    assert f[10][1]._type_ is C.c_float and f[10][1]._length_ == 3 and f[11][1] is C.c_int and f[12][1]._type_ is C.c_float and f[13][1] is C.c_void_p
    # 5 ints and padding, pointer, 2 sizes, 2 ints, 3 floats, int, 2 pointers
    assert C.sizeof(aefft.RawDesc) == 24 + 3 * C.sizeof(C.c_void_p) + 24 + 2 * C.sizeof(C.c_void_p) == 88
    assert aefft.RawDesc.data.offset == 24 and aefft.RawDesc.black.offset == 48 and aefft.RawDesc.method.offset == 68 and aefft.RawDesc.ccm.offset == 72


def test_python_signatures():
    p = inspect.signature(aefft.Context.raw_to_image).parameters
    assert list(p) == ["self", "raw", "pattern", "bits", "packed", "black", "white", "gains", "method", "order", "ccm", "lut", "out"]
    assert [p[n].default for n in list(p)[3:]] == [8, False, 0, None, (1, 1, 1), "mhc", "bgr", None, None, None]
    assert p["raw"].default is inspect.Parameter.empty and p["pattern"].default is inspect.Parameter.empty
    assert list(inspect.signature(aefft.gamma_lut).parameters) == ["gamma"] and inspect.signature(aefft.gamma_lut).parameters["gamma"].default == 2.2
    assert list(inspect.signature(aefft.srgb_lut).parameters) == []


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 1024)()
    base = C.addressof(buf)
    d = aefft.RawDesc()
    d.pattern, d.container, d.bits, d.W, d.H = 0, 0, 8, 8, 8
    d.data, d.pitch, d.stride, d.black, d.white, d.method = base, 8, 64, 0, 255, 1
    d.gain[0] = d.gain[1] = d.gain[2] = 1.0
    assert L.aefft_raw_to_image(None, C.byref(d), 0, C.c_void_p(base + 512), 24, 192, 1) == A.EINVAL
    assert L.aefft_raw_to_image(None, None, 0, None, 0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(1024)


def test_header_describes_the_call():
    doc = A.doc(*DOC)
    for word in ("GigE / USB3 Vision", "BayerRG12p", "Mono8 / Mono12 / Mono16", "bit for bit", "need not outlive", "4..8192", "odd sizes included", "ANY", "pitch >= W.",
                 "pitch >= 2 W", "multiples of 2", "low `bits` bits", "10p / 12p", "[x * bits, (x + 1) * bits)", "little-endian bit", "pitch >= ceil(W * bits / 8)",
                 "MIPI RAW10 / RAW12", "out of scope", "never read", "pixels (0,0), (1,0) of row 0 and (0,1), (1,1) of row 1", "GenICam's naming", "OpenCV's COLOR_Bayer*",
                 "shifted by one pixel", "selects the other pattern", "m_c = floor(gain_c * 255 * 65536 / (white - black) + 0.5)", "m_c > 2^30", "s = max(r - black, 0)",
                 "u = min(s * m_c, 255 << 16)", "ceil((255 << 16) / m_c)", "BEFORE the demosaic", "0 <= black < white <= 2^bits - 1", "0..64",
                 "-1 -> 1, -2 -> 2, W -> W - 2, W + 1 -> W - 3", "keeps the mosaic's parity", "swaps with B by symmetry",
                 "(N + S + E + W + 2) >> 2", "(a + b + 1) >> 1", "(NE + NW + SE + SW + 2) >> 2", "Malvar-He-Cutler", "sixteenths", "clamp((sum + 8) >> 4, 0, 255 << 16)",
                 "arithmetic shift", "|sum| < 2^29", "8 c + 4 (N + S + E + W) - 2 (N2 + S2 + E2 + W2)", "10 c + 8 (E + W) - 2 (E2 + W2) + (N2 + S2) - 2 (NE + NW + SE + SW)",
                 "10 c + 8 (N + S) - 2 (N2 + S2) + (E2 + W2) - 2 (NE + NW + SE + SW)", "12 c + 4 (NE + NW + SE + SW) - 3 (N2 + S2 + E2 + W2)", "sum to 16",
                 "HOST pointer", "NULL is the identity", "floor(ccm_ij * 1024 + 0.5)", "|entry| < 4", "q_j = (v_j + 128) >> 8", "|o| < 2^30",
                 "clamp((o + 2^17) >> 18, 0, 255)", "lut[clamp((o + 2^13) >> 14, 0, 4080)]", "4096 bytes", "entries above 4080 are never read", "rounds twice",
                 "o = 1024 q", "D = 1", "its raw byte", "constant image", "bytes of the U16 source", "y * pitch + x * D + d", "image_stride >= (H - 1) * pitch + W * D",
                 "multiples of 4", "never written", "One launch", "no allocation", "no workspace", "stream capture", "Out-of-place", "profile id `image`",
                 "bytes read plus the bytes written", "AEFFT_EINVAL", '"aefft_raw_to_image: "', "nothing enqueued", "overlap", "overflow the address"):
        assert word in doc, word


def test_flag_option_and_profiler_tables_are_unchanged():
    """the call adds no development switch, no net option and no profiling id (it is accounted under `image`)"""
    names = A.tables_unchanged("RAW", "BAYER", profiler=("raw", "bayer"))[1]
    assert names.count("image") == 1


def test_bayer_kernels_use_no_scratch_and_cover_what_the_launcher_names():
    """build/bayer_kernels.rsrc: bayer_kernel<CONT, METHOD> for the three containers and two methods and mono_kernel<CONT> for the three containers --
    exactly the cases of the launcher's switches --, each with zero scratch and zero spills; not specialised on the pattern, bits, ccm or table"""
    src = open(os.path.join(CSRC, "bayer_kernels.hip")).read()
    bayer_named = {(c, m) for c, m in re.findall(r"BA_CASE\((\d), (\d)\)", src)}
    mono_named = {(c,) for c in re.findall(r"MONO_CASE\((\d)\)", src)}
    assert bayer_named == {(c, m) for c in "012" for m in "01"} and mono_named == {(c,) for c in "012"}
    bayer, mono = A.instantiations("bayer_kernels.rsrc", r"\d+bayer_kernelILi(\d)ELi(\d)EEE", r"\d+mono_kernelILi(\d)EEE")
    assert bayer == bayer_named and mono == mono_named
    for name, (_, ints) in A.rsrc("bayer_kernels.rsrc").items():
        assert ints["VGPRs"] <= 128, (name, ints)                                # (four waves a SIMD at the least)


def test_host_check_builds_and_its_quick_form_passes(tmp_path):
    """tools/bayer_hostcheck.cpp: the kernel file compiled for the host under -fsanitize=address,undefined, a program of its own (never loaded into
    Python), against its own scalar C restatement; the quick form is the three smallest sizes, the full sweep is run by hand"""
    src = A.host_check_stands_alone("bayer_hostcheck.cpp", "bayer_kernels.hip")
    assert "LD_PRELOAD" not in src and "int main(int argc" in src
    kern = open(os.path.join(CSRC, "bayer_kernels.hip")).read()
    assert "#ifndef AEFFT_HOSTCHECK" in kern
    exe = str(tmp_path / "bayer_hostcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(ROOT, "tools", "bayer_hostcheck.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    print(r.stdout[-500:])
    assert r.returncode == 0 and re.search(r"all \d+ runs exact", r.stdout), (r.stdout[-2000:], r.stderr[-2000:])


# ------------------------------------------------------------------------------------------
# properties of the restatement
# ------------------------------------------------------------------------------------------
BAYER = R.PATTERNS[:4]


def test_eight_bit_identity_native_channel_is_the_raw_byte():
    rng = np.random.default_rng(1)
    s = rng.integers(0, 256, (2, 9, 11))
    for pattern in BAYER:
        col = R.colour_map(pattern, 11, 9)
        for method in R.METHODS:
            img = R.raw_to_image(s, pattern, 0, 255, (1, 1, 1), method, "rgb")
            native = np.take_along_axis(img, np.broadcast_to(col, s.shape)[..., None], axis=-1)[..., 0]
            assert np.array_equal(native, s), (pattern, method)
            assert np.array_equal(R.raw_to_image(s, pattern, 0, 255, (1, 1, 1), method, "bgr"), img[..., ::-1])
    assert np.array_equal(R.raw_to_image(s, "mono", 0, 255, (1,))[..., 0], s)
    assert R.multiplier(1, 0, 255) == 65536 and R.multiplier(64, 0, 1) == 64 * 255 * 65536 < 2 ** 30


def test_constant_in_constant_out():
    for pattern in BAYER:
        for method in R.METHODS:
            for value in (0, 1, 777, 4095):
                img = R.raw_to_image(np.full((1, 7, 10), value), pattern, 64, 4000, (1, 1, 1), method, "bgr")
                assert (img == img[0, 0, 0, 0]).all(), (pattern, method, value)


def test_every_filters_coefficients_sum_to_sixteen():
    for t in (R.MHC_G, R.MHC_ROW, R.MHC_COL, R.MHC_DIAG):
        assert sum(map(sum, t)) == 16 and len(t) == 5 and all(len(r) == 5 for r in t)
    assert R.MHC_COL == [list(r) for r in zip(*R.MHC_ROW)] and R.MHC_G == [list(r) for r in zip(*R.MHC_G)] and R.MHC_DIAG == [list(r) for r in zip(*R.MHC_DIAG)]
    assert [sum(map(sum, t)) for t in (R.BIL_G, R.BIL_ROW, R.BIL_COL, R.BIL_DIAG)] == [4, 2, 2, 4]


@pytest.mark.parametrize("method", R.METHODS)
def test_exact_in_the_interior_on_a_linear_image(method):
    """G = 40 + 2 x + 4 y, R = G + 30, B = G - 20 (even steps: the rounded means are exact; no clamp acts): both methods reproduce the image at
    every pixel further than 2 from the border (there the reflected samples break the linearity) -- the gradient corrections of MHC vanish on a
    linear G and constant colour differences"""
    W, H = 20, 14
    y, x = np.mgrid[0:H, 0:W]
    G = 40 + 2 * x + 4 * y
    rgb = np.stack([G + 30, G, G - 20], axis=-1)
    assert rgb.min() >= 0 and rgb.max() <= 255
    for pattern in BAYER:
        col = R.colour_map(pattern, W, H)
        mosaic = np.take_along_axis(rgb, col[..., None], axis=-1)[..., 0][None]
        img = R.raw_to_image(mosaic, pattern, 0, 255, (1, 1, 1), method, "rgb")[0]
        assert np.array_equal(img[2:-2, 2:-2], rgb[2:-2, 2:-2]), (pattern, method)


def test_packed_equals_u16():
    rng = np.random.default_rng(2)
    for bits in (10, 12):
        for W in (4, 5, 7, 16, 33):
            s = rng.integers(0, 1 << bits, (2, 3, W))
            p = R.pack(s, bits)
            assert p.shape == (2, 3, (W * bits + 7) // 8) and p.dtype == np.uint8
            assert np.array_equal(R.samples_of(p, "packed", bits, W), s) and np.array_equal(R.samples_of(s.astype(np.uint16), "u16", bits, W), s)
    # GenICam's 12p: two samples in three bytes, the first one's low byte first; 10p: four samples in five bytes
    assert R.pack(np.array([[0xABC, 0x123]]), 12).tolist() == [[0xBC, 0x3A, 0x12]]
    assert R.pack(np.array([[0x3FF, 0, 0x3FF, 0]]), 10).tolist() == [[0xFF, 0x03, 0xF0, 0x3F, 0x00]]


def test_lut_helpers_are_monotone_and_reach_both_ends():
    for lut, ref in ((aefft.gamma_lut(), R.gamma_lut(2.2)), (aefft.gamma_lut(1.0), R.gamma_lut(1.0)), (aefft.srgb_lut(), R.srgb_lut())):
        assert lut.dtype == np.uint8 and lut.shape == (4096,) and np.array_equal(lut, ref)
        assert lut[0] == 0 and lut[4080] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    with pytest.raises(ValueError):
        aefft.gamma_lut(0)


def test_python_argument_checks_need_no_device():
    f = lambda raw, pattern, bits=8, packed=False, black=0, white=None, gains=(1, 1, 1), method="mhc", order="bgr", ccm=None: \
        aefft._raw_source(raw, pattern, bits, packed, black, white, gains, method, order, ccm, "t")
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    i16 = lambda *s: torch.zeros(*s, dtype=torch.int16)
    d, B, W, H, D, _ = f(u8(2, 9, 11), "rggb")
    assert (B, W, H, D) == (2, 11, 9, 3) and (d.pattern, d.container, d.bits, d.pitch, d.stride, d.black, d.white, d.method) == (0, 0, 8, 11, 99, 0, 255, 1)
    d, B, W, H, D, _ = f(i16(9, 11), "mono", bits=12, gains=2.0, method="bilinear")
    assert (B, W, H, D) == (1, 11, 9, 1) and (d.pattern, d.container, d.bits, d.pitch, d.white, d.method) == (4, 1, 12, 22, 4095, 0) and d.gain[0] == 2.0
    d, B, W, H, D, _ = f(u8(2, 9, 17), "bggr", bits=12, packed=True, black=64, white=4000)
    assert (B, W, H, D) == (2, 11, 9, 3) and (d.pattern, d.container, d.bits, d.pitch, d.stride) == (3, 2, 12, 17, 153)
    assert f(u8(9, 7), "grbg", bits=10, packed=True)[2] == 5                                          # 7 bytes hold 5 samples of 10 bits
    big = i16(3, 20, 40)
    d, B, W, H, D, _ = f(big[:, 2:11, 3:14], "gbrg", bits=10, ccm=np.eye(3))                           # a region of interest
    assert (B, W, H) == (3, 11, 9) and (d.pitch, d.stride) == (80, 1600) and d.data == big.data_ptr() + 2 * (2 * 40 + 3) and d.ccm[4] == 1.0
    bad = [dict(raw=u8(9, 11), pattern="rgbg"), dict(raw=u8(9, 11), pattern="rggb", method="vng"), dict(raw=u8(9, 11), pattern="rggb", order="gray"),
           dict(raw=u8(9, 11), pattern="rggb", bits=10), dict(raw=u8(9, 11), pattern="rggb", bits=8, packed=True), dict(raw=i16(9, 11), pattern="rggb", bits=8),
           dict(raw=i16(9, 11), pattern="rggb", bits=12, packed=True), dict(raw=u8(9, 11).float(), pattern="rggb"), dict(raw=u8(2, 2, 9, 11), pattern="rggb"),
           dict(raw=u8(9, 22)[:, ::2], pattern="rggb"), dict(raw=u8(9, 3), pattern="rggb"), dict(raw=u8(3, 11), pattern="rggb"), dict(raw=u8(4, 8193), pattern="mono"),
           dict(raw=u8(9, 11), pattern="rggb", black=255), dict(raw=u8(9, 11), pattern="rggb", white=256), dict(raw=u8(9, 11), pattern="rggb", black=-1),
           dict(raw=u8(9, 11), pattern="rggb", gains=(1, 1)), dict(raw=u8(9, 11), pattern="rggb", gains=(1, 65, 1)), dict(raw=u8(9, 11), pattern="rggb", gains=(1, float("nan"), 1)),
           dict(raw=u8(9, 11), pattern="rggb", ccm=np.ones(8)), dict(raw=u8(9, 11), pattern="rggb", ccm=4 * np.eye(3)), dict(raw=None, pattern="rggb")]
    for kw in bad:
        with pytest.raises(ValueError):
            f(**kw)
