"""aefft_image_resize_to_frames at the boundary (no GPU): declared, exported and prototyped; the two mode values; the argument error that
needs no device; the header's description of the arithmetic; the development-switch, net-option and profiler tables unchanged; every
instantiation of the resize kernel in the back end's resource table (no scratch, no spills), D = 1..4 x {8-bit, float} x {linear, area}; the
Python layout helper."""
import ctypes as C
import inspect
import os
import re

import torch

import abi_checks as A
from abi_checks import CSRC, aefft

NAME = "aefft_image_resize_to_frames"
ARGS = ["aefft_ctx* ctx", "const unsigned char* image_d", "size_t pitch", "size_t image_stride", "int W", "int H", "int mode", "void* frames_d", "int frames_u8",
        "int B", "int D", "int Nx", "int Ny"]


def test_declared_exported_and_prototyped():
    A.check_call(NAME, ARGS)
    # in the image-boundary block: after aefft_frames_to_image, before the network level
    A.in_order(A.header(), "int aefft_frames_to_image(", "enum { AEFFT_RESIZE_LINEAR", "int " + NAME, "/* ---- network level")


def test_mode_values_are_pinned():
    m = re.search(r"enum\s*\{\s*AEFFT_RESIZE_LINEAR\s*=\s*(\d+)\s*,\s*AEFFT_RESIZE_AREA\s*=\s*(\d+)\s*\}", A.header())
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert aefft.RESIZE_MODES == {"linear": 0, "area": 1}


def test_context_method_signature():
    p = inspect.signature(aefft.Context.image_resize_to_frames).parameters
    assert list(p) == ["self", "image", "size", "mode", "out", "dtype"]
    assert p["image"].default is inspect.Parameter.empty and p["size"].default is inspect.Parameter.empty
    assert p["mode"].default == "linear" and p["out"].default is None and p["dtype"].default is torch.uint8


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 512)()
    src, dst = C.cast(buf, C.c_void_p), C.c_void_p(C.addressof(buf) + 256)
    f = L.aefft_image_resize_to_frames
    for mode in (0, 1):
        assert f(None, src, 24, 192, 8, 8, mode, dst, 1, 1, 3, 4, 4) == A.EINVAL
    assert f(None, None, 0, 0, 0, 0, 0, None, 0, 0, 0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(512)


def test_header_describes_the_call():
    doc = A.doc("/* aefft_image_resize_to_frames", "enum { AEFFT_RESIZE_LINEAR")
    for word in ("autoencoder.cpp:124-125", "b * image_stride", "y * pitch + x * D + d", "pitch >= W * D", "image_stride >= (H - 1) * pitch + W * D",
                 "ANY alignment", "region\n * of interest", "image_d + y0 * pitch + x0 * D", "never read", "16-byte aligned", "destination column i, destination row j",
                 "D in 1..4", "1..8192", "all-integer", "half-pixel centres", "edges replicated", "1/2048", "n = (2i+1) S - N", "den = 2N", "s = floor(n / den)",
                 "(4096 r + den) / (2 den)", "halves up", "min(s+1, S-1)", "(2048-wy) ((2048-wx) p[y0][x0] + wx p[y0][x1])", "< 2^30", "(v + 2^21) >> 22",
                 "(v + 32) >> 6", "q < 2^24", "exact box average", "Nx <= W and Ny <= H", "min((i+1) S, (k+1) N) - max(i S, k N)", "64 bits",
                 "(2 num + W H) / (2 W H)", "65536 num", "exactly aefft_image_to_frames' output", "rounded block mean", "NOT promised byte-identical",
                 "INTER_AREA", "never\n * switches modes", "one grey level", "unmeasured", "One launch", "no allocation", "no workspace", "stream capture",
                 "Out-of-place", "AEFFT_EINVAL", "unknown mode", "enlarging axis", "overlap"):
        assert word in doc, word


def test_flag_option_and_profiler_tables_are_unchanged():
    """the call adds no development switch, no net option and no profiling id (it is accounted under `image`)"""
    names = A.tables_unchanged("RESIZE", "IMAGE", profiler=("image_",))[1]
    assert names.count("image") == 1


def test_resize_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/resize_kernels.rsrc: resize_kernel<D, F32, MODE> for D = 1..4 x {8-bit, float} x {linear, area} -- what launch_image_resize's switch
    selects -- nothing else, each with zero scratch and zero spills; the launcher's source names exactly those"""
    [got] = A.instantiations("resize_kernels.rsrc", r"\d+resize_kernelILi(\d)ELb([01])ELi([01])EEE")
    want = {(d, f, m) for d in "1234" for f in "01" for m in "01"}
    assert got == want, sorted(got ^ want)
    src = open(os.path.join(CSRC, "resize_kernels.hip")).read()
    assert re.findall(r"RZ_CASES\((\d)\)", src.split("switch (D * 4")[1]) == ["1", "2", "3", "4"]
    assert "RZ_CASE(DD, 0, 0) RZ_CASE(DD, 0, 1) RZ_CASE(DD, 1, 0) RZ_CASE(DD, 1, 1)" in src
    assert "resize_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # image_kernels.hip is left alone: the resize kernels live in a file of their own
    assert "resize" not in open(os.path.join(CSRC, "image_kernels.hip")).read()


def test_python_layout_rules_need_no_device():
    """Context.image_resize_to_frames accepts padded and region-of-interest views and refuses layouts the C call cannot describe, before
    anything reaches the library"""
    f = aefft._resize_layout
    img = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    v, pitch, stride = f(img, "t")
    assert (tuple(v.shape), pitch, stride) == ((2, 5, 7, 3), 21, 105)
    v, pitch, stride = f(img[0], "t")
    assert (tuple(v.shape), pitch) == ((1, 5, 7, 3), 21) and stride >= 4 * 21 + 21
    padded = torch.zeros(2, 5, 32, dtype=torch.uint8)[:, :, :21].view(2, 5, 7, 3)
    assert f(padded, "t")[1:] == (32, 160)
    big = torch.zeros(3, 20, 30, 3, dtype=torch.uint8)
    roi = big[:, 3:3 + 5, 5:5 + 7]
    v, pitch, stride = f(roi, "t")
    assert (tuple(v.shape), pitch, stride) == ((3, 5, 7, 3), 90, 1800) and stride != 5 * pitch
    assert v.data_ptr() == big.data_ptr() + 3 * 90 + 5 * 3
    assert f(big[::2, 3:8, 5:12], "t")[2] == 3600                              # every other image: still one batch stride
    assert f(torch.zeros(2, 1, 7, 3, dtype=torch.uint8), "t")[1:] == (21, 21)      # H == 1: the pitch is the row itself
    grey = torch.zeros(2, 5, 7, 1, dtype=torch.uint8)
    assert f(grey, "t")[1] == 7
    for bad in (img.float(), img[:, :, :, :2], img[:, :, ::2], img.permute(0, 2, 1, 3), img[0, 0], img.as_strided((2, 5, 7, 3), (10, 21, 3, 1))):
        try:
            f(bad, "t")
        except ValueError:
            continue
        raise AssertionError((tuple(bad.shape), tuple(bad.stride())))
