"""aefft_image_to_frames / aefft_frames_to_image at the boundary (no GPU): declared, exported and prototyped; the two Context methods'
signatures; the argument error that needs no device; the header's description; the development-switch tables unchanged; every
instantiation of the two image kernels in the back end's resource table (no scratch, no spills), D = 1..4 x {8-bit, float}."""
import ctypes as C
import inspect

import torch

import abi_checks as A
from abi_checks import aefft

# name: the argument list of include/aefft.h
CALLS = {
    "aefft_image_to_frames": ["aefft_ctx* ctx", "const unsigned char* image_d", "size_t pitch", "void* frames_d", "int frames_u8", "int B", "int D", "int Nx", "int Ny"],
    "aefft_frames_to_image": ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "unsigned char* image_d", "size_t pitch", "int B", "int D", "int Nx", "int Ny"],
}


def test_declared_exported_and_prototyped():
    for name, args in CALLS.items():
        A.check_call(name, args)
    # the block stands between the spatial ops and the network level
    A.in_order(A.header(), "int aefft_step_spatial(", "/* ---- image boundary", "int aefft_image_to_frames", "/* ---- network level")


def test_context_method_signatures():
    p = inspect.signature(aefft.Context.image_to_frames).parameters
    assert list(p) == ["self", "image", "out", "dtype"]
    assert p["image"].default is inspect.Parameter.empty and p["out"].default is None and p["dtype"].default is torch.uint8
    p = inspect.signature(aefft.Context.frames_to_image).parameters
    assert list(p) == ["self", "frames", "out"]
    assert p["frames"].default is inspect.Parameter.empty and p["out"].default is None


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 256)()
    vp = C.cast(buf, C.c_void_p)
    assert L.aefft_image_to_frames(None, vp, 24, vp, 1, 1, 3, 8, 8) == A.EINVAL
    assert L.aefft_frames_to_image(None, vp, 1, vp, 24, 1, 3, 8, 8) == A.EINVAL
    assert L.aefft_image_to_frames(None, None, 0, None, 0, 0, 0, 0, 0) == A.EINVAL
    assert L.aefft_frames_to_image(None, None, 0, None, 0, 0, 0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(256)


def test_header_describes_the_calls():
    doc = A.doc("/* ---- image boundary", "int aefft_image_to_frames")
    for word in ("j * pitch + i * D + d", "frames[b][d][i][j] = image[b][j][i][d]", "pitch >= Nx * D", "b * Ny * pitch", "never written", "never read",
                 "ImageToSpin_C", "SpinToImage_C", "netlib.cpp:37-51", ":54-77", "Nx = img.cols", "AEFFT_EINVAL", "16-byte aligned", "ANY alignment",
                 "D in 1..4", "1..8192", "halves away from zero", "NaN -> 0", "One launch", "no allocation", "stream capture", "overlap"):
        assert word in doc, word


def test_python_layout_rules_need_no_device():
    """Context.image_to_frames / frames_to_image refuse layouts the C call cannot describe, before anything reaches the library"""
    f = aefft._image_layout
    img = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    assert f(img, "t")[1] == 21 and f(img[0], "t")[0].shape == (1, 5, 7, 3)
    padded = torch.zeros(2, 5, 32, dtype=torch.uint8)[:, :, :21].view(2, 5, 7, 3)
    assert f(padded, "t")[1] == 32
    for bad in (img.float(), img[:, :, :, :2], img[:, :, ::2], img[:, ::2], img.permute(0, 2, 1, 3), img[0, 0]):
        try:
            f(bad, "t")
        except ValueError:
            continue
        raise AssertionError(tuple(bad.shape))


def test_flag_tables_are_unchanged():
    """the calls add no development switch and no net option"""
    A.tables_unchanged("IMAGE", "PITCH")


def test_image_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/image_kernels.rsrc: image_unpack_kernel<D, F32> and image_pack_kernel<D, F32> for D = 1..4 x {8-bit, float}, nothing else, each with
    zero scratch and zero spills"""
    [got] = A.instantiations("image_kernels.rsrc", r"\d+image_(unpack|pack)_kernelILi(\d)ELb([01])EEE")
    assert got == {(k, d, f) for k in ("unpack", "pack") for d in "1234" for f in "01"}, sorted(got)
