"""aefft_frames_resize_to_image and aefft_map_overlay_image at the boundary (no GPU): declared in the image-boundary block, exported and
prototyped; the Context methods and heat_lut; the argument error that needs no device; the header's statement of the rules; every
instantiation of the two kernels in the back end's resource table (no scratch, no spills); the tap formulas stated once; the Python layout
rules."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
from abi_checks import CSRC, ROOT, aefft

CALLS = {
    "aefft_frames_resize_to_image": ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "int Nx", "int Ny", "int mode", "unsigned char* image_d", "size_t pitch",
                                     "size_t image_stride", "int W", "int H", "int B", "int D"],
    "aefft_map_overlay_image": ["aefft_ctx* ctx", "const float* map_d", "int Mx", "int My", "float lo", "float hi", "int smooth", "const unsigned char* lut_d", "int alpha",
                                "unsigned char* image_d", "size_t pitch", "size_t image_stride", "int W", "int H", "int B", "int D"],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_prototyped(name):
    A.check_call(name, CALLS[name])


def test_both_calls_stand_in_the_image_boundary_block():
    A.in_order(A.header(), "int aefft_image_resize_to_frames(", "int aefft_frames_resize_to_image(", "int aefft_map_overlay_image(", "/* ---- network level")
    # the mode enum and its text are where and what they were
    assert A.header().count("enum { AEFFT_RESIZE_LINEAR = 0, AEFFT_RESIZE_AREA = 1 };") == 1 and aefft.RESIZE_MODES == {"linear": 0, "area": 1}


def test_context_methods_and_heat_lut():
    p = inspect.signature(aefft.Context.frames_resize_to_image).parameters
    assert list(p) == ["self", "frames", "size", "mode", "out"]
    assert p["frames"].default is inspect.Parameter.empty and p["size"].default is inspect.Parameter.empty
    assert p["mode"].default == "linear" and p["out"].default is None
    p = inspect.signature(aefft.Context.map_overlay).parameters
    assert list(p) == ["self", "map", "image", "lut", "lo", "hi", "alpha", "smooth"]
    assert all(p[n].default is inspect.Parameter.empty for n in ("map", "image", "lut", "lo", "hi"))
    assert p["alpha"].default == 128 and p["smooth"].default is True
    assert inspect.signature(aefft.heat_lut).parameters["D"].default == 3
    for D in (1, 2, 3, 4):
        t = aefft.heat_lut(D)
        assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and t.shape == (256, D) and t.flags["C_CONTIGUOUS"]
    assert aefft.heat_lut().shape == (256, 3)
    t = aefft.heat_lut(3)                                   # BGR: blue at 0, red at 255
    assert tuple(t[0]) == (255, 0, 0) and tuple(t[255]) == (0, 0, 255) and t[128, 1] > 250
    assert (np.diff(t[:, 2].astype(int)) == 1).all() and (np.diff(t[:, 0].astype(int)) == -1).all()
    assert np.array_equal(aefft.heat_lut(1)[:, 0], np.arange(256))
    t4 = aefft.heat_lut(4)
    assert np.array_equal(t4[:, :3], t) and (t4[:, 3] == 255).all()
    with pytest.raises(ValueError):
        aefft.heat_lut(5)


def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 2048)()
    base = C.addressof(buf)
    base += -base % 16
    frames, image, lut = C.c_void_p(base), C.c_void_p(base + 256), C.c_void_p(base + 1024)
    for mode in (0, 1):
        assert L.aefft_frames_resize_to_image(None, frames, 1, 4, 4, mode, image, 12, 48, 4, 4, 1, 3) == A.EINVAL
    assert L.aefft_frames_resize_to_image(None, None, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, 0) == A.EINVAL
    assert L.aefft_map_overlay_image(None, frames, 2, 2, 0.0, 1.0, 1, lut, 128, image, 12, 48, 4, 4, 1, 3) == A.EINVAL
    assert L.aefft_map_overlay_image(None, None, 0, 0, 0.0, 0.0, 0, None, 0, None, 0, 0, 0, 0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(2048)


def test_header_states_the_rules():
    one = A.doc("/* aefft_frames_resize_to_image", "int aefft_frames_resize_to_image(")
    for word in ("mirror of aefft_image_resize_to_frames", "autoencoder.cpp:217-223", "16-byte aligned", "p[y][x] = frames[b][d][x][y]", "px_u8(frames[b][d][x][y])",
                 "clamp((int)round(v), 0, 255)", "halves away from zero", "NaN -> 0", "first turned into pixels, then resized", "b * image_stride",
                 "y * pitch + x * D + d", "pitch >= W * D", "image_stride >= (H - 1) * pitch + W * D", "ANY alignment", "never written", "region of interest",
                 "D in 1..4", "1..8192", "all-integer", "roles swapped", "always 8-bit", "(v + 2^21) >> 22", "floor((2 num + Nx Ny) / (2 Nx Ny))",
                 "W <= Nx and H <= Ny", "exactly aefft_frames_to_image's bytes", "composition of three existing calls", "bit for bit",
                 "no intermediate image", "unmeasured", "One launch", "no allocation", "no workspace", "stream capture", "Out-of-place", "AEFFT_EINVAL",
                 '"aefft_frames_resize_to_image: "', "unknown mode", "enlarging axis", "overlap", "overflow the address space"):
        assert word in one, word
    two = A.doc("/* aefft_map_overlay_image", "int aefft_map_overlay_image(")
    for word in ("in place", "[B][Mx][My]", "16-byte aligned", "Mx along image columns", "My contiguous", "1..1024", "256 * D bytes", "k * D + d", "any alignment",
                 "ships no colour map", "alpha in 0..256", "hi < lo inverts the scale", "inv = 255.0f / (hi - lo)", "px_u8((map[b][I][J] - lo) * inv)",
                 "each rounded to float32", "NaN -> 0", "halves away from zero", "k0[floor(x Mx / W)][floor(y My / H)]", "AEFFT_RESIZE_LINEAR taps",
                 "k = (v + 2^21) >> 22", "(alpha * lut[k][d] + (256 - alpha) * image[y][x][d] + 128) >> 8", "alpha = 0 leaves every byte as it was",
                 "alpha = 256 writes the table's colour exactly", "neither read nor written", "One launch", "no allocation", "stream capture",
                 "profile id `image`", "AEFFT_EINVAL", '"aefft_map_overlay_image: "', "non-finite or equal", "overlapping the image range"):
        assert word in two, word


def test_present_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/present_kernels.rsrc: frames_resize_kernel<D, F32, MODE> for D = 1..4 x {8-bit, float} x {linear, area} and map_overlay_kernel<D> for
    D = 1..4 -- what the two launchers select -- nothing else, each with zero scratch and zero spills"""
    resize, overlay = A.instantiations("present_kernels.rsrc", r"\d+frames_resize_kernelILi(\d)ELb([01])ELi([01])EEE", r"\d+map_overlay_kernelILi(\d)EEE")
    assert resize == {(d, f, m) for d in "1234" for f in "01" for m in "01"}
    assert overlay == {(d,) for d in "1234"}
    assert "present_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_older_kernel_files_keep_their_kernels_and_the_taps_are_stated_once():
    got = {re.search(r"aefft\d+(\w+?_kernel)I", fn).group(1) for fn in A.rsrc("resize_kernels.rsrc")}
    assert got == {"resize_kernel"} and len(A.rsrc("resize_kernels.rsrc")) == 16
    got = {re.search(r"aefft\d+(\w+?_kernel)I", fn).group(1) for fn in A.rsrc("image_kernels.rsrc")}
    assert got == {"image_unpack_kernel", "image_pack_kernel"}
    # one definition of the tap formulas, in the header both kernel files include
    defs = {}
    for fn in os.listdir(CSRC):
        if fn.endswith((".hip", ".h", ".cpp")):
            src = open(os.path.join(CSRC, fn)).read()
            if re.search(r"RzTap\s+rz_tap\s*\(int mode", src):
                defs[fn] = src
    assert list(defs) == ["resize_taps.h"]
    for fn in ("resize_kernels.hip", "present_kernels.hip"):
        assert '#include "resize_taps.h"' in open(os.path.join(CSRC, fn)).read()
    assert "4096 * (n - s * den) + den" not in open(os.path.join(CSRC, "present_kernels.hip")).read()
    # one statement of what the tile bodies do with the taps -- AREA's vertical weight in the band sums, AREA's rounding of float frames, the
    # correction loop of pr_div_u8 -- in the header all four kernel files that resize through a staged band include
    srcs = {fn: open(os.path.join(CSRC, fn)).read() for fn in os.listdir(CSRC) if fn.endswith((".hip", ".h", ".cpp"))}
    for text in ("rz_weight(Y[k], y,", "65536ull * num", "while ((unsigned long long)q * den > n) --q;"):
        assert [fn for fn in srcs if text in srcs[fn]] == ["resize_tile.h"], text
    assert len(re.findall(r"unsigned\s+pr_div_u8\s*\(", srcs["resize_tile.h"])) == 1 and "fy_div_u8" not in "".join(srcs.values())
    for fn in ("resize_kernels.hip", "yuv_kernels.hip", "present_kernels.hip", "yuv_out_kernels.hip"):
        assert '#include "resize_tile.h"' in srcs[fn], fn
    for tool in ("resize_hostcheck.cpp", "present_hostcheck.cpp"):
        assert os.path.exists(os.path.join(ROOT, "tools", tool))
        assert '#include "hostlanes.h"' in open(os.path.join(ROOT, "tools", tool)).read()


def test_python_layout_rules_need_no_device():
    """the checks of Context.frames_resize_to_image and Context.map_overlay run before anything reaches the library: CPU tensors suffice"""
    fr, ov = aefft._frames_resize_args, aefft._overlay_args
    frames = torch.zeros(2, 3, 8, 6, dtype=torch.uint8)
    assert fr(frames, (11, 9), "linear", None) == (11, 9, 0) and fr(frames.float(), (4, 3), "area", None) == (4, 3, 1)
    assert fr(frames, (11, 9), "linear", torch.zeros(2, 9, 11, 3, dtype=torch.uint8)) == (11, 9, 0)
    for bad in (dict(frames=frames.double()), dict(frames=frames[0]), dict(frames=frames.permute(0, 1, 3, 2)), dict(mode="cubic"), dict(size=(11,)), dict(size=(0, 9)),
                dict(size=7), dict(out=torch.zeros(2, 11, 9, 3, dtype=torch.uint8)), dict(out=torch.zeros(9, 11, 3, dtype=torch.uint8))):
        kw = dict(frames=frames, size=(11, 9), mode="linear", out=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            fr(**kw)
    # the destination goes through the same layout helper as the source of image_resize_to_frames
    big = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    roi = big[:, 3:12, 5:16]
    v, pitch, stride = aefft._resize_layout(roi, "t")
    assert (tuple(v.shape), pitch, stride) == ((2, 9, 11, 3), 90, 1800)
    for out in (roi.permute(0, 2, 1, 3), big[:, 3:12, 5:27:2], roi.float()):
        with pytest.raises(ValueError):
            aefft._resize_layout(out, "t")
    # map_overlay
    img = torch.zeros(2, 9, 11, 3, dtype=torch.uint8)
    lut = torch.as_tensor(aefft.heat_lut(3))
    m, v, pitch, stride = ov(torch.zeros(2, 4, 5), img, lut, 0.0, 1.0, 128)
    assert (tuple(m.shape), tuple(v.shape), pitch, stride) == ((2, 4, 5), (2, 9, 11, 3), 33, 297)
    m, v, pitch, stride = ov(torch.zeros(4, 5), img[0], lut, 1.0, 0.0, 256)
    assert (tuple(m.shape), tuple(v.shape), pitch) == ((1, 4, 5), (1, 9, 11, 3), 33)
    good = dict(map=torch.zeros(2, 4, 5), image=img, lut=lut, lo=0.0, hi=1.0, alpha=128)
    for bad in (dict(map=torch.zeros(3, 4, 5)), dict(map=torch.zeros(2, 4, 5, dtype=torch.float64)), dict(map=torch.zeros(2, 5, 4).permute(0, 2, 1)),
                dict(map=torch.zeros(2, 1, 4, 5)), dict(image=img.permute(0, 2, 1, 3)), dict(image=img.float()), dict(lut=torch.as_tensor(aefft.heat_lut(4))),
                dict(lut=lut.float()), dict(lut=lut[:128]), dict(lo=1.0), dict(hi=float("nan")), dict(lo=float("inf")), dict(alpha=257), dict(alpha=-1),
                dict(alpha=0.5)):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            ov(**kw)
