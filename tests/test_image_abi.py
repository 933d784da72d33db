"""aefft_image_to_frames / aefft_frames_to_image at the boundary (no GPU): declared, exported and prototyped; the two Context methods'
signatures; the argument error that needs no device; the header's description; the development-switch tables unchanged; every
instantiation of the two image kernels in the back end's resource table (no scratch, no spills), D = 1..4 x {8-bit, float}."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
aefft = importlib.import_module("autoencoder-fft_amd")
NFLAGS = 26      # AEFFT_F_* switches of the library

# name: the argument list of include/aefft.h, by leading type
CALLS = {
    "aefft_image_to_frames": ["aefft_ctx*", "const unsigned char*", "size_t", "void*", "int", "int", "int", "int", "int"],
    "aefft_frames_to_image": ["aefft_ctx*", "const void*", "int", "unsigned char*", "size_t", "int", "int", "int", "int"],
}
CTYPES = {"aefft_ctx*": C.c_void_p, "const unsigned char*": C.c_void_p, "unsigned char*": C.c_void_p, "void*": C.c_void_p, "const void*": C.c_void_p,
          "size_t": C.c_size_t, "int": C.c_int}


def _header():
    return open(os.path.join(ROOT, "include", "aefft.h")).read()


def _lib():
    if not os.path.exists(aefft.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return aefft.lib()


def test_declared_exported_and_prototyped():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", aefft.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, want in CALLS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, f"include/aefft.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(want), (name, args)
        for a, w in zip(args, want):
            assert a.startswith(w + " "), (name, a, w)
        assert [a.split()[-1] for a in args][-4:] == ["B", "D", "Nx", "Ny"]
        assert any(l.split()[-1] == name and " T " in l for l in out.splitlines()), name
        res, argt = aefft.SIGNATURES[name]
        assert res is C.c_int and len(argt) == len(want)
        for t, w in zip(argt, want):
            assert t is CTYPES[w], (name, w)
    # the block stands between the spatial ops and the network level
    h = _header()
    assert h.index("int aefft_step_spatial(") < h.index("/* ---- image boundary") < h.index("int aefft_image_to_frames") < h.index("/* ---- network level")


def test_context_method_signatures():
    p = inspect.signature(aefft.Context.image_to_frames).parameters
    assert list(p) == ["self", "image", "out", "dtype"]
    assert p["image"].default is inspect.Parameter.empty and p["out"].default is None and p["dtype"].default is torch.uint8
    p = inspect.signature(aefft.Context.frames_to_image).parameters
    assert list(p) == ["self", "frames", "out"]
    assert p["frames"].default is inspect.Parameter.empty and p["out"].default is None


def test_null_context_is_einval_without_a_device():
    L = _lib()
    buf = (C.c_ubyte * 256)()
    einval = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", _header()).group(1))
    vp = C.cast(buf, C.c_void_p)
    assert L.aefft_image_to_frames(None, vp, 24, vp, 1, 1, 3, 8, 8) == einval
    assert L.aefft_frames_to_image(None, vp, 1, vp, 24, 1, 3, 8, 8) == einval
    assert L.aefft_image_to_frames(None, None, 0, None, 0, 0, 0, 0, 0) == einval
    assert L.aefft_frames_to_image(None, None, 0, None, 0, 0, 0, 0, 0) == einval
    assert bytes(buf) == bytes(256)


def test_header_describes_the_calls():
    h = _header()
    doc = h[h.index("/* ---- image boundary"):h.index("int aefft_image_to_frames")]
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
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", _header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if "IMAGE" in n or "PITCH" in n]
    opts = re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", _header())
    assert opts == ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]


def test_image_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/image_kernels.rsrc: image_unpack_kernel<D, F32> and image_pack_kernel<D, F32> for D = 1..4 x {8-bit, float}, nothing else, each with
    zero scratch and zero spills"""
    _lib()
    path = os.path.join(ROOT, "autoencoder-fft_amd", "csrc", "build", "image_kernels.rsrc")
    assert os.path.exists(path), f"{path}: the build writes the back end's resource table beside every object (csrc/Makefile)"
    got = set()
    for b in re.split(r"(?=remark: [^\n]*Function Name: )", open(path).read()):
        m = re.search(r"Function Name: (\S+)", b)
        if not m:
            continue
        k = re.search(r"\d+image_(unpack|pack)_kernelILi(\d)ELb([01])EEE", m.group(1))
        assert k, m.group(1)
        got.add((k.group(1), int(k.group(2)), k.group(3) == "1"))
        for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
            v = re.search(key + r": (\d+)", b)
            assert v and int(v.group(1)) == 0, (m.group(1), key)
    assert got == {(k, d, f) for k in ("unpack", "pack") for d in (1, 2, 3, 4) for f in (False, True)}, sorted(got)
