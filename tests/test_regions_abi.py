"""aefft_map_regions, aefft_map_regions_workspace and aefft_region_to_pixels at the boundary (no GPU): declared in the image-boundary block behind
aefft_image_compare_map, exported and prototyped; aefft_region's 32 bytes; the header's statement of the definition and the rules; the pinned
tables; the null-context error; the workspace query; the pixel boxes against the ceil formulas; the Python checks on CPU tensors; the kernels'
resource table (no scratch, no spills); the host check program; the restatement of regions_ref.py against scipy.ndimage where scipy is there."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
import regions_ref as R
from abi_checks import CSRC, ROOT, aefft

NAME = "aefft_map_regions"
PROTO = ["aefft_ctx* ctx", "const float* map_d", "const float* ref_d", "int Mx", "int My", "int B", "int sense", "float lo", "float hi", "int connectivity",
         "int min_area", "int* labels_d", "aefft_region* regions_d", "int max_regions", "int* count_d", "void* work_d", "size_t work_bytes"]
PIXELS = ["const aefft_region* r", "int Mx", "int My", "int W", "int H", "int* x0", "int* y0", "int* x1", "int* y1"]
FIELDS = ["i0", "j0", "i1", "j1", "area", "peak_i", "peak_j", "peak"]
# C argument type -> ctypes type: abi_checks.CTYPES and what these calls add (a device pointer travels as void*, a host pointer as what it points to)
CTYPES = dict(A.CTYPES, **{"int*": C.c_void_p, "aefft_region*": C.c_void_p})
HOST = {"const aefft_region*": aefft.Region, "int*": C.c_int}


# 1.
def test_declared_exported_and_prototyped():
    assert A.prototype(NAME) == PROTO and A.prototype("aefft_region_to_pixels") == PIXELS
    assert re.search(r"size_t\s+aefft_map_regions_workspace\s*\(\s*int Mx,\s*int My,\s*int B\s*\)", A.header_code())
    for n in (NAME, "aefft_map_regions_workspace", "aefft_region_to_pixels"):
        assert n in A.exported(), n
    res, argt = aefft.SIGNATURES[NAME]
    assert res is C.c_int and [CTYPES[a.rsplit(" ", 1)[0]] for a in PROTO] == argt
    assert aefft.SIGNATURES["aefft_map_regions_workspace"] == (C.c_size_t, [C.c_int] * 3)
    res, argt = aefft.SIGNATURES["aefft_region_to_pixels"]
    assert res is C.c_int and len(argt) == len(PIXELS)
    for t, a in zip(argt, PIXELS):
        typ = a.rsplit(" ", 1)[0]
        assert (t._type_ is HOST[typ]) if typ in HOST else (t is A.CTYPES[typ]), a
    assert re.search(r"enum\s*\{\s*AEFFT_REGIONS_ABOVE\s*=\s*0,\s*AEFFT_REGIONS_BELOW\s*=\s*1\s*\}", A.header_code())
    assert aefft.REGIONS_SENSE == {"above": 0, "below": 1}
    p = inspect.signature(aefft.Context.map_regions).parameters
    assert list(p) == ["self", "map", "lo", "hi", "ref", "sense", "connectivity", "min_area", "max_regions", "labels", "regions", "count"]
    assert [p[n].default for n in list(p)[3:]] == [None, None, "above", 8, 1, 256, None, None, None]
    p = inspect.signature(aefft.Net.detect_tiled).parameters
    assert list(p)[:8] == ["self", "image", "overlap", "rim", "tile", "metric", "lo", "hi"] and [p[n].default for n in list(p)[3:6]] == [0, 16, "mse"]
    assert list(inspect.signature(aefft.region_pixels).parameters) == ["region", "cells", "W", "H"]


# 2.
def test_the_region_is_32_bytes_without_padding():
    assert A.struct_fields("aefft_region") == ["int i0, j0, i1, j1", "int area", "int peak_i, peak_j", "float peak"]
    assert C.sizeof(aefft.Region) == 32 and [f[0] for f in aefft.Region._fields_] == FIELDS
    assert [getattr(aefft.Region, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert aefft.REGION.itemsize == 32 and list(aefft.REGION.names) == FIELDS and [aefft.REGION.fields[f][1] for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert aefft.REGION == R.REGION and aefft.REGION["peak"] == np.dtype("<f4") and all(aefft.REGION[f] == np.dtype("<i4") for f in FIELDS[:7])
    src = open(os.path.join(CSRC, "regions_kernels.hip")).read()
    assert "static_assert(sizeof(aefft_region) == RG_WORDS * sizeof(int) && sizeof(RgSlot) == 16" in src


# 3.
def test_the_calls_stand_behind_compare_map_in_the_image_boundary_block():
    A.in_order(A.header(), "int aefft_image_compare_map(", "/* aefft_map_regions", "} aefft_region;", "AEFFT_REGIONS_ABOVE = 0", "size_t aefft_map_regions_workspace(",
               "int %s(" % NAME, "int aefft_region_to_pixels(", "/* ---- network level")
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    # (in the host unit the calls stand behind the YUV writers and in front of the compare and tile sections, whose own tests pin those as the last two)
    A.in_order(ops, "// image boundary", 'extern "C" int aefft_frames_resize_to_yuv(', 'extern "C" size_t aefft_map_regions_workspace(', 'extern "C" int %s(' % NAME,
               'extern "C" int aefft_region_to_pixels(', 'extern "C" int aefft_image_compare_map(')
    entry = ops[ops.index('extern "C" int %s(' % NAME):ops.index('extern "C" int aefft_region_to_pixels(')]
    assert "ranges_overlap(" in entry and entry.count("aligned16(") == 6 and "join_recon(ctx)" in entry and entry.count("KID_IMAGE") == 1
    assert "hipMalloc" not in entry and "Synchronize" not in entry and "ws_get" not in entry                  # the caller's workspace, no waiting
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_map_regions" not in rest and "aefft_region" not in rest


# 4.
def test_header_states_the_definition_and_the_rules():
    doc = A.doc("/* aefft_map_regions", "typedef struct {\n    int i0, j0, i1, j1;", margin=False)
    for word in ("float [B][Mx][My]", "My contiguous", "the layout the map calls write and the overlay reads", "per-cell baseline [Mx][My] shared by the batch", "or NULL",
                 "int [B][Mx][My]", "aefft_region [B][max_regions]", "NULL exactly when max_regions == 0", "int [B]", "aefft_map_regions_workspace(Mx, My, B)",
                 "16 a cell", "Mx, My in 1..1024", "B >= 1", "B * Mx * My <= 2^31 - 1", "min_area >= 1", "max_regions in 0..65536", "every pointer 16-byte aligned",
                 "disjoint from the inputs and from each other", "lo and hi finite", "linear index is I * My + J",
                 "v = map[b][I][J] when ref_d is NULL", "v = map[b][I][J] - ref[I][J], rounded once to float32", "A -0 result counts as +0",
                 "AEFFT_REGIONS_ABOVE requires lo <= hi", "foreground when v >= lo and strong when v >= hi", "AEFFT_REGIONS_BELOW", "requires hi <= lo",
                 "foreground when v <= lo and strong when v <= hi", "NaN is background", "every comparison with it is false", "+inf and -inf are ordinary values",
                 "maximal connected sets of foreground cells of one image", "4- or 8-connectivity", "no wrap-around", "nothing connects across images",
                 "at least one strong cell and area >= min_area", "hi == lo means a plain threshold",
                 "numbered 1..n in ascending order of their smallest linear index I * My + J", "background cells and cells of dropped components get 0",
                 "count[b] = n, also when n > max_regions", "regions[b * max_regions + r - 1] is written for r <= min(n, max_regions)",
                 "the maximal v under ABOVE, the minimal v under BELOW", "at the smallest linear index that attains it", "min(n, max_regions) on are left untouched",
                 "aefft_image_compare_map's cell rule", "x0 = ceil(i0 W / Mx)", "x1 = ceil((i1+1) W / Mx)", "y0 = ceil(j0 H / My)", "y1 = ceil((j1+1) H / My)",
                 "the full grid gives (0, 0, W, H)", "0 <= i0 <= i1 < Mx", "0 <= j0 <= j1 < My", "W, H in 1..8192", "1 <= Mx <= min(W, 1024)",
                 "Six launches on the context's stream", "tiled union-find", "atomicMin", "integer add / min / max", "one 64-bit max", "no host synchronisation",
                 "no allocation", "the caller supplies the workspace", "safe under stream capture", "no workgroup waits for another",
                 "a function of the inputs alone, on every run", "profile id `image`", "B Mx My (4 + 4 + 16) + 32 B max_regions bytes",
                 "AEFFT_EINVAL", '"aefft_map_regions: "', "naming the rule", "nothing enqueued", "every output untouched", "a null pointer", "a size out of range",
                 "an unknown sense or connectivity", "non-finite or in the wrong order for the sense", "misalignment", "overlap", "work_bytes below the query",
                 "regions_d and max_regions disagreeing", "B * Mx * My beyond an int"):
        assert word in doc, word


# 5.
def test_no_new_switch_option_or_profiling_id():
    flags, names = A.tables_unchanged("REGION", "LABEL", profiler=("region", "label"))
    assert "image" in names
    assert not [k for k in aefft.FLAGS if "REGION" in k]


# 6.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 8192)(*([0x5A] * 8192))
    base = C.addressof(buf)
    base += -base % 16
    m, lab, reg, cnt, work = (C.c_void_p(base + k * 1024) for k in range(5))
    assert L.aefft_map_regions_workspace(4, 3, 2) == 16 * 24
    for sense, lo, hi in ((0, 0.5, 0.75), (1, 0.5, 0.25)):
        assert L.aefft_map_regions(None, m, None, 4, 3, 2, sense, lo, hi, 8, 1, lab, reg, 4, cnt, work, 16 * 24) == aefft.EINVAL
    assert L.aefft_map_regions(None, None, None, 0, 0, 0, 0, 0.0, 0.0, 0, 0, None, None, 0, None, None, 0) == aefft.EINVAL
    assert bytes(buf) == bytes([0x5A] * 8192)


# 7.
def test_the_workspace_query():
    L = A.lib()
    for Mx, My, B in ((1, 1, 1), (40, 30, 32), (240, 135, 8), (1024, 1024, 1), (1024, 1024, 2047), (1, 1, 2 ** 31 - 1), (17, 3, 5)):
        w = L.aefft_map_regions_workspace(Mx, My, B)
        assert 0 < w <= 16 * B * Mx * My and w % 16 == 0, (Mx, My, B)
    for Mx, My, B in ((0, 3, 1), (3, 0, 1), (3, 3, 0), (1025, 3, 1), (3, 1025, 1), (-1, 3, 1), (3, 3, -1), (1024, 1024, 2048), (2, 1, 2 ** 30)):
        assert L.aefft_map_regions_workspace(Mx, My, B) == 0, (Mx, My, B)


# 8.
def test_region_to_pixels_is_the_ceil_formulas():
    L = A.lib()
    ceil = lambda a, b: -(-a // b)
    box = [C.c_int(-7) for _ in range(4)]
    refs = [C.byref(v) for v in box]
    n = 0
    assert 13 % 4 and 130 % 9 and 1030 % 1024 and 1080 % 68                     # (sizes that are no multiple of the grid among them)
    for Mx, My, W, H in ((4, 3, 13, 9), (9, 5, 130, 70), (120, 68, 1920, 1080), (1, 1, 1, 1), (1024, 1024, 8192, 8192), (7, 7, 7, 7), (1024, 3, 1030, 8192)):
        r = aefft.Region(0, 0, Mx - 1, My - 1, Mx * My, 0, 0, 1.0)
        assert L.aefft_region_to_pixels(C.byref(r), Mx, My, W, H, *refs) == aefft.OK and [v.value for v in box] == [0, 0, W, H]      # the full grid
        assert aefft.region_pixels(r, (Mx, My), W, H) == (0, 0, W, H)
        rng = np.random.default_rng(Mx + W)
        for _ in range(40):
            i0, i1 = sorted(rng.integers(0, Mx, 2).tolist())
            j0, j1 = sorted(rng.integers(0, My, 2).tolist())
            r = aefft.Region(i0, j0, i1, j1, 1, i0, j0, 0.0)
            assert L.aefft_region_to_pixels(C.byref(r), Mx, My, W, H, *refs) == aefft.OK
            want = (ceil(i0 * W, Mx), ceil(j0 * H, My), ceil((i1 + 1) * W, Mx), ceil((j1 + 1) * H, My))
            assert tuple(v.value for v in box) == want == R.to_pixels(dict(i0=i0, j0=j0, i1=i1, j1=j1), Mx, My, W, H)
            # the box is the union of compare_map's cells: pixel x lies in it exactly when floor(x Mx / W) is in i0..i1
            if W <= 2048:
                x = np.arange(W)
                assert np.array_equal((x >= want[0]) & (x < want[2]), (x * Mx // W >= i0) & (x * Mx // W <= i1))
            n += 1
    assert n == 280
    good = dict(i0=1, j0=1, i1=2, j1=1, Mx=4, My=3, W=13, H=9)
    for kw in (dict(i0=-1), dict(i0=3), dict(i1=4), dict(j0=2), dict(j1=3), dict(j0=-1), dict(Mx=0), dict(My=0), dict(Mx=14), dict(My=10), dict(W=0), dict(H=0),
               dict(W=8193), dict(H=8193), dict(Mx=1025, W=2000)):
        v = dict(good, **kw)
        for b in box:
            b.value = -7
        r = aefft.Region(v["i0"], v["j0"], v["i1"], v["j1"], 1, 0, 0, 0.0)
        assert L.aefft_region_to_pixels(C.byref(r), v["Mx"], v["My"], v["W"], v["H"], *refs) == aefft.EINVAL, kw
        assert [b.value for b in box] == [-7] * 4
        with pytest.raises(ValueError):
            aefft.region_pixels(r, (v["Mx"], v["My"]), v["W"], v["H"])
    r = aefft.Region(1, 1, 2, 1, 1, 0, 0, 0.0)
    assert L.aefft_region_to_pixels(None, 4, 3, 13, 9, *refs) == aefft.EINVAL and L.aefft_region_to_pixels(C.byref(r), 4, 3, 13, 9, refs[0], None, refs[2], refs[3]) == aefft.EINVAL


# 9.
def test_python_checks_need_no_device():
    """the checks of Context.map_regions run before anything reaches the device: CPU tensors suffice"""
    args = aefft._map_regions_args
    m = torch.zeros(2, 5, 7)
    good = dict(map=m, lo=0.5, hi=None, ref=None, sense="above", connectivity=8, min_area=1, max_regions=256, labels=None, regions=None, count=None)
    mm, lo, hi, s, conn, area, mr = args(**good)
    assert (tuple(mm.shape), lo, hi, s, conn, area, mr) == ((2, 5, 7), 0.5, 0.5, 0, 8, 1, 256)
    assert tuple(args(**dict(good, map=m[0], sense="below", lo=0.5, hi=0.25, connectivity=4))[0].shape) == (1, 5, 7)
    args(**dict(good, ref=torch.zeros(5, 7), labels=torch.zeros(2, 5, 7, dtype=torch.int32), regions=torch.zeros(2, 256, 8, dtype=torch.int32), count=torch.zeros(2, dtype=torch.int32)))
    for bad in (dict(map=m.double()), dict(map=m.permute(0, 2, 1)), dict(map=torch.zeros(7)), dict(map=torch.zeros(1, 1025, 2)), dict(sense="up"), dict(sense=0),
                dict(connectivity=6), dict(connectivity=True), dict(lo=0.8, hi=0.5), dict(sense="below", hi=0.8), dict(lo=float("nan")), dict(hi=float("inf")),
                dict(lo=1e39), dict(lo="high"), dict(min_area=0), dict(max_regions=-1), dict(max_regions=65537), dict(ref=torch.zeros(7, 5)), dict(ref=torch.zeros(2, 5, 7)),
                dict(labels=torch.zeros(2, 5, 7)), dict(labels=torch.zeros(2, 7, 5, dtype=torch.int32)), dict(regions=torch.zeros(2, 256, 8)),
                dict(regions=torch.zeros(2, 255, 8, dtype=torch.int32)), dict(regions=torch.zeros(2, 0, 8, dtype=torch.int32), max_regions=0),
                dict(count=torch.zeros(3, dtype=torch.int32)), dict(count=torch.zeros(2))):
        with pytest.raises(ValueError):
            args(**dict(good, **bad))


# 10.
def test_regions_kernels_use_no_scratch_and_are_the_six():
    """build/regions_kernels.rsrc: the six kernels the launcher enqueues, nothing else, each with zero scratch and zero spills"""
    names = ("tile", "border", "flatten", "count", "rank", "final")
    got = A.instantiations("regions_kernels.rsrc", *[r"\d+(regions_%s_kernel)ENS_6RgArgsE" % n for n in names])
    assert got == [{("regions_%s_kernel" % n,)} for n in names]
    src = open(os.path.join(CSRC, "regions_kernels.hip")).read()
    launcher = src[src.index("hipError_t launch_map_regions("):]
    assert re.findall(r"regions_(\w+)_kernel<<<", launcher) == list(names)
    assert "regions_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    internal = open(os.path.join(CSRC, "internal.h")).read()
    assert "hipError_t launch_map_regions(" in internal and "size_t map_regions_workspace(" in internal
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h"}
    # order-independent atomics only: integer min / max / add / or and the 64-bit max; no float atomic, no compare-and-swap on the device side, no
    # cooperative launch, no spinning on a flag
    device = src[:src.index("#else\nRG_HD int rg_ld(")] + src[src.index("RG_HD int rg_clz(unsigned v) { return __builtin_clz(v); }"):]
    code = re.sub(r"//[^\n]*", "", device)                                       # (without the comments)
    assert set(re.findall(r"\batomic(\w+)\(", code)) == {"Min", "Max", "Add", "Or"}
    assert "atomicCAS" not in code and "atomicExch" not in code and "cooperative" not in code and "while" not in code
    # the only unbounded-looking loops are find and union, whose bounds the header comment states; the others count up to a constant or a size
    assert code.count("for (;;)") == 2 and "Termination:" in src and "Determinism:" in src and "strictly decreasing" in src


# 11.
def test_the_host_check_program_is_there_and_stands_alone():
    src = A.host_check_stands_alone("regions_hostcheck.cpp", "regions_kernels.hip")
    for body in ("tile", "border", "flatten", "count", "rank", "final"):
        assert "regions_%s_body(" % body in src, body
    assert "hipcc" not in src and "LD_PRELOAD" not in src
    assert os.path.exists(os.path.join(ROOT, "tools", "regions_bench.py"))
    kernel = open(os.path.join(CSRC, "regions_kernels.hip")).read()
    assert "#ifndef AEFFT_HOSTCHECK" in kernel and "__atomic_compare_exchange_n" in kernel and "__atomic_fetch_add" in kernel
    # the product never imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "regions_ref" not in open(os.path.join(dirpath, f)).read(), f


# 12.
def test_the_restatement_on_small_cases_by_hand():
    """maps small enough to label by eye: the numbering skips dropped components, the peak tie goes to the smallest index, -0 is +0"""
    m = np.array([[[0.9, 0.0, 0.6, 0.0, 0.8],
                   [0.0, 0.0, 0.0, 0.0, 0.8],
                   [0.6, 0.6, 0.0, 0.7, 0.0]]], np.float32)
    lab, reg, cnt = R.regions(m, 0.5, 0.75, connectivity=4, max_regions=4)
    assert lab.tolist() == [[[1, 0, 0, 0, 2], [0, 0, 0, 0, 2], [0, 0, 0, 0, 0]]] and cnt.tolist() == [2]
    assert reg[0, 0].tolist() == (0, 0, 0, 0, 1, 0, 0, np.float32(0.9)) and reg[0, 1].tolist() == (0, 4, 1, 4, 2, 0, 4, np.float32(0.8))
    assert reg[0, 2].tolist() == (0, 0, 0, 0, 0, 0, 0, 0.0)
    lab8, reg8, cnt8 = R.regions(m, 0.5, 0.75, connectivity=8, max_regions=1, fill=np.full((1, 1, 8), 7, np.int32).view(R.REGION)[..., 0])
    assert lab8.tolist() == [[[1, 0, 0, 0, 2], [0, 0, 0, 0, 2], [0, 0, 0, 2, 0]]] and cnt8.tolist() == [2] and reg8[0, 0]["area"] == 1
    lab, reg, cnt = R.regions(m, 0.5, connectivity=4, min_area=2, max_regions=4)
    assert lab.tolist() == [[[0, 0, 0, 0, 1], [0, 0, 0, 0, 1], [2, 2, 0, 0, 0]]] and reg[0, 1].tolist() == (2, 0, 2, 1, 2, 2, 0, np.float32(0.6))
    lab, reg, cnt = R.regions(1 - m, 0.5, 0.25, sense="below", connectivity=4, max_regions=4)
    assert cnt.tolist() == [2] and reg[0, 1]["peak"] == np.float32(1) - np.float32(0.8) and (reg[0, 1]["peak_i"], reg[0, 1]["peak_j"]) == (0, 4)
    z = np.array([[[-0.0, 0.0], [np.nan, -np.inf]]], np.float32)
    lab, reg, cnt = R.regions(z, 0.0, connectivity=4, max_regions=2)
    assert lab.tolist() == [[[1, 1], [0, 0]]] and reg[0, 0]["peak"].view(np.uint32) == 0 and (reg[0, 0]["peak_i"], reg[0, 0]["peak_j"]) == (0, 0)
    lab, reg, cnt = R.regions(z, 0.0, ref=np.array([[0.0, 0.0], [0.0, -np.inf]], np.float32), sense="below", connectivity=8, max_regions=2)
    assert lab.tolist() == [[[1, 1], [0, 0]]]                                     # (-inf) - (-inf) is NaN: background


# 13.
def test_the_restatement_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(29)
    for (Mx, My), kind in (((33, 15), "random30"), ((50, 67), "random50"), ((50, 67), "random60"), ((33, 15), "spiral"), ((17, 17), "checker"), ((40, 30), "bars")):
        for conn in (4, 8):
            mask = R.pattern(kind, Mx, My, rng)
            m = np.where(mask, 0.5 + rng.integers(0, 16, mask.shape) / 32.0, 0.25).astype(np.float32)[None]
            lab, reg, cnt = R.regions(m, 0.5, connectivity=conn, max_regions=2048)
            slab, n = ndimage.label(mask, structure=np.ones((3, 3)) if conn == 8 else None)      # scipy numbers in scan order too
            assert n == cnt[0] and np.array_equal(slab, lab[0]), (kind, conn)
            for k, sl in enumerate(ndimage.find_objects(slab)):
                r = reg[0, k]
                assert (r["i0"], r["i1"] + 1, r["j0"], r["j1"] + 1) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
                assert r["area"] == (slab == k + 1).sum() and r["peak"] == m[0][slab == k + 1].max() and m[0, r["peak_i"], r["peak_j"]] == r["peak"]
            # hysteresis: the kept components are scipy's components that hold a strong cell, renumbered in order
            lab, reg, cnt = R.regions(m, 0.5, 0.75, connectivity=conn, min_area=2, max_regions=2048)
            keep = [k for k in range(1, n + 1) if (m[0][slab == k] >= 0.75).any() and (slab == k).sum() >= 2]
            renum = np.zeros(n + 1, np.int32)
            renum[keep] = np.arange(1, len(keep) + 1)
            assert cnt[0] == len(keep) and np.array_equal(renum[slab], lab[0]), (kind, conn)
