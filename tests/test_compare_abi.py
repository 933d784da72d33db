"""aefft_image_compare_map at the boundary (no GPU): declared in the image-boundary block behind aefft_frames_resize_to_yuv, exported and
prototyped; the header's statement of the formulas and rules; the pinned tables; the null-context error; the Python layout rules on CPU tensors;
the properties of the definition on the numpy restatement of compare_ref.py (the cells partition the axis and are the overlay's, the integer
SSIM against the textbook formula, identical images, symmetry, the factors' width); every instantiation of the kernels in the back end's
resource table (no scratch, no spills); the host check program."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_checks as A
import compare_ref as R
from abi_checks import CSRC, ROOT, aefft

NAME = "aefft_image_compare_map"
PROTO = ["aefft_ctx* ctx", "const unsigned char* a_d", "size_t a_pitch", "size_t a_stride", "const unsigned char* b_d", "size_t b_pitch", "size_t b_stride",
         "int W", "int H", "int B", "int D", "int metric", "int Mx", "int My", "float* map_d", "float* score_d"]
WIDTHS = list(range(1, 41)) + [130, 641, 1080, 1920]


# 1.
def test_declared_exported_and_prototyped():
    A.check_call(NAME, PROTO)
    assert re.search(r"enum\s*\{\s*AEFFT_COMPARE_MSE\s*=\s*0,\s*AEFFT_COMPARE_SSIM\s*=\s*1\s*\}", A.header_code())
    assert aefft.COMPARE_METRICS == {"mse": 0, "ssim": 1}
    p = inspect.signature(aefft.Context.image_compare_map).parameters
    assert list(p) == ["self", "a", "b", "cells", "metric", "map", "score"] and [p[n].default for n in list(p)[4:]] == ["mse", None, None]
    p = inspect.signature(aefft.Net.score_tiled).parameters
    assert list(p) == ["self", "image", "overlap", "rim", "tile", "metric", "target", "map", "score", "out"]
    assert [p[n].default for n in list(p)[3:]] == [0, 16, "mse", None, None, None, None]
    assert list(inspect.signature(aefft.cells_for_tile).parameters) == ["W", "H", "tile"]


# 2.
def test_the_call_stands_behind_the_yuv_writers_in_the_image_boundary_block():
    A.in_order(A.header(), "int aefft_frames_resize_to_yuv(", "/* aefft_image_compare_map", "AEFFT_COMPARE_MSE = 0", "int %s(" % NAME, "/* ---- network level")
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    A.in_order(ops, "// image boundary", 'extern "C" int aefft_frames_resize_to_yuv(', 'extern "C" int %s(' % NAME, 'extern "C" int aefft_tile_plan_make(')
    entry = ops[ops.index('extern "C" int %s(' % NAME):ops.index('extern "C" int aefft_tile_plan_make(')]
    assert "ranges_overlap(" in entry and "aligned16(" in entry and "chk_rows(" in entry and "IMAGE_WORDS" in entry and entry.count("KID_IMAGE") == 2
    assert ops.count("static bool ranges_overlap(") == 1 and ops.count("static int chk_rows(") == 1 and ops.count("RowWords IMAGE_WORDS") == 1
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_image_" not in rest and "KID_IMAGE" not in rest


# 3.
def test_header_states_the_formulas_and_the_rules():
    doc = A.doc("/* aefft_image_compare_map", "enum { AEFFT_COMPARE_MSE", margin=False)
    for word in ("y * pitch + x * D + d", "any alignment", "pitch >= W * D", "stride >= (H - 1) * pitch + W * D", "ignored when B == 1", "never read",
                 "its own pitch and stride", "a_d == b_d", "any overlap of the two are allowed", "float [B][Mx][My]", "My contiguous", "16-byte aligned",
                 "aefft_net_score_map writes", "aefft_map_overlay_image reads", "float [B]", "or NULL",
                 "I = floor(x Mx / W)", "J = floor(y My / H)", "step 3 of aefft_map_overlay_image read backwards", "smooth = 0 colours exactly the pixels",
                 "[ceil(I W / Mx), ceil((I+1) W / Mx))", "floor(W / Mx) or ceil(W / Mx)", "with W = t Mx the cells are the t x t tiles",
                 "W, H in 1..8192", "D in 1..4", "B >= 1", "1 <= Mx <= min(W, 1024)", "1 <= My <= min(H, 1024)", "ceil(W / Mx) <= 64", "ceil(H / My) <= 64",
                 "n = nx_I ny_J <= 4096", "B * My <= 2^31 - 1", "B * My beyond an int", "numpy gives the same bits",
                 "e = sum over d < D and the cell's pixels of (x - r)^2", "< 2^31", "map = (float)((double)e / (double)(D n))",
                 "data range 255", "C1 = 6.5025", "C2 = 58.5225", "uniform weights", "population statistics", "aefft_net_ssim_map cleared of its denominators",
                 "Sx, Sr, Sxx, Srr, Sxr", "K1 = 65025", "K2 = 585225", "A1 = 20000 Sx Sr + K1 n^2", "A2 = 20000 (n Sxr - Sx Sr) + K2 n^2", "may be negative",
                 "B1 = 10000 (Sx^2 + Sr^2) + K1 n^2", "B2 = 10000 (n Sxx - Sx^2 + n Srr - Sr^2) + K2 n^2", "exact in signed 64 bits", "B1, B2 > 0",
                 "ssim_d = ((double)A1 * (double)A2) / ((double)B1 * (double)B2)", "four conversions", "round to nearest even", "two products", "one division",
                 "FMA", "map = (float)((ssim_0 + ... + ssim_{D-1}) / (double)D)", "ascending d",
                 "Identical images give exactly 0.0f (MSE) and exactly 1.0f (SSIM)", "swapping a and b gives the same bits",
                 "map AS STORED", "pixel-weighted mean", "r_I = ((m[I][0] n_I0 + m[I][1] n_I1) + ...)", "ascending J", "S = ((r_0 + r_1) + ...)", "ascending I",
                 "score[b] = (float)(S / (double)(W H))", "exact in double", "PSNR = 10 log10(255^2 / score)",
                 "One launch on the context's stream, two with score_d", "reads the map back", "no host synchronisation", "no allocation", "no workspace",
                 "no global atomics", "owned by one workgroup", "stream capture", "profile id `image`", "2 B W H D + 4 B Mx My bytes",
                 "AEFFT_EINVAL", '"aefft_image_compare_map: "', "naming the rule", "nothing enqueued", "both outputs untouched", "a null context, source or map",
                 "a size, D, B, Mx or My out of range", "a cell side above 64", "an unknown metric", "a pitch or stride that is too small",
                 "map_d or score_d not 16-byte aligned", "map_d or score_d overlapping either image or each other", "overflow the address space"):
        assert word in doc, word


# 4.
def test_no_new_switch_option_or_profiling_id():
    flags, names = A.tables_unchanged("COMPARE", "CMP", profiler=("compare", "cmp"))
    assert "image" in names
    assert not [k for k in aefft.FLAGS if "COMPARE" in k]


# 5.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 4096)(*([0x5A] * 4096))
    base = C.addressof(buf)
    base += -base % 16
    a, b, m, s = (C.c_void_p(base + k * 1024) for k in range(4))
    for metric in (0, 1):
        assert L.aefft_image_compare_map(None, a, 39, 0, b, 39, 0, 13, 9, 1, 3, metric, 4, 3, m, s) == aefft.EINVAL
    assert L.aefft_image_compare_map(None, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None) == aefft.EINVAL
    assert bytes(buf) == bytes([0x5A] * 4096)


# 6.
def test_python_layout_rules_need_no_device():
    """the checks of Context.image_compare_map run before anything reaches the device: CPU tensors suffice"""
    args = aefft._image_compare_args
    a = torch.zeros(2, 9, 13, 3, dtype=torch.uint8)
    ia, pa, sa, ib, pb, sb, cells, m = args(a, a, (4, 3), "mse", None, None)
    assert (pa, sa, pb, sb, cells, m) == (39, 9 * 39, 39, 9 * 39, (4, 3), 0) and ia.data_ptr() == ib.data_ptr()
    big = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    roi = big[:, 3:12, 5:18]                                                               # a region of interest against a tight image: each its own pitch
    ia, pa, sa, ib, pb, sb, cells, m = args(roi, a, (13, 9), "ssim", torch.zeros(2, 13, 9), torch.zeros(2))
    assert (pa, sa, pb, sb, cells, m) == (90, 20 * 90, 39, 9 * 39, (13, 9), 1) and ia.data_ptr() == big.data_ptr() + 3 * 90 + 15
    assert tuple(args(a[0], roi[1], (1, 1), "mse", None, False)[0].shape) == (1, 9, 13, 3)
    good = dict(a=a, b=a, cells=(4, 3), metric="mse", map=None, score=None)
    for bad in (dict(a=a.float()), dict(b=a[0]), dict(b=a[:, :, :12]), dict(a=a.permute(0, 2, 1, 3), b=a.permute(0, 2, 1, 3)), dict(a=a[0, 0], b=a[0, 0]),
                dict(a=torch.zeros(1, 4, 4, 5, dtype=torch.uint8), b=torch.zeros(1, 4, 4, 5, dtype=torch.uint8)), dict(cells=4), dict(cells=(0, 3)), dict(cells=(14, 3)),
                dict(cells=(4, 10)), dict(cells=(4, 3, 1)), dict(metric="psnr"), dict(metric=0), dict(map=torch.zeros(2, 3, 4)), dict(map=torch.zeros(2, 4, 3, dtype=torch.float64)),
                dict(map=torch.zeros(2, 3, 4).permute(0, 2, 1)), dict(score=torch.zeros(3)), dict(score=torch.zeros(2, dtype=torch.float64)),
                dict(a=torch.zeros(1, 9, 130, 3, dtype=torch.uint8), b=torch.zeros(1, 9, 130, 3, dtype=torch.uint8), cells=(2, 3))):      # cells of 65 columns
        with pytest.raises(ValueError):
            args(**dict(good, **bad))
    assert aefft.cells_for_tile(1920, 1080, 16) == (120, 68) and aefft.cells_for_tile(130, 70, (16, 35)) == (9, 2) and aefft.cells_for_tile(5, 5, 1) == (5, 5)
    assert aefft.cells_for_tile(8192, 1, 64) == (128, 1)
    for bad in (0, 65, (16, 0), 1.5, True, "16", (16,)):
        with pytest.raises(ValueError):
            aefft.cells_for_tile(130, 70, bad)
    with pytest.raises(ValueError):
        aefft.cells_for_tile(0, 70, 16)


# 7.
def test_the_cells_partition_the_axis_and_are_the_overlays():
    n = 0
    for W in WIDTHS:
        for Mx in range(1, min(W, 1024) + 1):
            e = np.array(R.edges(W, Mx))
            assert e[0] == 0 and e[-1] == W and (np.diff(e) >= 1).all()
            assert set(np.diff(e).tolist()) <= {W // Mx, -(-W // Mx)}
            assert np.array_equal(np.repeat(np.arange(Mx), np.diff(e)), np.arange(W) * Mx // W), (W, Mx)      # floor(x Mx / W): the overlay's step 3
            n += 1
    assert n == sum(min(W, 1024) for W in WIDTHS)
    assert R.edges(64, 4) == [0, 16, 32, 48, 64]                                           # W = t Mx: the t x t tiles


# 8.
def test_the_integer_ssim_is_the_textbook_formula():
    rng = np.random.default_rng(17)
    worst = 0.0
    for k in range(300):
        ny, nx = rng.integers(1, 65, 2)
        x = rng.integers(0, 256, (ny, nx), dtype=np.uint8)
        r = [rng.integers(0, 256, (ny, nx), dtype=np.uint8), (x.astype(int) + rng.integers(-6, 7, (ny, nx))).clip(0, 255).astype(np.uint8), 255 - x,
             np.full_like(x, rng.integers(0, 256))][k % 4]
        worst = max(worst, abs(float(R.ssim_channel(x, r)) - float(R.ssim_textbook(x, r))))
    print("largest difference between the integer form and the float64 formula:", worst)
    assert worst <= 1e-12


# 9.
def test_identical_images_symmetry_and_the_width_of_the_factors():
    rng = np.random.default_rng(23)
    a = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    for cells in ((4, 3), (13, 9), (1, 1)):
        m, s = R.compare(a, a, cells, "mse")
        assert (m.view(np.uint32) == 0).all() and (s.view(np.uint32) == 0).all()           # exactly +0.0
        m, s = R.compare(a, a, cells, "ssim")
        assert (m == np.float32(1.0)).all() and (s == np.float32(1.0)).all()
        for metric in ("mse", "ssim"):
            (m1, s1), (m2, s2) = R.compare(a, b, cells, metric), R.compare(b, a, cells, metric)
            assert np.array_equal(m1.view(np.uint32), m2.view(np.uint32)) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    # the vectorised route of the restatement (many cells) gives the bits of the cell-by-cell route (Python integers)
    big_a, big_b = rng.integers(0, 256, (2, 35, 67, 3), dtype=np.uint8), rng.integers(0, 256, (2, 35, 67, 3), dtype=np.uint8)
    ex, ey = R.edges(67, 9), R.edges(35, 5)
    for metric in ("mse", "ssim"):
        fast = R.compare_map(big_a, big_b, (9, 5), metric)
        slow = np.array([[[R.cell(big_a[k, ey[J]:ey[J + 1], ex[I]:ex[I + 1]], big_b[k, ey[J]:ey[J + 1], ex[I]:ex[I + 1]], metric) for J in range(5)]
                          for I in range(9)] for k in range(2)], np.float32)
        assert np.array_equal(fast.view(np.uint32), slow.view(np.uint32))
    # the extreme cells at n = 4096: all four factors stay below 2^63, B1 and B2 positive
    zero, full = np.zeros((64, 64), np.int64), np.full((64, 64), 255, np.int64)
    alt = (np.indices((64, 64)).sum(axis=0) % 2) * 255
    for x, r in ((zero, full), (full, zero), (full, full), (alt, 255 - alt), (alt, alt), (zero, zero)):
        f = R.ssim_factors(4096, x.sum(), r.sum(), (x * x).sum(), (r * r).sum(), (x * r).sum())
        assert all(isinstance(v, int) for v in f) and max(abs(v) for v in f) < 2 ** 63 and f[2] > 0 and f[3] > 0, f
    assert 4 * 4096 * 65025 < 2 ** 31 and 4096 * 65025 < 2 ** 32                         # e, and a cell's word of any moment
    assert float(R.ssim_channel(alt.astype(np.uint8), (255 - alt).astype(np.uint8))) < 0    # (A2 may be negative)
    # the score is the pixel-weighted mean of the stored map
    m = R.compare_map(a, b, (4, 3), "mse")
    nx, ny = np.diff(R.edges(13, 4)), np.diff(R.edges(9, 3))
    assert np.allclose(R.score(m, 13, 9), (m.astype(np.float64) * np.outer(nx, ny)).sum(axis=(1, 2)) / (13 * 9), rtol=1e-6)
    d = a.astype(np.float64) - b.astype(np.float64)
    assert np.allclose(R.score(m, 13, 9), (d * d).mean(axis=(1, 2, 3)), rtol=1e-5)


# 10.
def test_compare_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/compare_kernels.rsrc: compare_map_kernel<D, METRIC> for D = 1..4 x {MSE, SSIM} -- what the launcher selects (the dword and byte routes
    are chosen inside a kernel) -- and compare_score_kernel, nothing else, each with zero scratch and zero spills"""
    maps, score = A.instantiations("compare_kernels.rsrc", r"\d+compare_map_kernelILi(\d)ELi([01])EEE", r"\d+(compare_score_kernel)E")
    assert maps == {(d, m) for d in "1234" for m in "01"} and score == {("compare_score_kernel",)}
    src = open(os.path.join(CSRC, "compare_kernels.hip")).read()
    launcher = src[src.index("hipError_t launch_compare_map("):src.index("hipError_t launch_compare_score(")]
    assert set(re.findall(r"compare_map_kernel<(\d), CM_(MSE|SSIM)>", launcher)) == {(d, m) for d in "1234" for m in ("MSE", "SSIM")}
    assert "compare_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    internal = open(os.path.join(CSRC, "internal.h")).read()
    assert "hipError_t launch_compare_map(" in internal and "hipError_t launch_compare_score(" in internal
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h", "fft_common.h"}
    assert "atomicAdd" not in src and "__atomic" not in src                              # (no atomics at all: the sums meet in LDS behind barriers)


# 11.
def test_the_host_check_program_is_there_and_stands_alone():
    A.host_check_stands_alone("compare_hostcheck.cpp", "compare_kernels.hip")
    assert os.path.exists(os.path.join(ROOT, "tools", "compare_bench.py"))
    # the product never imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "compare_ref" not in open(os.path.join(dirpath, f)).read(), f
