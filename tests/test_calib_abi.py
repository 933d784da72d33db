"""aefft_map_stats_bytes, aefft_map_stats_update, aefft_map_stats_merge, aefft_map_stats_finish and aefft_map_peak at the boundary (no GPU): declared in
the image-boundary block behind aefft_raw_to_image, exported and prototyped; the header's statement of the layout, the empty state and every rule; the
pinned tables; the bytes query; the null-context error; the Python checks on CPU tensors; the kernels' resource table (no scratch, no spills); the
host check program, built and run in its quick form; the restatement of calib_ref.py on cells small enough to do on paper."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks as A
import calib_ref as R
from abi_checks import CSRC, ROOT, aefft

UPDATE = ["aefft_ctx* ctx", "const float* map_d", "int Mx", "int My", "int B", "void* stats_d", "size_t stats_bytes"]
MERGE = ["aefft_ctx* ctx", "void* dst_d", "const void* src_d", "int Mx", "int My", "size_t stats_bytes"]
FINISH = ["aefft_ctx* ctx", "const void* stats_d", "size_t stats_bytes", "int Mx", "int My", "int mode", "int sense", "float k", "int rank", "float empty", "float* ref_d"]
PEAK = ["aefft_ctx* ctx", "const float* map_d", "const float* ref_d", "int Mx", "int My", "int B", "int sense", "float* peak_d", "int* cell_d"]
CALLS = {"aefft_map_stats_update": UPDATE, "aefft_map_stats_merge": MERGE, "aefft_map_stats_finish": FINISH, "aefft_map_peak": PEAK}
KERNELS = ("update", "merge", "finish", "peak")


# 1.
def test_declared_exported_and_prototyped(monkeypatch):
    monkeypatch.setitem(A.CTYPES, "int*", C.c_void_p)                            # (a device pointer travels as void*)
    for name, args in CALLS.items():
        A.check_call(name, args)
    assert re.search(r"size_t\s+aefft_map_stats_bytes\s*\(\s*int Mx,\s*int My\s*\)", A.header_code()) and "aefft_map_stats_bytes" in A.exported()
    assert aefft.SIGNATURES["aefft_map_stats_bytes"] == (C.c_size_t, [C.c_int] * 2)
    assert re.search(r"enum\s*\{\s*AEFFT_CALIB_SIGMA\s*=\s*0,\s*AEFFT_CALIB_RANK\s*=\s*1\s*\}", A.header_code())
    assert aefft.CALIB_MODE == {"sigma": 0, "rank": 1} == R.MODES and aefft.REGIONS_SENSE == R.SENSES
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(aefft.Context.map_stats)) == ["self", "Mx", "My"] and list(sig(aefft.Context.map_stats_update)) == ["self", "state", "map"]
    assert list(sig(aefft.Context.map_stats_merge))[:3] == ["self", "dst", "src"]
    p = sig(aefft.Context.map_stats_finish)
    assert list(p) == ["self", "state", "cells", "mode", "sense", "k", "rank", "empty", "ref"]
    assert [p[n].default for n in list(p)[3:]] == ["rank", "above", 3.0, 1, float("inf"), None]
    p = sig(aefft.Context.map_peak)
    assert list(p) == ["self", "map", "ref", "sense", "peak", "cell"] and [p[n].default for n in list(p)[2:]] == [None, "above", None, None]
    p = sig(aefft.Net.calibrate_tiled)
    assert list(p) == ["self", "image", "overlap", "rim", "tile", "metric", "state", "target"] and [p[n].default for n in list(p)[3:]] == [0, 16, "mse", None, None]
    assert list(sig(aefft.map_stats_view)) == ["state", "Mx", "My"]


# 2.
def test_the_calls_stand_behind_raw_to_image_and_in_the_gap_of_the_host_unit():
    A.in_order(A.header(), "int aefft_raw_to_image(", "/* aefft_map_stats_update", "AEFFT_CALIB_SIGMA = 0", "size_t aefft_map_stats_bytes(", "int aefft_map_stats_update(",
               "int aefft_map_stats_merge(", "int aefft_map_stats_finish(", "int aefft_map_peak(", "/* ---- network level")
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    A.in_order(ops, 'extern "C" int aefft_region_to_pixels(', "// calibration", 'extern "C" size_t aefft_map_stats_bytes(', 'extern "C" int aefft_map_stats_update(',
               'extern "C" int aefft_map_stats_merge(', 'extern "C" int aefft_map_stats_finish(', 'extern "C" int aefft_map_peak(', "// raw sensor data")
    section = ops[ops.index("// calibration"):ops.index("// raw sensor data")]
    assert section.count("KID_IMAGE") == 4 and section.count("join_recon(ctx)") == 4 and section.count("launch_or_fail(") == 4 and section.count("ranges_overlap(") >= 7
    assert section.count("const Bad bad{ctx,") == 4 and "aligned16(" in section
    assert "hipMalloc" not in section and "Synchronize" not in section and "ws_get" not in section and "hipMemset" not in section
    for helper in ("struct Bad {", "static bool ranges_overlap("):
        assert ops.count(helper) == 1, helper
    host = open(os.path.join(CSRC, "host.h")).read()
    assert host.count("inline bool aligned16(") == 1 and host.count("int join_recon(") == 1 and host.count("int launch_or_fail(") == 1
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_map_stats" not in rest and "aefft_map_peak" not in rest


# 3.
def test_header_states_the_layout_the_empty_state_and_the_rules():
    doc = A.doc("/* aefft_map_stats_update", "enum { AEFFT_CALIB_SIGMA", margin=False)
    for word in ("float [B][Mx][My]", "My contiguous", "linear index I * My + J", "n = Mx * My", "Mx, My in 1..1024", "B >= 1", "B * Mx * My <= 2^31 - 1",
                 "every pointer 16-byte aligned", "caller-owned device memory", "aefft_map_stats_bytes(Mx, My) bytes", "52 * Mx * My rounded up to a multiple of 16",
                 "planar", "[0, 8n) double S1[n]", "[8n, 16n) double S2[n]", "[16n, 32n) float hi[4][n]", "hi[0] the largest", "[32n, 48n) float lo[4][n]",
                 "lo[0] the smallest", "[48n, 52n) int c[n]", "All-zero bytes are the empty state", "no reset call", "hipMemsetAsync",
                 "Only the first min(c, 4) slots of hi and lo are live", "the others hold +0.0f", "a function of the multiset of values alone", "c <= 2^31 - 1",
                 "for b = 0 .. B-1 in ascending order", "A non-finite x (NaN, +inf, -inf) is skipped and not counted", "-0 counts as +0", "S1 = S1 + (double)x",
                 "S2 = S2 + (double)x * (double)x", "c = c + 1", "among the four largest seen so far", "among the four smallest", "Multiplicity is kept",
                 "The product of two floats is exact in double", "do not depend on whether the product is fused into the addition", "in place",
                 "S1 = S1_dst + S1_src", "one addition each", "c = c_dst + c_src", "the four largest of the up to eight live values", "dead slots end up +0.0f",
                 "src is only read", "dst and src must not overlap", "float [Mx][My], exactly what aefft_map_regions takes", "a cell with c == 0 gets `empty`",
                 "+inf under ABOVE switches the cell off", "AEFFT_CALIB_RANK", "rank in 1..4", "r = min(rank, c)", "ref = hi[r-1] under AEFFT_REGIONS_ABOVE",
                 "lo[r-1] under AEFFT_REGIONS_BELOW", "rank - 1 outliers tolerated", "No arithmetic", "independent of the order the footage arrived in",
                 "AEFFT_CALIB_SIGMA", "k is a finite float, negative for BELOW", "sense and rank are ignored but must be valid values", "each operation rounded once",
                 "mean = S1 / (double)c", "If c == 1, sd = 0", "p = S1 * mean", "d = S2 - p", "d = d < 0 ? 0 : d", "var = d / (double)(c - 1)", "sd = sqrt(var), correctly rounded",
                 "t = (double)k * sd", "ref = (float)(mean + t)", "neither is fused", "log2(mean^2 / var) of double's 53 bits", "not a general-purpose variance",
                 "exactly aefft_map_regions' step 1", "rounded once to float32", "a -0 result counts as +0", "the maximal v under AEFFT_REGIONS_ABOVE",
                 "the minimal v under AEFFT_REGIONS_BELOW", "the cells whose v is not NaN", "the smallest linear index I * My + J that attains it",
                 "the quiet NaN 0x7FC00000", "cell = -1", "float [B]", "int [B]", "One launch each", "the order of the sums is the definition", "No atomics", "no workspace",
                 "no host synchronisation", "no allocation", "safe under stream capture", "a function of the inputs alone", "up to 240 x 135", "profile id `image`",
                 "4 B n + 104 n bytes (update)", "156 n (merge)", "56 n (finish)", "4 B n (+ 4 n with ref_d) + 8 B (peak)", "AEFFT_EINVAL", '"aefft_map_stats_update: "',
                 '"aefft_map_stats_merge: "', '"aefft_map_stats_finish: "', '"aefft_map_peak: "', "naming the rule", "nothing enqueued", "every output and the state untouched",
                 "ref_d of aefft_map_peak may be NULL", "Mx, My outside 1..1024", "B < 1", "beyond an int", "not 16-byte aligned", "stats_bytes below the query",
                 "an unknown mode or sense", "rank outside 1..4", "a non-finite k", "outputs that overlap inputs or each other"):
        assert word in doc, word
    kern = open(os.path.join(CSRC, "calib_kernels.hip")).read()
    assert "(double)x * (double)x is exact" in kern and "asm(\"\" : \"+v\"(v))" in kern and "__builtin_fma(-s, s, x)" in kern


# 4.
def test_no_new_switch_option_or_profiling_id():
    flags, names = A.tables_unchanged("CALIB", "STATS", "PEAK", profiler=("calib", "stats", "peak"))
    assert names.count("image") == 1
    assert not [k for k in aefft.FLAGS if "CALIB" in k or "STATS" in k]


# 5.
def test_the_bytes_query():
    L = A.lib()
    assert L.aefft_map_stats_bytes(1, 1) == 64 and L.aefft_map_stats_bytes(40, 30) == 62400 and L.aefft_map_stats_bytes(1024, 1024) == 52 * 1024 * 1024
    for Mx, My in ((1, 1), (1, 7), (15, 17), (16, 16), (1, 257), (3, 1024), (240, 135), (1024, 1024), (1, 3), (5, 1)):
        got = L.aefft_map_stats_bytes(Mx, My)
        assert got == (52 * Mx * My + 15) // 16 * 16 == aefft.map_stats_bytes(Mx, My) == R.stats_bytes(Mx, My) and got % 16 == 0, (Mx, My)
    for Mx, My in ((0, 3), (3, 0), (1025, 3), (3, 1025), (-1, 3), (3, -1), (0, 0), (2 ** 31 - 1, 1)):
        assert L.aefft_map_stats_bytes(Mx, My) == 0 == aefft.map_stats_bytes(Mx, My) == R.stats_bytes(Mx, My), (Mx, My)


# 6.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 8192)(*([0x5A] * 8192))
    base = C.addressof(buf)
    base += -base % 16
    m, st, st2, ref, pk, cl = (C.c_void_p(base + k * 1024) for k in range(6))
    need = L.aefft_map_stats_bytes(4, 3)
    assert need == 624
    assert L.aefft_map_stats_update(None, m, 4, 3, 2, st, need) == aefft.EINVAL
    assert L.aefft_map_stats_merge(None, st, st2, 4, 3, need) == aefft.EINVAL
    for mode in (0, 1):
        assert L.aefft_map_stats_finish(None, st, need, 4, 3, mode, 0, 3.0, 1, 0.0, ref) == aefft.EINVAL
    for r in (None, ref):
        assert L.aefft_map_peak(None, m, r, 4, 3, 2, 0, pk, cl) == aefft.EINVAL
    assert L.aefft_map_stats_update(None, None, 0, 0, 0, None, 0) == aefft.EINVAL and L.aefft_map_peak(None, None, None, 0, 0, 0, 0, None, None) == aefft.EINVAL
    assert bytes(buf) == bytes([0x5A] * 8192)


# 7.
def test_python_checks_need_no_device():
    """the checks of the five wrappers run before anything reaches the device: CPU tensors suffice"""
    m = torch.zeros(2, 5, 7)
    st = torch.zeros(aefft.map_stats_bytes(5, 7), dtype=torch.uint8)
    assert st.numel() == 1824
    assert tuple(aefft._map_stats_update_args(st, m).shape) == (2, 5, 7) and tuple(aefft._map_stats_update_args(st, m[0]).shape) == (1, 5, 7)
    for bad in (dict(map=m.double()), dict(map=m.permute(0, 2, 1)), dict(map=torch.zeros(7)), dict(map=torch.zeros(1, 1025, 2)), dict(state=st[:-16]),
                dict(state=st.float()), dict(state=st.view(2, -1)), dict(state=torch.zeros(2 * st.numel(), dtype=torch.uint8)[::2]), dict(state=None)):
        with pytest.raises(ValueError):
            aefft._map_stats_update_args(**dict(dict(state=st, map=m), **bad))
    # merge: the grid comes with the call or from what Context.map_stats noted on a state
    st2 = st.clone()
    assert aefft._map_stats_merge_args(st, st2, (5, 7)) == (5, 7)
    st2.cells = (5, 7)
    assert aefft._map_stats_merge_args(st, st2, None) == (5, 7)
    for bad in (dict(src=st.clone()), dict(src=st), dict(cells=(7, 6)), dict(cells=5), dict(cells=(0, 7)), dict(dst=st[:-16]), dict(src=st2.float())):
        with pytest.raises(ValueError):
            aefft._map_stats_merge_args(**dict(dict(dst=st, src=st2, cells=None), **bad))
    good = dict(state=st, cells=(5, 7), mode="rank", sense="above", k=3.0, rank=1, empty=float("inf"), ref=None)
    assert aefft._map_stats_finish_args(**good) == (5, 7, 1, 0, 3.0, 1, float("inf"))
    assert aefft._map_stats_finish_args(**dict(good, mode="sigma", sense="below", k=-2.5, rank=4, empty=0, ref=torch.zeros(5, 7))) == (5, 7, 0, 1, -2.5, 4, 0.0)
    for bad in (dict(mode="mean"), dict(mode=1), dict(sense="up"), dict(k=float("nan")), dict(k=float("inf")), dict(k=1e39), dict(k="three"), dict(rank=0), dict(rank=5),
                dict(rank=1.5), dict(rank=True), dict(empty="none"), dict(cells=(7, 6)), dict(cells=(5, 7, 1)), dict(ref=torch.zeros(7, 5)), dict(ref=torch.zeros(5, 7).double()),
                dict(state=st[:-16])):
        with pytest.raises(ValueError):
            aefft._map_stats_finish_args(**dict(good, **bad))
    good = dict(map=m, ref=None, sense="above", peak=None, cell=None)
    mm, s = aefft._map_peak_args(**good)
    assert tuple(mm.shape) == (2, 5, 7) and s == 0
    assert aefft._map_peak_args(**dict(good, map=m[0], ref=torch.zeros(5, 7), sense="below", peak=torch.zeros(1), cell=torch.zeros(1, dtype=torch.int32)))[1] == 1
    for bad in (dict(map=m.double()), dict(map=torch.zeros(7)), dict(sense="up"), dict(ref=torch.zeros(7, 5)), dict(ref=torch.zeros(2, 5, 7)), dict(peak=torch.zeros(3)),
                dict(peak=torch.zeros(2).double()), dict(cell=torch.zeros(2)), dict(cell=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            aefft._map_peak_args(**dict(good, **bad))
    # the views are the planes of the layout
    raw = torch.arange(st.numel(), dtype=torch.int64).to(torch.uint8)
    S1, S2, hi, lo, c = aefft.map_stats_view(raw, 5, 7)
    n = 35
    assert (S1.dtype, S2.dtype, hi.dtype, lo.dtype, c.dtype) == (torch.float64, torch.float64, torch.float32, torch.float32, torch.int32)
    assert (tuple(S1.shape), tuple(S2.shape), tuple(hi.shape), tuple(lo.shape), tuple(c.shape)) == ((5, 7), (5, 7), (4, 5, 7), (4, 5, 7), (5, 7))
    off = [(t.data_ptr() - raw.data_ptr()) for t in (S1, S2, hi, lo, c)]
    assert off == [0, 8 * n, 16 * n, 32 * n, 48 * n]
    got = R.from_bytes(raw.numpy(), 5, 7)
    assert np.array_equal(hi.numpy().reshape(4, n).view(np.uint32), got["hi"].view(np.uint32)) and np.array_equal(c.numpy().reshape(n), got["c"])
    with pytest.raises(ValueError):
        aefft.map_stats_view(raw[:-16], 5, 7)


# 8.
def test_calib_kernels_use_no_scratch_and_are_the_four():
    """build/calib_kernels.rsrc: the four kernels the launchers enqueue, nothing else, each with zero scratch and zero spills"""
    got = A.instantiations("calib_kernels.rsrc", *[r"\d+(calib_%s_kernel)ENS_6CbArgsE" % n for n in KERNELS])
    assert got == [{("calib_%s_kernel" % n,)} for n in KERNELS]
    for name, (_, ints) in A.rsrc("calib_kernels.rsrc").items():
        assert ints["VGPRs"] <= 64, (name, ints)                                 # (eight waves a SIMD)
    src = open(os.path.join(CSRC, "calib_kernels.hip")).read()
    assert re.findall(r"calib_(\w+)_kernel<<<", src) == list(KERNELS)
    assert "calib_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read().split("SRCS =")[1].split("\n")[0]
    internal = open(os.path.join(CSRC, "internal.h")).read()
    for fn in ("size_t map_stats_bytes(", "hipError_t launch_map_stats_update(", "hipError_t launch_map_stats_merge(", "hipError_t launch_map_stats_finish(", "hipError_t launch_map_peak("):
        assert fn in internal, fn
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h"}
    code = re.sub(r"//[^\n]*", "", src)                                          # (without the comments)
    assert "atomic" not in code and "while" not in code and "cooperative" not in code and "hipMalloc" not in code and "Synchronize" not in code


# 9.
def test_host_check_builds_and_its_quick_form_passes(tmp_path):
    """tools/calib_hostcheck.cpp: the kernel file compiled for the host under -fsanitize=address,undefined, a program of its own (never loaded into
    Python), against its own scalar C restatement; the quick form is the grids around one workgroup, the full sweep is run by hand"""
    src = A.host_check_stands_alone("calib_hostcheck.cpp", "calib_kernels.hip")
    for body in KERNELS:
        assert re.search(r"calib_%s_body(<HOST_LANES>)?\(" % body, src), body
    assert "hipcc" not in src and "LD_PRELOAD" not in src and "int main(int argc" in src and "cb_sqrt_fix(" in src
    assert os.path.exists(os.path.join(ROOT, "tools", "calib_bench.py"))
    assert "#ifndef AEFFT_HOSTCHECK" in open(os.path.join(CSRC, "calib_kernels.hip")).read()
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):  # the product never imports the restatement
        for f in files:
            if f.endswith(".py"):
                assert "calib_ref" not in open(os.path.join(dirpath, f)).read(), f
    exe = str(tmp_path / "calib_hostcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(ROOT, "tools", "calib_hostcheck.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    print(r.stdout[-500:])
    assert r.returncode == 0 and re.search(r"all \d+ runs exact", r.stdout), (r.stdout[-2000:], r.stderr[-2000:])


# 10.
def test_the_restatement_on_cells_by_hand():
    """four cells small enough to do on paper: the values {3, 1, 2, 2, 5, 4}, one value only, NaN only, -0"""
    nan, f32 = np.nan, np.float32
    frames = np.array([[3, 7, nan, -0.0], [1, nan, nan, nan], [2, np.inf, nan, nan], [2, -np.inf, np.inf, nan], [5, nan, -np.inf, nan], [4, nan, nan, nan]], f32).reshape(6, 1, 4)
    st = R.update(R.empty(1, 4), frames)
    assert st["c"].tolist() == [6, 1, 0, 1] and st["S1"].tolist() == [17.0, 7.0, 0.0, 0.0] and st["S2"].tolist() == [59.0, 49.0, 0.0, 0.0]
    assert st["hi"].T.tolist() == [[5, 4, 3, 2], [7, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and st["lo"].T.tolist() == [[1, 2, 2, 3], [7, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert not np.signbit(st["hi"]).any() and not np.signbit(st["lo"]).any() and not np.signbit(st["S1"]).any()           # -0 was counted as +0, dead slots are +0
    # the same frames in two updates and in another order: the same extremes and counts
    two = R.update(R.update(R.empty(1, 4), frames[:2]), frames[2:])
    assert all(np.array_equal(two[k].view(np.uint8), st[k].view(np.uint8)) for k in st)
    back = R.update(R.empty(1, 4), frames[::-1])
    assert all(np.array_equal(back[k], st[k]) for k in ("hi", "lo", "c"))
    # the bytes: 52 * 4 = 208, the planes where the header puts them
    raw = R.to_bytes(st, 1, 4)
    assert raw.size == 208 and raw[:8].view("<f8")[0] == 17.0 and raw[32:40].view("<f8")[0] == 59.0 and raw[64:68].view("<f4")[0] == 5.0
    assert raw[64 + 16:64 + 20].view("<f4")[0] == 4.0 and raw[128:132].view("<f4")[0] == 1.0 and raw[192:208].view("<i4").tolist() == [6, 1, 0, 1]
    assert not R.to_bytes(R.empty(1, 4), 1, 4).any()                              # all-zero bytes are the empty state
    assert all(np.array_equal(R.from_bytes(raw, 1, 4)[k], st[k]) for k in st)
    # merge: a split of the frames in two
    mg = R.merge(R.update(R.empty(1, 4), frames[:4]), R.update(R.empty(1, 4), frames[4:]))
    assert all(np.array_equal(mg[k], st[k]) for k in st)                          # (small integers: the sums are exact in any order)
    # finish, RANK: the r-th largest / smallest, r = min(rank, c); the empty cell gets `empty`
    for rank, want in ((1, [5, 7, 9, 0]), (2, [4, 7, 9, 0]), (4, [2, 7, 9, 0])):
        assert R.finish(st, 1, 4, "rank", "above", rank=rank, empty=9).tolist() == [want]
    assert R.finish(st, 1, 4, "rank", "below", rank=3, empty=np.inf).tolist() == [[2, 7, np.inf, 0]]
    # finish, SIGMA: mean 17/6, variance (59 - 17 * 17/6) / 5 = 13/6 up to the roundings of the definition; one value: sd = 0
    mean = np.float64(17) / 6
    sd = np.sqrt((np.float64(59) - np.float64(17) * mean) / 5)
    assert abs(sd * sd - 13 / 6) < 1e-14
    got = R.finish(st, 1, 4, "sigma", "above", k=3.0, empty=np.inf)
    assert got.dtype == f32 and got.tolist() == [[f32(mean + 3.0 * sd), 7, np.inf, 0]]
    assert R.finish(st, 1, 4, "sigma", "below", k=-2.5, empty=0).tolist() == [[f32(mean + np.float64(-2.5) * sd), 7, 0, 0]]
    assert R.finish(st, 1, 4, "sigma", k=0.0, empty=-1).tolist() == [[f32(mean), 7, -1, 0]]
    # a constant cell: d = S2 - S1 * mean is rounding noise of either sign (clamped at 0 when negative); the baseline is the constant to within
    # k sqrt(a few ulps of S2 / 6), a float ulp or so
    const = R.update(R.empty(1, 1), np.full((7, 1, 1), 0.1, f32))
    assert abs(np.float64(R.finish(const, 1, 1, "sigma", k=3.0)[0, 0]) - np.float64(f32(0.1))) < 1e-7
    # peak: the smallest index among equals, NaN skipped, -0 as +0, an image of NaN only
    maps = np.array([[[1, 5, 5], [nan, -2, -2]], [[nan, nan, nan], [nan, nan, nan]], [[-0.0, 0, 0], [0, 0, 0]], [[-np.inf, nan, np.inf], [np.inf, 0, 0]]], f32)
    pk, cell = R.peak(maps, None, "above")
    assert cell.tolist() == [1, -1, 0, 2] and pk[0] == 5 and pk.view(np.uint32)[1] == 0x7FC00000 and pk.view(np.uint32)[2] == 0 and pk[3] == np.inf
    pk, cell = R.peak(maps, None, "below")
    assert cell.tolist() == [4, -1, 0, 0] and pk[0] == -2 and pk.view(np.uint32)[1] == 0x7FC00000 and pk[3] == -np.inf
    ref = np.array([[0, 4, 5], [0, 0, -3]], f32)
    pk, cell = R.peak(maps[:1], ref, "above")
    assert (pk.tolist(), cell.tolist()) == ([1.0], [0])                            # 1 - 0, 5 - 4 and -2 + 3 tie at 1: the first
