"""aefft_frames_register_ref and aefft_frames_register at the boundary (no GPU): declared behind aefft_image_remap, exported and prototyped; the
enum and the 16-byte aefft_shift; the two size queries against their stated formulas; the null-context error; the Python signatures and the checks
that need no device; the restatement of register_ref.py on cases done by hand; the accuracy of the DEFINITION on the restatement alone (textures
cropped from a 2 x canvas, so the shift is not circular); the kernels' resource table (no scratch, no spills); the host check program, built and
run in its quick form."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks as A
import register_ref as R
from abi_checks import CSRC, ROOT, aefft

REF = ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "int nref", "int D", "int Nx", "int Ny", "int window", "float* spec_d", "void* work_d", "size_t work_bytes"]
REG = ["aefft_ctx* ctx", "const void* frames_d", "int frames_u8", "int B", "int D", "int Nx", "int Ny", "int window", "const float* ref_spec_d", "int nref", "float cutoff",
       "float min_response", "double scale_x", "double scale_y", "aefft_shift* shift_d", "aefft_affine* affine_d", "void* work_d", "size_t work_bytes"]
SIZES = [(16, 16), (32, 8), (64, 64), (48, 40), (8, 2048), (2048, 10), (256, 256), (640, 480)]
BAD_SIZES = [(7, 16), (16, 6), (14, 16), (16, 22), (4096, 16), (16, 0), (-8, 8), (15, 16), (2050, 16)]

# the accuracy cases: 256 x 256, shifts within +-32 pixels, eight integer and eight fractional, fixed seeds
_rng = np.random.default_rng(7)
INT_SHIFTS = [(int(a), int(b)) for a, b in _rng.integers(-32, 33, (8, 2))]
FRAC_SHIFTS = [(float(a), float(b)) for a, b in np.round(_rng.uniform(-32, 32, (8, 2)), 3)]


# 1.
def test_declared_exported_and_prototyped(monkeypatch):
    for typ, ct in (("double", C.c_double), ("aefft_shift*", C.c_void_p), ("aefft_affine*", C.c_void_p)):       # (a device pointer travels as void*)
        monkeypatch.setitem(A.CTYPES, typ, ct)
    A.check_call("aefft_frames_register_ref", REF)
    A.check_call("aefft_frames_register", REG)
    code = A.header_code()
    for name in ("aefft_register_spec_floats", "aefft_register_workspace"):
        assert name in A.exported() and aefft.SIGNATURES[name][0] is C.c_size_t
    assert re.search(r"size_t\s+aefft_register_spec_floats\s*\(\s*int Nx,\s*int Ny\s*\)", code)
    assert re.search(r"size_t\s+aefft_register_workspace\s*\(\s*int Nx,\s*int Ny,\s*int B\s*\)", code)
    assert re.search(r"enum\s*\{\s*AEFFT_REGISTER_HANN\s*=\s*0,\s*AEFFT_REGISTER_NOWINDOW\s*=\s*1\s*\}", code)
    assert aefft.REGISTER_WINDOW == {"hann": 0, "nowindow": 1} == R.WINDOW
    assert A.struct_fields("aefft_shift") == ["float dx, dy, response", "int cell"]
    assert C.sizeof(aefft.Shift) == 16 and aefft.SHIFT.itemsize == 16 and [f[0] for f in aefft.Shift._fields_] == list(aefft.SHIFT.names) == ["dx", "dy", "response", "cell"]


# 2.
def test_the_calls_stand_behind_remap_in_a_unit_of_their_own():
    A.in_order(A.header(), "int aefft_image_remap(", "/* aefft_frames_register_ref, aefft_frames_register", "AEFFT_REGISTER_HANN = 0", "} aefft_shift;",
               "size_t aefft_register_spec_floats(", "size_t aefft_register_workspace(", "int aefft_frames_register_ref(", "int aefft_frames_register(", "/* ---- network level")
    ops = open(os.path.join(CSRC, "register_ops.hip")).read()
    for word in ('extern "C" size_t aefft_register_spec_floats(', 'extern "C" size_t aefft_register_workspace(', 'extern "C" int aefft_frames_register_ref(',
                 'extern "C" int aefft_frames_register(', "do_r2c(", "do_c2r(", "join_recon(ctx)", "launch_or_fail(", "KID_IMAGE"):
        assert word in ops, word
    assert "hipMalloc" not in ops and "Synchronize" not in ops and "hipMemset" not in ops and "hipMemcpy" not in ops
    for other in ("image_ops.hip", "ops.hip"):
        assert "aefft_frames_register" not in open(os.path.join(CSRC, other)).read(), other
    mk = open(os.path.join(CSRC, "Makefile")).read().split("SRCS =")[1].split("\n")[0]
    assert "register_kernels.hip" in mk and "register_ops.hip" in mk
    internal = open(os.path.join(CSRC, "internal.h")).read()
    for fn in ("hipError_t launch_register_prepare(", "hipError_t launch_register_cross(", "hipError_t launch_register_peak(", "size_t register_workspace("):
        assert fn in internal, fn
    lanes = open(os.path.join(ROOT, "tools", "hostlanes.h")).read()
    assert lanes.count("#define RG_HD static inline") == 1


# 3.
def test_header_states_the_definition():
    doc = A.doc("/* aefft_frames_register_ref, aefft_frames_register", "enum { AEFFT_REGISTER_HANN", margin=False)
    for word in ("phase correlation", "[B][D][Nx][Ny]", "axis i is the image column and axis j the image row", "D in 1..4", "B >= 1", "powers of two in 8..2048",
                 "even smooth sizes in 10..2048", "g[b][i][j] = wx[i] wy[j] sum_d p[b][d][i][j]", "w[n] = 0.5 - 0.5 cos(2 pi n / N)", "periodic content",
                 "G = r2c(g), unnormalised", "R = G_img conj(G_ref)", "Q = R / |R|", "|R| > 0", "2|u| <= cutoff Nx", "2|v| <= cutoff Ny", "the DC bin alone",
                 "the nine bins with |u| <= 1 and |v| <= 1", "float in (0, 1]", "kept bins of the FULL Nx x Ny spectrum", "s = c2r(Q) / K", "scale = 1 / K",
                 "the smallest index i Ny + j on ties", "5 x 5 circular neighbourhood", "w = max(s, 0)", "in double", "cx = sum w di / sum w", "reduced by Nx when >= Nx / 2",
                 "response = s[pi][pj]", "cell = pi Ny + pj", "16 bytes", "each in (0, 32]", "response >= min_response (false for NaN)",
                 "rint((double)dx scale_x 2^24)", "{2^24, 0, 0, 0, 2^24, 0}", "ties to even", "2^39", "img(x) = ref(x - d)", "(dx, dy) = +d", "src = dst + d",
                 "np.roll(ref, 3, axis=-2)", "Non-finite float frames give unspecified numbers", "cell is always inside the grid", "nref == 1", "nref == B",
                 "round16(4 B Nx Ny)", "round16(8 B Nx (Ny/2+1))", "round16(8 B ceil(Nx Ny / 4096))", "exactly as aefft_r2c does", "may allocate",
                 "must not be the first one made under stream capture", "later calls are safe under capture", "no host synchronisation", "no atomics",
                 "no workgroup waits for another", "the same bytes from run to run", "profile id `image`", "AEFFT_EINVAL", '"aefft_frames_register: "',
                 '"aefft_frames_register_ref: "', "nothing enqueued and the outputs untouched", "affine_d may be NULL", "an unknown window", "cutoff outside (0, 1] or NaN",
                 "keeps no bin (K = 0)", "a scale outside (0, 32] or non-finite", "not 16-byte aligned", "work_bytes too small", "overlap inputs, the workspace or each other"):
        assert word in doc, word


# 4.
def test_no_new_switch_option_or_profiling_id():
    flags, names = A.tables_unchanged("REGISTER", "SHIFT", profiler=("register", "shift", "phase"))
    assert names.count("image") == 1
    assert not [k for k in aefft.FLAGS if "REGISTER" in k]


# 5.
def test_size_queries_match_their_formulas():
    L = A.lib()
    r16 = lambda v: (v + 15) & ~15
    for Nx, Ny in SIZES:
        assert L.aefft_register_spec_floats(Nx, Ny) == 2 * Nx * (Ny // 2 + 1) == R.spec_floats(Nx, Ny)
        for B in (1, 3, 32):
            want = r16(4 * B * Nx * Ny) + r16(8 * B * Nx * (Ny // 2 + 1)) + r16(8 * B * ((Nx * Ny + 4095) // 4096))
            assert L.aefft_register_workspace(Nx, Ny, B) == want == R.workspace(Nx, Ny, B), (Nx, Ny, B)
    for Nx, Ny in BAD_SIZES:
        assert L.aefft_register_spec_floats(Nx, Ny) == 0 == R.spec_floats(Nx, Ny) and L.aefft_register_workspace(Nx, Ny, 1) == 0 == R.workspace(Nx, Ny, 1), (Nx, Ny)
    assert L.aefft_register_workspace(16, 16, 0) == 0 and L.aefft_register_workspace(16, 16, -1) == 0
    assert L.aefft_register_workspace(2048, 2048, 128) == 0 and L.aefft_register_workspace(2048, 2048, 127) > 0      # B Nx Ny < 2^29


# 6.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 16384)(*([0x5A] * 16384))
    base = C.addressof(buf)
    base += -base % 16
    frames, spec, shift, aff, work = (C.c_void_p(base + k * 3072) for k in range(5))
    need = L.aefft_register_workspace(16, 16, 1)
    for window in (0, 1):
        assert L.aefft_frames_register_ref(None, frames, 1, 1, 3, 16, 16, window, spec, work, need) == aefft.EINVAL
        assert L.aefft_frames_register(None, frames, 1, 1, 3, 16, 16, window, spec, 1, 0.5, 0.0, 1.0, 1.0, shift, aff, work, need) == aefft.EINVAL
    assert L.aefft_frames_register_ref(None, None, 0, 0, 0, 0, 0, 0, None, None, 0) == aefft.EINVAL
    assert L.aefft_frames_register(None, None, 0, 0, 0, 0, 0, 0, None, 0, 0.0, 0.0, 0.0, 0.0, None, None, None, 0) == aefft.EINVAL
    assert bytes(buf) == bytes([0x5A] * 16384)


# 7.
def test_python_signatures_and_checks_need_no_device():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(aefft.Context.frames_register_ref)
    assert list(p) == ["self", "frames", "window"] and p["window"].default == "hann"
    p = sig(aefft.Context.frames_register)
    assert list(p) == ["self", "frames", "ref", "cutoff", "min_response", "scale", "affine"]
    assert [p[n].default for n in list(p)[3:]] == [0.5, 0.0, (1.0, 1.0), False]
    p = sig(aefft.Context.image_align)
    assert list(p)[:4] == ["self", "image", "ref", "frame_size"] and all(p[n].default is not inspect.Parameter.empty for n in list(p)[4:])
    frames = torch.zeros(3, 2, 16, 32, dtype=torch.uint8)
    one = aefft.RegisterRef(torch.zeros(1, 16, 17, dtype=torch.complex64), "hann", 2, 16, 32)
    per = aefft.RegisterRef(torch.zeros(3, 16, 17, dtype=torch.complex64), "nowindow", 2, 16, 32)
    assert (one.nref, per.nref, per.window) == (1, 3, "nowindow")
    good = dict(frames=frames, ref=one, cutoff=0.5, min_response=0.0, scale=(1.0, 1.0))
    assert aefft._register_args(**good) == (3, 2, 16, 32, 1.0, 1.0)
    assert aefft._register_args(**dict(good, ref=per, cutoff=1, scale=(2, 1.5), frames=frames.float())) == (3, 2, 16, 32, 2.0, 1.5)
    two = aefft.RegisterRef(torch.zeros(2, 16, 17, dtype=torch.complex64), "hann", 2, 16, 32)
    other = aefft.RegisterRef(torch.zeros(1, 32, 9, dtype=torch.complex64), "hann", 2, 32, 16)
    for bad in (dict(frames=frames.double()), dict(frames=frames[0]), dict(frames=frames.permute(0, 1, 3, 2)), dict(ref=two), dict(ref=other), dict(ref=one.spec),
                dict(cutoff=0.0), dict(cutoff=1.01), dict(cutoff=float("nan")), dict(min_response=float("nan")), dict(scale=(0.0, 1.0)), dict(scale=(1.0, 32.5)),
                dict(scale=(1.0, float("inf"))), dict(scale=1.0), dict(scale=(1.0,))):
        with pytest.raises(ValueError):
            aefft._register_args(**dict(good, **bad))


# 8.
def test_the_restatement_on_cases_by_hand():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (1, 3, 16, 16), dtype=np.uint8)
    (r,), s = R.register(x, x, "nowindow", 1.0)
    assert r[3] == 0 and r[0] == 0.0 and r[1] == 0.0 and abs(r[2] - 1.0) <= 1e-9
    for grid in ((16, 16), (32, 8), (48, 40)):
        x = rng.integers(0, 256, (1, 2) + grid, dtype=np.uint8)
        for d in ((3, -2), (-5, 7) if grid[1] > 14 else (-5, 3)):
            (r,), s = R.register(np.roll(x, d, (2, 3)), x, "nowindow", 1.0)
            assert abs(r[0] - d[0]) <= 1e-9 and abs(r[1] - d[1]) <= 1e-9 and abs(r[2] - 1.0) <= 1e-9, (grid, d, r)
            assert r[3] == (d[0] % grid[0]) * grid[1] + d[1] % grid[1]
    # K
    assert int(R.kept(16, 16, "hann", 1.0).sum()) == 256 - 9
    brute = sum(1 for i in range(32) for j in range(8) if 2 * abs(i if i <= 16 else i - 32) <= 0.5 * 32 and 2 * abs(j if j <= 4 else j - 8) <= 0.5 * 8 and (i, j) != (0, 0))
    assert int(R.kept(32, 8, "nowindow", 0.5).sum()) == brute == 17 * 5 - 1
    assert int(R.kept(16, 16, "nowindow", 1.0).sum()) == 255 and int(R.kept(16, 16, "nowindow", 0.01).sum()) == 0
    # the tie rule and the wrap to signed shifts
    s = np.zeros((8, 8))
    s[6, 7] = s[2, 3] = 0.5
    assert R.peak(s) == (2.0, 3.0, 0.5, 2 * 8 + 3)
    s[2, 3] = 0.0
    assert R.peak(s) == (-2.0, -1.0, 0.5, 6 * 8 + 7)
    s[7, 7] = 0.5                                                                # the centroid between two equal cells, across nothing
    assert R.peak(s)[:2] == (-1.5, -1.0)
    s = np.zeros((8, 8))
    s[0, 0], s[7, 0] = 0.75, 0.25                                                # the neighbourhood is circular: the neighbour at i = -1
    assert R.peak(s) == (-0.25, 0.0, 0.75, 0)
    assert R.peak(np.full((8, 8), -1.0)) == (0.0, 0.0, -1.0, 0)                  # sum w = 0: the centroid is the cell
    # the affine
    assert R.affine(3.0, -2.0, 0.9, 0.5, (1.0, 1.0)) == [R.Q, 0, 3 * R.Q, 0, R.Q, -2 * R.Q]
    assert R.affine(3.0, -2.0, 0.4, 0.5, (1.0, 1.0)) == [R.Q, 0, 0, 0, R.Q, 0] == R.affine(3.0, -2.0, float("nan"), 0.0, (1.0, 1.0))
    assert R.affine(0.5, 1.0 / R.Q, 1.0, 0.0, (2.0, 1.5)) == [R.Q, 0, R.Q, 0, R.Q, 2]                # 1.5 rounds to even


# 9.
@pytest.mark.parametrize("cutoff", [1.0, 0.5])
def test_accuracy_of_the_definition_on_textures(cutoff):
    """Gaussian-low-passed noise (sigma = 0.08 cycles per pixel) cropped from a 2 x canvas and quantised to 8 bits, 256 x 256, HANN: every estimate
    within 0.25 pixel of the truth.  Observed maxima (CPU, double): 0.066 at cutoff 1.0, 0.052 at cutoff 0.5."""
    worst = 0.0
    for k, shift in enumerate(INT_SHIFTS + FRAC_SHIFTS):
        ref, img = R.texture_pair(256, 256, 100 + k, shift)
        (r,), _ = R.register(img[None], ref[None], "hann", cutoff)
        worst = max(worst, abs(r[0] - shift[0]), abs(r[1] - shift[1]))
    print("cutoff %.1f: largest |estimate - truth| = %.4f px" % (cutoff, worst))
    assert all(abs(v) <= 32 for s in INT_SHIFTS + FRAC_SHIFTS for v in s) and len(INT_SHIFTS) == len(FRAC_SHIFTS) == 8
    assert worst <= 0.25


# 10.
def test_register_kernels_use_no_scratch_and_are_the_launched_ones():
    """build/register_kernels.rsrc: prepare at D = 1..4 for 8-bit and float frames, the cross-power and the two peak stages, nothing else, each with
    zero scratch and zero spills"""
    got = A.instantiations("register_kernels.rsrc", r"\d+(register_prepare_kernel)ILi(\d)ELb([01])EEEvNS_6RgArgsE", r"\d+(register_cross_kernel)ENS_6RgArgsEj",
                           r"\d+(register_peak[12]_kernel)ENS_6RgArgsE")
    assert got[0] == {("register_prepare_kernel", str(D), u8) for D in (1, 2, 3, 4) for u8 in "01"}
    assert got[1] == {("register_cross_kernel",)} and got[2] == {("register_peak1_kernel",), ("register_peak2_kernel",)}
    for name, (_, ints) in A.rsrc("register_kernels.rsrc").items():
        assert ints["VGPRs"] <= 64, (name, ints)                                 # (eight waves a SIMD)
    src = open(os.path.join(CSRC, "register_kernels.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h"}
    code = re.sub(r"//[^\n]*", "", src)                                          # (without the comments)
    assert "atomic" not in code and "hipMalloc" not in code and "Synchronize" not in code and "cosf(" in code and code.count("<<<") == 5
    assert "#ifndef AEFFT_HOSTCHECK" in src and "#define RG_HD __device__ __forceinline__" in src


# 11.
def test_host_check_builds_and_its_quick_form_passes(tmp_path):
    """tools/register_hostcheck.cpp: the kernel file compiled for the host under -fsanitize=address,undefined, a program of its own (never loaded into
    Python), every buffer at its exact extent, against its own scalar C restatement; the quick form is a thinned sweep, the full one is run by hand"""
    src = A.host_check_stands_alone("register_hostcheck.cpp", "register_kernels.hip")
    for body in ("register_prepare_body<D, U8>(", "register_cross_body(", "register_peak1_body(", "register_peak2_body("):
        assert body in src, body
    assert "hipcc" not in src and "LD_PRELOAD" not in src and "int main(int argc" in src and "rg_kept(" in src and "rg_workspace(" in src
    assert os.path.exists(os.path.join(ROOT, "tools", "register_bench.py"))
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):  # the product never imports the restatement
        for f in files:
            if f.endswith(".py"):
                assert not re.search(r"(import|from)\s+register_ref\b", open(os.path.join(dirpath, f)).read()), f
    exe = str(tmp_path / "register_hostcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(ROOT, "tools", "register_hostcheck.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    print(r.stdout[-500:])
    assert r.returncode == 0 and re.search(r"all \d+ runs exact", r.stdout), (r.stdout[-2000:], r.stderr[-2000:])
