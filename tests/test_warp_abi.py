"""aefft_affine_make, aefft_image_warp_affine and aefft_image_remap at the boundary (no GPU): declared in the image-boundary block behind
aefft_map_peak, exported and prototyped; the enums; the null-context error; aefft_affine_make against Python integers; the Python checks on CPU
tensors; the restatement of warp_ref.py on cases done by hand; the table makers; the kernels' resource table (no scratch, no spills); the host check
program, built and run in its quick form."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks as A
import warp_ref as R
from abi_checks import CSRC, ROOT, aefft

IMG = ["const unsigned char* src_d", "size_t src_pitch", "size_t src_stride", "int Ws", "int Hs"]
TAIL = ["int interp", "int border", "unsigned border_value", "unsigned char* dst_d", "size_t dst_pitch", "size_t dst_stride", "int Wd", "int Hd", "int B", "int D"]
WARP = ["aefft_ctx* ctx"] + IMG + ["const aefft_affine* m_d", "int nm"] + TAIL
REMAP = ["aefft_ctx* ctx"] + IMG + ["const int* map_d"] + TAIL
Q = 1 << 24


# 1.
def test_declared_exported_and_prototyped(monkeypatch):
    for typ, ct in (("unsigned", C.c_uint), ("const int*", C.c_void_p), ("const aefft_affine*", C.c_void_p)):   # (a device pointer travels as void*)
        monkeypatch.setitem(A.CTYPES, typ, ct)
    A.check_call("aefft_image_warp_affine", WARP)
    A.check_call("aefft_image_remap", REMAP)
    assert A.prototype("aefft_affine_make") == ["const double m[6]", "aefft_affine* out"] and "aefft_affine_make" in A.exported()
    res, argt = aefft.SIGNATURES["aefft_affine_make"]
    assert res is C.c_int and argt[0]._type_ is C.c_double and argt[1]._type_ is aefft.Affine
    assert A.struct_fields("aefft_affine") == ["long long a[6]"] and C.sizeof(aefft.Affine) == 48
    code = A.header_code()
    assert re.search(r"enum\s*\{\s*AEFFT_WARP_NEAREST\s*=\s*0,\s*AEFFT_WARP_LINEAR\s*=\s*1\s*\}", code)
    assert re.search(r"enum\s*\{\s*AEFFT_BORDER_CONSTANT\s*=\s*0,\s*AEFFT_BORDER_REPLICATE\s*=\s*1,\s*AEFFT_BORDER_REFLECT\s*=\s*2\s*\}", code)
    assert aefft.WARP_INTERP == {"nearest": 0, "linear": 1} == R.INTERP and aefft.WARP_BORDER == {"constant": 0, "replicate": 1, "reflect": 2} == R.BORDER
    sig = lambda f: inspect.signature(f).parameters
    p = sig(aefft.Context.image_warp)
    assert list(p) == ["self", "image", "matrix", "size", "interp", "border", "value", "out"]
    assert [p[n].default for n in list(p)[3:]] == [None, "linear", "constant", 0, None]
    p = sig(aefft.Context.image_remap)
    assert list(p) == ["self", "image", "table", "interp", "border", "value", "out"] and [p[n].default for n in list(p)[3:]] == ["linear", "constant", 0, None]
    assert list(sig(aefft.affine_q)) == ["m"] and list(sig(aefft.affine_table)) == ["m", "size"] and list(sig(aefft.homography_table)) == ["Hm", "size"]
    p = sig(aefft.undistort_table)
    assert list(p) == ["K", "dist", "size", "new_K"] and p["new_K"].default is None


# 2.
def test_the_calls_stand_behind_map_peak_and_in_a_section_of_their_own_in_the_host_unit():
    A.in_order(A.header(), "int aefft_map_peak(", "/* aefft_image_warp_affine, aefft_image_remap", "AEFFT_WARP_NEAREST = 0", "AEFFT_BORDER_CONSTANT = 0", "} aefft_affine;",
               "int aefft_affine_make(", "int aefft_image_warp_affine(", "int aefft_image_remap(", "/* ---- network level")
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    # (between the regions and the calibration: the sections behind it, the file's end included, are counted by the files of their calls)
    A.in_order(ops, 'extern "C" int aefft_region_to_pixels(', "// align and rectify", 'extern "C" int aefft_affine_make(', 'extern "C" int aefft_image_warp_affine(',
               'extern "C" int aefft_image_remap(', "// calibration")
    section = ops[ops.index("// align and rectify"):ops.index("// calibration")]
    assert section.count("KID_IMAGE") == 2 and section.count("join_recon(ctx)") == 2 and section.count("launch_or_fail(") == 2 and section.count("ranges_overlap(") == 3
    assert section.count("const Bad bad{ctx,") == 2 and section.count("aligned16(") == 2 and section.count("chk_rows(") == 2 and "chk_dims(" in section
    assert "hipMalloc" not in section and "Synchronize" not in section and "ws_get" not in section and "hipMemset" not in section
    for helper in ("struct Bad {", "static bool ranges_overlap(", "static int chk_rows("):
        assert ops.count(helper) == 1, helper
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_image_warp" not in rest and "aefft_image_remap" not in rest
    lanes = open(os.path.join(ROOT, "tools", "hostlanes.h")).read()
    assert lanes.count("#define WP_HD static inline") == 1


# 3.
def test_header_states_the_definition():
    doc = A.doc("/* aefft_image_warp_affine, aefft_image_remap", "enum { AEFFT_WARP_NEAREST", margin=False)
    for word in ("the layout and rules of aefft_image_resize_to_frames", "y * pitch + x * D + d", "ANY alignment", "pitch >= W * D", "stride >= (H - 1) * pitch + W * D",
                 "never read or written", "D in 1..4", "Ws, Hs, Wd, Hd in 1..8192", "B >= 1", "must not overlap", "maps a DESTINATION pixel to the source position",
                 "WARP_INVERSE_MAP", "cv::remap", "pixel centres", "NOT byte-identical to OpenCV", "5 fraction bits", "times 2048", "int map[Hd][Wd][2], x first",
                 "16-byte aligned", "shared by all B images", "Any int32 value is legal", "Q24 (48 bytes)", "nm == 1", "nm == B", "U = a[0] x + a[1] y + a[2]",
                 "V = a[3] x + a[4] y + a[5]", "wrapping 64-bit arithmetic", "tx = clamp((U + 2^12) >> 13, -2^31, 2^31 - 1)", "arithmetic shift", "every bit pattern",
                 "no byte outside the source images is read", "neither the wrap nor the clamp is ever active", "2^30 + 2^27", "a[k] = m[k] * 2^24", "ties to even",
                 "nothing written", "a non-finite entry", "> 2^29", "> 2^39", "below 2^-11 pixel", "sx = (tx + 1024) >> 11 (halves up)", "sx = tx >> 11 and wx = tx & 2047",
                 "(sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1)", "v = (2048-wy) ((2048-wx) p00 + wx p01) + wy ((2048-wx) p10 + wx p11) < 2^30", "(v + 2^21) >> 22",
                 "each tap on its own, per axis", "(border_value >> 8 d) & 255", "clamp(s, 0, S-1)", "for S = 1 the result is 0", "P = 2(S-1)", "m = s mod P taken non-negative",
                 "r = m when m < S, else P - m", "the identity gives the source's bytes", "an integer translation gives the shifted bytes", "{0, 1, 0, -1, 0, Hs-1}",
                 "rot90(src, -1)", "{0, -1, Ws-1, 1, 0, 0}", "rot90(src, 1)", "between bytes 10 and 20 gives 15", "gives the constant everywhere", "byte for byte",
                 "one launch each", "no host synchronisation", "no allocation", "no workspace", "no atomics", "safe under stream capture", "the same bytes", "profile id `image`",
                 "B D (Ws Hs + Wd Hd) bytes plus 48 nm", "8 Wd Hd", "AEFFT_EINVAL", '"aefft_image_warp_affine: "', '"aefft_image_remap: "', "naming the rule", "nothing enqueued",
                 "the destination untouched", "nm not 1 or B", "an unknown interp or border", "not 16-byte aligned", "overlapping the source, the affines or the table",
                 "overflow the address space"):
        assert word in doc, word


# 4.
def test_no_new_switch_option_or_profiling_id():
    flags, names = A.tables_unchanged("WARP", "REMAP", "AFFINE", profiler=("warp", "remap", "affine"))
    assert names.count("image") == 1
    assert not [k for k in aefft.FLAGS if "WARP" in k or "REMAP" in k]


# 5.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 8192)(*([0x5A] * 8192))
    base = C.addressof(buf)
    base += -base % 16
    src, dst, m, tab = (C.c_void_p(base + k * 1536) for k in range(4))
    for interp in (0, 1):
        for border in (0, 1, 2):
            assert L.aefft_image_warp_affine(None, src, 21, 200, 7, 5, m, 1, interp, border, 0x010203, dst, 24, 240, 8, 6, 2, 3) == aefft.EINVAL
            assert L.aefft_image_remap(None, src, 21, 200, 7, 5, tab, interp, border, 0x010203, dst, 24, 240, 8, 6, 2, 3) == aefft.EINVAL
    assert L.aefft_image_warp_affine(None, None, 0, 0, 0, 0, None, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, 0) == aefft.EINVAL
    assert L.aefft_image_remap(None, None, 0, 0, 0, 0, None, 0, 0, 0, None, 0, 0, 0, 0, 0, 0) == aefft.EINVAL
    assert bytes(buf) == bytes([0x5A] * 8192)


def _make(m):
    """aefft_affine_make on six doubles: (the code, the six coefficients as the call left them in a struct preset to 77)"""
    q = aefft.Affine((C.c_longlong * 6)(*[77] * 6))
    rc = A.lib().aefft_affine_make((C.c_double * 6)(*m), C.byref(q))
    return rc, list(q.a)


# 6.
def test_affine_make_against_python_integers():
    L = A.lib()
    # exact values, both signs; ties to even at k + 0.5 units of 2^-24
    assert _make([1, 0, 0, 0, 1, 0]) == (0, [Q, 0, 0, 0, Q, 0])
    assert _make([-0.5, 0.25, -3, 2, -1, 7.5]) == (0, [-Q // 2, Q // 4, -3 * Q, 2 * Q, -Q, 15 * Q // 2])
    for k in (0, 1, 2, 3, 4, 5, 1000, 1001, -1, -2, -3, -1001, 2 ** 28 + 1, 2 ** 28 + 2):
        tie = (k + 0.5) / Q                                                      # (exact in double: k + 0.5 has at most 31 bits)
        even = k if k % 2 == 0 else k + 1
        for slot in range(6):
            m = [0.0] * 6
            m[slot] = tie
            rc, a = _make(m)
            assert rc == 0 and a[slot] == even and a == R.affine_make(m), (k, slot, a)
    # near a tie: one ulp of the double to either side decides
    for k in (2, 3, -4, -5):
        lo, hi = np.nextafter((k + 0.5) / Q, -np.inf), np.nextafter((k + 0.5) / Q, np.inf)
        assert _make([lo] + [0] * 5)[1][0] == k and _make([hi] + [0] * 5)[1][0] == k + 1
    # the restatement on random doubles
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = (rng.uniform(-32, 32, 6) * np.array([1, 1, 1000, 1, 1, 1000])).tolist()
        assert _make(m) == (0, R.affine_make(m))
    # both range limits accepted, one unit beyond rejected with `out` untouched
    for slot in range(6):
        limit = R.OFF_LIMIT if slot % 3 == 2 else R.LIN_LIMIT
        for sign in (1, -1):
            m = [0.0] * 6
            m[slot] = sign * limit / Q
            rc, a = _make(m)
            assert rc == 0 and a[slot] == sign * limit and R.affine_make(m) == a
            m[slot] = sign * (limit + 1) / Q
            assert _make(m) == (aefft.EINVAL, [77] * 6) and R.affine_make(m) is None, (slot, sign)
            m[slot] = sign * (limit + 0.25) / Q                                  # rounds onto the limit: accepted
            assert _make(m) == (0, R.affine_make(m)) and R.affine_make(m)[slot] == sign * limit
    assert _make([32, -32, 32768, -32, 32, -32768])[0] == 0
    for bad in (float("nan"), float("inf"), float("-inf"), 1e300, -1e300):
        for slot in range(6):
            m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            m[slot] = bad
            assert _make(m) == (aefft.EINVAL, [77] * 6), (bad, slot)
            assert R.affine_make(m) is None
    q = aefft.Affine()
    assert L.aefft_affine_make(None, C.byref(q)) == aefft.EINVAL and L.aefft_affine_make((C.c_double * 6)(), None) == aefft.EINVAL
    # the Python form
    got = aefft.affine_q([[1, 0, 0.5], [0, 1, -2]])
    assert got.dtype == np.int64 and got.tolist() == [[Q, 0, Q // 2, 0, Q, -2 * Q]]
    three = aefft.affine_q(np.stack([np.eye(2, 3) * s for s in (1, 2, 0.5)]))
    assert three.shape == (3, 6) and three[:, 0].tolist() == [Q, 2 * Q, Q // 2]
    for bad in ([[1, 0, 0], [0, 1, float("nan")]], [[33, 0, 0], [0, 1, 0]], [[1, 0, 40000], [0, 1, 0]], np.zeros((3, 2)), np.zeros((2, 3, 3)), "matrix", np.zeros((0, 2, 3))):
        with pytest.raises(ValueError):
            aefft.affine_q(bad)
    # within the accepted ranges neither the wrap nor the clamp is active: |tx| < 2^30 + 2^27 at the limits and x, y = 8191
    worst = 2 * R.LIN_LIMIT * 8191 + R.OFF_LIMIT
    assert (worst + 4096) >> 13 < 2 ** 30 + 2 ** 27 and worst < 2 ** 63


# 7.
def test_python_checks_need_no_device():
    """the checks of the two wrappers run before anything reaches the device: CPU tensors suffice"""
    img = torch.zeros(3, 5, 7, 3, dtype=torch.uint8)
    eye = [[1, 0, 0], [0, 1, 0]]
    good = dict(image=img, matrix=eye, size=None, interp="linear", border="constant", value=0, out=None)
    i, pitch, stride, q, size, it, bo, v = aefft._image_warp_args(**good)
    assert tuple(i.shape) == (3, 5, 7, 3) and (pitch, stride, size, it, bo, v) == (21, 105, (7, 5), 1, 0, 0) and q.tolist() == [[Q, 0, 0, 0, Q, 0]]
    big = torch.zeros(3, 9, 11, 3, dtype=torch.uint8)
    i, pitch, stride, q, size, it, bo, v = aefft._image_warp_args(**dict(good, image=big[:, 2:7, 1:8], matrix=[eye] * 3, size=(4, 6), interp="nearest", border="reflect",
                                                                        value=(1, 2, 3), out=torch.zeros(3, 6, 4, 3, dtype=torch.uint8)))
    assert (pitch, stride, size, it, bo, v) == (33, 297, (4, 6), 0, 2, 0x030201) and q.shape == (3, 6)
    dev = torch.zeros(3, 6, dtype=torch.int64)
    assert aefft._image_warp_args(**dict(good, matrix=dev))[3] is dev and aefft._image_warp_args(**dict(good, image=img[0], matrix=dev[:1]))[0].shape[0] == 1
    for bad in (dict(image=img.float()), dict(image=img[0, 0]), dict(image=img.permute(0, 2, 1, 3)), dict(image=torch.zeros(1, 2, 2, 5, dtype=torch.uint8)), dict(matrix=[eye] * 2),
                dict(matrix=dev[:2]), dict(matrix=torch.zeros(3, 5, dtype=torch.int64)), dict(matrix=torch.zeros(6, 3, dtype=torch.int64).t()), dict(matrix=[[1, 0], [0, 1]]),
                dict(matrix=[[40, 0, 0], [0, 1, 0]]), dict(size=(0, 5)), dict(size=(8193, 5)), dict(size=5), dict(interp="cubic"), dict(interp=1), dict(border="wrap"),
                dict(value=256), dict(value=-1), dict(value=(1, 2)), dict(value=1.5), dict(value=True), dict(out=torch.zeros(3, 5, 7, 3)),
                dict(out=torch.zeros(3, 7, 5, 3, dtype=torch.uint8)), dict(size=(4, 6), out=torch.zeros(3, 5, 7, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            aefft._image_warp_args(**dict(good, **bad))
    tab = torch.zeros(6, 4, 2, dtype=torch.int32)
    good = dict(image=img, table=tab, interp="linear", border="constant", value=0, out=None)
    i, pitch, stride, size, it, bo, v = aefft._image_remap_args(**good)
    assert (pitch, stride, size, it, bo, v) == (21, 105, (4, 6), 1, 0, 0)
    assert aefft._image_remap_args(**dict(good, interp="nearest", border="replicate", value=(9, 8, 7), out=torch.zeros(3, 6, 4, 3, dtype=torch.uint8)))[4:] == (0, 1, 0x070809)
    for bad in (dict(table=tab.long()), dict(table=tab[..., 0]), dict(table=torch.zeros(6, 4, 3, dtype=torch.int32)), dict(table=tab[:, ::2]), dict(table=np.zeros((6, 4, 2), np.int32)),
                dict(table=torch.zeros(0, 4, 2, dtype=torch.int32)), dict(image=img.float()), dict(interp="area"), dict(border="zero"), dict(value=(1, 2, 3, 4)),
                dict(out=torch.zeros(3, 4, 6, 3, dtype=torch.uint8)), dict(out=torch.zeros(3, 6, 4, 3))):
        with pytest.raises(ValueError):
            aefft._image_remap_args(**dict(good, **bad))


def _q(*m):
    return [int(round(v * Q)) for v in m]


# 8.
def test_the_restatement_on_cases_by_hand():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    Hs, Ws = 5, 7
    word = R.border_word((200, 100, 50), 3)
    assert word == 0x3264C8
    for interp in R.INTERP:
        for border in R.BORDER:
            kw = dict(interp=interp, border=border, value=word)
            # the identity gives the source's bytes
            assert np.array_equal(R.warp_affine(src, _q(1, 0, 0, 0, 1, 0), (Ws, Hs), **kw), src)
            # an integer translation: dst(x, y) = src(x + 2, y - 1), the border rule in the uncovered strip
            out = R.warp_affine(src, _q(1, 0, 2, 0, 1, -1), (Ws, Hs), **kw)
            assert np.array_equal(out[:, 1:, :5], src[:, :4, 2:])
            const = np.array([200, 100, 50], np.uint8)
            want_top = {"constant": np.broadcast_to(const, (2, 5, 3)), "replicate": src[:, 0, 2:], "reflect": src[:, 1, 2:]}[border]
            assert np.array_equal(out[:, 0, :5], want_top), (interp, border)
            want_right = {"constant": np.broadcast_to(const, (2, 4, 2, 3)), "replicate": src[:, :4, 6:7].repeat(2, 2),
                          "reflect": src[:, :4, [5, 4]]}[border]
            assert np.array_equal(out[:, 1:, 5:], want_right), (interp, border)
            # the quarter turns, into a destination of Hs x Ws
            assert np.array_equal(R.warp_affine(src, _q(0, 1, 0, -1, 0, Hs - 1), (Hs, Ws), **kw), np.rot90(src, -1, axes=(1, 2)))
            assert np.array_equal(R.warp_affine(src, _q(0, -1, Ws - 1, 1, 0, 0), (Hs, Ws), **kw), np.rot90(src, 1, axes=(1, 2)))
            # a mirror
            assert np.array_equal(R.warp_affine(src, _q(-1, 0, Ws - 1, 0, 1, 0), (Ws, Hs), **kw), src[:, :, ::-1])
        # entirely outside: the constant everywhere; the other rules never give it (the source has no such pixel here)
        out = R.warp_affine(src, _q(1, 0, 100, 0, 1, -100), (Ws, Hs), interp=interp, border="constant", value=word)
        assert (out == np.array([200, 100, 50], np.uint8)).all()
        assert np.array_equal(R.warp_affine(src, _q(1, 0, 100, 0, 1, -100), (Ws, Hs), interp=interp, border="replicate"), np.broadcast_to(src[:, :1, 6:7], src.shape))
    # a half-pixel offset between bytes 10 and 20 gives 15; nearest takes the upper one (halves up)
    line = np.array([[[10], [20]]], np.uint8)[None]
    assert R.warp_affine(line, _q(1, 0, 0.5, 0, 1, 0), (1, 1), "linear")[0, 0, 0, 0] == 15 and R.warp_affine(line, _q(1, 0, 0.5, 0, 1, 0), (1, 1), "nearest")[0, 0, 0, 0] == 20
    assert R.warp_affine(line, _q(1, 0, 0.25, 0, 1, 0), (1, 1), "linear")[0, 0, 0, 0] == 13       # 12.5 rounds up
    assert R.warp_affine(line.transpose(0, 2, 1, 3), _q(1, 0, 0, 0, 1, 0.5), (1, 1), "linear")[0, 0, 0, 0] == 15
    # half a pixel over the edge: half the constant
    assert R.sample(line[0], [[-1024]], [[0]], "linear", "constant", 30)[0, 0, 0] == 20 and R.sample(line[0], [[-1024]], [[0]], "linear", "replicate", 30)[0, 0, 0] == 10
    # each border rule on a 1-pixel and a 2-pixel axis
    s = np.arange(-6, 8)
    idx, live = R.border_index(s, 1, "reflect")
    assert idx.tolist() == [0] * 14 and live.all()
    idx, live = R.border_index(s, 1, "replicate")
    assert idx.tolist() == [0] * 14 and live.all()
    idx, live = R.border_index(s, 1, "constant")
    assert live.tolist() == [v == 0 for v in s]
    idx, live = R.border_index(s, 2, "reflect")
    assert idx.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1] and live.all()
    idx, live = R.border_index(s, 2, "replicate")
    assert idx.tolist() == [0] * 6 + [0, 1] + [1] * 6 and live.all()
    idx, live = R.border_index(s, 2, "constant")
    assert live.tolist() == [v in (0, 1) for v in s]
    idx, live = R.border_index(np.arange(-5, 9), 4, "reflect")
    assert idx.tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    # the wrap and the clamp of the affine: coefficients no aefft_affine_make gives
    tx, ty = R.affine_txty([2 ** 62, 0, 0, 0, 2 ** 63 - 1, 5], 5, 3)
    assert tx[0].tolist() == [0, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 0] and ty[:, 0].tolist() == [0, -2 ** 31, 0]           # V = 5, 2^63 + 4 -> -2^63 + 4, 2^64 + 3 -> 3
    tx, _ = R.affine_txty([0, 0, 2 ** 63 - 1, 0, 0, 0], 1, 1)
    assert tx[0, 0] == -2 ** 31                                                    # U + 2^12 wraps to the most negative values


# 9.
def test_the_table_makers():
    size = (37, 23)
    for m in ([[0.8125, -0.40625, 3.5], [0.40625, 0.8125, -2.25]], [[1 + 3 / Q, 5 / Q, -7 / Q], [-11 / Q, 1 - 9 / Q, 13 / Q]], [[-3.7, 0, 40.5], [0, 3.7, -3]]):
        tab = aefft.affine_table(m, size)
        assert tab.dtype == np.int32 and tab.shape == (23, 37, 2) and tab.flags.c_contiguous
        tx, ty = R.affine_txty(R.affine_make(m), *size)
        assert np.array_equal(tab[..., 0], tx) and np.array_equal(tab[..., 1], ty)
    # an affine homography, wherever m * 2^24 is exact (and 2048 u is a whole number or far from a tie: both round alike)
    for m in ([[0.8125, -0.40625, 3.5], [0.40625, 0.8125, -2.25]], [[1 + 3 / Q, 5 / Q, -7 / Q], [-11 / Q, 1 - 9 / Q, 13 / Q]]):
        assert np.array_equal(aefft.homography_table(m + [[0, 0, 1]], size), aefft.affine_table(m, size))
        assert np.array_equal(aefft.homography_table((4 * np.array(m + [[0, 0, 1]])).tolist(), size), aefft.affine_table(m, size))    # (a homography has no scale)
    # a non-positive denominator: INT32_MIN for both entries
    tab = aefft.homography_table([[1, 0, 0], [0, 1, 0], [-0.125, 0, 1]], (12, 3))
    assert (tab[:, 8:] == -2 ** 31).all() and (tab[:, :8] > -2 ** 31).all() and tab[1, 4].tolist() == [2048 * 8, 2048 * 2]
    # the lens: zero distortion and new_K == K is the identity table, exactly
    K = [[811.3, 0, 19.7], [0, 803.9, 11.2], [0, 0, 1]]
    y, x = np.meshgrid(np.arange(23), np.arange(37), indexing="ij")
    assert np.array_equal(aefft.undistort_table(K, (0, 0, 0, 0, 0), size), np.stack([2048 * x, 2048 * y], -1))
    assert np.array_equal(aefft.undistort_table(K, (0, 0, 0, 0), size, new_K=K), np.stack([2048 * x, 2048 * y], -1))
    # k1 != 0 (and the other terms): a handful of pixels against a scalar evaluation in Python floats, within one unit of 2^-11 -- the two
    # evaluations may round the last ulp differently, and one unit is the most a flipped rint can give
    Kb = [[40.0, 0, 18.2], [0, 38.5, 11.4], [0, 0, 1]]
    Kn = [[36.0, 0, 18.0], [0, 36.0, 11.0], [0, 0, 1]]
    for dist in ((-0.21, 0, 0, 0, 0), (0.17, -0.05, 0.002, -0.003, 0.01)):
        tab = aefft.undistort_table(Kb, dist, size, new_K=Kn)
        k1, k2, p1, p2, k3 = dist
        for (px, py) in ((0, 0), (36, 22), (18, 11), (5, 20), (30, 2), (36, 0)):
            xn, yn = (px - 18.0) / 36.0, (py - 11.0) / 36.0
            r2 = xn * xn + yn * yn
            c = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            u = 40.0 * (xn * c + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)) + 18.2
            v = 38.5 * (yn * c + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn) + 11.4
            assert abs(int(tab[py, px, 0]) - 2048.0 * u) <= 1.0 and abs(int(tab[py, px, 1]) - 2048.0 * v) <= 1.0, (dist, px, py)
        assert not np.array_equal(tab, aefft.undistort_table(Kb, (0, 0, 0, 0, 0), size, new_K=Kn))
    for bad in (dict(K=np.zeros((2, 3))), dict(dist=(1, 2, 3)), dict(size=(0, 4)), dict(K=[[0, 0, 1], [0, 1, 1], [0, 0, 1]]), dict(dist=(float("nan"), 0, 0, 0))):
        with pytest.raises(ValueError):
            aefft.undistort_table(**dict(dict(K=K, dist=(0, 0, 0, 0), size=size), **bad))
    for bad in (np.zeros((2, 3)), [[1, 0, 0], [0, 1, 0], [0, 0, float("inf")]]):
        with pytest.raises(ValueError):
            aefft.homography_table(bad, size)
    with pytest.raises(ValueError):
        aefft.affine_table([[[1, 0, 0], [0, 1, 0]]] * 2, size)


# 10.
def test_warp_kernels_use_no_scratch_and_are_the_launched_ones():
    """build/warp_kernels.rsrc: the two kernels at D = 1..4, nothing else, each with zero scratch and zero spills"""
    got = A.instantiations("warp_kernels.rsrc", r"\d+(warp_affine_kernel)ILi(\d)EEEvNS_6WpArgsE", r"\d+(warp_remap_kernel)ILi(\d)EEEvNS_6WpArgsE")
    assert got == [{("warp_%s_kernel" % n, str(D)) for D in (1, 2, 3, 4)} for n in ("affine", "remap")]
    for name, (_, ints) in A.rsrc("warp_kernels.rsrc").items():
        assert ints["VGPRs"] <= 128, (name, ints)                                # (four waves a SIMD at the least)
    src = open(os.path.join(CSRC, "warp_kernels.hip")).read()
    assert sorted(set(re.findall(r"warp_(\w+)_kernel<(\d)><<<", src))) == sorted((n, str(D)) for n in ("affine", "remap") for D in (1, 2, 3, 4))
    assert "warp_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read().split("SRCS =")[1].split("\n")[0]
    internal = open(os.path.join(CSRC, "internal.h")).read()
    for fn in ("hipError_t launch_image_warp_affine(", "hipError_t launch_image_remap("):
        assert fn in internal, fn
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"internal.h"}
    code = re.sub(r"//[^\n]*", "", src)                                          # (without the comments)
    assert "atomic" not in code and "__shared__" not in code and "__syncthreads" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert "#ifndef AEFFT_HOSTCHECK" in src and "#define WP_HD __device__ __forceinline__" in src


# 11.
def test_host_check_builds_and_its_quick_form_passes(tmp_path):
    """tools/warp_hostcheck.cpp: the kernel file compiled for the host under -fsanitize=address,undefined, a program of its own (never loaded into
    Python), every buffer at its exact extent, against its own scalar C restatement; the quick form is a thinned sweep, the full one is run by hand"""
    src = A.host_check_stands_alone("warp_hostcheck.cpp", "warp_kernels.hip")
    for body in ("affine", "remap"):
        assert re.search(r"warp_%s_body<\d>\(" % body, src), body
    assert "hipcc" not in src and "LD_PRELOAD" not in src and "int main(int argc" in src and "wp_geometry(" in src and "wp_remap_split(" in src
    assert os.path.exists(os.path.join(ROOT, "tools", "warp_bench.py"))
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):  # the product never imports the restatement
        for f in files:
            if f.endswith(".py"):
                assert "warp_ref" not in open(os.path.join(dirpath, f)).read(), f
    exe = str(tmp_path / "warp_hostcheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(ROOT, "tools", "warp_hostcheck.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    print(r.stdout[-500:])
    assert r.returncode == 0 and re.search(r"all \d+ runs exact", r.stdout), (r.stdout[-2000:], r.stderr[-2000:])
