"""aefft_net_score_target, aefft_net_score_map_target and aefft_net_ssim_map at the boundary (no GPU): declared, exported and prototyped; the
wrappers' signatures; the argument error that needs no device; the header's text; the development-switch tables unchanged; the two SSIM
kernels and every SSIM instantiation of the two inverse row kernels in the back end's resource tables (no scratch, no spills), the same size /
thread-class set as the mapping ones."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
aefft = importlib.import_module("autoencoder-fft_amd")
NFLAGS = 26      # AEFFT_F_* switches of the library

# name: the leading words of every argument in the header, the ctypes prototype
CALLS = {
    "aefft_net_score_target": (["aefft_net*", "const void*", "int", "const void*", "int", "float*", "float*"],
                               [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aefft_net_score_map_target": (["aefft_net*", "const void*", "int", "const void*", "int", "int", "float*", "float*", "float*"],
                                   [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aefft_net_ssim_map": (["aefft_net*", "const void*", "int", "const void*", "int", "int", "float", "float*", "float*", "float*"],
                           [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
}


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
    for name, (words, proto) in CALLS.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, f"include/aefft.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(words), (name, args)
        for a, w in zip(args, words):
            assert a.startswith(w) and (w.endswith("*") or not a.startswith(w + "*")), (name, a, w)
        assert any(l.split()[-1] == name and " T " in l for l in out.splitlines()), name
        res, argt = aefft.SIGNATURES[name]
        assert res is C.c_int and list(argt) == proto, name          # (device float* travels as void*, as in every entry of the table)
    # the plain calls keep theirs
    assert len(aefft.SIGNATURES["aefft_net_score"][1]) == 5 and len(aefft.SIGNATURES["aefft_net_score_map"][1]) == 7


def test_wrapper_signatures():
    E = inspect.Parameter.empty
    want = {
        "score_target": [("frames", E), ("targets", E), ("score", None), ("recon", None)],
        "score_map_target": [("frames", E), ("targets", E), ("tile", E), ("map", None), ("score", None), ("recon", None)],
        "ssim_map": [("frames", E), ("tile", E), ("targets", None), ("data_range", 255.0), ("map", None), ("score", None), ("recon", None)],
        "score": [("frames", E), ("score", None), ("recon", None)],
        "score_map": [("frames", E), ("tile", E), ("map", None), ("score", None), ("recon", None)],
    }
    for fn, args in want.items():
        p = inspect.signature(getattr(aefft.Net, fn)).parameters
        assert list(p) == ["self"] + [a for a, _ in args], fn
        for a, d in args:
            assert p[a].default is d or p[a].default == d, (fn, a)


def test_null_net_is_einval_without_a_device():
    L = _lib()
    buf = (C.c_float * 64)()
    einval = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", _header()).group(1))
    v = C.cast(buf, C.c_void_p)
    assert L.aefft_net_score_target(None, v, 0, v, 0, v, v) == einval
    assert L.aefft_net_score_target(None, None, 1, None, 1, None, None) == einval
    assert L.aefft_net_score_map_target(None, v, 0, v, 0, 8, v, v, v) == einval
    assert L.aefft_net_score_map_target(None, None, 1, None, 0, 0, None, None, None) == einval
    assert L.aefft_net_ssim_map(None, v, 0, v, 0, 8, 255.0, v, v, v) == einval
    assert L.aefft_net_ssim_map(None, None, 1, None, 0, 0, 0.0, None, None, None) == einval


def test_header_describes_the_calls():
    h = _header()
    doc = h[h.index("against a TARGET"):h.index("int aefft_net_score_target")]
    for word in ("aefft_net_step_grad_target", "t_b[d][i][j]", "the net still reads frames_d", "each on its own", "the bits of the plain calls",
                 "no new kernel", "bit for bit undisturbed", "float targets only", "10 log10(L^2 / score_d[b])", "AEFFT_EINVAL", "misaligned targets_d"):
        assert word in doc, word
    doc = h[h.index("Block SSIM of the reconstruction"):h.index("int aefft_net_ssim_map")]
    for word in ("targets_d == NULL", "ROUNDED", "8, 16, 32, 64", "divide both Nx", "data_range > 0", "255 for 8-bit", "uniform weights", "population statistics",
                 "mx = sum x / n", "vx = max(sum x^2 / n - mx^2, 0)", "c = sum x r / n - mx mr", "C1 = (0.01 L)^2", "C2 = (0.03 L)^2",
                 "(2 mx mr + C1)(2 c + C2) / ((mx^2 + mr^2 + C1)(vx + vr + C2))", "map_d[b][I][J]", "mean over d < D", "a function of the map",
                 "bit for bit what aefft_net_infer writes", "x' = x - L/2", "do not depend on it", "ssim_finish_kernel", "no atomics",
                 "does not depend on the other frames", "aefft_net_step_form", "five launches", "six with score_d", "AEFFT_ESTATE",
                 "stream capture", "AEFFT_F_CHIRPZ", "they need recon_d", "AEFFT_EINVAL", "16-byte aligned", "not finite"):
        assert word in doc, word
    # aefft_net_step_grad_target's list of what is not offered no longer names the score calls
    tgt = h[h.index("Not offered: targets for"):h.index("int aefft_net_step_grad_target")]
    assert "aefft_net_score / _score_map" not in tgt and "pairs l >= 1" in tgt


def test_flag_tables_are_unchanged():
    """the calls add no development switch and no net option"""
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", _header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if "SSIM" in n or "TARGET" in n]
    opts = re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", _header())
    assert opts == ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]


def test_profiler_id_is_appended():
    L = _lib()
    L.aefft_prof_name.restype = C.c_char_p
    names = [L.aefft_prof_name(k).decode() for k in range(L.aefft_prof_count())]
    assert names[-2:] == ["target", "ssim"], names[-4:]


def _blocks(fn):
    path = os.path.join(ROOT, "autoencoder-fft_amd", "csrc", "build", fn)
    assert os.path.exists(path), f"{path}: the build writes the back end's resource table beside every object (csrc/Makefile)"
    for b in re.split(r"(?=remark: [^\n]*Function Name: )", open(path).read()):
        m = re.search(r"Function Name: (\S+)", b)
        if m:
            yield m.group(1), b


def _no_scratch(name, block):
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        v = re.search(key + r": (\d+)", block)
        assert v and int(v.group(1)) == 0, (name, key)


def _rows(sc):
    """the instantiations of the two inverse row kernels whose last template argument is one of `sc`, U8 = false: {file: set of groups}"""
    rows = {}
    for fn, pat in (("fft_kernels.rsrc", r"\d+c2r_rows_kernelILi(\d+)ELb([01])ELb0ELi([%s])EEE" % sc), ("fft_mixed_kernels.rsrc", r"mix_c2r_rows_kernelILi(\d+)ELb0ELi([%s])EEE" % sc)):
        got = set()
        for name, b in _blocks(fn):
            m = re.search(pat, name)
            if m:
                got.add(m.groups())
                _no_scratch(name, b)
        rows[fn] = got
    return rows


def test_ssim_kernels_use_no_scratch():
    """build/<file>.rsrc: ssim_finish_kernel, both ssim_diff_kernel instantiations, and every SSIM instantiation of the two inverse row kernels --
    the last template argument 5 (float reference) or 6 (8-bit reference) -- for exactly the sizes and thread classes of the mapping ones (3, 4)"""
    _lib()
    seen = {"ssim_finish_kernel": 0, "ssim_diff_kernel": 0}
    for name, b in _blocks("ssim_kernels.rsrc"):
        for k in seen:
            if k in name:
                seen[k] += 1
                _no_scratch(name, b)
    assert seen == {"ssim_finish_kernel": 1, "ssim_diff_kernel": 2}, seen
    new, old = _rows("56"), _rows("34")
    sizes = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    want = {(str(n), sp, sc) for n in sizes for sp in "01" for sc in "56" if sp == "0" or n >= 128}
    assert new["fft_kernels.rsrc"] == want, sorted(new["fft_kernels.rsrc"] ^ want)
    assert new["fft_mixed_kernels.rsrc"] == {(str(t), sc) for t in (16, 32, 64, 128, 256) for sc in "56"}, sorted(new["fft_mixed_kernels.rsrc"])
    shift = {"3": "5", "4": "6"}
    for fn in new:
        assert {g[:-1] + (shift[g[-1]],) for g in old[fn]} == new[fn], fn
    # nothing beyond 6
    assert not any(_rows("789")[fn] for fn in new)
