"""aefft_net_score_map at the boundary (no GPU): declared, exported and prototyped; Net.score_map's signature; the argument error that needs
no device; the development-switch tables unchanged; the two map kernels and every mapping instantiation of the two inverse row kernels in
the back end's resource tables (no scratch, no spills), the same size / thread-class set as the scoring ones."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
aefft = importlib.import_module("autoencoder-fft_amd")
NFLAGS = 26      # AEFFT_F_* switches of the library


def _header():
    return open(os.path.join(ROOT, "include", "aefft.h")).read()


def _lib():
    if not os.path.exists(aefft.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return aefft.lib()


def test_declared_exported_and_prototyped():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"int\s+aefft_net_score_map\s*\(([^)]*)\)", txt)
    assert m, "include/aefft.h does not declare aefft_net_score_map"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[0].startswith("aefft_net*") and args[1].startswith("const void*") and args[2].startswith("int") and args[3].startswith("int")
    assert args[4].startswith("float*") and args[5].startswith("float*") and args[6].startswith("float*")
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", aefft.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == "aefft_net_score_map" and " T " in l for l in out.splitlines())
    res, argt = aefft.SIGNATURES["aefft_net_score_map"]
    assert res is C.c_int and len(argt) == 7
    assert argt[0] is C.c_void_p and argt[1] is C.c_void_p and argt[2] is C.c_int and argt[3] is C.c_int
    assert all(t is C.c_void_p for t in argt[4:])          # (device float* travels as void*, as in every entry of the table)


def test_net_score_map_signature():
    p = inspect.signature(aefft.Net.score_map).parameters
    assert list(p) == ["self", "frames", "tile", "map", "score", "recon"]
    assert p["frames"].default is inspect.Parameter.empty and p["tile"].default is inspect.Parameter.empty
    assert p["map"].default is None and p["score"].default is None and p["recon"].default is None


def test_null_net_is_einval_without_a_device():
    L = _lib()
    buf = (C.c_float * 64)()
    einval = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", _header()).group(1))
    fp = C.cast(buf, C.POINTER(C.c_float))
    assert L.aefft_net_score_map(None, C.cast(buf, C.c_void_p), 0, 8, fp, fp, fp) == einval
    assert L.aefft_net_score_map(None, None, 1, 0, None, None, None) == einval


def test_header_describes_the_call():
    h = _header()
    doc = h[h.index("Per-tile reconstruction error"):h.index("int aefft_net_score_map")]
    for word in ("map_d[b][I][J]", "(D t t)", "ROUNDED", "8, 16, 32, 64", "divide both Nx", "NOT bit for bit", "a function of the map",
                 "bit for bit what aefft_net_infer writes", "aefft_net_step_form", "aefft_net_step_grad", "AEFFT_ESTATE", "no atomics",
                 "does not depend on the other frames", "AEFFT_F_CHIRPZ", "AEFFT_EINVAL", "16-byte aligned", "no allocation", "five launches"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", _header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if "SCORE" in n or "MAP" in n]
    opts = re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", _header())
    assert opts == ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]


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


def test_score_map_kernels_use_no_scratch():
    """build/<file>.rsrc: score_map_finish_kernel, both score_map_diff_kernel instantiations, and every mapping instantiation of the two inverse
    row kernels -- the last template argument 3 (float frames) or 4 (8-bit frames) -- for exactly the sizes and thread classes of the scoring
    ones (1, 2): there is no template axis over the tile"""
    _lib()
    seen = {"score_map_finish_kernel": 0, "score_map_diff_kernel": 0}
    for name, b in _blocks("score_map_kernels.rsrc"):
        for k in seen:
            if k in name:
                seen[k] += 1
                _no_scratch(name, b)
    assert seen == {"score_map_finish_kernel": 1, "score_map_diff_kernel": 2}, seen
    new, old = _rows("34"), _rows("12")
    sizes = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    want = {(str(n), sp, sc) for n in sizes for sp in "01" for sc in "34" if sp == "0" or n >= 128}
    assert new["fft_kernels.rsrc"] == want, sorted(new["fft_kernels.rsrc"] ^ want)
    assert new["fft_mixed_kernels.rsrc"] == {(str(t), sc) for t in (16, 32, 64, 128, 256) for sc in "34"}, sorted(new["fft_mixed_kernels.rsrc"])
    shift = {"1": "3", "2": "4"}
    for fn in new:
        assert {g[:-1] + (shift[g[-1]],) for g in old[fn]} == new[fn], fn
