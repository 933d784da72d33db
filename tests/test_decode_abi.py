"""aefft_net_decode at the boundary (no GPU): declared, exported and prototyped; Net.decode's signature; the argument error that needs no
device; the development-switch tables unchanged; the two decode kernels in the back end's resource tables (no scratch, no spills)."""
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
    m = re.search(r"int\s+aefft_net_decode\s*\(([^)]*)\)", txt)
    assert m, "include/aefft.h does not declare aefft_net_decode"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 5
    assert args[0].startswith("aefft_net*") and args[1].startswith("int") and args[2].startswith("const float*")
    assert args[3].startswith("void*") and args[4].startswith("int")
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", aefft.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == "aefft_net_decode" and " T " in l for l in out.splitlines())
    res, argt = aefft.SIGNATURES["aefft_net_decode"]
    assert res is C.c_int and len(argt) == 5
    assert [argt[i] for i in (1, 4)] == [C.c_int] * 2


def test_net_decode_signature():
    p = inspect.signature(aefft.Net.decode).parameters
    assert list(p) == ["self", "code", "hidden_pair", "recon"]
    assert all(v.default is inspect.Parameter.empty for v in p.values())


def test_null_net_is_einval_without_a_device():
    L = _lib()
    buf = (C.c_float * 64)()
    einval = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", _header()).group(1))
    assert L.aefft_net_decode(None, 0, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), 0) == einval
    assert L.aefft_net_decode(None, -1, None, None, 1) == einval


def test_header_describes_the_call():
    h = _header()
    doc = h[h.index("Decode: the reconstruction from a STORED hidden layer"):h.index("int aefft_net_decode")]
    for word in ("autoenc_fft", "fft_backproplib.cu:1331-1376", "aefft_net_step_form", "aefft_net_set_pair", "aefft_net_load_spectra",
                 "aefft_net_step_apply", "aefft_net_train_pair", "AEFFT_ESTATE", "AEFFT_EINVAL", "16-byte aligned", "SpinToImage_C"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", _header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if "DECODE" in n]
    opts = re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", _header())
    assert opts == ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]


def test_decode_kernels_use_no_scratch():
    """build/<file>.rsrc (the back end's resource table): decode_op_kernel and every decode_apply_kernel instantiation, with zero scratch and
    no spills"""
    _lib()
    build = os.path.join(ROOT, "autoencoder-fft_amd", "csrc", "build")
    seen = {"decode_op_kernel": 0, "decode_apply_kernel": 0}
    for fn in ("decode_kernels.rsrc", "opform_kernels.rsrc"):
        path = os.path.join(build, fn)
        if not os.path.exists(path):
            continue
        for b in re.split(r"(?=remark: [^\n]*Function Name: )", open(path).read()):
            m = re.search(r"Function Name: (\S+)", b)
            if not m:
                continue
            for k in seen:
                if k in m.group(1):
                    seen[k] += 1
                    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
                        v = re.search(key + r": (\d+)", b)
                        assert v and int(v.group(1)) == 0, (m.group(1), key)
    assert seen["decode_op_kernel"] >= 1 and seen["decode_apply_kernel"] >= 1, seen
