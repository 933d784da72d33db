"""aefft_net_step_grad_target at the boundary (no GPU): declared, exported and prototyped; Net.step_grad_target's signature; the argument
error that needs no device; the development-switch tables unchanged; the eight instantiations of the two target kernels in the back end's
resource table (no scratch, no spills)."""
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
    m = re.search(r"int\s+aefft_net_step_grad_target\s*\(([^)]*)\)", txt)
    assert m, "include/aefft.h does not declare aefft_net_step_grad_target"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6
    assert args[0].startswith("aefft_net*") and args[1].startswith("const void*") and args[2].startswith("int")
    assert args[3].startswith("const void*") and args[4].startswith("int") and args[5].startswith("float*")
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", aefft.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-1] == "aefft_net_step_grad_target" and " T " in l for l in out.splitlines())
    res, argt = aefft.SIGNATURES["aefft_net_step_grad_target"]
    assert res is C.c_int and len(argt) == 6
    assert argt[0] is C.c_void_p and argt[1] is C.c_void_p and argt[2] is C.c_int and argt[3] is C.c_void_p and argt[4] is C.c_int
    assert argt[5] is C.c_void_p          # (device float* travels as void*, as in every entry of the table)


def test_net_step_grad_target_signature():
    p = inspect.signature(aefft.Net.step_grad_target).parameters
    assert list(p) == ["self", "frames", "targets", "recon"]
    assert p["frames"].default is inspect.Parameter.empty and p["targets"].default is inspect.Parameter.empty and p["recon"].default is None


def test_null_net_is_einval_without_a_device():
    L = _lib()
    buf = (C.c_float * 64)()
    einval = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", _header()).group(1))
    vp = C.cast(buf, C.c_void_p)
    assert L.aefft_net_step_grad_target(None, vp, 0, vp, 0, C.cast(buf, C.POINTER(C.c_float))) == einval
    assert L.aefft_net_step_grad_target(None, None, 1, None, 1, None) == einval


def test_header_describes_the_call():
    h = _header()
    doc = h[h.index("Training toward a TARGET frame"):h.index("int aefft_net_step_grad_target")]
    for word in (":395-475", "fft_backproplib.cu:1381-1463", "autoencoder.cpp:126-127,192-193", "PAIR 0", "pool_fft(fft(target_b), s_0)", "expout = in",
                 "mse_fft(T, O')", "aefft_net_last_mse", "mse_d = NULL", "a plain aefft_net_step_grad clears it", "aefft_net_step_form",
                 "aefft_net_set_input_ready(1)", "never prefetched", "stream capture", "allocate nothing", "no atomics", "AEFFT_EINVAL",
                 "16-byte aligned", "spatial net", "D > 4", "DESIGN.md section 18"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", _header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if "TARGET" in n]
    opts = re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", _header())
    assert opts == ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]


def _blocks(fn):
    path = os.path.join(ROOT, "autoencoder-fft_amd", "csrc", "build", fn)
    assert os.path.exists(path), f"{path}: the build writes the back end's resource table beside every object (csrc/Makefile)"
    for b in re.split(r"(?=remark: [^\n]*Function Name: )", open(path).read()):
        m = re.search(r"Function Name: (\S+)", b)
        if m:
            yield m.group(1), b


def test_target_kernels_use_no_scratch():
    """build/target_kernels.rsrc: target_terms_kernel<D> and target_mse_kernel<D>, D = 1..4 -- eight kernels, zero scratch, zero spills"""
    _lib()
    seen = set()
    for name, b in _blocks("target_kernels.rsrc"):
        m = re.search(r"(target_terms_kernel|target_mse_kernel)ILi(\d)EEE", name)
        if not m:
            continue
        seen.add((m.group(1), int(m.group(2))))
        for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
            v = re.search(key + r": (\d+)", b)
            assert v and int(v.group(1)) == 0, (name, key)
    assert seen == {(k, d) for k in ("target_terms_kernel", "target_mse_kernel") for d in (1, 2, 3, 4)}, sorted(seen)
