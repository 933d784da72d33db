"""What the no-GPU boundary tests share (test_abi.py and the test_*_abi.py files), each once: the header's text, the build-on-demand loader, the
exported symbols, a call's prototype against the header, the export table and the ctypes table, the pinned switch / option / profiler tables, the
back end's per-kernel resource tables (csrc/build/*.rsrc) and the assertions on a stand-alone host-check source.  A plain module -- pytest
collects nothing from it.  What belongs to one call (its prototype, the header's phrases, the expected instantiations, its argument sweeps) stays
in that call's file."""
import ctypes as C
import functools
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autoencoder-fft_amd", "csrc")
aefft = importlib.import_module("autoencoder-fft_amd")

NFLAGS = 27      # AEFFT_F_* switches of the library: a new one is one edit in include/aefft.h, one in aefft.FLAGS and this one
NET_OPTIONS = ["AEFFT_NET_SMOOTH_SIZES", "AEFFT_NET_SPATIAL", "AEFFT_NET_SMOOTH_OPFORM"]
PROFILER_TAIL = ["target", "ssim"]
# C argument type -> ctypes type of the binding's table (a device pointer travels as void*, as in every entry of aefft.SIGNATURES)
CTYPES = dict({t: C.c_void_p for t in ("aefft_ctx*", "aefft_net*", "const void*", "void*", "const float*", "float*", "const unsigned char*", "unsigned char*")},
              **{"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong})


# ------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def header(name="aefft.h"):
    return open(os.path.join(ROOT, "include", name)).read()


@functools.lru_cache(None)
def header_code(name="aefft.h"):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", header(name), flags=re.S)


def doc(start, end, margin=True):
    """the header's text from `start` up to `end`; margin=False: without the comment's ` * ` margin and its line breaks"""
    h = header()
    text = h[h.index(start):h.index(end)]
    return text if margin else " ".join(re.sub(r"\n \* ?", "\n", text).split())


def in_order(text, *markers):
    at = [text.index(m) for m in markers]
    assert all(a < b for a, b in zip(at, at[1:])), list(zip(markers, at))


EINVAL = int(re.search(r"AEFFT_EINVAL\s*=\s*(-?\d+)", header()).group(1))


def prototype(name):
    """the declared arguments of `int name(...)`, each as "type name" with single blanks"""
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header_code())
    assert m, f"include/aefft.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def struct_fields(name):
    """the declarations of `typedef struct { ... } name;`, in order"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, header_code())
    assert m, name
    return [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]


# ------------------------------------------------------------------------------------------
# the library
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def lib():
    if not os.path.exists(aefft.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return aefft.lib()


@functools.lru_cache(None)
def exported(path=aefft.LIB_PATH):
    """the symbols a shared library defines in its text"""
    lib()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return frozenset(l.split()[-1] for l in out.splitlines() if " T " in l)


def check_call(name, args, structs={}):
    """`name` is declared with exactly these "type name" arguments, exported, and prototyped in aefft.SIGNATURES with an int result and the ctypes
    type of every argument; structs: {C type of a pointer-to-struct argument: its ctypes.Structure}"""
    assert prototype(name) == args, (name, prototype(name))
    assert name in exported(), name
    res, argt = aefft.SIGNATURES[name]
    assert res is C.c_int and len(argt) == len(args), name
    for t, a in zip(argt, args):
        typ = a.rsplit(" ", 1)[0]
        if typ in structs:
            assert t._type_ is structs[typ], (name, a)
        else:
            assert t is CTYPES[typ], (name, a)


def tables_unchanged(*words, profiler=None):
    """the development switches and the net options are the ones the library has, and no switch name holds one of `words`; with `profiler` (a
    tuple of words, maybe empty) the profiling ids end as they did and no id holds one of those.  Returns (switch names, profiling ids or None)."""
    bits = dict((n, int(b)) for n, b in re.findall(r"\b(AEFFT_F_[A-Z0-9]+)\s*=\s*1\s*<<\s*(\d+)", header()))
    assert len(bits) == NFLAGS and len(set(bits.values())) == NFLAGS
    assert not [n for n in bits if any(w in n for w in words)]
    assert re.findall(r"\b(AEFFT_NET_[A-Z_]+)\s*=\s*1u\s*<<\s*\d+", header()) == NET_OPTIONS
    if profiler is None:
        return list(bits), None
    L = lib()
    names = [L.aefft_prof_name(k).decode() for k in range(L.aefft_prof_count())]
    assert names[-2:] == PROFILER_TAIL, names[-4:]
    assert not [n for n in names if any(w in n for w in profiler)]
    return list(bits), names


# ------------------------------------------------------------------------------------------
# the back end's resource tables
# ------------------------------------------------------------------------------------------
RSRC_INTS = {"ScratchSize": r"ScratchSize \[bytes/lane\]", "SGPRs Spill": "SGPRs Spill", "VGPRs Spill": "VGPRs Spill", "VGPRs": " VGPRs"}


@functools.lru_cache(None)
def rsrc(file):
    """build/<file>: {kernel's mangled name: (its block of the table, {"ScratchSize", "SGPRs Spill", "VGPRs Spill", "VGPRs": int})}"""
    lib()
    path = os.path.join(CSRC, "build", file)
    assert os.path.exists(path), f"{path}: the build writes the back end's resource table beside every object (csrc/Makefile)"
    rows = {}
    for b in re.split(r"(?=remark: [^\n]*Function Name: )", open(path).read()):
        m = re.search(r"Function Name: (\S+)", b)
        if m:
            assert m.group(1) not in rows, m.group(1)
            found = {k: re.search(pat + r": (\d+)", b) for k, pat in RSRC_INTS.items()}
            rows[m.group(1)] = (b, {k: int(v.group(1)) for k, v in found.items() if v})
    return rows


def no_scratch(name, block):
    for key in ("ScratchSize", "SGPRs Spill", "VGPRs Spill"):
        v = re.search(RSRC_INTS[key] + r": (\d+)", block)
        assert v and int(v.group(1)) == 0, (name, key)


def instantiations(file, *patterns, every=True):
    """for each pattern the set of its groups over the kernels of build/<file> whose name it matches, every such kernel with zero scratch and no
    spills; every=True: the file holds no kernel that matches none of the patterns"""
    got = [set() for _ in patterns]
    for name, (block, _) in rsrc(file).items():
        hits = [(g, m) for g, m in zip(got, (re.search(p, name) for p in patterns)) if m]
        assert hits or not every, name
        for g, m in hits:
            g.add(m.groups())
            no_scratch(name, block)
    return got


def scoring_rows(sc):
    """the instantiations of the two inverse row kernels whose last template argument is one of `sc`, U8 = false: {file: set of groups}"""
    return {fn: instantiations(fn, pat % sc, every=False)[0] for fn, pat in (
        ("fft_kernels.rsrc", r"\d+c2r_rows_kernelILi(\d+)ELb([01])ELb0ELi([%s])EEE"), ("fft_mixed_kernels.rsrc", r"mix_c2r_rows_kernelILi(\d+)ELb0ELi([%s])EEE"))}


# ------------------------------------------------------------------------------------------
# the host-check programs
# ------------------------------------------------------------------------------------------
def host_check_stands_alone(tool, kernel_file):
    """tools/<tool> includes the kernel file by path behind tools/hostlanes.h, has a main of its own and takes nothing from HIP or Python; returns
    its text"""
    path = os.path.join(ROOT, "tools", tool)
    assert os.path.exists(path)
    src = open(path).read()
    assert '#include "../autoencoder-fft_amd/csrc/%s"' % kernel_file in src and "int main(" in src and "-fsanitize=address,undefined" in src
    assert "Python.h" not in src and "hip_runtime" not in src
    lanes = open(os.path.join(ROOT, "tools", "hostlanes.h")).read()
    assert '#include "hostlanes.h"' in src and "#define AEFFT_HOSTCHECK" in lanes
    assert "Python.h" not in lanes and "hip_runtime" not in lanes and "LD_PRELOAD" not in lanes
    return src
