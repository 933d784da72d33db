"""aefft_net_decode at the boundary (no GPU): declared, exported and prototyped; Net.decode's signature; the argument error that needs no
device; the development-switch tables unchanged; the two decode kernels in the back end's resource tables (no scratch, no spills)."""
import ctypes as C
import inspect

import abi_checks as A
from abi_checks import aefft


def test_declared_exported_and_prototyped():
    A.check_call("aefft_net_decode", ["aefft_net* net", "int hidden_pair", "const float* code_d", "void* recon_d", "int recon_u8"])


def test_net_decode_signature():
    p = inspect.signature(aefft.Net.decode).parameters
    assert list(p) == ["self", "code", "hidden_pair", "recon"]
    assert all(v.default is inspect.Parameter.empty for v in p.values())


def test_null_net_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_float * 64)()
    assert L.aefft_net_decode(None, 0, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), 0) == A.EINVAL
    assert L.aefft_net_decode(None, -1, None, None, 1) == A.EINVAL


def test_header_describes_the_call():
    doc = A.doc("Decode: the reconstruction from a STORED hidden layer", "int aefft_net_decode")
    for word in ("autoenc_fft", "fft_backproplib.cu:1331-1376", "aefft_net_step_form", "aefft_net_set_pair", "aefft_net_load_spectra",
                 "aefft_net_step_apply", "aefft_net_train_pair", "AEFFT_ESTATE", "AEFFT_EINVAL", "16-byte aligned", "SpinToImage_C"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    A.tables_unchanged("DECODE")


def test_decode_kernels_use_no_scratch():
    """build/<file>.rsrc (the back end's resource table): decode_op_kernel and every decode_apply_kernel instantiation, with zero scratch and
    no spills"""
    op, apply = set(), set()
    for fn in ("decode_kernels.rsrc", "opform_kernels.rsrc"):
        o, a = A.instantiations(fn, r"(\S*decode_op_kernel\S*)", r"(\S*decode_apply_kernel\S*)", every=False)
        op |= o
        apply |= a
    assert len(op) >= 1 and len(apply) >= 1, (op, apply)
