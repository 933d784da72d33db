"""aefft_net_infer at the boundary (no GPU): declared, exported and prototyped; Net.infer's signature; the argument errors that need no
device; the development-switch tables unchanged; the new row-pass instantiations in the back end's resource tables (no scratch)."""
import ctypes as C
import inspect
import os

import abi_checks as A
from abi_checks import ROOT, aefft


def test_declared_exported_and_prototyped():
    A.check_call("aefft_net_infer", ["aefft_net* net", "const void* frames_d", "int frames_u8", "void* recon_d", "int recon_u8", "int hidden_pair",
                                     "float* hidden_d"])


def test_net_infer_signature():
    p = inspect.signature(aefft.Net.infer).parameters
    assert list(p) == ["self", "frames", "recon", "hidden_pair", "hidden"]
    assert p["recon"].default is None and p["hidden_pair"].default is None and p["hidden"].default is None


def test_null_net_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_float * 64)()
    assert L.aefft_net_infer(None, C.cast(buf, C.c_void_p), 0, C.cast(buf, C.c_void_p), 0, 0, None) == A.EINVAL
    assert L.aefft_net_infer(None, None, 1, None, 1, -1, None) == A.EINVAL


def test_header_describes_the_call_and_the_u8_sizes():
    doc = A.doc("Frozen-weight inference", "int aefft_net_infer")
    for word in ("SpinToImage_C", "aefft_net_step_form", "aefft_net_set_pair", "aefft_net_step_apply", "AEFFT_EINVAL", "16-byte aligned"):
        assert word in doc, word
    u8 = A.doc("The same calls on 8-BIT frames", "int aefft_net_step_grad_u8")
    assert "Power-of-two frame\n * sizes" not in u8 and "smooth sizes" in u8


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option: the header's AEFFT_F_* bits and the aefft_net_create_ex options are the ones
    the library had, and Context.set_flags takes every switch by name"""
    src = open(os.path.join(ROOT, "autoencoder-fft_amd", "__init__.py")).read()
    for n in A.tables_unchanged("INFER", "U8")[0]:
        assert n[len("AEFFT_F_"):] in src, n


def test_new_row_pass_instantiations_use_no_scratch():
    """build/<file>.rsrc (the back end's resource table): every 8-bit-output row kernel is there, with zero scratch and no spills"""
    [dense] = A.instantiations("fft_kernels.rsrc", r"(\S*c2r_rows_kernelILi\d+ELb[01]ELb1E\S*)", every=False)
    [mixed] = A.instantiations("fft_mixed_kernels.rsrc", r"(\S*mix_c2r_rows_kernelILi\d+ELb1E\S*)", every=False)
    assert len(dense) + len(mixed) == 14 + 5, (sorted(dense), sorted(mixed))
