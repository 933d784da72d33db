"""aefft_net_step_grad_target at the boundary (no GPU): declared, exported and prototyped; Net.step_grad_target's signature; the argument
error that needs no device; the development-switch tables unchanged; the eight instantiations of the two target kernels in the back end's
resource table (no scratch, no spills)."""
import ctypes as C
import inspect

import abi_checks as A
from abi_checks import aefft


def test_declared_exported_and_prototyped():
    A.check_call("aefft_net_step_grad_target", ["aefft_net* net", "const void* frames_d", "int frames_u8", "const void* targets_d", "int targets_u8",
                                                "float* recon_d"])


def test_net_step_grad_target_signature():
    p = inspect.signature(aefft.Net.step_grad_target).parameters
    assert list(p) == ["self", "frames", "targets", "recon"]
    assert p["frames"].default is inspect.Parameter.empty and p["targets"].default is inspect.Parameter.empty and p["recon"].default is None


def test_null_net_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_float * 64)()
    vp = C.cast(buf, C.c_void_p)
    assert L.aefft_net_step_grad_target(None, vp, 0, vp, 0, C.cast(buf, C.POINTER(C.c_float))) == A.EINVAL
    assert L.aefft_net_step_grad_target(None, None, 1, None, 1, None) == A.EINVAL


def test_header_describes_the_call():
    doc = A.doc("Training toward a TARGET frame", "int aefft_net_step_grad_target")
    for word in (":395-475", "fft_backproplib.cu:1381-1463", "autoencoder.cpp:126-127,192-193", "PAIR 0", "pool_fft(fft(target_b), s_0)", "expout = in",
                 "mse_fft(T, O')", "aefft_net_last_mse", "mse_d = NULL", "a plain aefft_net_step_grad clears it", "aefft_net_step_form",
                 "aefft_net_set_input_ready(1)", "never prefetched", "stream capture", "allocate nothing", "no atomics", "AEFFT_EINVAL",
                 "16-byte aligned", "spatial net", "D > 4", "DESIGN.md section 18"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    A.tables_unchanged("TARGET")


def test_target_kernels_use_no_scratch():
    """build/target_kernels.rsrc: target_terms_kernel<D> and target_mse_kernel<D>, D = 1..4 -- eight kernels, zero scratch, zero spills"""
    [seen] = A.instantiations("target_kernels.rsrc", r"(target_terms_kernel|target_mse_kernel)ILi(\d)EEE", every=False)
    assert seen == {(k, d) for k in ("target_terms_kernel", "target_mse_kernel") for d in "1234"}, sorted(seen)
