"""aefft_net_score at the boundary (no GPU): declared, exported and prototyped; Net.score's signature; the argument error that needs no
device; the development-switch tables unchanged; the two score kernels and every scoring instantiation of the two inverse row kernels in
the back end's resource tables (no scratch, no spills)."""
import ctypes as C
import inspect

import abi_checks as A
from abi_checks import aefft


def test_declared_exported_and_prototyped():
    A.check_call("aefft_net_score", ["aefft_net* net", "const void* frames_d", "int frames_u8", "float* score_d", "float* recon_d"])


def test_net_score_signature():
    p = inspect.signature(aefft.Net.score).parameters
    assert list(p) == ["self", "frames", "score", "recon"]
    assert p["frames"].default is inspect.Parameter.empty and p["score"].default is None and p["recon"].default is None


def test_null_net_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_float * 64)()
    fp = C.cast(buf, C.POINTER(C.c_float))
    assert L.aefft_net_score(None, C.cast(buf, C.c_void_p), 0, fp, fp) == A.EINVAL
    assert L.aefft_net_score(None, None, 1, None, None) == A.EINVAL


def test_header_describes_the_call():
    doc = A.doc("Per-frame reconstruction error", "int aefft_net_score")
    for word in ("autoenc_fft", "fft_backproplib.cu:1331-1376", "Parseval", "mse_fft", ":480-498", ":1178-1192", "2*dM", "ROUNDED", "contracting",
                 "bit for bit what aefft_net_infer writes", "no 8-bit reconstruction", "aefft_net_step_form", "aefft_net_step_grad", "AEFFT_ESTATE",
                 "no atomics", "does not depend on the other frames", "AEFFT_F_CHIRPZ", "AEFFT_EINVAL", "16-byte aligned", "no allocation"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    A.tables_unchanged("SCORE")


def test_score_kernels_use_no_scratch():
    """build/<file>.rsrc (the back end's resource table): score_finish_kernel, both score_diff_kernel instantiations, and every scoring
    instantiation of the two inverse row kernels -- the last template argument (1: float frames, 2: 8-bit frames) behind U8 = false: nine
    dense and five sparse sizes of the power-of-two kernel, five thread classes of the mixed-radix one, each for both frame types"""
    finish, diff = A.instantiations("score_kernels.rsrc", r"(\S*score_finish_kernel\S*)", r"(\S*score_diff_kernel\S*)", every=False)
    assert (len(finish), len(diff)) == (1, 2), (finish, diff)
    rows = A.scoring_rows("12")
    sizes = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    want = {(str(n), sp, sc) for n in sizes for sp in "01" for sc in "12" if sp == "0" or n >= 128}
    assert rows["fft_kernels.rsrc"] == want, sorted(rows["fft_kernels.rsrc"] ^ want)
    assert rows["fft_mixed_kernels.rsrc"] == {(str(t), sc) for t in (16, 32, 64, 128, 256) for sc in "12"}, sorted(rows["fft_mixed_kernels.rsrc"])
