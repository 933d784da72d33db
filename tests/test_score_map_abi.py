"""aefft_net_score_map at the boundary (no GPU): declared, exported and prototyped; Net.score_map's signature; the argument error that needs
no device; the development-switch tables unchanged; the two map kernels and every mapping instantiation of the two inverse row kernels in
the back end's resource tables (no scratch, no spills), the same size / thread-class set as the scoring ones."""
import ctypes as C
import inspect

import abi_checks as A
from abi_checks import aefft


def test_declared_exported_and_prototyped():
    A.check_call("aefft_net_score_map", ["aefft_net* net", "const void* frames_d", "int frames_u8", "int tile", "float* map_d", "float* score_d",
                                         "float* recon_d"])


def test_net_score_map_signature():
    p = inspect.signature(aefft.Net.score_map).parameters
    assert list(p) == ["self", "frames", "tile", "map", "score", "recon"]
    assert p["frames"].default is inspect.Parameter.empty and p["tile"].default is inspect.Parameter.empty
    assert p["map"].default is None and p["score"].default is None and p["recon"].default is None


def test_null_net_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_float * 64)()
    fp = C.cast(buf, C.POINTER(C.c_float))
    assert L.aefft_net_score_map(None, C.cast(buf, C.c_void_p), 0, 8, fp, fp, fp) == A.EINVAL
    assert L.aefft_net_score_map(None, None, 1, 0, None, None, None) == A.EINVAL


def test_header_describes_the_call():
    doc = A.doc("Per-tile reconstruction error", "int aefft_net_score_map")
    for word in ("map_d[b][I][J]", "(D t t)", "ROUNDED", "8, 16, 32, 64", "divide both Nx", "NOT bit for bit", "a function of the map",
                 "bit for bit what aefft_net_infer writes", "aefft_net_step_form", "aefft_net_step_grad", "AEFFT_ESTATE", "no atomics",
                 "does not depend on the other frames", "AEFFT_F_CHIRPZ", "AEFFT_EINVAL", "16-byte aligned", "no allocation", "five launches"):
        assert word in doc, word


def test_flag_tables_are_unchanged():
    """the call adds no development switch and no net option"""
    A.tables_unchanged("SCORE", "MAP")


def test_score_map_kernels_use_no_scratch():
    """build/<file>.rsrc: score_map_finish_kernel, both score_map_diff_kernel instantiations, and every mapping instantiation of the two inverse
    row kernels -- the last template argument 3 (float frames) or 4 (8-bit frames) -- for exactly the sizes and thread classes of the scoring
    ones (1, 2): there is no template axis over the tile"""
    finish, diff = A.instantiations("score_map_kernels.rsrc", r"(\S*score_map_finish_kernel\S*)", r"(\S*score_map_diff_kernel\S*)", every=False)
    assert (len(finish), len(diff)) == (1, 2), (finish, diff)
    new, old = A.scoring_rows("34"), A.scoring_rows("12")
    sizes = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    want = {(str(n), sp, sc) for n in sizes for sp in "01" for sc in "34" if sp == "0" or n >= 128}
    assert new["fft_kernels.rsrc"] == want, sorted(new["fft_kernels.rsrc"] ^ want)
    assert new["fft_mixed_kernels.rsrc"] == {(str(t), sc) for t in (16, 32, 64, 128, 256) for sc in "34"}, sorted(new["fft_mixed_kernels.rsrc"])
    shift = {"1": "3", "2": "4"}
    for fn in new:
        assert {g[:-1] + (shift[g[-1]],) for g in old[fn]} == new[fn], fn
