"""aefft_net_score_target, aefft_net_score_map_target and aefft_net_ssim_map at the boundary (no GPU): declared, exported and prototyped; the
wrappers' signatures; the argument error that needs no device; the header's text; the development-switch tables unchanged; the two SSIM
kernels and every SSIM instantiation of the two inverse row kernels in the back end's resource tables (no scratch, no spills), the same size /
thread-class set as the mapping ones."""
import ctypes as C
import inspect

import abi_checks as A
from abi_checks import aefft

# name: the argument list of include/aefft.h
_TARGETS = ["aefft_net* net", "const void* frames_d", "int frames_u8", "const void* targets_d", "int targets_u8"]
CALLS = {
    "aefft_net_score_target": _TARGETS + ["float* score_d", "float* recon_d"],
    "aefft_net_score_map_target": _TARGETS + ["int tile", "float* map_d", "float* score_d", "float* recon_d"],
    "aefft_net_ssim_map": _TARGETS + ["int tile", "float data_range", "float* map_d", "float* score_d", "float* recon_d"],
}


def test_declared_exported_and_prototyped():
    for name, args in CALLS.items():
        A.check_call(name, args)
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
    L = A.lib()
    buf = (C.c_float * 64)()
    v = C.cast(buf, C.c_void_p)
    assert L.aefft_net_score_target(None, v, 0, v, 0, v, v) == A.EINVAL
    assert L.aefft_net_score_target(None, None, 1, None, 1, None, None) == A.EINVAL
    assert L.aefft_net_score_map_target(None, v, 0, v, 0, 8, v, v, v) == A.EINVAL
    assert L.aefft_net_score_map_target(None, None, 1, None, 0, 0, None, None, None) == A.EINVAL
    assert L.aefft_net_ssim_map(None, v, 0, v, 0, 8, 255.0, v, v, v) == A.EINVAL
    assert L.aefft_net_ssim_map(None, None, 1, None, 0, 0, 0.0, None, None, None) == A.EINVAL


def test_header_describes_the_calls():
    doc = A.doc("against a TARGET", "int aefft_net_score_target")
    for word in ("aefft_net_step_grad_target", "t_b[d][i][j]", "the net still reads frames_d", "each on its own", "the bits of the plain calls",
                 "no new kernel", "bit for bit undisturbed", "float targets only", "10 log10(L^2 / score_d[b])", "AEFFT_EINVAL", "misaligned targets_d"):
        assert word in doc, word
    doc = A.doc("Block SSIM of the reconstruction", "int aefft_net_ssim_map")
    for word in ("targets_d == NULL", "ROUNDED", "8, 16, 32, 64", "divide both Nx", "data_range > 0", "255 for 8-bit", "uniform weights", "population statistics",
                 "mx = sum x / n", "vx = max(sum x^2 / n - mx^2, 0)", "c = sum x r / n - mx mr", "C1 = (0.01 L)^2", "C2 = (0.03 L)^2",
                 "(2 mx mr + C1)(2 c + C2) / ((mx^2 + mr^2 + C1)(vx + vr + C2))", "map_d[b][I][J]", "mean over d < D", "a function of the map",
                 "bit for bit what aefft_net_infer writes", "x' = x - L/2", "do not depend on it", "ssim_finish_kernel", "no atomics",
                 "does not depend on the other frames", "aefft_net_step_form", "five launches", "six with score_d", "AEFFT_ESTATE",
                 "stream capture", "AEFFT_F_CHIRPZ", "they need recon_d", "AEFFT_EINVAL", "16-byte aligned", "not finite"):
        assert word in doc, word
    # aefft_net_step_grad_target's list of what is not offered no longer names the score calls
    tgt = A.doc("Not offered: targets for", "int aefft_net_step_grad_target")
    assert "aefft_net_score / _score_map" not in tgt and "pairs l >= 1" in tgt


def test_flag_tables_are_unchanged():
    """the calls add no development switch and no net option"""
    A.tables_unchanged("SSIM", "TARGET")


def test_profiler_id_is_appended():
    A.tables_unchanged("SSIM", "TARGET", profiler=())


def test_ssim_kernels_use_no_scratch():
    """build/<file>.rsrc: ssim_finish_kernel, both ssim_diff_kernel instantiations, and every SSIM instantiation of the two inverse row kernels --
    the last template argument 5 (float reference) or 6 (8-bit reference) -- for exactly the sizes and thread classes of the mapping ones (3, 4)"""
    finish, diff = A.instantiations("ssim_kernels.rsrc", r"(\S*ssim_finish_kernel\S*)", r"(\S*ssim_diff_kernel\S*)", every=False)
    assert (len(finish), len(diff)) == (1, 2), (finish, diff)
    new, old = A.scoring_rows("56"), A.scoring_rows("34")
    sizes = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    want = {(str(n), sp, sc) for n in sizes for sp in "01" for sc in "56" if sp == "0" or n >= 128}
    assert new["fft_kernels.rsrc"] == want, sorted(new["fft_kernels.rsrc"] ^ want)
    assert new["fft_mixed_kernels.rsrc"] == {(str(t), sc) for t in (16, 32, 64, 128, 256) for sc in "56"}, sorted(new["fft_mixed_kernels.rsrc"])
    shift = {"3": "5", "4": "6"}
    for fn in new:
        assert {g[:-1] + (shift[g[-1]],) for g in old[fn]} == new[fn], fn
    # nothing beyond 6
    assert not any(A.scoring_rows("789")[fn] for fn in new)
