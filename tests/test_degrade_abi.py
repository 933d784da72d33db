"""aefft_frames_degrade at the boundary (no GPU): declared in the image-boundary block behind aefft_map_overlay_image, exported and prototyped; the
header's statement of the rules; every instantiation of the kernel in the back end's resource table (no scratch, no spills); the argument error
that needs no device; the Python layout rules; the host check program; and the definition itself on the numpy restatement of degrade_ref.py --
Philox's published known answers and the statistics of the noise and the impulses, every bound derived from the sample count."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import abi_checks as A
import degrade_ref as R
from abi_checks import CSRC, ROOT, aefft

NAME = "aefft_frames_degrade"
ARGS = ["aefft_ctx* ctx", "const void* src_d", "int src_u8", "void* dst_d", "int dst_u8", "int B", "int D", "int Nx", "int Ny", "int blur", "float sigma", "float impulse",
        "unsigned long long seed", "unsigned long long first_frame"]


# 1.
def test_declared_exported_and_prototyped():
    A.check_call(NAME, ARGS)
    p = inspect.signature(aefft.Context.frames_degrade).parameters
    assert list(p) == ["self", "frames", "blur", "sigma", "impulse", "seed", "first_frame", "out", "dtype"]
    assert p["frames"].default is inspect.Parameter.empty
    assert [p[n].default for n in list(p)[2:]] == [0, 0.0, 0.0, 0, 0, None, None]


# 2.
def test_the_call_stands_behind_map_overlay_in_the_image_boundary_block():
    A.in_order(A.header(), "int aefft_map_overlay_image(", "/* aefft_frames_degrade", "int aefft_frames_degrade(", "/* ---- network level")


# 3.
def test_header_states_the_rules():
    doc = A.doc("/* aefft_frames_degrade", "int aefft_frames_degrade(")
    for word in ("[B][D][Nx][Ny]", "16-byte aligned", "D in 1..4", "1..8192", "odd sizes included", "B >= 1",
                 # 1.
                 "px_u8(src[b][d][i][j])", "NaN -> 0", "clamp to 0..255", "halves away from zero", "first turned into pixels",
                 # 2.
                 "blur = r in 0..4", "w_k = C(2r, k)", "sum 4^r", "edges replicated", "h[i][j] = sum_k w_k p[clamp(i+k-r)][j]",
                 "v[i][j] = sum_l w_l h[i][clamp(j+l-r)]", "255 * 16^r < 2^24", "u = v << (16 - 4r)", "no rounding anywhere", "u = p << 16",
                 # 3.
                 "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "seed low word, seed high word", "n = (d Nx + i) Ny + j",
                 "g = first_frame + b", "(n >> 1, 0, g low word, g high word)", "one call serves two elements", "(a, c) = (x0, x1)", "(x2, x3)",
                 "T = (sum of the four bytes of a) + (sum of the two low bytes of c) - 765", "hsel = c >> 16",
                 # 4.
                 "m = floor(((double)sigma * 65536.0) / sqrt(32767.5) + 0.5)", "u += T * m", "Irwin-Hall", "zero mean", "sqrt(32767.5) exactly",
                 "excess kurtosis -0.2", "+-4.23", "APPROXIMATELY", "not normal", "m sqrt(32767.5) / 65536", "1/362", "|u| < 2^27",
                 # 5.
                 "t = floor((double)impulse * 65536.0 + 0.5)", "hsel < t", "u = 255 << 16 when", "a & 1", "1/65536", "impulse = 1 replaces every element",
                 # 6.
                 "clamp((u + 32768) >> 16, 0, 255)", "arithmetic shift", "(float)u * 2^-16", "nearest even", "not clamped", "clips as a sensor does",
                 # consequences, in place, launch, errors
                 "is a copy for 8-bit -> 8-bit", "px_u8 for float -> 8-bit", "exact conversion", "depends only on (seed, first_frame + b)",
                 "degrade(B = 2, first_frame = f)[1] == degrade(B = 1, first_frame = f + 1)[0]", "first_frame = step * global_batch + rank * B",
                 "constant", "same arguments always give the same bytes", "dst_d == src_d is allowed exactly when blur == 0 and src_u8 == dst_u8",
                 "element-wise", "any other overlap", "One launch", "no host synchronisation", "no allocation", "no workspace", "stream capture",
                 "profile id `image`", "bytes read plus the bytes written", "AEFFT_EINVAL", '"aefft_frames_degrade: "', "nothing enqueued",
                 "outputs untouched", "blur outside 0..4", "sigma not finite, negative or above 255", "impulse not finite or outside", "not 16-byte aligned",
                 "overflow the address space"):
        assert word in doc, word


# 4.
def test_degrade_kernels_use_no_scratch_and_cover_every_instantiation():
    """build/degrade_kernels.rsrc: degrade_kernel<R, SF32, DF32, WORDS> for R = 0..4 x {8-bit, float} source x {8-bit, float} destination x
    {elements, dwords} -- what the launcher selects -- nothing else, each with zero scratch and zero spills"""
    [got] = A.instantiations("degrade_kernels.rsrc", r"\d+degrade_kernelILi(\d)ELb([01])ELb([01])ELb([01])EEE")
    assert got == {(r, s, d, w) for r in "01234" for s in "01" for d in "01" for w in "01"}
    assert "degrade_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # the launcher is declared with the others, the entry point stands with the image calls and shares their helpers
    assert "hipError_t launch_degrade(" in open(os.path.join(CSRC, "internal.h")).read()
    ops = open(os.path.join(CSRC, "image_ops.hip")).read()
    entry = ops[ops.index('extern "C" int aefft_frames_degrade('):]
    assert ops.index("// image boundary") < ops.index('extern "C" int aefft_map_overlay_image(') < ops.index('extern "C" int aefft_frames_degrade(')
    assert "ranges_overlap(" in entry and "aligned16(" in entry and "KID_IMAGE" in entry and ops.count("static bool ranges_overlap(") == 1
    rest = open(os.path.join(CSRC, "ops.hip")).read()
    assert "aefft_image_" not in rest and "KID_IMAGE" not in rest


# 5.
def test_null_context_is_einval_without_a_device():
    L = A.lib()
    buf = (C.c_ubyte * 2048)()
    base = C.addressof(buf)
    base += -base % 16
    src, dst = C.c_void_p(base), C.c_void_p(base + 1024)
    for su8, du8 in ((1, 1), (0, 1), (1, 0), (0, 0)):
        assert L.aefft_frames_degrade(None, src, su8, dst, du8, 1, 3, 4, 4, 2, 25.0, 0.02, 7, 0) == A.EINVAL
    assert L.aefft_frames_degrade(None, src, 1, src, 1, 1, 3, 4, 4, 0, 25.0, 0.02, 7, 0) == A.EINVAL
    assert L.aefft_frames_degrade(None, None, 0, None, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0) == A.EINVAL
    assert bytes(buf) == bytes(2048)


# 6.
def test_python_layout_rules_need_no_device():
    """the checks of Context.frames_degrade run before anything reaches the library: CPU tensors suffice"""
    fn = aefft._frames_degrade_args
    frames = torch.zeros(2, 3, 8, 6, dtype=torch.uint8)
    good = dict(frames=frames, blur=0, sigma=0.0, impulse=0.0, seed=0, first_frame=0, out=None, dtype=None)
    assert fn(**good) == (0, 0.0, 0.0, 0, 0, torch.uint8)
    assert fn(frames.float(), 4, 255, 1, 2 ** 64 - 1, 2 ** 64 - 1, None, None) == (4, 255.0, 1.0, 2 ** 64 - 1, 2 ** 64 - 1, torch.float32)
    assert fn(frames, 2, 25.0, 0.02, 7, 5, None, torch.float32)[-1] == torch.float32
    assert fn(frames, 2, 25.0, 0.02, 7, 5, torch.zeros(2, 3, 8, 6), None)[-1] == torch.float32
    assert fn(frames, 0, 25.0, 0.02, 7, 5, frames, None)[-1] == torch.uint8                      # in place
    assert fn(frames, np.int64(1), np.float32(1.5), 0, np.int64(3), 0, None, None)[:2] == (1, 1.5)
    for bad in (dict(frames=frames.double()), dict(frames=frames[0]), dict(frames=frames.permute(0, 1, 3, 2)), dict(frames=torch.zeros(1, 5, 4, 4)),
                dict(frames=torch.zeros(1, 3, 0, 4)), dict(blur=5), dict(blur=-1), dict(blur=1.5), dict(blur=True), dict(sigma=-1.0), dict(sigma=255.5),
                dict(sigma=float("nan")), dict(sigma=float("inf")), dict(impulse=-0.1), dict(impulse=1.01), dict(impulse=float("nan")), dict(seed=-1),
                dict(seed=2 ** 64), dict(seed=0.5), dict(first_frame=-1), dict(first_frame=2 ** 64), dict(dtype=torch.float64), dict(dtype=torch.int8),
                dict(out=torch.zeros(2, 3, 8, 7, dtype=torch.uint8)), dict(out=torch.zeros(2, 3, 6, 8, dtype=torch.uint8).permute(0, 1, 3, 2)),
                dict(out=torch.zeros(2, 3, 8, 6, dtype=torch.float64)), dict(out=torch.zeros(2, 3, 8, 6), dtype=torch.uint8),
                dict(out=frames, blur=1), dict(out=frames.view(torch.int8))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            fn(**kw)


# 7.
def test_the_host_check_program_is_there_and_stands_alone():
    A.host_check_stands_alone("degrade_hostcheck.cpp", "degrade_kernels.hip")
    # the product never imports the restatement
    for dirpath, _, files in os.walk(os.path.join(ROOT, "autoencoder-fft_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "degrade_ref" not in open(os.path.join(dirpath, f)).read(), f


# 8.
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))],
    ids=["zeros", "ones", "pi"])
def test_the_restatement_reproduces_philox_known_answers(counter, key, want):
    assert tuple(int(v) for v in R.philox4x32(counter, key)) == want


# 9.
SHAPE = (4, 3, 128, 128)
N = int(np.prod(SHAPE))


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_the_noise_of_the_definition_has_the_stated_statistics():
    """sigma = 10, seed = 2024 on a constant 128 frame, float out: the bounds are five standard errors of each estimate at N = 196608 samples.
    The variance estimate of a distribution of kurtosis 3 - 0.2 has relative standard error sqrt((kurtosis - 1) / N) = sqrt(1.8 / N), the standard
    deviation half of it; a correlation estimate over n pairs 1 / sqrt(n)."""
    assert N == 196608
    noise = R.degrade(np.full(SHAPE, 128, np.uint8), sigma=10.0, seed=2024, dtype=np.float32).astype(np.float64) - 128.0
    se = R.sigma_eff(10.0)
    assert abs(se - 10.0) < 10.0 / 362
    mean, std = noise.mean(), noise.std()
    c_frames, c_neigh = _corr(noise[0].ravel(), noise[1].ravel()), _corr(noise[..., :-1].ravel(), noise[..., 1:].ravel())
    peak = np.abs(noise).max() / se
    z = noise / std
    print(f"mean {mean:.4f} (bound {5 * se / np.sqrt(N):.4f}); std {std:.4f} against {se:.4f}: relative {std / se - 1:.5f} (bound {5 * np.sqrt(1.8 / (4 * N)):.5f}); "
          f"frame correlation {c_frames:.5f}, neighbour correlation {c_neigh:.5f} (bound {5 / np.sqrt(N / 4):.5f}); kurtosis {(z ** 4).mean():.3f}; peak {peak:.3f} sigma")
    assert abs(mean) <= 5 * se / np.sqrt(N)
    assert abs(std / se - 1) <= 5 * np.sqrt(1.8 / (4 * N))
    assert abs(c_frames) <= 5 / np.sqrt(N / 4) and abs(c_neigh) <= 5 / np.sqrt(N / 4)
    assert peak <= 4.23
    assert 765 / R.SIGMA_T < 4.23 and 766 / R.SIGMA_T > 4.23                     # the bound itself: |T| <= 765


def test_the_impulses_of_the_definition_have_the_stated_statistics():
    src = np.full(SHAPE, 128, np.uint8)
    every = R.degrade(src, impulse=1.0, seed=7)
    assert set(np.unique(every)) == {0, 255}
    share = (every == 255).mean()
    print(f"impulse = 1: share of 255 {share:.5f} (bound {5 * 0.5 / np.sqrt(N):.5f} off 1/2)")
    assert abs(share - 0.5) <= 5 * 0.5 / np.sqrt(N)
    some = R.degrade(src, impulse=0.05, seed=7)
    hits = some != 128
    assert set(np.unique(some)) == {0, 128, 255}
    rate, salt = hits.mean(), (some[hits] == 255).mean()
    print(f"impulse = 0.05: hit rate {rate:.5f} (bound {5 * np.sqrt(0.05 * 0.95 / N):.5f} off 0.05); salt share {salt:.4f} (bound {5 * 0.5 / np.sqrt(hits.sum()):.4f} off 1/2)")
    assert abs(rate - 0.05) <= 5 * np.sqrt(0.05 * 0.95 / N)
    assert abs(salt - 0.5) <= 5 * 0.5 / np.sqrt(hits.sum())


def test_the_identities_of_the_definition_hold_on_the_restatement():
    rng = np.random.default_rng(3)
    f8 = rng.integers(0, 256, (2, 3, 10, 6), dtype=np.uint8)
    assert np.array_equal(R.degrade(f8), f8) and np.array_equal(R.degrade(f8, dtype=np.float32), f8.astype(np.float32))
    two = R.degrade(f8, 2, 25.0, 0.02, seed=9, first_frame=2 ** 32 - 1)
    assert np.array_equal(two[1:], R.degrade(f8[1:], 2, 25.0, 0.02, seed=9, first_frame=2 ** 32))
    for r in range(5):
        assert (R.degrade(np.full((1, 2, 9, 7), 77, np.uint8), r) == 77).all()
    delta = np.zeros((1, 1, 17, 17), np.uint8)
    delta[0, 0, 8, 8] = 255
    w = R.weights(4)
    want = np.zeros((17, 17))
    want[4:13, 4:13] = 255 * np.outer(w, w) / 65536
    assert np.array_equal(R.degrade(delta, 4, dtype=np.float32)[0, 0], want.astype(np.float32))
