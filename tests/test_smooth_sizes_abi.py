"""CPU-side checks of the smooth-size surface (no compute call is made): libaefft.so exports aefft_net_create_ex, include/aefft.h declares
it and AEFFT_NET_SMOOTH_SIZES, and AEFFT_FLAGS accepts CHIRPZ (the switch back to Bluestein's transforms)."""
import os
import re
import subprocess
import sys

import pytest

import abi_checks as A
from abi_checks import ROOT, aefft


@pytest.fixture(scope="module")
def built():
    return A.lib()


def test_create_ex_exported_and_declared(built):
    assert "aefft_net_create_ex" in A.exported()
    txt = A.header_code()
    assert re.search(r"int\s+aefft_net_create_ex\s*\(\s*aefft_ctx\s*\*\s*\w*\s*,\s*const\s+aefft_net_desc\s*\*\s*\w*\s*,\s*unsigned\s+\w*\s*,\s*aefft_net\s*\*\*", txt)
    m = re.search(r"AEFFT_NET_SMOOTH_SIZES\s*=\s*1u?\s*<<\s*(\d+)", txt)
    assert m and 1 << int(m.group(1)) == aefft.NET_SMOOTH_SIZES
    assert built.aefft_net_create_ex(None, None, aefft.NET_SMOOTH_SIZES, None) == aefft.EINVAL


def test_chirpz_is_a_known_flag_name(built):
    """AEFFT_FLAGS=CHIRPZ is accepted: aefft_ctx_create does not fail with AEFFT_EINVAL (without a device it returns AEFFT_EHIP) and
    nothing names the flag on stderr"""
    assert aefft.FLAGS["CHIRPZ"] == 1 << 24
    code = ("import ctypes as C, importlib, sys; sys.path.insert(0, %r); m = importlib.import_module('autoencoder-fft_amd'); L = m.lib(); "
            "h = C.c_void_p(); print(L.aefft_ctx_create(C.byref(h), 0, None, 1))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, AEFFT_FLAGS="CHIRPZ"))
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) != aefft.EINVAL and "CHIRPZ" not in out.stderr, (out.stdout, out.stderr)
