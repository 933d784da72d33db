"""CPU-side checks of the spatial net's surface (no compute call is made): include/aefft.h declares AEFFT_NET_SPATIAL, AEFFT_FORM_SPATIAL
and aefft_net_set_inertia, libaefft.so exports the function, and the Python constants match the header."""
import re

import pytest

import abi_checks as A
from abi_checks import aefft


@pytest.fixture(scope="module")
def built():
    return A.lib()


def test_header_declares_the_spatial_net():
    txt = A.header_code()
    m = re.search(r"AEFFT_NET_SPATIAL\s*=\s*1u?\s*<<\s*(\d+)", txt)
    assert m and int(m.group(1)) == 1
    assert 1 << int(m.group(1)) == aefft.NET_SPATIAL
    assert re.search(r"AEFFT_FORM_SPATIAL\s*=\s*3\b", txt)
    assert re.search(r"int\s+aefft_net_set_inertia\s*\(\s*aefft_net\s*\*\s*\w*\s*,\s*float\s+\w*\s*\)\s*;", txt)


def test_set_inertia_exported_and_checks_its_net(built):
    assert "aefft_net_set_inertia" in A.exported()
    assert "aefft_net_set_inertia" in aefft.SIGNATURES
    assert built.aefft_net_set_inertia(None, 0.5) == aefft.EINVAL


def test_create_ex_without_a_descriptor_is_refused_with_the_spatial_bit(built):
    assert built.aefft_net_create_ex(None, None, aefft.NET_SPATIAL, None) == aefft.EINVAL
    assert built.aefft_net_create_ex(None, None, aefft.NET_SPATIAL | aefft.NET_SMOOTH_SIZES, None) == aefft.EINVAL
