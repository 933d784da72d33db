"""AEFFT_NET_SMOOTH_OPFORM at the boundary (no GPU): the header's value, the Python constant and Net's keyword, and the exported symbol
set of libaefft.so -- the option adds no entry point."""
import inspect
import re

import abi_checks as A
from abi_checks import aefft


def test_header_declares_the_option_as_bit_2():
    m = re.search(r"AEFFT_NET_SMOOTH_OPFORM\s*=\s*1u\s*<<\s*(\d+)", A.header())
    assert m and int(m.group(1)) == 2
    # in the option enum of aefft_net_create_ex, next to its neighbours
    enum = re.search(r"enum\s*\{([^}]*AEFFT_NET_SMOOTH_SIZES[^}]*)\}", A.header()).group(1)
    assert "AEFFT_NET_SMOOTH_OPFORM" in enum and "AEFFT_NET_SPATIAL" in enum


def test_python_constant_and_keyword():
    assert aefft.NET_SMOOTH_OPFORM == 1 << 2
    assert aefft.NET_SMOOTH_OPFORM not in (aefft.NET_SMOOTH_SIZES, aefft.NET_SPATIAL)
    p = inspect.signature(aefft.Net.__init__).parameters
    assert "operator_form" in p and p["operator_form"].default is False
    assert p["smooth_sizes"].default is False


def test_exported_symbols_are_the_declared_ones():
    """every aefft_* symbol libaefft.so exports is one include/aefft.h declares, and the reverse: the option came without an entry point"""
    declared = set(re.findall(r"\b(aefft_[a-z0-9_]+)\s*\(", A.header_code()))
    exported = {n for n in A.exported() if n.startswith("aefft_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert exported == set(aefft.SIGNATURES)
    assert not [n for n in exported if "opform" in n]
