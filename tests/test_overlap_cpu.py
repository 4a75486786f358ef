"""The refusal of an `out` that overlaps an input (rs_pack_dev, rs_rekey_dev, rs_ring_rekey_dev, rs_ring_cmux_dev,
rs_ring_lookup_dev, rs_ring_selector_dev, rs_circuit_bootstrap_dev) on the CPU: the range arithmetic of the ABI (rs_host.h
first_overlap, which rs_api_client.cpp refuse_overlap reports) through the emulator library, the same decision in the Python
binding, and the documents. The calls themselves are refused on the device in the *_invalid_arguments* tests of the GPU files."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu_lib
from redsec_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 64) - 1


def _first(written, others):
    flat = (C.c_uint64 * (2 * len(others)))(*[v for pair in others for v in pair])
    return emu_lib.lib().rs_emu_first_overlap(written[0], written[1], flat, len(others))


class _Tensor:
    """what backend._refuse_overlap reads of a tensor"""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def test_ranges_that_share_a_byte_and_ranges_that_only_touch():
    out = (4096, 256)
    for other, hit in (((4096, 256), True),          # the same range
                       ((4096 + 255, 64), True),     # begins on out's last byte
                       ((4096 + 256, 64), False),    # begins where out ends
                       ((4096 - 64, 64), False),     # ends where out begins
                       ((4096 - 64, 65), True),      # ends on out's first byte
                       ((4096 + 100, 1), True),      # inside out
                       ((16, 1 << 20), True),        # holds out
                       ((4096, 0), False),           # an empty range
                       ((0, 256), False)):           # a null pointer: rs_ring_cmux_dev's d1, a depth-1 lookup's scratch
        assert (_first(out, [other]) == 0) == hit, other
        assert (_first(other, [out]) == 0) == hit, other
    assert _first((4096, 0), [(4000, 1000)]) == -1 and _first((0, 256), [(0, 256)]) == -1


def test_the_first_overlapping_argument_is_the_one_named_and_inputs_may_overlap_each_other():
    d0, d1, sel = (1000, 300), (1100, 300), (5000, 100)                      # d0 and d1 share 200 bytes: never looked at
    assert _first((2000, 100), [d0, d1, sel]) == -1
    assert _first((1250, 100), [d0, d1, sel]) == 0                          # both: the first is reported
    assert _first((1350, 100), [d0, d1, sel]) == 1
    assert _first((4950, 100), [d0, d1, sel]) == 2
    assert _first((1000, 100), []) == -1


def test_ranges_at_the_top_of_the_address_space_do_not_wrap():
    assert _first((TOP - 99, 100), [(TOP - 9, 10)]) == 0
    assert _first((TOP - 99, 100), [(16, 64)]) == -1                         # address + bytes wraps to 0: no overlap with low memory
    assert _first((16, 64), [(TOP - 99, 100)]) == -1
    assert _first((TOP - 99, 50), [(TOP - 49, 50)]) == -1


def test_the_python_binding_decides_as_the_abi_does():
    """random word ranges: backend._refuse_overlap raises exactly where first_overlap finds one, and names the same argument"""
    rng = np.random.default_rng(4)
    names = ["d0", "d1", "sel"]
    hits = 0
    for _ in range(400):
        start = [int(v) * 4 + 4096 for v in rng.integers(0, 64, 4)]
        words = [int(v) for v in rng.integers(0, 24, 4)]
        others = [(n, _Tensor(a), w) for n, a, w in zip(names, start[1:], words[1:])]
        if rng.integers(0, 4) == 0:
            others[1] = ("d1", None, words[2])                               # a null d1
        want = _first((start[0], 4 * words[0]), [(0, 0) if t is None else (t.data_ptr(), 4 * w) for _, t, w in others])
        if want < 0:
            backend._refuse_overlap("out", _Tensor(start[0]), words[0], others)
        else:
            hits += 1
            with pytest.raises(ValueError, match="out overlaps %s$" % names[want]):
                backend._refuse_overlap("out", _Tensor(start[0]), words[0], others)
    assert 50 < hits < 350


def test_every_call_names_the_refusal_in_the_header_the_source_and_the_guide():
    header = open(os.path.join(ROOT, "include", "redsec_hip.h")).read()
    source = open(os.path.join(ROOT, "redsec_amd", "csrc", "rs_api_client.cpp")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header, integration = (re.sub(r"[\s*]+", " ", text) for text in (header, integration))    # a comment breaks its lines anywhere
    assert "overlaps neither" not in header + integration and "overlaps no input" not in header + integration
    for message in ("rlwe overlaps ct", "out overlaps ct", "out overlaps rlwe", "out overlaps d0", "sel overlaps ct"):
        assert message in header and message in integration, message
    # one helper, called by the seven entry points (the lookup and the composed bootstrap twice: out, then scratch)
    assert source.count("int refuse_overlap(") == 1 and source.count("refuse_overlap(") == 1 + 9
    for name in ('"rlwe"', '"ct"', '"pack_key"', '"rekey_key"', '"ring_key"', '"d0"', '"d1"', '"sel"', '"table"', '"scratch"', '"sel_key"', '"bits"'):
        assert name in source, name
