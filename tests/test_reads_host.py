"""The .bps / .arw read side, host part (no GPU): dx_reads_unpack and dx_reads_uncompress -- Load_Read / Load_Subread /
Load_Arrow (DB.c:1232-1381, 1508-1548) for a selection at once -- are declared, exported and bound, refuse a NULL context,
and Context.reads_uncompress refuses a selection that does not fit its reads before anything reaches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_reads_unpack", "dx_reads_uncompress"]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("reads_unpack", "reads_uncompress"):
        assert callable(getattr(api.Context, m))
    assert L.DX_LETTERS_NUMBERS == 3


def test_no_context_is_an_argument_error():
    lib = L.load()
    out, n, toff, bad = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    boff, rlen = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    assert lib.dx_reads_uncompress(None, L.DX_LETTERS_NUMBERS, b"\x1b", 1, boff.ctypes.data, rlen.ctypes.data, None, None, None, 1,
                                   C.byref(out), C.byref(n), C.byref(toff)) == -1
    assert lib.dx_reads_unpack(None, L.DX_LETTERS_NUMBERS, None, 0, None, None, None, 0, None, None, C.byref(bad)) == -1
    assert lib.dx_reads_unpack(None, L.DX_LETTERS_NUMBERS, None, 0, None, None, None, 1, None, None, None) == -1


class _NoDevice(api.Context):
    """A context that was never opened: whatever reaches its library handle fails the test."""

    def __init__(self):
        self.h = None

    @property
    def lib(self):
        raise AssertionError("the selection reached the library")


BOFF, RLEN = np.array([0, 3, 5], np.uint64), np.array([10, 7, 0], np.uint32)


@pytest.mark.parametrize("kw,exc", [
    (dict(ids=[0, 1], beg=[0, 0], end=[10, 8]), ValueError),       # end > rlen
    (dict(beg=[0, 0, 0], end=[10, 7, 1]), ValueError),             # ... of an empty read
    (dict(ids=[1], beg=[5], end=[4]), ValueError),                 # beg > end
    (dict(ids=[0, 3]), IndexError),                                # an id beyond rlen
    (dict(ids=[0], beg=[1]), ValueError),                          # beg without end
    (dict(ids=[0, 1], beg=[1], end=[2]), ValueError),              # not one pair a selected read
    (dict(ids=[0], beg=[-1], end=[2]), ValueError),
], ids=["end_gt_rlen", "end_gt_rlen_empty", "beg_gt_end", "id_beyond", "beg_alone", "too_few_pairs", "negative"])
def test_selection_is_checked_before_any_device_call(kw, exc):
    with pytest.raises(exc):
        _NoDevice().reads_uncompress(b"\x00" * 8, BOFF, RLEN, **kw)


def test_fewer_offsets_than_lengths():
    with pytest.raises(IndexError):
        _NoDevice().reads_uncompress(b"\x00" * 8, BOFF[:2], RLEN)


def test_a_good_selection_passes_the_checks():
    boff, rlen, ids, beg, end, n = api.Context._reads_selection(BOFF, RLEN, [2, 0, 0], [0, 3, 10], [0, 10, 10])
    assert n == 3 and ids.dtype == np.uint64 and beg.dtype == np.uint32 and end.tolist() == [0, 10, 10]
    assert api.Context._reads_selection(BOFF, RLEN, None, None, None)[2:] == (None, None, None, 3)
