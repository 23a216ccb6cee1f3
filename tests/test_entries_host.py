"""Records at known starts, host side (no GPU): dx_qv_walk_records -- the segment sizes of a record whose start and
length are known (what Load_QVentry, DB.c:2575-2621, has for a .qvs track) -- against the whole-file walk of the
reference-made .dexqv goldens, whose records are those of a .qvs with framing bytes in front."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["qv_tiny", "qv_mid", "qv_full", "qv_lossy", "qv_nodel", "qv_type2", "qv_runs"]
NEW = ["dx_qv_walk_records", "dx_qv_walk_records_device", "dx_entries_uncompress"]


@functools.lru_cache(maxsize=None)
def golden_walk(name):
    """(image, whole-file walk, coding, start of every record's deletion segment): computed once, never changed"""
    img = O.golden(name + ".dexqv")
    w = api.qv_walk(img)
    assert w["newv"] == 1 and w["flip"] == 0 and w["n"] > 0
    coding = api.qv_read_coding(img[2:])[0]
    start = (w["rec_off"][:-1] + (w["hdr_off"][1:] - w["hdr_off"][:-1])).astype(np.uint64)
    for a in (w["seg"], w["len"], start):
        a.setflags(write=False)
    return img, w, coding, start


def selections(n):
    """(name, indices): file order, reversed, every third entry listed twice"""
    fwd = np.arange(n)
    twice = np.sort(np.concatenate([fwd, fwd[::3]]))
    return [("forward", fwd), ("reversed", fwd[::-1]), ("thirds_twice", twice)]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    assert callable(api.qv_walk_records)
    for m in ("entries_compress", "entries_uncompress", "qv_walk_records_device"):
        assert callable(getattr(api.Context, m))


@pytest.mark.parametrize("name", GOLDENS)
def test_segment_sizes_equal_the_whole_file_walk(name):
    img, w, coding, start = golden_walk(name)
    for what, sel in selections(w["n"]):
        seg = api.qv_walk_records(img, start[sel], w["len"][sel], coding)
        assert seg.dtype == np.uint32 and seg.shape == (len(sel), 5)
        assert (seg == w["seg"][sel]).all(), (name, what, np.nonzero((seg != w["seg"][sel]).any(axis=1))[0][:5])
    # the records tile the image: every start plus its five sizes is the next record's first byte
    assert (start + w["seg"].sum(axis=1, dtype=np.uint64) == w["rec_off"][1:]).all()


@pytest.mark.parametrize("name", GOLDENS)
def test_byte_swapped_stream(name):
    img, w, coding, start = golden_walk(name)
    fl = O.byteswap_dexqv(img, w)
    assert fl != img and len(fl) == len(img)
    for what, sel in selections(w["n"]):
        seg = api.qv_walk_records(fl, start[sel], w["len"][sel], coding, flip=True)
        assert (seg == w["seg"][sel]).all(), (name, what)


@pytest.mark.parametrize("name", GOLDENS)
def test_truncated_buffer_names_the_record(name):
    img, w, coding, start = golden_walk(name)
    n = w["n"]
    last = n - 1
    total = int(w["seg"][last].sum())
    assert w["len"][last] > 0 and total >= 8
    for cut in (int(start[last]) + total // 2, int(start[last]) + total - 1, int(start[last]) + 1):
        buf = img[:cut]
        with pytest.raises(L.DexGPUError) as e:
            api.qv_walk_records(buf, start, w["len"], coding)
        assert e.value.code == -3 and e.value.bad_entry == last, (name, cut)
        # listed first, it is still the one that is named; the entries before it, in a call of their own, are unaffected
        with pytest.raises(L.DexGPUError) as e:
            api.qv_walk_records(buf, start[::-1], w["len"][::-1], coding)
        assert e.value.code == -3 and e.value.bad_entry == 0
        if last:
            seg = api.qv_walk_records(buf, start[:last], w["len"][:last], coding)
            assert (seg == w["seg"][:last]).all()
    # a start behind the buffer's end
    with pytest.raises(L.DexGPUError) as e:
        api.qv_walk_records(img, np.array([start[0], len(img) + 1], np.uint64), w["len"][[0, 0]], coding)
    assert e.value.code == -3 and e.value.bad_entry == 1


def test_empty_entries_and_empty_selection():
    img, w, coding, start = golden_walk("qv_tiny")
    # an entry of no symbols has no words (QV.c:436-442): five zeros, wherever it is said to start -- the buffer's end included
    seg = api.qv_walk_records(img, np.array([start[0], len(img), 0], np.uint64), np.array([w["len"][0], 0, 0], np.uint32), coding)
    assert (seg[0] == w["seg"][0]).all() and not seg[1:].any()
    assert api.qv_walk_records(img, np.zeros(0, np.uint64), np.zeros(0, np.uint32), coding).shape == (0, 5)
    assert api.qv_walk_records(b"", np.zeros(1, np.uint64), np.zeros(1, np.uint32), coding).tolist() == [[0] * 5]
    # NULL arrays with entries to walk are an argument error, not a crash
    bad = C.c_uint64()
    assert L.load().dx_qv_walk_records(img, len(img), None, None, 1, C.byref(coding), 0, None, C.byref(bad)) == -1
