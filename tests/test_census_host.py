"""The census's host side (no GPU): the C-ABI of dx_code_counts / dx_byte_hist_ranges / dx_census_lengths / dx_file_census, the layout
of dx_census, and dx_census_lengths against a numpy restatement of its definition."""
import ctypes
import os
import re

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dx_code_counts", "dx_byte_hist_ranges", "dx_census_lengths", "dx_file_census")


def header():
    return open(os.path.join(ROOT, "include", "dexgpu.h")).read()


def declared_arguments(hdr, name):
    """how many arguments the header's declaration of `name` has (comments dropped first: they hold commas and semicolons)"""
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m, f"{name} is not declared in dexgpu.h"
    return len(m.group(1).split(","))


def test_abi_has_the_census():
    hdr, lib = header(), L.load()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by libdexgpu.so"
        assert name in L.SIGNATURES
        assert len(L.SIGNATURES[name][1]) == declared_arguments(hdr, name), name
    assert [declared_arguments(hdr, n) for n in NAMES] == [10, 11, 3, 8]
    for name in ("code_counts", "byte_hist_ranges", "census"):
        assert callable(getattr(api.Context, name, None)), name
    assert callable(getattr(api, "census_lengths", None))
    assert "DEXGPU_CENSUS" in open(os.path.join(ROOT, "dextractor_amd", "csrc", "dx_env.h")).read()


def test_census_layout_matches_the_header():
    """dx_census as ctypes sees it: the header's fields in the header's order, two 64-bit counts, four 32-bit words, code[4], hist[5][256]"""
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*dx_census\s*;", header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [re.match(r"\w+", w).group(0) for w in words[1:]]
    assert fields == [f for f, _ in L.Census._fields_] == ["records", "symbols", "min_len", "max_len", "n50", "reserved", "code", "hist"]
    assert ctypes.sizeof(L.Census) == 16 + 16 + 32 + 5 * 256 * 8
    c = L.Census
    assert (c.records.offset, c.symbols.offset, c.min_len.offset, c.max_len.offset, c.n50.offset, c.reserved.offset,
            c.code.offset, c.hist.offset) == (0, 8, 16, 20, 24, 28, 32, 64)
    assert (c.code.size, c.hist.size) == (32, 5 * 256 * 8)


def restated(lengths):
    """the definition, with Python's integers: over the lengths sorted downward, the first at which 2 * running >= total"""
    a = sorted((int(x) for x in lengths), reverse=True)
    total, run, n50 = sum(a), 0, 0
    if total:
        for v in a:
            run += v
            if 2 * run >= total:
                n50 = v
                break
    return {"records": len(a), "symbols": total, "min_len": min(a) if a else 0, "max_len": max(a) if a else 0, "n50": n50}


CASES = {
    "none": [],
    "one_empty": [0],
    "all_empty": [0] * 7,
    "one": [12345],
    "equal": [800] * 33,
    "lognormal": np.random.default_rng(20261019).lognormal(9.0, 0.5, 1000).astype(np.uint32),
    "exactly_half": [10, 4, 3, 2, 1],                      # 10 of 20: the running sum IS half at the first read
    "exactly_half_later": [6, 5, 4, 4, 3],                 # 11 of 22 behind the second
    "just_short_of_half": [9, 5, 3, 2, 1],                 # 9 of 20, then 14
    "near_2_31": [2**31 - 1, 2**31 - 2, 2**31 - 1, 5, 2**31 - 3],
    "near_2_32": [2**32 - 1, 2**32 - 1, 2**32 - 2, 1, 0],
    "one_bucket": [65536 + k for k in range(300)],         # all in one bucket of the first pass
    "bucket_edges": [65535, 65536, 65537, 131071, 131072, 1, 0, 65535],
    "heavy_tail": [1] * 5000 + [3000, 2000],
}


@pytest.mark.parametrize("name", list(CASES))
def test_census_lengths_is_the_definition(name):
    lens = np.asarray(CASES[name], dtype=np.uint32)
    want = restated(lens)
    assert api.census_lengths(lens) == want
    assert api.census_lengths(lens[::-1]) == want                                # (the order does not matter)


def test_census_lengths_hard_cases_are_what_they_claim():
    assert restated(CASES["exactly_half"])["n50"] == 10 and restated(CASES["exactly_half_later"])["n50"] == 5
    assert restated(CASES["just_short_of_half"])["n50"] == 5
    assert restated(CASES["near_2_31"])["symbols"] > 2**32
    assert restated(CASES["none"]) == {"records": 0, "symbols": 0, "min_len": 0, "max_len": 0, "n50": 0}


def test_census_lengths_leaves_the_other_fields_alone():
    cs = L.Census()
    cs.code[2] = 77
    cs.hist[4][255] = 99
    a = np.array([5, 6, 7], np.uint32)
    assert L.load().dx_census_lengths(a.ctypes.data, 3, ctypes.byref(cs)) == 0
    assert (cs.records, cs.symbols, cs.n50, cs.code[2], cs.hist[4][255]) == (3, 18, 6, 77, 99)
    assert L.load().dx_census_lengths(None, 3, ctypes.byref(cs)) == -1
    assert L.load().dx_census_lengths(a.ctypes.data, 3, None) == -1
