"""dx_file_compare's host side (no GPU): the three new entry points are declared, exported and bound; and the oracle of the GPU tests
-- tests/_diff.py, numpy on two texts or on two packed buffers -- is valid on its own: it finds in the reference's own lossless and
lossy images of one .quiva what was counted from their texts by hand, and nothing between the key and byte-order variants of one
.dexta."""
import ctypes as C
import os
import re

import numpy as np

import _diff as D
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_diff_ranges", "dx_code_diff", "dx_file_compare"]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("diff_ranges", "code_diff", "compare"):
        assert callable(getattr(api.Context, m))
    assert C.sizeof(L.DiffTally) == 32 and C.sizeof(L.Compare) == 16 + 8 * 8 + 8 + 4 * 5 * 8


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    cm, first, bad, tot = L.Compare(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 2)()
    assert lib.dx_file_compare(None, L.DX_KIND_FASTA, img, len(img), img, len(img), 0, C.byref(cm), None) == -1
    assert lib.dx_diff_ranges(None, None, 0, None, None, 0, None, None, None, 1, None, 0, None, None, None, C.byref(first), C.byref(bad)) == -1
    assert lib.dx_code_diff(None, None, 0, None, None, 0, None, None, 0, None, None, C.byref(tot), C.byref(first), C.byref(bad)) == -1


def test_the_report_finds_what_dexqv_l_does_to_the_golden():
    """qv_full.dexqv and qv_lossy.dexqv are the real reference's images of one .quiva, without and with -l"""
    full, lossy = O.undexqv(O.golden("qv_full.dexqv")), O.undexqv(O.golden("qv_lossy.dexqv"))
    r = D.report("quiva", full, lossy)
    assert (r["records_a"], r["records_b"], r["lines"]) == (24, 24, 5)
    assert sum(len(rec[2][0]) for rec in D.records("quiva", full)) == 235179
    assert (r["headers_differ"], r["first_header"], r["lengths_differ"], r["prefix_differs"]) == (0, None, 0, False)
    assert list(r["differ"]) == [0, 0, 134598, 183845, 0]
    assert list(r["sum_abs"]) == [0, 0, 134598, 356544, 0]
    assert list(r["max_abs"]) == [0, 0, 1, 3, 0]
    assert r["records_differ"] == 24 and list(r["line_records"]) == [0, 0, 24, 24, 0] and not r["same"]
    assert r["first_record"] == 0 and r["first_line"] == 2
    assert int(r["rec_differ"].sum()) == 134598 + 183845 and (r["rec_differ"][:, [0, 1, 4]] == 0).all()
    m = D.report("quiva", full, lossy, lossy=True)                 # with 0xFE / 0xFC on side a: b is what -l keeps of a
    assert m["same"] and int(m["differ"].sum()) == 0 and m["records_differ"] == 0 and m["first_record"] is None
    assert not D.report("quiva", lossy, full, lossy=True)["same"]  # (the other way round it is not)
    assert D.report("quiva", full, full)["same"]


def test_the_packed_reference_sees_no_difference_between_the_variants_of_one_dexta():
    base = O.golden("ta_small.dexta")
    off, ln = D.packed_reads(base)
    assert len(ln) > 1 and int(ln.sum()) == sum(len(r[2][0]) for r in D.records("fasta", O.golden("ta_small.fasta")))
    for v in ("legacy", "swapped", "legacy_swapped"):
        img = O.golden(f"ta_small.{v}.dexta")
        voff, vln = D.packed_reads(img)
        assert np.array_equal(vln, ln), v
        r = D.code_diff(base, off, img, voff, ln)
        assert (r["symbols"], r["units"], r["first"]) == (0, 0, None), v
    hurt = bytearray(base)
    hurt[int(off[1])] ^= 0x0C                                     # the third symbol of read 1
    r = D.code_diff(base, off, bytes(hurt), off, ln)
    assert (r["symbols"], r["units"], r["first"]) == (1, 1, (1, 2)) and r["rec_differ"][1] == 1


def test_pad_bits_differ_and_are_not_counted():
    """a read of 4 k + r symbols ends in a byte of which only the top 2 r bits are symbols: the rest may hold anything"""
    rng = np.random.default_rng(3)
    for n in range(1, 14):
        a = bytearray(rng.integers(0, 256, (n + 3) // 4 + 1, dtype=np.uint8).tobytes())
        b = bytearray(a)
        pad = (1 << (8 - 2 * (n & 3))) - 1 if n & 3 else 0
        b[(n + 3) // 4 - 1] ^= pad                                # every pad bit of the last byte,
        b[(n + 3) // 4] ^= 0xFF                                   # ... and the byte behind the read
        assert (bytes(a) != bytes(b))
        r = D.code_diff(a, [0], b, [0], [n])
        assert (r["symbols"], r["first"]) == (0, None), n
        if n & 3:
            b[(n + 3) // 4 - 1] ^= pad + 1                        # the lowest bit that IS a symbol's: the last symbol
            assert D.code_diff(a, [0], b, [0], [n])["first"] == (0, n - 1), n


def test_diff_ranges_reference_on_a_case_done_by_hand():
    a, b = bytes([10, 20, 31, 40, 50, 61]), bytes([10, 21, 30, 40, 90, 60])
    r = D.diff_ranges(a, [0, 3], b, [0, 3], [3, 3], kind=[0, 1], nkinds=2)
    assert list(r["rec_differ"]) == [2, 2] and list(r["rec_first"]) == [1, 1] and r["first"] == (0, 1)
    assert list(r["differ"]) == [2, 2] and list(r["units"]) == [1, 1] and list(r["sum_abs"]) == [2, 41] and list(r["max_abs"]) == [1, 40]
    r = D.diff_ranges(a, [0, 3], b, [0, 3], [3, 3], kind=[0, 1], nkinds=2, a_and=[0xFE, 0xFF])       # 31 & 0xFE = 30
    assert list(r["rec_differ"]) == [1, 2] and list(r["sum_abs"]) == [1, 41]
