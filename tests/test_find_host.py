"""dx_file_find's host side (no GPU): the two new entry points are declared, exported and bound; calls without a context are argument
errors; and the oracle of the GPU tests -- tests/_find.py, a naive numpy search of the oracle's text -- is valid on its own: it
finds in ta_edge and ta_small what was counted in their texts by hand."""
import ctypes as C
import os
import re

import numpy as np

import _find as F
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_find", "dx_file_find"]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("code_find", "find"):
        assert callable(getattr(api.Context, m))
    assert C.sizeof(L.Query) == 16 and C.sizeof(L.Hit) == 16 and C.sizeof(L.Find) == 4 * 8 + 64 * 2 * 8
    assert api.HIT_DTYPE.itemsize == 16 and api.HIT_DTYPE == F.HIT
    assert [api.HIT_DTYPE.fields[f][1] for f in ("record", "pos", "query", "strand", "mis")] == [0, 8, 12, 14, 15]
    assert [getattr(L.Hit, f).offset for f in ("record", "pos", "query", "strand", "mis")] == [0, 8, 12, 14, 15]


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    q, fd, hits, bad = (L.Query * 1)(L.Query(0, 1, 0)), L.Find(), C.c_uint64(), C.c_uint64()
    pats = (C.c_char_p * 1)(b"ACGT")
    assert lib.dx_code_find(None, None, 0, None, None, None, 0, q, 1, None, None, 0, None, C.byref(hits), C.byref(bad)) == -1
    assert lib.dx_file_find(None, L.DX_KIND_FASTA, img, len(img), pats, 1, 0, 0, 0, C.byref(fd), None, None) == -1


def test_the_reference_kernel_on_a_case_done_by_hand():
    """ACGTACGA, symbols 1 .. 7 of it: CGTACGA.  CG lies at 0 and 4, GT at 1; CA is one mismatch from CG (0, 4), TA (2) and GA (5) and
    two from GT and AC"""
    packed = F.pack([0, 1, 2, 3, 0, 1, 2, 0])
    r = F.code_find(packed, [0], [1], [7], [([1, 2], 0), ([2, 3], 0), ([1, 0], 1)], cap=100)
    assert r["total"].tolist() == [2, 1, 4] and r["hits"] == 7 and r["count"].tolist() == [7]
    assert [tuple(h) for h in r["list"]] == [(0, 0, 0, 0, 0), (0, 0, 2, 0, 1), (0, 1, 1, 0, 0), (0, 2, 2, 0, 1), (0, 4, 0, 0, 0),
                                             (0, 4, 2, 0, 1), (0, 5, 2, 0, 1)]
    assert F.query([1, 2, 3]) == (0b011011, 3, 0)
    assert len(F.code_find(packed, [0], [1], [7], [([1, 0], 1)], cap=3)["list"]) == 3


def test_the_reference_finds_what_was_counted_by_hand_in_ta_edge():
    """ta_edge's reads as undexta -U prints them: ACGTA (the N is stored as a), none, ACGTACG, GT, TTTT, C, AAAAAA (nNaAxX), ACGT x 43
    + G (173), T x 80.
      ACGT: read 0 at 0, read 2 at 0, read 7 at 0, 4 .. 168: 1 + 1 + 43.        TTTT: read 4 once, read 8 at 0 .. 76: 1 + 77.
      AAAA: read 6 at 0, 1, 2.        TACG: read 2 at 3, read 7 at 3, 7 .. 167: 1 + 42.
      CGTA, TACG's reverse complement: read 0 at 1, read 2 at 1, read 7 at 1, 5 .. 165: 1 + 1 + 42.  ACGT is its own."""
    text = F.text_of("fasta", O.golden("ta_edge.dexta"))
    rep, lst = F.file_find("fasta", text, ["ACGT", "TTTT", "AAAA", "tacg"])
    assert (rep["records"], rep["records_hit"], rep["hits"], rep["listed"]) == (9, 6, 169, 169)
    assert rep["per_pattern"].tolist() == [[45, 0], [78, 0], [3, 0], [43, 0]]
    assert rep["rec_hits"].tolist() == [1, 0, 2, 0, 1, 0, 3, 85, 77]
    assert [tuple(h) for h in lst[:6]] == [(0, 0, 0, 0, 0), (2, 0, 0, 0, 0), (2, 3, 3, 0, 0), (4, 0, 1, 0, 0), (6, 0, 2, 0, 0), (6, 1, 2, 0, 0)]
    rep, lst = F.file_find("fasta", text, ["TACG", "ACGT"], both_strands=True)
    assert rep["per_pattern"].tolist() == [[43, 44], [45, 0]] and rep["hits"] == 132 and rep["records_hit"] == 3
    assert [tuple(h) for h in lst[:5]] == [(0, 0, 1, 0, 0), (0, 1, 0, 1, 0), (2, 0, 1, 0, 0), (2, 1, 0, 1, 0), (2, 3, 0, 0, 0)]
    rep, lst = F.file_find("fasta", text, ["ACGTAC"], max_mis=1)      # read 2 once (ACGTAC); read 7 at 0, 4 .. 164 (and ACGTG at the end is too short by one)
    assert rep["per_pattern"].tolist() == [[43, 0]] and rep["rec_hits"][[2, 7]].tolist() == [1, 42]
    rep, lst = F.file_find("fasta", text, ["TTTT"], max_hits=5)
    assert (rep["hits"], rep["listed"], len(lst)) == (78, 5, 5) and [int(h["pos"]) for h in lst] == [0, 0, 1, 2, 3]


def test_the_reference_finds_what_was_counted_by_hand_in_ta_small():
    """counted in ta_small.fasta with a text search, record by record (overlaps included)"""
    text = F.text_of("fasta", O.golden("ta_small.dexta"))
    want = {"GATC": [4, 1, 4, 2, 5, 4, 2, 1, 4, 3, 0, 4], "TTTTCC": [1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0],
            "ACGTT": [0, 0, 0, 0, 2, 0, 2, 1, 1, 1, 0, 1]}
    rep, lst = F.file_find("fasta", text, list(want))
    assert rep["records"] == 12 and rep["hits"] == 34 + 3 + 8 and rep["records_hit"] == 11
    assert rep["per_pattern"][:, 0].tolist() == [34, 3, 8]
    assert rep["rec_hits"].tolist() == [sum(v) for v in zip(*want.values())]
    for p, name in enumerate(want):
        assert np.bincount(lst["record"][lst["query"] == p].astype(np.int64), minlength=12).tolist() == want[name]
    rep, _ = F.file_find("fasta", text, ["GGCC", "CAAAC"], both_strands=True)          # GGCC is its own reverse complement; CAAAC's is GTTTG
    assert rep["per_pattern"].tolist() == [[33, 0], [9, 10]]
    for v in ("legacy", "swapped", "legacy_swapped"):                                   # the variants hold the same reads
        assert F.text_of("fasta", O.golden(f"ta_small.{v}.dexta")) == text
