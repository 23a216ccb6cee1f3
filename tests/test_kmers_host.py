"""dx_file_kmers' host side (no GPU): the new entry points are declared, exported and bound; calls without a context are argument
errors; dx_kmer_code / dx_kmer_letters against string arithmetic; and the oracle of the GPU tests -- tests/_kmers.py, numpy's
sliding windows over the oracle's text -- is valid on its own: it agrees with a dict over Python string slices, and it counts in
ta_edge what was counted in its text by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _kmers as K
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_kmers", "dx_kmer_spectrum", "dx_kmer_list", "dx_file_kmers_add", "dx_file_kmers", "dx_kmer_code", "dx_kmer_letters"]
E_ARG = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for t in ("dx_kmer", "dx_kmers"):
        assert re.search(r"\}\s*%s\s*;" % t, hdr), f"{t} is not declared in dexgpu.h"
    for m in ("code_kmers", "kmer_spectrum", "kmer_list", "kmers_add", "kmers"):
        assert callable(getattr(api.Context, m))
    assert callable(api.kmer_code) and callable(api.kmer_letters)
    assert C.sizeof(L.Kmer) == 16 and C.sizeof(L.Kmers) == 48
    assert [(f, getattr(L.Kmer, f).offset) for f, _ in L.Kmer._fields_] == [("count", 0), ("code", 8), ("reserved", 12)]
    assert [(f, getattr(L.Kmers, f).offset) for f, _ in L.Kmers._fields_] == [
        ("records", 0), ("symbols", 8), ("windows", 16), ("distinct", 24), ("max_count", 32), ("max_code", 40), ("k", 44)]
    assert api.KMER_DTYPE.itemsize == 16 and api.KMER_DTYPE == K.KMER
    assert [api.KMER_DTYPE.fields[f][1] for f in ("count", "code", "reserved")] == [0, 8, 12]


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    km, a, b, c, code = L.Kmers(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.dx_code_kmers(None, None, 0, None, None, None, 0, 4, 0, None, C.byref(a), C.byref(b)) == E_ARG
    assert lib.dx_kmer_spectrum(None, None, 4, None, 0, C.byref(a), C.byref(b), C.byref(code)) == E_ARG
    assert lib.dx_kmer_list(None, None, 4, 1, None, 0, C.byref(a)) == E_ARG
    assert lib.dx_file_kmers_add(None, L.DX_KIND_FASTA, img, len(img), 4, 0, None, C.byref(a), C.byref(b), C.byref(c)) == E_ARG
    assert lib.dx_file_kmers(None, L.DX_KIND_FASTA, img, len(img), 4, 0, 0, 0, C.byref(km), None, 0, None, C.byref(a), None) == E_ARG


# ---- dx_kmer_code, dx_kmer_letters -----------------------------------------------------------------------------------------------------
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def by_hand(s, letters="ACGT"):
    v = 0
    for ch in s:
        v = 4 * v + letters.index(ch)
    return v


def test_letters_and_codes_round_trip():
    for k in range(1, 6):
        for code in range(4 ** k):
            s = api.kmer_letters(code, k).decode()
            assert len(s) == k and by_hand(s) == code
            assert api.kmer_code(s) == code and api.kmer_code(s.lower()) == code
            assert api.kmer_code(s, canonical=True) == min(code, by_hand(revcomp(s)))
            a = api.kmer_letters(code, k, arrow=True).decode()
            assert a == s.translate(str.maketrans("ACGT", "1234")) and api.kmer_code(a, arrow=True) == code
    rng = np.random.default_rng(14)
    for code in [0, 4 ** 14 - 1] + [int(c) for c in rng.integers(0, 4 ** 14, 200)]:
        s = api.kmer_letters(code, 14).decode()
        assert by_hand(s) == code and api.kmer_code(s) == code
        assert api.kmer_code(s, canonical=True) == min(code, by_hand(revcomp(s)))
    assert api.kmer_letters(0b00011011, 4) == b"ACGT" and api.kmer_code("ACGT") == 27 == api.kmer_code("ACGT", canonical=True)
    assert api.kmer_code("TTTT", canonical=True) == 0 and api.kmer_code("CGTG", canonical=True) == by_hand("CACG")


def test_letters_and_codes_refusals():
    lib = L.load()
    code, out = C.c_uint32(77), C.create_string_buffer(16)
    for bad in ("ACNT", "AC1T", "ACG ", ""):
        with pytest.raises(L.DexGPUError) as e:
            api.kmer_code(bad)
        assert e.value.code == E_ARG
    with pytest.raises(L.DexGPUError):
        api.kmer_code("ACGT", arrow=True)
    with pytest.raises(L.DexGPUError):
        api.kmer_code("1235", arrow=True)
    with pytest.raises(L.DexGPUError):
        api.kmer_code("A" * 15)
    assert lib.dx_kmer_code(0, b"ACGTACGTACGTACGT", 0, 0, C.byref(code)) == E_ARG
    assert lib.dx_kmer_code(0, b"ACGTACGTACGTACGT", 15, 0, C.byref(code)) == E_ARG
    assert lib.dx_kmer_code(0, b"ACG", 4, 0, C.byref(code)) == E_ARG                # (the text's end is no letter)
    assert lib.dx_kmer_code(0, None, 4, 0, C.byref(code)) == E_ARG and lib.dx_kmer_code(0, b"ACGT", 4, 0, None) == E_ARG
    assert code.value == 77
    assert lib.dx_kmer_code(0, b"ACGTACGTACGTACGT", 14, 0, C.byref(code)) == 0 and code.value == by_hand("ACGTACGTACGTAC")
    assert lib.dx_kmer_letters(0, 0, 0, out) == E_ARG and lib.dx_kmer_letters(0, 0, 15, out) == E_ARG
    assert lib.dx_kmer_letters(0, 256, 4, out) == E_ARG and lib.dx_kmer_letters(0, 255, 4, None) == E_ARG
    assert lib.dx_kmer_letters(0, 255, 4, out) == 0 and out.value == b"TTTT"
    assert lib.dx_kmer_letters(0, 4 ** 14 - 1, 14, out) == 0 and out.value == b"T" * 14 and lib.dx_kmer_letters(0, 4 ** 14, 14, out) == E_ARG


# ---- the statement against an independent formulation ----------------------------------------------------------------------------------
def text_records(text):
    """the letters of every record of a text, as strings (a second reading of the text: no numpy, no codes)"""
    recs = []
    for line in text.decode().split("\n"):
        if line.startswith(">"):
            recs.append("")
        elif line:
            recs[-1] += line
    return recs


def dict_counts(recs, k, canonical, letters):
    comp = str.maketrans(letters, letters[::-1])
    out, windows = {}, 0
    for r in recs:
        for p in range(len(r) - k + 1):
            w = r[p:p + k]
            if canonical:
                w = min(w, w[::-1].translate(comp), key=lambda s: by_hand(s, letters))
            out[w] = out.get(w, 0) + 1
            windows += 1
    return out, windows


@pytest.mark.parametrize("kind,name", [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
@pytest.mark.parametrize("canonical", [False, True])
def test_the_statement_agrees_with_a_dict_over_string_slices(kind, name, k, canonical):
    text = F.text_of(kind, O.golden(name))
    letters = "ACGT" if kind == "fasta" else "1234"
    want, windows = dict_counts(text_records(text), k, canonical, letters)
    rep, spec, lst, t = K.file_kmers(kind, text, k, canonical, nspec=16, min_count=1, max_list=4 ** k)
    assert rep["windows"] == windows == int(t.sum()) and rep["distinct"] == len(want) == rep["listed"]
    assert rep["records"] == len(text_records(text)) and rep["symbols"] == sum(len(r) for r in text_records(text))
    assert {l.decode(): c for c, _, l in lst} == want
    assert [code for _, code, _ in lst] == sorted(by_hand(w, letters) for w in want)           # ascending codes
    assert all(int(t[by_hand(w, letters)]) == c for w, c in want.items())
    m = max(want.values())
    assert rep["max_count"] == m and rep["max_code"] == min(by_hand(w, letters) for w, c in want.items() if c == m)
    for c in range(1, 15):
        assert spec[c] == sum(1 for v in want.values() if v == c)
    assert spec[0] == 0 and spec[15] == sum(1 for v in want.values() if v >= 15)
    found, some = K.listing(t, m, 1)
    assert found == sum(1 for v in want.values() if v == m) and some["code"][0] == rep["max_code"] and some["count"][0] == m


@pytest.mark.parametrize("canonical", [False, True])
def test_the_statement_without_a_table_is_the_statement(monkeypatch, canonical):
    """beyond K.DENSE file_kmers keeps only the cells in use: the same report, spectrum and list"""
    text = F.text_of("fasta", O.golden("ta_small.dexta"))
    for k in (2, 8):
        dense = K.file_kmers("fasta", text, k, canonical, nspec=8, min_count=2, max_list=50)
        monkeypatch.setattr(K, "DENSE", 0)
        thin = K.file_kmers("fasta", text, k, canonical, nspec=8, min_count=2, max_list=50)
        monkeypatch.undo()
        assert thin[3] is None and dense[0] == thin[0] and np.array_equal(dense[1], thin[1]) and dense[2] == thin[2] and len(dense[2]) > 3
        seen, cnt, windows = K.sparse(F.reads("fasta", text), k, canonical)
        assert np.array_equal(np.flatnonzero(dense[3]), seen) and np.array_equal(dense[3][seen], cnt) and windows == dense[0]["windows"]


def test_the_statement_counts_what_was_counted_by_hand_in_ta_edge():
    """ta_edge's reads as undexta -U prints them: ACGTA, none, ACGTACG, GT, TTTT, C, AAAAAA, ACGT x 43 + G (173), T x 80.
    k = 2, windows = sum (len - 1) = 4 + 6 + 1 + 3 + 5 + 172 + 79 = 270:
      TT: read 4 three times, read 8 79 times: 82.   AA: read 6: 5.   AC: read 0 once, read 2 at 0 and 4, read 7 at 0, 4 .. 168: 1 + 2 + 43.
      CG: the same places + 1: 46.   GT: read 0, read 2, read 3, read 7 43 times: 46.   TA: read 0, read 2, read 7 at 3 .. 167: 1 + 1 + 42.
      TG: the end of read 7: 1.   82 + 5 + 46 + 46 + 46 + 44 + 1 = 270.
    k = 4, windows = sum (len - 3) = 2 + 4 + 1 + 3 + 170 + 77 = 257 (tests/test_find_host.py counts four of these as patterns):
      TTTT 1 + 77, AAAA 3, ACGT 1 + 1 + 43, CGTA 1 + 1 + 42, GTAC 1 + 42, TACG 1 + 42, CGTG 1: 78 + 3 + 45 + 44 + 43 + 43 + 1 = 257.
      canonical: TTTT goes to AAAA (81), TACG to CGTA (87), CGTG to CACG (1); ACGT and GTAC are their own: counted once a window."""
    text = F.text_of("fasta", O.golden("ta_edge.dexta"))
    rep, spec, lst, t = K.file_kmers("fasta", text, 2, nspec=64, min_count=1, max_list=100)
    assert (rep["records"], rep["symbols"], rep["windows"], rep["distinct"]) == (9, 278, 270, 7)
    assert [(l.decode(), c) for c, _, l in lst] == [("AA", 5), ("AC", 46), ("CG", 46), ("GT", 46), ("TA", 44), ("TG", 1), ("TT", 82)]
    assert (rep["max_count"], rep["max_code"]) == (82, 15)
    assert spec[1] == 1 and spec[5] == 1 and spec[44] == 1 and spec[46] == 3 and spec[63] == 1 and spec.sum() == 7
    rep, spec, lst, t = K.file_kmers("fasta", text, 4, nspec=256, min_count=40, max_list=3)
    assert (rep["windows"], rep["distinct"], rep["max_count"], rep["max_code"]) == (257, 7, 78, 255)
    assert [(l.decode(), c) for c, _, l in lst] == [("ACGT", 45), ("CGTA", 44), ("GTAC", 43)] and rep["listed"] == 3
    assert t[by_hand("TACG")] == 43 and t[by_hand("CGTG")] == 1 and t[0] == 3
    rep, spec, lst, t = K.file_kmers("fasta", text, 4, canonical=True, min_count=1, max_list=100)
    assert [(l.decode(), c) for c, _, l in lst] == [("AAAA", 81), ("ACGT", 45), ("CACG", 1), ("CGTA", 87), ("GTAC", 43)]
    assert (rep["windows"], rep["distinct"], rep["max_count"], rep["max_code"]) == (257, 5, 87, by_hand("CGTA"))
