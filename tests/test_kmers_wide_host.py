"""dx_file_kmers_wide's host side (no GPU): the new entry points are declared, exported and bound; calls without a context are
argument errors; dx_kmer_code64 / dx_kmer_letters64 against string arithmetic with Python integers; and the oracle of the GPU tests --
tests/_kmers_wide.py, numpy's uint64 codes over the oracle's text -- agrees with a dict over Python string slices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _kmers_wide as W
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_sort_u64", "dx_code_kmer_codes", "dx_kmer_runs", "dx_file_kmers_wide", "dx_kmer_code64", "dx_kmer_letters64"]
E_ARG = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for t in ("dx_kmer64", "dx_kmers64"):
        assert re.search(r"\}\s*%s\s*;" % t, hdr), f"{t} is not declared in dexgpu.h"
    for m in ("sort_u64", "code_kmer_codes", "kmer_runs", "kmers_wide"):
        assert callable(getattr(api.Context, m))
    assert callable(api.kmer_code64) and callable(api.kmer_letters64)
    assert C.sizeof(L.Kmer64) == 16 and C.sizeof(L.Kmers64) == 56
    assert [(f, getattr(L.Kmer64, f).offset) for f, _ in L.Kmer64._fields_] == [("code", 0), ("count", 8)]
    assert [(f, getattr(L.Kmers64, f).offset) for f, _ in L.Kmers64._fields_] == [
        ("records", 0), ("symbols", 8), ("windows", 16), ("distinct", 24), ("max_count", 32), ("max_code", 40), ("k", 48), ("reserved", 52)]
    assert api.KMER64_DTYPE.itemsize == 16 and api.KMER64_DTYPE == W.KMER64
    assert api.KMER64_LIST_DTYPE.fields["letters"][0].itemsize == 32


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    km, a, b, c, d = L.Kmers64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.dx_sort_u64(None, None, None, 0, 8) == E_ARG
    assert lib.dx_code_kmer_codes(None, None, 0, None, None, None, 0, 21, 0, None, 0, C.byref(a), C.byref(b)) == E_ARG
    assert lib.dx_kmer_runs(None, None, 0, 1, None, 0, C.byref(a), None, 0, C.byref(b), C.byref(c), C.byref(d)) == E_ARG
    assert lib.dx_file_kmers_wide(None, L.DX_KIND_FASTA, img, len(img), 21, 0, 0, 0, C.byref(km), None, 0, None, C.byref(a)) == E_ARG


# ---- dx_kmer_code64, dx_kmer_letters64 -------------------------------------------------------------------------------------------------
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def by_hand(s, letters="ACGT"):
    v = 0
    for ch in s:
        v = 4 * v + letters.index(ch)
    return v


def test_letters_and_codes_round_trip():
    rng = np.random.default_rng(32)
    for k in range(1, 33):
        for s in ["A" * k, "T" * k, "".join("ACGT"[i % 4] for i in range(k))] + ["".join("ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(20)]:
            code = by_hand(s)
            assert api.kmer_code64(s) == code and api.kmer_code64(s.lower()) == code
            assert api.kmer_letters64(code, k) == s.encode()
            assert api.kmer_code64(s, canonical=True) == min(code, by_hand(revcomp(s)))
            a = s.translate(str.maketrans("ACGT", "1234"))
            assert api.kmer_letters64(code, k, arrow=True) == a.encode() and api.kmer_code64(a, arrow=True) == code
    assert api.kmer_code64("T" * 32) == 2 ** 64 - 1 and api.kmer_code64("A" * 32) == 0
    assert api.kmer_code64("T" * 32, canonical=True) == 0
    own = "ACGT" * 8                                               # its own reverse complement
    assert revcomp(own) == own and api.kmer_code64(own, canonical=True) == api.kmer_code64(own) == by_hand(own)
    assert api.kmer_letters64(2 ** 64 - 1, 32) == b"T" * 32 and api.kmer_letters64(0, 32) == b"A" * 32
    hi = "G" + "A" * 31                                            # the top bit in use: compared unsigned
    assert api.kmer_code64(hi) == 2 << 62 and api.kmer_code64(hi, canonical=True) == min(2 << 62, by_hand(revcomp(hi)))


def test_letters_and_codes_refusals():
    lib = L.load()
    code, out = C.c_uint64(77), C.create_string_buffer(40)
    for bad in ("ACNT", "AC1T", "ACG ", "", "A" * 33):
        with pytest.raises(L.DexGPUError) as e:
            api.kmer_code64(bad)
        assert e.value.code == E_ARG
    with pytest.raises(L.DexGPUError):
        api.kmer_code64("ACGT", arrow=True)
    with pytest.raises(L.DexGPUError):
        api.kmer_code64("1235", arrow=True)
    long = b"ACGT" * 10
    assert lib.dx_kmer_code64(0, long, 0, 0, C.byref(code)) == E_ARG and lib.dx_kmer_code64(0, long, 33, 0, C.byref(code)) == E_ARG
    assert lib.dx_kmer_code64(0, b"ACG", 4, 0, C.byref(code)) == E_ARG              # (the text's end is no letter)
    assert lib.dx_kmer_code64(0, b"ACGT" * 5, 21, 0, C.byref(code)) == E_ARG        # ... at 20 letters of 21 too
    assert lib.dx_kmer_code64(0, None, 4, 0, C.byref(code)) == E_ARG and lib.dx_kmer_code64(0, b"ACGT", 4, 0, None) == E_ARG
    assert code.value == 77
    assert lib.dx_kmer_code64(0, long, 32, 0, C.byref(code)) == 0 and code.value == by_hand("ACGT" * 8)
    assert lib.dx_kmer_letters64(0, 0, 0, out) == E_ARG and lib.dx_kmer_letters64(0, 0, 33, out) == E_ARG
    assert lib.dx_kmer_letters64(0, 256, 4, out) == E_ARG and lib.dx_kmer_letters64(0, 255, 4, None) == E_ARG
    assert lib.dx_kmer_letters64(0, 4 ** 31, 31, out) == E_ARG and lib.dx_kmer_letters64(0, 4 ** 31 - 1, 31, out) == 0 and out.value == b"T" * 31
    assert lib.dx_kmer_letters64(0, 2 ** 64 - 1, 32, out) == 0 and out.value == b"T" * 32
    with pytest.raises(L.DexGPUError):
        api.kmer_letters64(4 ** 21, 21)
    with pytest.raises(L.DexGPUError):
        api.kmer_letters64(2 ** 64, 32)


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
@pytest.mark.parametrize("k", [15, 31, 32])
@pytest.mark.parametrize("canonical", [False, True])
def test_the_statement_agrees_with_a_dict_over_string_slices(kind, name, k, canonical):
    text = F.text_of(kind, O.golden(name))
    letters = "ACGT" if kind == "fasta" else "1234"
    want, windows = dict_counts(text_records(text), k, canonical, letters)
    rep, spec, lst = W.file_kmers_wide(kind, text, k, canonical, nspec=16, min_count=1, max_list=1 << 30)
    assert rep["windows"] == windows and rep["distinct"] == len(want) == rep["listed"]
    assert rep["records"] == len(text_records(text)) and rep["symbols"] == sum(len(r) for r in text_records(text))
    assert {l.decode(): c for c, _, l in lst} == want
    assert [code for _, code, _ in lst] == sorted(by_hand(w, letters) for w in want)           # ascending codes, as Python integers
    m = max(want.values())
    assert rep["max_count"] == m and rep["max_code"] == min(by_hand(w, letters) for w, c in want.items() if c == m)
    for c in range(1, 15):
        assert spec[c] == sum(1 for v in want.values() if v == c)
    assert spec[0] == 0 and spec[15] == sum(1 for v in want.values() if v >= 15)
    rep2, _, few = W.file_kmers_wide(kind, text, k, canonical, nspec=2, min_count=2, max_list=3)
    assert few == [e for e in lst if e[0] >= 2][:3] and rep2["listed"] == len(few)


def test_the_codes_and_the_reverse_strand_at_the_top_bit():
    s = np.array([3] * 32 + [0] * 32 + [2, 1, 0, 3], np.uint8)
    c = W.codes(s, 32)
    assert c.dtype == np.uint64 and int(c[0]) == 2 ** 64 - 1 and int(c[32]) == 0 and len(c) == 37
    as_str = "".join("ACGT"[v] for v in s)
    assert [int(v) for v in c] == [by_hand(as_str[p:p + 32]) for p in range(37)]
    assert [int(v) for v in W.rc(c, 32)] == [by_hand(revcomp(as_str[p:p + 32])) for p in range(37)]
    assert [int(v) for v in W.unit_codes(s, 32, True)] == [min(by_hand(as_str[p:p + 32]), by_hand(revcomp(as_str[p:p + 32]))) for p in range(37)]
    found, lst, fig = W.runs(np.array([1, 1, 5, 5, 5, 2 ** 64 - 1], np.uint64), 2, 10, 3)
    assert found == 2 and [(int(e["code"]), int(e["count"])) for e in lst] == [(1, 2), (5, 3)]
    assert fig["spectrum"].tolist() == [0, 1, 2] and (fig["distinct"], fig["max_count"], fig["max_code"]) == (3, 3, 5)
