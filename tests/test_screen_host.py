"""The screen's host side (no GPU): the new entry points are declared, exported and bound, the structs have their sizes and offsets;
calls without a context are argument errors; dx_screen_select against a plain Python loop; and the oracle of the GPU tests --
tests/_screen.py, numpy over uint64 codes -- agrees with a formulation over Python string slices and sets of strings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _oracle as O
import _screen as S
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_kmer_set_from_codes", "dx_kmer_set_from_sorted", "dx_file_kmer_set", "dx_kmer_set_info", "dx_kmer_set_codes", "dx_kmer_set_free",
       "dx_code_kmer_screen", "dx_file_screen", "dx_screen_select"]
E_ARG = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for t in ("dx_kmer_set", "dx_set_info", "dx_screen", "dx_screen_report"):
        assert re.search(r"[}\s]\s*%s\s*;" % t, hdr), f"{t} is not declared in dexgpu.h"
    assert re.search(r"#define\s+DX_SCREEN_KEEP\s+0\b", hdr) and re.search(r"#define\s+DX_SCREEN_DROP\s+1\b", hdr)
    assert (L.DX_SCREEN_KEEP, L.DX_SCREEN_DROP) == (0, 1)
    for m in ("kmer_set", "kmer_set_from_codes", "code_kmer_screen", "screen"):
        assert callable(getattr(api.Context, m))
    assert callable(api.screen_select)
    for m in ("codes", "free", "__enter__", "__exit__"):
        assert callable(getattr(api.KmerSet, m))
    assert isinstance(api.KmerSet.info, property)
    assert C.sizeof(L.Screen) == 16 and C.sizeof(L.ScreenReport) == 56 and C.sizeof(L.KmerSetInfo) == 32
    assert [(f, getattr(L.Screen, f).offset) for f, _ in L.Screen._fields_] == [("hits", 0), ("covered", 4), ("first", 8), ("last", 12)]
    assert [(f, getattr(L.ScreenReport, f).offset) for f, _ in L.ScreenReport._fields_] == [
        ("records", 0), ("symbols", 8), ("windows", 16), ("hits", 24), ("covered", 32), ("records_hit", 40), ("k", 48), ("reserved", 52)]
    assert [(f, getattr(L.KmerSetInfo, f).offset) for f, _ in L.KmerSetInfo._fields_] == [
        ("codes", 0), ("device_bytes", 8), ("k", 16), ("canonical", 20), ("arrow", 24), ("index_bits", 28)]
    assert api.SCREEN_DTYPE.itemsize == 16 and api.SCREEN_DTYPE == S.SCREEN


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    h, km, info, rp = C.c_void_p(), L.Kmers64(), L.KmerSetInfo(), L.ScreenReport()
    codes, tot, bad = (C.c_uint64 * 2)(1, 2), (C.c_uint64 * 4)(), C.c_uint64()
    assert lib.dx_kmer_set_from_codes(None, codes, 2, 15, 0, 0, C.byref(h)) == E_ARG
    assert lib.dx_kmer_set_from_sorted(None, None, 0, 1, 15, 0, 0, C.byref(h)) == E_ARG
    assert lib.dx_file_kmer_set(None, L.DX_KIND_FASTA, img, len(img), 15, 0, 1, C.byref(h), C.byref(km)) == E_ARG
    assert lib.dx_kmer_set_info(None, C.byref(info)) == E_ARG
    assert lib.dx_kmer_set_codes(None, None, codes, 2) == E_ARG
    assert lib.dx_kmer_set_free(None, None) == E_ARG
    assert lib.dx_code_kmer_screen(None, None, 0, None, None, None, 0, None, None, C.byref(tot), C.byref(bad)) == E_ARG
    assert lib.dx_file_screen(None, L.DX_KIND_FASTA, img, len(img), None, C.byref(rp), None, None) == E_ARG
    assert h.value is None


# ---- dx_screen_select ------------------------------------------------------------------------------------------------------------------
def entries(rows):
    return np.array(rows, S.SCREEN)


def both(rec, ln, **kw):
    got = api.screen_select(rec, ln, **kw)
    assert got.dtype == np.uint64 and got.tolist() == S.select(rec, ln, **kw)
    return got.tolist()


def test_select_at_the_permille_threshold():
    # 900 permille of 1000 symbols: 900 covered passes, 899 does not; of 7 symbols: 7 * 900 = 6300 <= 1000 * 7 only
    rec = entries([(5, 900, 0, 800), (5, 899, 0, 800), (1, 7, 0, 0), (1, 6, 0, 0), (2, 1000, 0, 0)])
    ln = [1000, 1000, 7, 7, 1000]
    assert both(rec, ln, min_permille=900) == [0, 2, 4]
    assert both(rec, ln, min_permille=900, drop=True) == [1, 3]
    assert both(rec, ln, min_permille=1000) == [2, 4]
    assert both(rec, ln, min_permille=0) == [0, 1, 2, 3, 4]
    big = entries([(1, 2 ** 31 - 1, 0, 0), (1, 2 ** 31 - 2, 0, 0)])                  # the products leave 32 bits
    assert both(big, [2 ** 31 - 1, 2 ** 31 - 1], min_permille=1000) == [0]


def test_select_hits_lengths_and_modes():
    rng = np.random.default_rng(4)
    n = 300
    ln = rng.integers(0, 400, n).astype(np.uint32)
    hits = np.where(rng.integers(0, 3, n) == 0, 0, rng.integers(1, 30, n))
    cov = np.where(hits > 0, np.minimum(ln, rng.integers(1, 400, n)), 0)
    rec = np.zeros(n, S.SCREEN)
    rec["hits"], rec["covered"] = hits, cov
    rec["first"] = rec["last"] = np.where(hits > 0, 0, S.NONE)
    for kw in ({}, {"min_hits": 0}, {"min_hits": 5}, {"min_permille": 500}, {"min_hits": 3, "min_permille": 250}):
        keep, drop = both(rec, ln, **kw), both(rec, ln, drop=True, **kw)
        assert keep == sorted(keep) and drop == sorted(drop) and sorted(keep + drop) == list(range(n))      # a partition, ascending
    assert both(rec, ln, min_hits=0) == both(rec, ln, min_hits=1) == np.flatnonzero(hits > 0).tolist()      # 0 acts as 1
    # a record of length 0 never matches: it has no window, so no hit -- whatever the permille
    empty = entries([(0, 0, S.NONE, S.NONE), (1, 20, 0, 0)])
    assert both(empty, [0, 20], min_permille=0) == [1] and both(empty, [0, 20], min_permille=0, drop=True) == [0]


def test_select_zero_records_and_refusals():
    assert both(np.zeros(0, S.SCREEN), []) == [] and both(np.zeros(0, S.SCREEN), [], drop=True) == []
    lib, ids, n = L.load(), C.c_void_p(), C.c_uint64(7)
    assert lib.dx_screen_select(None, None, 0, 1, 0, L.DX_SCREEN_KEEP, C.byref(ids), C.byref(n)) == 0 and n.value == 0
    lib.dx_file_free(ids)
    rec, ln = entries([(1, 5, 0, 0)]), np.array([10], np.uint32)
    assert lib.dx_screen_select(rec.ctypes.data, ln.ctypes.data, 1, 1, 1001, 0, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_screen_select(rec.ctypes.data, ln.ctypes.data, 1, 1, 0, 2, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_screen_select(rec.ctypes.data, ln.ctypes.data, 1, 1, 0, -1, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_screen_select(None, ln.ctypes.data, 1, 1, 0, 0, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_screen_select(rec.ctypes.data, None, 1, 1, 0, 0, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_screen_select(rec.ctypes.data, ln.ctypes.data, 1, 1, 0, 0, None, C.byref(n)) == E_ARG
    assert lib.dx_screen_select(rec.ctypes.data, ln.ctypes.data, 1, 1, 0, 0, C.byref(ids), None) == E_ARG
    assert ids.value is None
    with pytest.raises(L.DexGPUError):
        api.screen_select(rec, ln, min_permille=1001)
    with pytest.raises(L.DexGPUError):
        api.screen_select(rec, [10, 20])


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


def by_hand(s, letters):
    v = 0
    for ch in s:
        v = 4 * v + letters.index(ch)
    return v


def canon(w, canonical, letters):
    if not canonical:
        return w
    r = w[::-1].translate(str.maketrans(letters, letters[::-1]))
    return min(w, r, key=lambda s: by_hand(s, letters))


@pytest.mark.parametrize("kind,name", [("fasta", "ta_small.dexta"), ("fasta", "ta_edge.dexta"), ("arrow", "ar_small.dexar")])
@pytest.mark.parametrize("k", [15, 32])
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
def test_the_statement_agrees_with_string_slices(kind, name, k, canonical):
    text = F.text_of(kind, O.golden(name))
    letters = "ACGT" if kind == "fasta" else "1234"
    recs = text_records(text)
    # the set: the windows of every other record at every third position of its first half, as strings; and as codes for the statement
    words = {canon(r[p:p + k], canonical, letters) for r in recs[1::2] for p in range(0, (len(r) - k + 1) // 2, 3)}
    codes = np.array(sorted(by_hand(w, letters) for w in words), np.uint64)
    assert len(words) > 0
    want, tot = [], [0, 0, 0, 0]
    for r in recs:
        pos = [p for p in range(len(r) - k + 1) if canon(r[p:p + k], canonical, letters) in words]
        cov = {q for p in pos for q in range(p, p + k)}
        want.append((len(pos), len(cov), pos[0] if pos else S.NONE, pos[-1] if pos else S.NONE))
        tot = [tot[0] + max(0, len(r) - k + 1), tot[1] + len(pos), tot[2] + len(cov), tot[3] + (1 if pos else 0)]
    rep, rec, rec_len = S.file_screen(kind, text, k, canonical, codes)
    assert [tuple(int(v) for v in e) for e in rec] == want
    assert rec_len.tolist() == [len(r) for r in recs]
    assert (rep["records"], rep["symbols"], rep["k"]) == (len(recs), sum(len(r) for r in recs), k)
    assert [rep["windows"], rep["hits"], rep["covered"], rep["records_hit"]] == tot and tot[1] > 0
    assert any(0 < e[1] < n for e, n in zip(want, rec_len.tolist()))                  # some record is covered in part
    assert S.distinct(F.reads(kind, text), k, canonical).tolist() == sorted(
        {by_hand(canon(r[p:p + k], canonical, letters), letters) for r in recs for p in range(len(r) - k + 1)})
