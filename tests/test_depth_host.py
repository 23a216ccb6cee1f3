"""The depth feature's host side (no GPU): the new entry points are declared, exported and bound, the structs have their sizes and
offsets; calls without a context are argument errors; dx_depth_select against a plain Python loop; and the oracle of the GPU tests --
tests/_depth.py, numpy over uint64 codes -- agrees with a formulation over Python string slices and a dict of counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _depth as D
import _find as F
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_kmer_set_counted", "dx_kmer_set_counts", "dx_kmer_set_from_sorted_counted", "dx_kmer_set_from_kmers", "dx_file_kmer_set_counted",
       "dx_files_kmer_set_counted", "dx_code_kmer_depths", "dx_depth_stats", "dx_file_depth", "dx_depth_select"]
E_ARG = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for t in ("dx_depth", "dx_depth_report"):
        assert re.search(r"[}\s]\s*%s\s*;" % t, hdr), f"{t} is not declared in dexgpu.h"
    for i, s in enumerate(("MIN", "Q1", "MEDIAN", "Q3", "MAX")):
        assert re.search(r"#define\s+DX_DEPTH_%s\s+%d\b" % (s, i), hdr) and getattr(L, "DX_DEPTH_" + s) == i
    for m in ("kmer_set_counted", "kmer_set_files_counted", "kmer_set_from_kmers", "kmer_set_from_sorted_counted", "code_kmer_depths",
              "depth_stats", "depth"):
        assert callable(getattr(api.Context, m))
    assert callable(api.depth_select) and callable(api.KmerSet.counts) and isinstance(api.KmerSet.counted, property)
    assert C.sizeof(L.Depth) == 32 and C.sizeof(L.DepthReport) == 56 and C.sizeof(L.KmerSetInfo) == 32
    assert [(f, getattr(L.Depth, f).offset) for f, _ in L.Depth._fields_] == [
        ("windows", 0), ("hits", 4), ("sum", 8), ("min", 16), ("q1", 18), ("median", 20), ("q3", 22), ("max", 24), ("reserved", 26)]
    assert [(f, getattr(L.DepthReport, f).offset) for f, _ in L.DepthReport._fields_] == [
        ("records", 0), ("symbols", 8), ("windows", 16), ("hits", 24), ("sum", 32), ("records_hit", 40), ("k", 48), ("reserved", 52)]
    assert [getattr(L.DepthReport, f).offset for f, _ in L.DepthReport._fields_] == [getattr(L.ScreenReport, f).offset
                                                                                      for f, _ in L.ScreenReport._fields_]
    assert api.DEPTH_DTYPE.itemsize == 32 and api.DEPTH_DTYPE == D.DEPTH
    assert [api.DEPTH_DTYPE.fields[f][1] for f in D.DEPTH.names] == [0, 4, 8, 16, 18, 20, 22, 24, 26]


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    h, km, rp = C.c_void_p(), L.Kmers64(), L.DepthReport()
    pairs, counts, tot, win, bad = (L.Kmer64 * 1)(), (C.c_uint32 * 2)(), (C.c_uint64 * 4)(), C.c_uint64(), C.c_uint64()
    imgs, sizes = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    assert lib.dx_kmer_set_counted(None) == E_ARG
    assert lib.dx_kmer_set_counts(None, None, counts, 2) == E_ARG
    assert lib.dx_kmer_set_from_sorted_counted(None, None, 0, 1, 15, 0, 0, C.byref(h)) == E_ARG
    assert lib.dx_kmer_set_from_kmers(None, pairs, 1, 15, 0, 0, C.byref(h)) == E_ARG
    assert lib.dx_file_kmer_set_counted(None, L.DX_KIND_FASTA, img, len(img), 15, 0, 1, C.byref(h), C.byref(km)) == E_ARG
    assert lib.dx_files_kmer_set_counted(None, L.DX_KIND_FASTA, imgs, sizes, 0, 15, 0, 1, 0, C.byref(h), C.byref(km), None) == E_ARG
    assert lib.dx_code_kmer_depths(None, None, 0, None, None, None, 0, None, None, 0, None, C.byref(win), C.byref(bad)) == E_ARG
    assert lib.dx_depth_stats(None, None, None, 0, None, C.byref(tot)) == E_ARG
    assert lib.dx_file_depth(None, L.DX_KIND_FASTA, img, len(img), None, C.byref(rp), None, None, None, None) == E_ARG
    assert h.value is None


# ---- dx_depth_select -------------------------------------------------------------------------------------------------------------------
def entries(rows):
    """rows of (windows, min, q1, median, q3, max)"""
    out = np.zeros(len(rows), D.DEPTH)
    for j, r in enumerate(rows):
        out[j]["windows"] = r[0]
        for f, x in zip(D.STATS, r[1:]):
            out[j][f] = x
    return out


def both(rec, **kw):
    got = api.depth_select(rec, **kw)
    assert got.dtype == np.uint64 and got.tolist() == D.select(rec, **kw)
    return got.tolist()


def test_select_every_stat_both_modes_and_the_window_floor():
    rng = np.random.default_rng(6)
    n = 300
    five = np.sort(rng.integers(0, 65536, (n, 5)), axis=1)
    five[::7] = five[::7] // 1000                                   # (small depths too: the bounds below cut through them)
    win = np.where(rng.integers(0, 4, n) == 0, 0, rng.integers(1, 50, n))
    rec = entries([(int(w),) + tuple(int(x) for x in f) for w, f in zip(win, five)])
    rec[win == 0] = entries([(0, 0, 0, 0, 0, 0)])[0]                # a record without a window is all zeros
    for stat in D.STATS:
        for lo, hi in ((0, 65535), (0, 0), (10, 40), (30000, 65535), (65535, 65535)):
            for min_windows in (0, 1, 20):
                keep = both(rec, stat=stat, lo=lo, hi=hi, min_windows=min_windows)
                drop = both(rec, stat=stat, lo=lo, hi=hi, min_windows=min_windows, drop=True)
                assert keep == sorted(keep) and drop == sorted(drop) and sorted(keep + drop) == list(range(n))
    assert both(rec, min_windows=0) == both(rec, min_windows=1) == np.flatnonzero(win > 0).tolist()       # 0 acts as 1
    # a record with windows == 0 never matches, though its median 0 lies in [0, 0]; dropped, it is listed
    none = entries([(0, 0, 0, 0, 0, 0), (4, 0, 0, 0, 0, 9)])
    assert both(none, lo=0, hi=0) == [1] and both(none, lo=0, hi=0, drop=True) == [0]
    for i, stat in enumerate(D.STATS):                               # the DX_DEPTH_* numbers choose the same fields
        assert api.depth_select(rec, stat=i, lo=10, hi=4000).tolist() == D.select(rec, stat=stat, lo=10, hi=4000)


def test_select_zero_records_and_refusals():
    assert both(np.zeros(0, D.DEPTH)) == [] and both(np.zeros(0, D.DEPTH), drop=True) == []
    lib, ids, n = L.load(), C.c_void_p(), C.c_uint64(7)
    assert lib.dx_depth_select(None, 0, L.DX_DEPTH_MEDIAN, 0, 5, 1, L.DX_SCREEN_KEEP, C.byref(ids), C.byref(n)) == 0 and n.value == 0
    lib.dx_file_free(ids)
    rec = entries([(5, 1, 2, 3, 4, 5)])
    p = rec.ctypes.data
    assert lib.dx_depth_select(p, 1, 5, 0, 9, 1, 0, C.byref(ids), C.byref(n)) == E_ARG          # an unknown stat
    assert lib.dx_depth_select(p, 1, -1, 0, 9, 1, 0, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_depth_select(p, 1, 2, 0, 9, 1, 2, C.byref(ids), C.byref(n)) == E_ARG          # an unknown mode
    assert lib.dx_depth_select(p, 1, 2, 0, 9, 1, -1, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_depth_select(p, 1, 2, 9, 8, 1, 0, C.byref(ids), C.byref(n)) == E_ARG          # lo > hi
    assert lib.dx_depth_select(None, 1, 2, 0, 9, 1, 0, C.byref(ids), C.byref(n)) == E_ARG
    assert lib.dx_depth_select(p, 1, 2, 0, 9, 1, 0, None, C.byref(n)) == E_ARG
    assert lib.dx_depth_select(p, 1, 2, 0, 9, 1, 0, C.byref(ids), None) == E_ARG
    assert ids.value is None
    with pytest.raises(L.DexGPUError):
        api.depth_select(rec, lo=9, hi=8)
    assert lib.dx_depth_select(p, 1, 2, 3, 3, 1, 0, C.byref(ids), C.byref(n)) == 0 and n.value == 1
    lib.dx_file_free(ids)


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
@pytest.mark.parametrize("k,min_count", [(4, 1), (4, 40), (6, 2), (15, 1), (32, 1)])
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
def test_the_statement_agrees_with_string_slices_and_a_dict(kind, name, k, min_count, canonical):
    text = F.text_of(kind, O.golden(name))
    letters = "ACGT" if kind == "fasta" else "1234"
    recs = text_records(text)
    seen = {}
    for r in recs:
        for p in range(len(r) - k + 1):
            w = canon(r[p:p + k], canonical, letters)
            seen[w] = seen.get(w, 0) + 1
    kept = {w: c for w, c in seen.items() if c >= min_count}
    codes, counts = D.counted(F.reads(kind, text), k, canonical, min_count)
    assert codes.tolist() == sorted(by_hand(w, letters) for w in kept)
    assert counts.tolist() == [c for _, c in sorted((by_hand(w, letters), c) for w, c in kept.items())]
    want, off, prof, tot = [], [0], [], [0, 0, 0, 0]
    for r in recs:
        v = [min(kept.get(canon(r[p:p + k], canonical, letters), 0), 65535) for p in range(len(r) - k + 1)]
        s, w = sorted(v), len(v)
        hits = sum(1 for x in v if x)
        want.append((w, hits, sum(v)) + ((s[0], s[(w - 1) // 4], s[2 * (w - 1) // 4], s[3 * (w - 1) // 4], s[-1]) if w else (0,) * 5))
        prof += v
        off.append(off[-1] + w)
        tot = [tot[0] + w, tot[1] + hits, tot[2] + sum(v), tot[3] + (1 if hits else 0)]
    rep, rec, rec_len, gprof, goff = D.file_depth(kind, text, k, canonical, codes, counts)
    assert [tuple(int(e[f]) for f in D.DEPTH.names[:8]) for e in rec] == want and (rec["reserved"] == 0).all()
    assert gprof.dtype == np.uint16 and gprof.tolist() == prof and goff.tolist() == off
    assert rec_len.tolist() == [len(r) for r in recs]
    assert (rep["records"], rep["symbols"], rep["k"]) == (len(recs), sum(len(r) for r in recs), k)
    assert [rep["windows"], rep["hits"], rep["sum"], rep["records_hit"]] == tot and tot[1] > 0
    # an uncounted set gives the membership
    member = D.file_depth(kind, text, k, canonical, codes)[3]
    assert member.tolist() == [1 if x else 0 for x in prof]


def test_from_kmers_and_the_clamps_by_hand():
    pairs = [(5, 3), (9, 0), (5, 4), (2, 2 ** 32 - 2), (2, 5), (7, 2 ** 33), (1, 65536)]
    codes, counts = D.from_kmers(pairs, 4)
    assert codes.tolist() == [1, 2, 5, 7] and counts.tolist() == [65536, 2 ** 32 - 1, 7, 2 ** 32 - 1]
    # canonical, k = 2: AC (0b0001) and its reverse complement GT (0b1011) are one k-mer
    assert api.kmer_code64("GT", canonical=True) == api.kmer_code64("AC") == 1
    codes, counts = D.from_kmers([(0b1011, 4), (0b0001, 6)], 2, canonical=True)
    assert codes.tolist() == [1] and counts.tolist() == [10]
    s = np.array([0, 0, 1, 3, 0, 0, 1], np.uint8)                   # windows of k = 2: 0, 1, 7, 12, 0, 1
    d = D.unit_depths(s, 2, False, np.array([0, 1, 7], np.uint64), np.array([65536, 9, 2 ** 32 - 1], np.uint32))
    assert d.tolist() == [65535, 9, 65535, 0, 65535, 9]
    assert D.entry(d) == (6, 5, 3 * 65535 + 18, 0, 9, 9, 65535, 65535)           # sorted 0 9 9 M M M: ranks 5 // 4, 10 // 4, 15 // 4
    assert D.entry([]) == (0,) * 8 and D.entry([7]) == (1, 1, 7, 7, 7, 7, 7, 7)
    c, n = D.from_sorted([3, 3, 3, 5, 9, 9], 2)
    assert c.tolist() == [3, 9] and n.tolist() == [3, 2]
