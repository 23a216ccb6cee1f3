"""dx_files_kmers_wide's host side (no GPU): the new entry points are declared, exported and bound; dx_kmer_range_plan against the
Python loop of tests/_kmers_files.py on random bins, with the properties a plan must have stated on their own; and the numpy
reference of the bins against a dict over Python string slices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _kmers_files as KF
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_kmer_bins", "dx_code_kmer_codes_range", "dx_kmer_range_plan", "dx_sorted_take", "dx_files_kmers_wide", "dx_files_kmer_set"]
E_ARG, E_NOMEM = -1, -6


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("code_kmer_bins", "code_kmer_codes_range", "sorted_take", "kmers_wide_files", "kmer_set_files"):
        assert callable(getattr(api.Context, m))
    assert callable(api.kmer_range_plan)


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    km, a, b, p, h = L.Kmers64(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_void_p()
    imgs, sizes = (C.c_void_p * 1)(C.cast(C.c_char_p(img), C.c_void_p)), (C.c_size_t * 1)(len(img))
    assert lib.dx_code_kmer_bins(None, None, 0, None, None, None, 0, 21, 0, 12, None, C.byref(a), C.byref(b)) == E_ARG
    assert lib.dx_code_kmer_codes_range(None, None, 0, None, None, None, 0, 21, 0, 12, 0, 1, None, 0, C.byref(a), C.byref(b)) == E_ARG
    assert lib.dx_sorted_take(None, None, 0, 1, None, 0, C.byref(a)) == E_ARG
    assert lib.dx_files_kmers_wide(None, L.DX_KIND_FASTA, imgs, sizes, 1, 21, 0, 0, 0, 0, C.byref(km), None, 0, None, C.byref(a), None,
                                   C.byref(p)) == E_ARG
    assert lib.dx_files_kmer_set(None, L.DX_KIND_FASTA, imgs, sizes, 1, 21, 0, 1, 0, C.byref(h), C.byref(km), C.byref(p)) == E_ARG
    assert h.value is None


# ---- dx_kmer_range_plan ----------------------------------------------------------------------------------------------------------------
def sums(bins, cut):
    return [int(np.asarray(bins, np.uint64)[a:b].sum()) for a, b in zip(cut[:-1], cut[1:])]


def check_plan(bins, room):
    """the library's plan is the loop's, and is a plan: ascending cuts that cover [0, nbins), every range within room, and greedy -- a
    range could not have taken the next range's first non-empty bin"""
    cut = api.kmer_range_plan(bins, room).tolist()
    assert cut == KF.plan(bins, room), (room, cut)
    assert cut[0] == 0 and cut[-1] == len(bins) and all(a < b for a, b in zip(cut[:-1], cut[1:]))
    s = sums(bins, cut)
    assert sum(s) == sum(int(v) for v in bins)
    if room:
        assert all(v <= room for v in s)
        for r in range(len(s) - 1):
            assert int(bins[cut[r + 1]]) > 0 and s[r] + int(bins[cut[r + 1]]) > room
    else:
        assert len(s) == 1
    return cut


@pytest.mark.parametrize("nbins", [1, 2, 4, 64, 4096])
def test_the_plan_is_the_python_loops(nbins):
    rng = np.random.default_rng(nbins)
    for trial in range(6):
        bins = rng.integers(0, 1000, nbins).astype(np.uint64)
        bins[rng.random(nbins) < 0.3] = 0                          # empty bins anywhere
        if trial % 2 and nbins >= 4:
            bins[:nbins // 4] = 0                                  # ... and at both ends
            bins[-(nbins // 4):] = 0
        if not bins.any():
            bins[nbins // 2] = 17
        total, largest = int(bins.sum()), int(bins.max())
        most = check_plan(bins, largest)                           # the most passes a plan can have
        assert len(most) - 1 >= -(-total // largest)                # (no plan has fewer: a range holds `largest` at most)
        assert len(check_plan(bins, total)) == 2                   # everything fits: one range
        assert len(check_plan(bins, 0)) == 2
        assert len(check_plan(bins, 2 ** 63)) == 2
        for room in (largest + 1, 2 * largest, -(-total // 3), total - 1):
            if room >= largest:
                assert len(check_plan(bins, room)) <= len(most)
    zeros = np.zeros(nbins, np.uint64)
    assert check_plan(zeros, 5) == [0, nbins] and check_plan(zeros, 0) == [0, nbins]


def test_the_plan_at_the_top_of_the_range_of_its_numbers():
    bins = np.array([2 ** 63, 0, 2 ** 63 - 1, 1, 0, 2 ** 63], np.uint64)             # (sums that would pass 2^64 if they were made)
    assert check_plan(bins, 2 ** 63) == [0, 2, 5, 6]
    assert check_plan(bins, 2 ** 64 - 1) == [0, 3, 6]


def test_a_bin_above_room_is_nomem_and_names_the_bin():
    bins = np.array([0, 5, 9, 0, 31, 7, 31, 0], np.uint64)
    for room in (30, 8, 1):
        with pytest.raises(KF.BinTooLarge) as want:
            KF.plan(bins, room)
        with pytest.raises(L.DexGPUError) as e:
            api.kmer_range_plan(bins, room)
        assert e.value.code == E_NOMEM
        assert "bin %d " % want.value.bin in str(e.value) and "%d windows" % want.value.windows in str(e.value)
    assert check_plan(bins, 31) == [0, 4, 5, 6, 8]
    lib, n = L.load(), C.c_uint32(9)
    cut = np.zeros(9, np.uint32)
    assert lib.dx_kmer_range_plan(None, None, 8, 5, cut.ctypes.data, C.byref(n)) == E_ARG
    assert lib.dx_kmer_range_plan(None, bins.ctypes.data, 0, 5, cut.ctypes.data, C.byref(n)) == E_ARG
    assert lib.dx_kmer_range_plan(None, bins.ctypes.data, 8, 5, None, C.byref(n)) == E_ARG
    assert lib.dx_kmer_range_plan(None, bins.ctypes.data, 8, 5, cut.ctypes.data, None) == E_ARG


# ---- the bins' statement against an independent formulation ----------------------------------------------------------------------------
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


@pytest.mark.parametrize("kind,name", [("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")])
@pytest.mark.parametrize("k,bits", [(1, 2), (5, 10), (6, 12), (7, 12), (21, 11), (32, 12), (32, 1)])
@pytest.mark.parametrize("canonical", [False, True])
def test_the_bins_agree_with_a_dict_over_string_slices(kind, name, k, bits, canonical):
    """a window's bin is the code of its first bits / 2 letters, and of half a letter more: the code as a Python integer, shifted"""
    text = F.text_of(kind, O.golden(name))
    letters = "ACGT" if kind == "fasta" else "1234"
    comp = str.maketrans(letters, letters[::-1])
    want = {}
    for r in text_records(text):
        for p in range(len(r) - k + 1):
            w = r[p:p + k]
            code = by_hand(w, letters)
            if canonical:
                code = min(code, by_hand(w[::-1].translate(comp), letters))
            want[code >> (2 * k - bits)] = want.get(code >> (2 * k - bits), 0) + 1
    codes = KF.text_codes(kind, [text], k, canonical)
    got = KF.bins(codes, k, bits)
    assert len(got) == 1 << bits and int(got.sum()) == len(codes) == sum(want.values()) > 0
    assert {b: int(c) for b, c in enumerate(got) if c} == want
    lo, hi = (1 << bits) // 4, (1 << bits) // 4 * 3 + 1
    mask = KF.in_range(codes, k, bits, lo, hi)
    assert int(mask.sum()) == sum(c for b, c in want.items() if lo <= b < hi) == int(got[lo:hi].sum())
    assert KF.files_kmers_wide(kind, [text, text], k, canonical)[0]["windows"] == 2 * len(codes)
