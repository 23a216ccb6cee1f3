"""Context.kmer_runs (dx_kmer_runs) on the GPU against np.unique of the same sorted array (tests/_kmers_wide.py): no key, one run, all
keys distinct, runs that begin or end on the borders of a tile (2048 keys) and of a thread's eight keys, a run far longer than a tile,
two codes that tie for the longest run, the spectrum's last bin, min_count, and a list shorter than what was found.  No expected
value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import _kmers_wide as W
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
TILE = 2048                                                        # TL_TILE of csrc/tiles/dx_tiles.hpp
GUARD = 4                                                          # entries behind the list's cap
MARK = np.uint64(0xD00DD00DD00DD00D)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def from_runs(codes, counts):
    return np.repeat(np.asarray(codes, np.uint64), np.asarray(counts, np.int64))


def check(ctx, keys, min_count=1, cap=None, nspec=256):
    """one call against the statement; the list's array has guard entries behind cap, which must stay"""
    keys = np.ascontiguousarray(keys, np.uint64)
    assert (keys[1:] >= keys[:-1]).all()
    found_w, lst_w, fig_w = W.runs(keys, min_count, len(keys) + 1 if cap is None else cap, nspec or 2)
    cap = found_w + 3 if cap is None else cap
    d_keys = ctx.to_device(keys) if len(keys) else ctx.alloc(16)
    d_out = ctx.alloc(16 * (cap + GUARD)).upload(np.full(2 * (cap + GUARD), MARK))
    found, d, m, mc = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    spec = np.full(nspec, 99, np.uint64) if nspec else None
    try:
        ctx._chk(ctx.lib.dx_kmer_runs(ctx.h, d_keys.ptr, len(keys), min_count, d_out.ptr if cap else None, cap, C.byref(found),
                                      spec.ctypes.data if nspec else None, nspec, C.byref(d), C.byref(m), C.byref(mc)))
        raw = d_out.download(np.uint64, 2 * (cap + GUARD))
    finally:
        d_keys.free(); d_out.free()
    got = min(cap, found.value)
    assert found.value == found_w
    assert (raw[2 * got:] == MARK).all(), "an entry at cap or beyond was written"
    lst = raw[:2 * got].view(W.KMER64)
    assert np.array_equal(lst["code"], lst_w["code"][:got]) and np.array_equal(lst["count"], lst_w["count"][:got])
    assert (d.value, m.value, mc.value) == (fig_w["distinct"], fig_w["max_count"], fig_w["max_code"])
    if nspec:
        assert np.array_equal(spec, fig_w["spectrum"]), (spec[:8], fig_w["spectrum"][:8])
        assert spec[0] == 0 and int(spec.sum()) == fig_w["distinct"]
    return found.value, lst, fig_w


def test_no_key(ctx):
    found, lst, fig = check(ctx, np.zeros(0, np.uint64))
    assert found == 0 and fig["distinct"] == 0 and fig["max_count"] == 0 and fig["max_code"] == 0


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 64, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_one_run(ctx, n):
    found, lst, fig = check(ctx, np.full(n, 2 ** 64 - 1, np.uint64))
    assert found == 1 and int(lst["count"][0]) == n and int(lst["code"][0]) == 2 ** 64 - 1


@pytest.mark.parametrize("n", [1, 8, 255, TILE - 1, TILE, TILE + 1, 5 * TILE + 77])
def test_all_distinct(ctx, n):
    rng = np.random.default_rng(n)
    keys = np.unique(rng.integers(0, 1 << 63, 2 * n, dtype=np.uint64))[:n] * np.uint64(2)
    keys[0] = 0                                                    # (code 0 is a code like any other)
    found, lst, fig = check(ctx, keys, nspec=5)
    assert found == n == fig["distinct"] and fig["max_count"] == 1 and fig["max_code"] == 0


def test_runs_on_the_borders_of_tiles_and_threads(ctx):
    """runs that end with a tile, begin with one, cover one exactly, cover several, and a tile without any begin between two others"""
    counts = [TILE - 3, 3, TILE, 1, TILE - 1, 5, 2 * TILE - 5, 8, 8, 7, 1, 9, 3 * TILE, TILE + 1, 1, 1, TILE - 2]
    keys = from_runs(np.arange(len(counts)) * 1000 + 7, counts)
    found, lst, fig = check(ctx, keys, nspec=4 * TILE)
    assert found == len(counts) and lst["count"].tolist() == counts
    check(ctx, keys, min_count=TILE)
    check(ctx, keys[1:-1], min_count=8, nspec=3)                   # (and everything a place to the left)


def test_a_run_far_longer_than_a_tile(ctx):
    rng = np.random.default_rng(1)
    rest = np.unique(rng.integers(0, 1 << 62, 120000, dtype=np.uint64))[:100000]
    keys = np.sort(np.concatenate([rest, np.full(100000, int(rest[40000]) + 1, np.uint64)]))       # a homopolymer's code among the others
    assert len(keys) == 200000
    found, lst, fig = check(ctx, keys, min_count=2, nspec=16)
    assert found >= 1 and fig["max_count"] >= 100000 and fig["spectrum"][15] >= 1


def test_a_run_whose_end_lies_more_than_256_tiles_away(ctx):
    """the search of the tiles that follow takes 256 of them a step: this run's next begin is found in its second step"""
    long = 257 * TILE + 3
    counts = [1] * (TILE // 2 + 5) + [long] + [1, 2, 1, 3, 1]        # the run begins in the middle of a tile
    keys = from_runs(np.arange(len(counts), dtype=np.uint64) * np.uint64(11) + np.uint64(3), counts)
    found, lst, fig = check(ctx, keys)
    assert found == len(counts) and lst["count"].tolist() == counts
    found, lst, fig = check(ctx, keys, min_count=long)
    assert found == 1 and int(lst["count"][0]) == long == fig["max_count"] and int(lst["code"][0]) == 11 * (TILE // 2 + 5) + 3


def test_two_codes_tie_for_the_longest_run(ctx):
    counts = [3, 900, 2, 5000, 1, 5000, 7, 5000, 4]
    codes = [5, 6, 1 << 40, (1 << 40) + 1, 1 << 50, 1 << 60, (1 << 63) + 5, 2 ** 64 - 2, 2 ** 64 - 1]
    found, lst, fig = check(ctx, from_runs(codes, counts), min_count=5000)
    assert fig["max_count"] == 5000 and fig["max_code"] == (1 << 40) + 1 and found == 3
    counts[5] = 5001
    assert check(ctx, from_runs(codes, counts))[2]["max_code"] == 1 << 60


def test_the_spectrum(ctx):
    rng = np.random.default_rng(4)
    counts = np.concatenate([rng.integers(1, 12, 3000), [5000, 4096, 4095, 300]])
    keys = from_runs(np.arange(len(counts), dtype=np.uint64) * np.uint64(3), counts)
    for nspec in (2, 3, 8, 256, 4097, 5001):                       # (two bins: everything in the last; 4097 and more: bins beyond those in LDS)
        found, lst, fig = check(ctx, keys, nspec=nspec)
        assert fig["spectrum"][nspec - 1] >= 1
    check(ctx, keys, nspec=0)                                       # no spectrum: the figures all the same


def test_min_count_and_a_list_shorter_than_what_was_found(ctx):
    rng = np.random.default_rng(6)
    codes = np.unique(rng.integers(0, 1 << 40, 8000, dtype=np.uint64))[:7000]
    counts = rng.integers(1, 9, len(codes))
    keys = from_runs(codes, counts)
    for min_count in (1, 2, 5, 8, 9):
        found, lst, fig = check(ctx, keys, min_count=min_count)
        assert found == int((counts >= min_count).sum())
    for cap in (0, 1, 100, 2049):
        found, lst, fig = check(ctx, keys, min_count=3, cap=cap)    # (check holds the entries behind cap against their mark)
        assert found == int((counts >= 3).sum()) > cap and len(lst) == cap


def test_the_method(ctx):
    keys = from_runs([1, 4, 9], [2, 1, 5])
    d = ctx.to_device(keys)
    try:
        found, lst, fig = ctx.kmer_runs(d, len(keys), 2, 10, nspec=4)
    finally:
        d.free()
    assert found == 2 and [(int(e["code"]), int(e["count"])) for e in lst] == [(1, 2), (9, 5)] and lst.dtype == api.KMER64_DTYPE
    assert fig["spectrum"].tolist() == [0, 1, 1, 1] and (fig["distinct"], fig["max_count"], fig["max_code"]) == (3, 5, 9)


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    f, spec = C.c_uint64(), np.zeros(4, np.uint64)
    try:
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 4, 0, None, 0, C.byref(f), None, 0, None, None, None) == E_ARG      # min_count 0
        assert b"min_count" in ctx.lib.dx_last_error(ctx.h)
        assert ctx.lib.dx_kmer_runs(ctx.h, None, 4, 1, None, 0, C.byref(f), None, 0, None, None, None) == E_ARG
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 4, 1, None, 2, C.byref(f), None, 0, None, None, None) == E_ARG      # a list and no place
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 4, 1, None, 0, None, None, 0, None, None, None) == E_ARG
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 4, 1, None, 0, C.byref(f), spec.ctypes.data, 1, None, None, None) == E_ARG
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 1 << 36, 1, None, 0, C.byref(f), None, 0, None, None, None) == E_ARG
        assert ctx.lib.dx_kmer_runs(ctx.h, d.ptr, 4, 1, None, 0, C.byref(f), None, 0, None, None, None) == 0 and f.value == 1
    finally:
        d.free()
