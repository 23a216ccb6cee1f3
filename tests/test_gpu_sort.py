"""Context.sort_u64 (dx_sort_u64) on the GPU against np.sort: every size around a wave, a tile of the sort (4096 keys) and a tile of the
prefix sum; every pass count, keys drawn below 2^bits; the distributions a radix sort can go wrong on -- all keys equal, sorted,
reversed, keys that differ in one digit only, one value that is 90 % of the keys --; the words in front of and behind both arrays;
and the refusals.  No expected value comes from the library."""
import ctypes as C

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
TILE = 4096                                                        # SORT_TILE of csrc/sort/dx_sort.hip
GUARD = 4                                                          # words in front of and behind an array
MARK = np.uint64(0xA5C3A5C3A5C3A5C3)
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 100003, (1 << 20) + 1]
BITS = [1, 2, 8, 9, 28, 30, 42, 62, 64]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def draw(rng, n, bits):
    k = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)      # all 64 bits
    return k if bits == 64 else k & np.uint64((1 << bits) - 1)


def sort_guarded(ctx, keys, bits):
    """the keys sorted on the device, between guard words; the guards of both arrays are held against what was put there"""
    keys = np.ascontiguousarray(keys, np.uint64)
    n = len(keys)
    host = np.concatenate([np.full(GUARD, MARK), keys, np.full(GUARD, MARK)])
    d_keys, d_tmp = ctx.alloc(8 * (n + 2 * GUARD)), ctx.alloc(8 * (n + 2 * GUARD))
    try:
        d_keys.upload(host)
        d_tmp.upload(np.full(n + 2 * GUARD, MARK))
        ctx._chk(ctx.lib.dx_sort_u64(ctx.h, d_keys.ptr + 8 * GUARD, d_tmp.ptr + 8 * GUARD, n, bits))
        got, tmp = d_keys.download(np.uint64, n + 2 * GUARD), d_tmp.download(np.uint64, n + 2 * GUARD)
    finally:
        d_keys.free(); d_tmp.free()
    for a in (got, tmp):
        assert (a[:GUARD] == MARK).all() and (a[GUARD + n:] == MARK).all(), "a guard word was written"
    return got[GUARD:GUARD + n]


def check(ctx, keys, bits):
    got = sort_guarded(ctx, keys, bits)
    want = np.sort(np.asarray(keys, np.uint64), kind="stable")
    assert np.array_equal(got, want), (len(keys), bits, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    rng = np.random.default_rng(n + 1)
    check(ctx, draw(rng, n, 64), 64)
    check(ctx, draw(rng, n, 42), 42)                               # (six passes: the keys end where they began)
    check(ctx, draw(rng, n, 9), 9)                                 # (two passes, the second of one bit)
    check(ctx, draw(rng, n, 8), 8)                                 # (one pass: the keys come back from the second array)


@pytest.mark.parametrize("bits", BITS)
def test_bits(ctx, bits):
    rng = np.random.default_rng(bits)
    for n in (1000, 3 * TILE + 17):
        check(ctx, draw(rng, n, bits), bits)


def test_bits_zero_and_no_keys_do_nothing(ctx):
    keys = np.array([5, 3, 9, 1], np.uint64)
    assert np.array_equal(sort_guarded(ctx, keys, 0), keys)
    assert len(sort_guarded(ctx, np.zeros(0, np.uint64), 64)) == 0
    assert ctx.lib.dx_sort_u64(ctx.h, None, None, 0, 64) == 0


def test_only_the_digits_under_bits_are_looked_at(ctx):
    """the caller's promise is the caller's: with bits = 16 the keys come back in the order of their low 16 bits, stable above"""
    rng = np.random.default_rng(5)
    keys = draw(rng, 3 * TILE + 5, 64)
    got = sort_guarded(ctx, keys, 16)
    want = keys[np.argsort(keys & np.uint64(0xffff), kind="stable")]
    assert np.array_equal(got, want)


DISTRIBUTIONS = ["equal", "sorted", "reversed", "top_digit", "low_digit", "extremes", "ninety"]


@pytest.mark.parametrize("what", DISTRIBUTIONS)
def test_distributions(ctx, what):
    rng = np.random.default_rng(DISTRIBUTIONS.index(what))
    n = 5 * TILE + 123
    if what == "equal":
        keys = np.full(n, 0x0123456789ABCDEF, np.uint64)
    elif what == "sorted":
        keys = np.sort(draw(rng, n, 64))
    elif what == "reversed":
        keys = np.sort(draw(rng, n, 64))[::-1]
    elif what == "top_digit":
        keys = (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00123456789ABCDE)
    elif what == "low_digit":
        keys = np.uint64(0xFEDCBA9876543200) | rng.integers(0, 256, n, dtype=np.uint64)
    elif what == "extremes":
        keys = draw(rng, n, 64)
        keys[rng.integers(0, n, 40)] = np.uint64(0)
        keys[rng.integers(0, n, 40)] = np.uint64(2 ** 64 - 1)
        keys[0], keys[-1] = np.uint64(2 ** 64 - 1), np.uint64(0)
    else:                                                          # one value is 90 % of the keys: a poly-A's code
        keys = draw(rng, n, 64)
        keys[rng.random(n) < 0.9] = np.uint64(0x5555AAAA5555AAAA)
    check(ctx, keys, 64)


def test_the_method_sorts_in_place_with_a_second_array_of_its_own(ctx):
    rng = np.random.default_rng(77)
    keys = draw(rng, 2 * TILE + 1, 30)
    d = ctx.alloc(8 * len(keys)).upload(keys)
    try:
        assert ctx.sort_u64(d, 30) is d
        assert np.array_equal(d.download(np.uint64, len(keys)), np.sort(keys))
    finally:
        d.free()


def test_refusals(ctx):
    d = ctx.alloc(64).zero()
    try:
        for args in ((d.ptr, d.ptr + 32, 4, 65), (None, d.ptr, 4, 64), (d.ptr, None, 4, 64), (d.ptr, d.ptr + 32, 1 << 36, 64)):
            assert ctx.lib.dx_sort_u64(ctx.h, *args) == E_ARG, args
            assert b"dx_sort_u64" in ctx.lib.dx_last_error(ctx.h)
        with pytest.raises(L.DexGPUError) as e:
            ctx.sort_u64(d, 65, n=4)
        assert e.value.code == E_ARG
    finally:
        d.free()
