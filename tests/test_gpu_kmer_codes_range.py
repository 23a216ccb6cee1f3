"""Context.code_kmer_codes_range (dx_code_kmer_codes_range) on the GPU against the reference's array under a boolean mask
(tests/_kmers_files.py over tests/_kmers_wide.py): the WHOLE output is compared, place by place, in (unit, position) order, for the
units of _kmers_files.shapes -- what tests/test_gpu_kmer_bins.py counts -- over all bins, single bins, an empty range and a partition
into three; a cap one short; two calls; the words behind the kept codes.  And Context.sorted_take (dx_sorted_take) against np.unique.
No expected value comes from the library."""
import numpy as np
import pytest

import _kmers_files as KF
import _kmers_wide as W
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT, E_NOMEM = -1, -3, -6
GUARD = 8             # words behind the last kept code
MARK = np.uint64(0xC0DEC0DEC0DEC0DE)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def case(ctx):
    """the shapes of a k on the device and the reference's codes for them, made once a (k, canonical)"""
    have, bufs = {}, []

    def of(k, canonical):
        if (k, canonical) not in have:
            packed, boff, beg, ln, bad = KF.shapes(k, 100 + k)
            want, wbad = W.packed_codes(packed, boff, beg, ln, k, canonical)
            assert wbad == bad
            dev = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.asarray(boff, np.uint64)),
                   ctx.to_device(np.asarray(beg, np.uint32)), ctx.to_device(np.asarray(ln, np.uint32))]
            bufs.extend(dev)
            have[k, canonical] = (dev, len(packed), len(ln), bad, want)
        return have[k, canonical]
    yield of
    for b in bufs:
        b.free()


def take(ctx, c, k, canonical, bits, lo, hi, short=0):
    """one call against the reference: (the words as the device left them, guard included; the kept codes wanted; the error or None)"""
    dev, nbytes, n, bad, want = c
    kept = want[KF.in_range(want, k, bits, lo, hi)]
    cap = len(kept) - short
    d_codes = ctx.alloc(8 * (len(kept) + GUARD)).upload(np.full(len(kept) + GUARD, MARK))
    err = None
    try:
        try:
            _, windows = ctx.code_kmer_codes_range(dev[0], dev[1], dev[2], dev[3], k, bits, lo, hi, canonical, cap=cap, codes=d_codes,
                                                   in_bytes=nbytes, n=n)
        except L.DexGPUError as e:
            err, windows = e, e.windows
        got = d_codes.download(np.uint64, len(kept) + GUARD)
    finally:
        d_codes.free()
    assert windows == len(kept)
    assert (got[len(kept):] == MARK).all(), "a word behind the last kept code was written"
    return got, kept, err


def check(ctx, c, k, canonical, bits, lo, hi):
    got, kept, err = take(ctx, c, k, canonical, bits, lo, hi)
    assert err is not None and err.code == E_FORMAT and err.bad_unit == c[3]          # (the shapes hold one unit outside the buffer)
    assert np.array_equal(got[:len(kept)], kept), (k, canonical, bits, lo, hi, np.flatnonzero(got[:len(kept)] != kept)[:5])
    return got[:len(kept)]


@pytest.mark.parametrize("k,canonical", KF.KS, ids=[f"k{k}{'c' if c else ''}" for k, c in KF.KS])
def test_all_bins_single_bins_an_empty_range_and_a_partition(ctx, case, k, canonical):
    c = case(k, canonical)
    dev, nbytes, n, bad, want = c
    bits = KF.bits_for(k)
    nbins, ref = 1 << bits, KF.bins(want, k, bits)
    assert len(check(ctx, c, k, canonical, bits, 0, nbins)) == len(want) > 0
    fullest = int(np.argmax(ref))
    for b in sorted({0, nbins - 1, fullest, int(np.flatnonzero(ref)[0]), int(np.flatnonzero(ref)[-1])}):
        assert len(check(ctx, c, k, canonical, bits, b, b + 1)) == int(ref[b])
    for lo in (0, fullest, nbins):                                 # an empty range keeps nothing
        assert len(check(ctx, c, k, canonical, bits, lo, lo)) == 0
    if k >= 2:                                                     # fewer bits than the planner takes: a bin is several of its
        few = min(3, bits - 1)
        assert len(check(ctx, c, k, canonical, few, 1, 2)) == int(KF.bins(want, k, few)[1])

    # three ranges of about a third of the windows each: what they keep, sorted, is what dx_code_kmer_codes writes, sorted
    cum = np.cumsum(ref.astype(np.int64))
    a, b = int(np.searchsorted(cum, cum[-1] // 3)), int(np.searchsorted(cum, 2 * cum[-1] // 3))
    cuts = [0, min(a + 1, nbins), min(max(b + 1, a + 1), nbins), nbins]
    parts = [check(ctx, c, k, canonical, bits, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    d_all = ctx.alloc(8 * len(want) + 8)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_codes(dev[0], dev[1], dev[2], dev[3], k, canonical, cap=len(want), codes=d_all, in_bytes=nbytes, n=n)
        assert e.value.code == E_FORMAT and e.value.bad_unit == bad
        whole = d_all.download(np.uint64, len(want))
    finally:
        d_all.free()
    assert sum(len(p) for p in parts) == len(want)
    assert np.array_equal(np.sort(np.concatenate(parts)), np.sort(whole))
    assert all(len(p) == 0 or len(q) == 0 or p.max() < q.min() for p, q in zip(parts[:-1], parts[1:]))       # the ranges ascend


@pytest.mark.parametrize("k,canonical", [(7, True), (21, False), (32, True)])
def test_a_cap_one_short_is_nomem_and_nothing_is_written(ctx, case, k, canonical):
    c = case(k, canonical)
    bits = KF.bits_for(k)
    ref = KF.bins(c[4], k, bits)
    lo = int(np.argmax(ref))
    got, kept, err = take(ctx, c, k, canonical, bits, lo, min(lo + 2, 1 << bits), short=1)
    assert len(kept) > 1 and err is not None and err.code == E_NOMEM and str(len(kept)) in str(err)
    assert (got == MARK).all()


@pytest.mark.parametrize("k,canonical", [(6, False), (21, True)])
def test_two_calls_give_identical_bytes(ctx, case, k, canonical):
    c = case(k, canonical)
    bits = KF.bits_for(k)
    nbins = 1 << bits
    a = take(ctx, c, k, canonical, bits, nbins // 8, nbins - nbins // 8)[0]
    b = take(ctx, c, k, canonical, bits, nbins // 8, nbins - nbins // 8)[0]
    assert len(a) > GUARD + 1000 and a.tobytes() == b.tobytes()


def test_units_without_d_beg_and_no_units(ctx):
    rng, b = np.random.default_rng(5), KF.Buffer()
    for j, n in enumerate([21, 70, 300, 0, 1100, 5003, 20]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=0)
    packed = b.packed()
    want, _ = W.packed_codes(packed, b.boff, None, b.ln, 21, True)
    kept = want[KF.in_range(want, 21, 12, 100, 3000)]
    dev = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.asarray(b.boff, np.uint64)), ctx.to_device(np.asarray(b.ln, np.uint32))]
    codes = None
    try:
        codes, windows = ctx.code_kmer_codes_range(dev[0], dev[1], None, dev[2], 21, 12, 100, 3000, canonical=True)      # (an array made by the method)
        assert windows == len(kept) > 0 and np.array_equal(codes.download(np.uint64, windows), kept)
        _, windows = ctx.code_kmer_codes_range(dev[0], dev[1], None, dev[2], 21, 12, 0, 4096, codes=codes, cap=0, n=0)
        assert windows == 0
    finally:
        for x in dev + [codes]:
            if x is not None:
                x.free()


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    try:
        for k, bits, lo, hi, word in ((0, 1, 0, 1, "k = 0"), (33, 12, 0, 1, "k = 33"), (21, 0, 0, 1, "bits = 0"), (21, 13, 0, 1, "bits = 13"),
                                      (3, 7, 0, 1, "bits = 7"), (21, 12, 5, 4, "bins [5, 4)"), (21, 12, 0, 4097, "bins [0, 4097)")):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_codes_range(d, d, None, d, k, bits, lo, hi, codes=d, cap=4, in_bytes=16, n=1)
            assert e.value.code == E_ARG and word in str(e.value)
        for args in ((None, d, d), (d, None, d), (d, d, None)):                       # the buffer, the offsets, the lengths
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_codes_range(args[0], args[1], None, args[2], 21, 12, 0, 4096, codes=d, cap=4, in_bytes=16, n=1)
            assert e.value.code == E_ARG
        win = api.C.c_uint64()
        lib = ctx.lib
        assert lib.dx_code_kmer_codes_range(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, 12, 0, 4096, None, 4, api.C.byref(win), None) == E_ARG
        assert lib.dx_code_kmer_codes_range(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, 12, 0, 4096, d.ptr, 4, None, None) == E_ARG
        assert lib.dx_code_kmer_codes_range(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, 21, 0, 12, 0, 4096, d.ptr, 4, api.C.byref(win), None) == E_ARG
    finally:
        d.free()


# ---- dx_sorted_take --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 20000])
def test_sorted_take_is_np_unique(ctx, n):
    """runs that are longer than a tile (2048 keys), that end at a tile's last key and begin at its first; the top bit in use"""
    rng = np.random.default_rng(n)
    keys = np.sort(np.concatenate([rng.integers(0, max(n // 4, 2), n // 2).astype(np.uint64), np.full(n - n // 2 - n // 8, 2 ** 64 - 5, np.uint64),
                                   np.full(n // 8, 7, np.uint64)]))
    assert len(keys) == n
    seen, cnt = np.unique(keys, return_counts=True)
    d = ctx.to_device(keys) if n else ctx.alloc(16)
    try:
        for min_count in (1, 2, 5):
            want = seen[cnt >= min_count]
            for cap in sorted({0, 1, len(want) // 2, max(len(want) - 1, 0), len(want), len(want) + 3}):
                found, got = ctx.sorted_take(d, n, min_count, cap)
                assert found == len(want) and np.array_equal(got, want[:cap]), (n, min_count, cap)
        with pytest.raises(L.DexGPUError) as e:
            ctx.sorted_take(d, n, 0, 4)
        assert e.value.code == E_ARG and "min_count" in str(e.value)
    finally:
        d.free()


def test_sorted_take_writes_nothing_at_cap_or_beyond(ctx):
    keys = np.repeat(np.arange(5000, dtype=np.uint64) * np.uint64(3), 2)
    d, out = ctx.to_device(keys), ctx.alloc(8 * 64).upload(np.full(64, MARK))
    try:
        found = api.C.c_uint64()
        assert ctx.lib.dx_sorted_take(ctx.h, d.ptr, len(keys), 2, out.ptr, 40, api.C.byref(found)) == 0 and found.value == 5000
        got = out.download(np.uint64, 64)
        assert np.array_equal(got[:40], np.arange(40, dtype=np.uint64) * np.uint64(3)) and (got[40:] == MARK).all()
        assert ctx.lib.dx_sorted_take(ctx.h, d.ptr, len(keys), 2, None, 40, api.C.byref(found)) == E_ARG
        assert ctx.lib.dx_sorted_take(ctx.h, d.ptr, len(keys), 2, out.ptr, 40, None) == E_ARG
    finally:
        d.free()
        out.free()
