"""Context.code_kmer_bins (dx_code_kmer_bins) on the GPU against np.bincount of the reference's codes (tests/_kmers_files.py over
tests/_kmers_wide.py), compared exactly: the units of _kmers_files.shapes -- every byte offset and phase, the lengths at the seams of
the kernel's three routes, units that overlap and repeat, a unit that ends in the buffer's last byte, one unit outside the buffer --
for every k and every width of the bins; adding twice; the sweep of the LDS cells forced at small shapes (bins_flush); a homopolymer.
Everything that is not a unit is Ts, so a window that reaches outside its unit falls into a bin the reference does not count it in.
No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_files as KF
import _kmers_wide as W
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3
BITS = [1, 2, 6, 11, 12]


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


def count(ctx, dev, nbytes, n, k, canonical, bits, bins=None, bad=None):
    """one call: (the bins as the device holds them, the windows); with `bad` the call must be DX_E_FORMAT and name that unit"""
    d_bins = bins if bins is not None else ctx.alloc(8 << bits).zero()
    try:
        if bad is None:
            _, windows = ctx.code_kmer_bins(dev[0], dev[1], dev[2], dev[3], k, bits, canonical, bins=d_bins, in_bytes=nbytes, n=n)
        else:
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_bins(dev[0], dev[1], dev[2], dev[3], k, bits, canonical, bins=d_bins, in_bytes=nbytes, n=n)
            assert e.value.code == E_FORMAT and e.value.bad_unit == bad
            windows = e.value.windows
        return d_bins.download(np.uint64, 1 << bits), windows
    finally:
        if bins is None:
            d_bins.free()


@pytest.mark.parametrize("k,canonical", KF.KS, ids=[f"k{k}{'c' if c else ''}" for k, c in KF.KS])
def test_every_route_offset_and_phase_at_every_width(ctx, case, k, canonical):
    dev, nbytes, n, bad, want = case(k, canonical)
    for bits in sorted({KF.bits_for(k, b) for b in BITS}):
        got, windows = count(ctx, dev, nbytes, n, k, canonical, bits, bad=bad)     # (the bad unit's windows are not counted)
        ref = KF.bins(want, k, bits)
        assert windows == len(want) == int(ref.sum())
        assert np.array_equal(got, ref), (k, canonical, bits, np.flatnonzero(got != ref)[:5])


@pytest.mark.parametrize("k,canonical", [(6, False), (21, True)])
def test_adding_twice_doubles_the_counts(ctx, case, k, canonical):
    dev, nbytes, n, bad, want = case(k, canonical)
    bits = KF.bits_for(k)
    d_bins = ctx.alloc(8 << bits).zero()
    try:
        count(ctx, dev, nbytes, n, k, canonical, bits, bins=d_bins, bad=bad)
        got, windows = count(ctx, dev, nbytes, n, k, canonical, bits, bins=d_bins, bad=bad)
    finally:
        d_bins.free()
    assert windows == len(want) and np.array_equal(got, 2 * KF.bins(want, k, bits))


@pytest.mark.parametrize("k,canonical,bits", [(1, False, 2), (7, True, 6), (21, True, 12), (32, False, 11)])
def test_the_sweep_gives_the_same_counts(ctx, case, monkeypatch, k, canonical, bits):
    """DEXGPU_TEST=bins_flush=64: a wave sweeps the workgroup's cells into the global words after every round and every step"""
    dev, nbytes, n, bad, want = case(k, canonical)
    set_flag(monkeypatch, "bins_flush", "64")
    got, windows = count(ctx, dev, nbytes, n, k, canonical, bits, bad=bad)
    assert windows == len(want) and np.array_equal(got, KF.bins(want, k, bits))


@pytest.mark.parametrize("k,canonical", [(1, False), (7, True), (32, True), (32, False)])
def test_a_homopolymer_is_one_bin(ctx, k, canonical):
    packed = F.pack(np.concatenate([np.full(7, KF.T), np.full(5000, 2), np.full(9, KF.T)]).astype(np.uint8), pad=0xff)
    dev = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array([1], np.uint64)), ctx.to_device(np.array([3], np.uint32)),
           ctx.to_device(np.array([5000], np.uint32))]
    try:
        bits = KF.bits_for(k)
        got, windows = count(ctx, dev, len(packed), 1, k, canonical, bits)
    finally:
        for b in dev:
            b.free()
    code = int(W.unit_codes(np.full(k, 2, np.uint8), k, canonical)[0])          # GG..G, or CC..C under canonical
    assert windows == 5000 - k + 1 and np.flatnonzero(got).tolist() == [code >> (2 * k - bits)] and int(got.sum()) == windows


def test_no_units_and_refusals(ctx):
    d = ctx.alloc(8 << 12).zero()
    try:
        _, windows = ctx.code_kmer_bins(d, d, None, d, 21, 12, bins=d, in_bytes=16, n=0)
        assert windows == 0 and not d.download(np.uint64, 1 << 12).any()
        for k, bits in ((0, 1), (33, 12), (21, 0), (21, 13), (3, 7), (1, 3)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_bins(d, d, None, d, k, bits, bins=d, in_bytes=16, n=1)
            assert e.value.code == E_ARG and ("k = %d" % k if k in (0, 33) else "bits = %d" % bits) in str(e.value)
        for args in ((None, d, d), (d, None, d), (d, d, None)):                       # the buffer, the offsets, the lengths
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_bins(args[0], args[1], None, args[2], 21, 12, bins=d, in_bytes=16, n=1)
            assert e.value.code == E_ARG
        win = api.C.c_uint64()
        assert ctx.lib.dx_code_kmer_bins(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, 12, None, api.C.byref(win), None) == E_ARG
        assert ctx.lib.dx_code_kmer_bins(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, 21, 0, 12, d.ptr, api.C.byref(win), None) == E_ARG
        assert ctx.lib.dx_code_kmer_bins(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, 12, d.ptr, None, None) == 0    # (windows may be NULL)
    finally:
        d.free()
