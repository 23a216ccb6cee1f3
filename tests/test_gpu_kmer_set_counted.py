"""Counted k-mer sets on the GPU against tests/_depth.py: Context.kmer_set_from_kmers (pairs in any order, equal codes adding, the two
strands of a k-mer folding into one, zero counts dropped, saturation) and Context.kmer_set_from_sorted_counted (runs that begin and end
on both sides of the seams of the 2048-key tiles and span whole tiles).  The codes are what the uncounted makers give, the counts are
numpy's; a forced index width changes nothing; the screen ignores the counts.  No expected value comes from the library."""
import numpy as np
import pytest

import _depth as D
import _kmers_wide as W
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM = -1, -6
U = np.uint64
KS = [1, 16, 32]
TILE = 2048           # TL_TILE (csrc/tiles/dx_tiles.hpp)
RUNS = [1, 2, 2047, 2048, 2049, 5000]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def mask(k):
    return U(4 ** k - 1 if k < 32 else 2 ** 64 - 1)


def same_set(s, codes, counts, k, canonical=False):
    assert s.counted is True and np.array_equal(s.codes(), codes), (s.codes()[:5], codes[:5])
    got = s.counts()
    assert got.dtype == np.uint32 and np.array_equal(got, counts), (got[:8], counts[:8])
    info = s.info
    assert (info["codes"], info["k"], info["canonical"]) == (len(codes), k, int(canonical))


# ---- from_kmers ------------------------------------------------------------------------------------------------------------------------
def some_pairs(k, seed, n=3000):
    """shuffled pairs: codes that repeat (their counts add), zero counts among them"""
    rng = np.random.default_rng(seed)
    base = np.unique(rng.integers(0, 2 ** 63, n, dtype=np.uint64) & mask(k))
    code = rng.choice(base, 2 * len(base))
    count = rng.integers(0, 9, len(code)) * rng.integers(1, 2000, len(code))
    return [(int(c), int(x)) for c, x in zip(code, count)]


@pytest.mark.parametrize("bits", [None, 1], ids=["natural", "set_bits1"])
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_from_kmers_shuffled_repeated_and_folded(ctx, monkeypatch, k, canonical, bits):
    if bits is not None:
        set_flag(monkeypatch, "set_bits", bits)
    pairs = some_pairs(k, 10 + k)
    codes, counts = D.from_kmers(pairs, k, canonical)
    assert 0 < len(codes) <= len({p[0] for p in pairs if p[1]})
    with ctx.kmer_set_from_kmers(pairs, k, canonical) as s, ctx.kmer_set_from_codes([p[0] for p in pairs if p[1]], k, canonical) as plain:
        same_set(s, codes, counts, k, canonical)
        assert plain.counted is False and np.array_equal(plain.codes(), codes)           # the codes of the uncounted maker
        assert s.info["device_bytes"] == plain.info["device_bytes"] + 4 * len(codes)
        assert s.info["index_bits"] == (bits if bits is not None else plain.info["index_bits"])
        with pytest.raises(L.DexGPUError) as e:
            plain.counts()
        assert e.value.code == E_ARG and "not counted" in str(e.value)


def test_from_kmers_the_two_strands_of_one_k_mer_add_into_one(ctx):
    k = 16
    rng = np.random.default_rng(2)
    fwd = np.unique(rng.integers(0, 4 ** k, 500, dtype=np.uint64))
    rev = W.rc(fwd, k)
    pairs = [(int(c), 3) for c in fwd] + [(int(c), 4) for c in rev]
    codes, counts = D.from_kmers(pairs, k, True)
    assert len(codes) == len(fwd) and (counts == 7).sum() >= len(fwd) - 2                   # (a palindrome would count 7 as well)
    with ctx.kmer_set_from_kmers(pairs, k, canonical=True) as s:
        same_set(s, codes, counts, k, True)
    with ctx.kmer_set_from_kmers(pairs, k, canonical=False) as s:                           # unfolded, they stay apart
        same_set(s, *D.from_kmers(pairs, k, False), k)


def test_from_kmers_zero_counts_saturation_and_the_empty_list(ctx):
    k = 21
    pairs = [(5, 2 ** 32 - 2), (9, 0), (5, 5), (7, 2 ** 33), (11, 2 ** 32 - 1), (12, 2 ** 32 - 2), (13, 1), (13, 2 ** 32 - 3), (14, 2 ** 64 - 1),
             (14, 2 ** 64 - 1), (3, 0), (3, 1)]
    codes, counts = D.from_kmers(pairs, k)
    assert codes.tolist() == [3, 5, 7, 11, 12, 13, 14] and counts.tolist() == [1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 2,
                                                                                 2 ** 32 - 2, 2 ** 32 - 1]
    with ctx.kmer_set_from_kmers(pairs, k) as s:
        same_set(s, codes, counts, k)
    for empty in ([], [(4, 0), (6, 0)]):
        with ctx.kmer_set_from_kmers(empty, k) as s:
            same_set(s, np.zeros(0, U), np.zeros(0, np.uint32), k)
    lst = np.zeros(3, api.KMER64_DTYPE)                              # the list of kmers_wide, as an array
    lst["code"], lst["count"] = [8, 2, 8], [1, 6, 2]
    with ctx.kmer_set_from_kmers(lst, k) as s:
        same_set(s, np.array([2, 8], U), np.array([6, 3], np.uint32), k)


def test_from_kmers_refusals(ctx):
    h = api.C.c_void_p()
    one = (L.Kmer64 * 2)()
    one[0].code, one[0].count, one[1].code, one[1].count = 1, 1, 4 ** 15, 1
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_set_from_kmers([(1, 1), (4 ** 15, 1)], 15)
    assert e.value.code == E_ARG and "code 1 " in str(e.value)                               # the index is named
    for k, canonical, arrow in ((0, 0, 0), (33, 0, 0), (15, 1, 1)):
        assert ctx.lib.dx_kmer_set_from_kmers(ctx.h, one, 1, k, canonical, arrow, api.C.byref(h)) == E_ARG and h.value is None
    assert ctx.lib.dx_kmer_set_from_kmers(ctx.h, None, 1, 15, 0, 0, api.C.byref(h)) == E_ARG
    assert ctx.lib.dx_kmer_set_from_kmers(ctx.h, one, 1, 15, 0, 0, None) == E_ARG
    with ctx.kmer_set_from_kmers([(1, 1)], 15) as s:
        buf = (api.C.c_uint32 * 1)()
        assert ctx.lib.dx_kmer_set_counts(ctx.h, s.h, None, 1) == E_ARG
        assert ctx.lib.dx_kmer_set_counts(ctx.h, s.h, buf, 0) == E_NOMEM
        assert ctx.lib.dx_kmer_set_counts(ctx.h, None, buf, 1) == E_ARG


# ---- from_sorted_counted ---------------------------------------------------------------------------------------------------------------
def run_arrays(k, seed):
    """sorted arrays whose runs have every length of RUNS, in an order that puts their ends on both sides of tile seams; k = 1 has four
    codes, so the lengths take two arrays there"""
    if k == 1:
        return [np.repeat(np.arange(4, dtype=U), lens) for lens in ([1, 2047, 2048, 2], [2049, 5000, 1, 2])]
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.array(RUNS * 3 + [1] * 40 + [2] * 20))
    code = np.sort(rng.choice(np.unique(rng.integers(0, 2 ** 63, 4 * len(lens), dtype=np.uint64) & mask(k)), len(lens), replace=False))
    if k == 32:
        code[-1] = U(2 ** 64 - 1)                                    # the top bit in use
    return [np.repeat(code, lens)]


@pytest.mark.parametrize("bits", [None, 1], ids=["natural", "set_bits1"])
@pytest.mark.parametrize("min_count", [1, 2, 2049])
@pytest.mark.parametrize("k", KS)
def test_from_sorted_counted_runs_across_tile_seams(ctx, monkeypatch, k, min_count, bits):
    if bits is not None:
        set_flag(monkeypatch, "set_bits", bits)
    seen = set()
    for a in run_arrays(k, 50 + k):
        codes, counts = D.from_sorted(a, min_count)
        assert len(a) > 2 * TILE
        seen |= set(np.unique(a, return_counts=True)[1].tolist())
        d = ctx.to_device(a)
        try:
            with ctx.kmer_set_from_sorted_counted(d, len(a), k, min_count) as s, ctx.kmer_set_from_sorted(d, len(a), k, min_count) as plain:
                same_set(s, codes, counts, k)
                assert plain.counted is False and plain.codes().tobytes() == s.codes().tobytes()
                with ctx.kmer_set_from_sorted_counted(d, len(a), k, min_count) as again:   # the same bytes on every call
                    assert again.counts().tobytes() == s.counts().tobytes() and again.codes().tobytes() == s.codes().tobytes()
        finally:
            d.free()
    assert seen == set(RUNS)


def test_from_sorted_counted_seams_exactly(ctx):
    """runs laid out by hand: one ends at a seam, one begins there, one spans two whole tiles, one is the array's last key"""
    k = 16
    lens = [TILE - 1, 1, 1, TILE - 2, 2 * TILE, 2, TILE + 1, 2049, 1]
    a = np.repeat(np.arange(7, 7 + 3 * len(lens), 3, dtype=U), lens)
    d = ctx.to_device(a)
    try:
        for min_count in (1, 2, 2049, 2 * TILE, 2 * TILE + 1):
            codes, counts = D.from_sorted(a, min_count)
            with ctx.kmer_set_from_sorted_counted(d, len(a), k, min_count) as s:
                same_set(s, codes, counts, k)
        with ctx.kmer_set_from_sorted_counted(None, 0, k, 1) as s:                            # no key at all
            same_set(s, np.zeros(0, U), np.zeros(0, np.uint32), k)
        h = api.C.c_void_p()
        assert ctx.lib.dx_kmer_set_from_sorted_counted(ctx.h, d.ptr, len(a), 0, k, 0, 0, api.C.byref(h)) == E_ARG        # min_count 0
        assert ctx.lib.dx_kmer_set_from_sorted_counted(ctx.h, None, len(a), 1, k, 0, 0, api.C.byref(h)) == E_ARG
        assert ctx.lib.dx_kmer_set_from_sorted_counted(ctx.h, d.ptr, len(a), 1, 33, 0, 0, api.C.byref(h)) == E_ARG and h.value is None
    finally:
        d.free()


# ---- the screen ignores the counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_screen_of_a_counted_set_is_the_screen_of_its_codes(ctx, k):
    rng, b = np.random.default_rng(k), D.Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, 257]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=j % 4, guard=8, tail=8)
    own = np.unique(W.all_codes(b.units, k, k != 32))
    codes = own[::2] if len(own) > 4 else own[:1]
    pairs = [(int(c), int(x)) for c, x in zip(codes, rng.integers(1, 2 ** 32, len(codes)))]
    d_in, d_boff = ctx.to_device(np.frombuffer(b.packed(), np.uint8)), ctx.to_device(np.asarray(b.boff, np.uint64))
    d_beg, d_len = ctx.to_device(np.asarray(b.beg, np.uint32)), ctx.to_device(np.asarray(b.ln, np.uint32))
    n = len(b.ln)
    outs = [ctx.alloc(16 * n).zero() for _ in range(2)]
    try:
        with ctx.kmer_set_from_kmers(pairs, k, canonical=k != 32) as s, ctx.kmer_set_from_codes(codes, k, canonical=k != 32) as plain:
            t0 = ctx.code_kmer_screen(d_in, d_boff, d_beg, d_len, s, out=outs[0], n=n)
            t1 = ctx.code_kmer_screen(d_in, d_boff, d_beg, d_len, plain, out=outs[1], n=n)
            sp0 = ctx.code_kmer_spans(d_in, d_boff, d_beg, d_len, s, cap=8192, n=n)
            sp1 = ctx.code_kmer_spans(d_in, d_boff, d_beg, d_len, plain, cap=8192, n=n)
        assert t0.tolist() == t1.tolist() and 0 < t0[1] < t0[0]
        assert outs[0].download(np.uint8, 16 * n).tobytes() == outs[1].download(np.uint8, 16 * n).tobytes()
        assert sp0[0].tolist() == sp1[0].tolist() and sp0[1].tobytes() == sp1[1].tobytes()
    finally:
        for x in (d_in, d_boff, d_beg, d_len, *outs):
            x.free()
