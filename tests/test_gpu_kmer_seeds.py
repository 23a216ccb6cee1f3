"""Context.code_kmer_seeds (dx_code_kmer_seeds) on the GPU against the numpy statement of tests/_place.py: the WHOLE seed list, the
units' counts and places and the four totals are compared -- units at every phase and byte offset, lengths around 64, 256 and
KC_GROUP chunks and below k, reads that are slices of the reference of either strand with substitutions, max_occ of 1 and 2 and
above and below a repeated code's count, counting alone, a list one short, a bad unit in the middle, units that overlap and repeat, an
empty index, and the same bytes on two calls.  Behind the last seed stand guard entries.  No expected value comes from the library."""
import numpy as np
import pytest

import _place as P
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

CHUNK, LANE, GROUP = 64, 4, 16          # KC_CHUNK, KC_LANE, KC_GROUP (csrc/kmers/dx_kmer_windows.hpp)
E_ARG, E_FORMAT, E_NOMEM = -1, -3, -6
GUARD, MARK = 8, 0xC0DEC0DE
U = np.uint64
REPEAT = 5                              # how often the repeated piece stands in the reference


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def reference(seed):
    """three targets; a piece of 200 symbols stands REPEAT times in them, once on the other strand"""
    rng = np.random.default_rng(seed)
    piece = rng.integers(0, 4, 200).astype(np.uint8)
    a = np.concatenate([rng.integers(0, 4, 2500).astype(np.uint8), piece, rng.integers(0, 4, 900).astype(np.uint8), piece])
    b = np.concatenate([piece, rng.integers(0, 4, 700).astype(np.uint8), (3 - piece)[::-1], rng.integers(0, 4, 50).astype(np.uint8)])
    c = np.concatenate([rng.integers(0, 4, 1300).astype(np.uint8), piece])
    return [a, b, c], piece


def lengths(k):
    return sorted({0, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, LANE * CHUNK - 1, LANE * CHUNK + 1, GROUP * CHUNK - k, GROUP * CHUNK + 1, 2300,
                   4097, 5003})                                               # (more than 64 chunks: a second step of the wave path)


def reads_of(targets, k, seed, piece=None):
    """a read of every length: a slice of a target, every second one of the other strand, a few symbols replaced; the last unit is
    the repeated piece itself"""
    rng, b = np.random.default_rng(seed), P.Buffer()
    for j, n in enumerate(lengths(k) * 2):
        t = targets[j % 2 * 2 if n > 1000 else j % 3]                        # (the long ones from the long targets)
        if n > len(t):
            t = np.concatenate([t] * (n // len(t) + 1))                       # (a read longer than its target: the target over and over)
        at = int(rng.integers(0, len(t) - n + 1))
        s = np.array(t[at:at + n], np.uint8)
        hit = rng.random(n) < 0.02
        s[hit] = (s[hit] + 1) % 4
        if j % 2:
            s = (3 - s)[::-1]
        b.add(s, phase=(5 * j) % 16, beg=j % 4 + 4 * (j % 3), guard=6, tail=6)
    assert {o % 16 for o in b.boff} == set(range(16))
    if piece is not None:
        b.add(piece, guard=6, tail=6)
    return b


def run(ctx, x, want_x, packed, boff, beg, ln, max_occ, cap=None, in_bytes=None, with_count=True, with_off=True):
    """one call against the statement: (the list's bytes, counts, off, totals, the error or None)"""
    units, bad = P.packed_units(packed, boff, beg, ln, in_bytes)
    want, woff, wtot = P.seeds(units, want_x, max_occ)
    n, total = len(ln), len(want)
    cap = total if cap is None else cap
    d_in = ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16)
    d_boff, d_len = ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(ln, np.uint32))
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    d_seeds = ctx.alloc(16 * (total + GUARD)).upload(np.full(4 * (total + GUARD), MARK, np.uint32))
    d_cnt = ctx.alloc(4 * (n + 2)).upload(np.full(n + 2, MARK, np.uint32))
    d_off = ctx.alloc(8 * (n + 3)).upload(np.full(n + 3, 2 ** 64 - 1, np.uint64))
    err = None
    try:
        try:
            tot, _ = ctx.code_kmer_seeds(d_in, d_boff, d_beg, d_len, x, max_occ=max_occ, count=d_cnt if with_count else None,
                                         off=d_off if with_off else None, cap=cap, seeds=d_seeds,
                                         in_bytes=len(packed) if in_bytes is None else in_bytes, n=n)
        except L.DexGPUError as e:
            err, tot = e, e.totals
        raw = d_seeds.download(np.uint32, 4 * (total + GUARD))
        cnt, off = d_cnt.download(np.uint32, n + 2), d_off.download(np.uint64, n + 3)
    finally:
        for v in (d_in, d_boff, d_len, d_beg, d_seeds, d_cnt, d_off):
            if v is not None:
                v.free()
    assert (raw[4 * total:] == MARK).all(), "an entry behind the last seed was written"
    assert (cnt[n:] == MARK).all() and (off[n + 1:] == U(2 ** 64 - 1)).all()
    assert tot.tolist() == wtot, (tot.tolist(), wtot)
    if with_count:
        assert np.array_equal(cnt[:n], np.diff(woff.astype(np.int64)).astype(np.uint32))
    else:
        assert (cnt == MARK).all()
    if cap == 0 or (err is not None and err.code == E_NOMEM):
        assert (raw == MARK).all(), "counting alone, or DX_E_NOMEM, and a seed was written"
    else:
        got = raw[:4 * total].view(P.SEED)
        P.same_entries(got, want, P.SEED)
    if with_off and not (err is not None and err.code == E_NOMEM):
        assert np.array_equal(off[:n + 1], woff)
    else:
        assert (off == U(2 ** 64 - 1)).all()
    if err is None or err.code == E_FORMAT:
        assert (bad is None) == (err is None) and (err is None or err.bad_unit == bad)
    return raw[:4 * total].tobytes(), cnt[:n], off[:n + 1], tot, err


def index_of(ctx, targets, k, canonical):
    letters = ["".join("ACGT"[c] for c in s) for s in targets]
    return ctx.kmer_index_from_letters(letters, k, canonical=canonical), P.Index(targets, k, canonical)


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", [5, 14, 21, 32])
def test_every_length_phase_and_offset(ctx, k, canonical):
    targets, piece = reference(k)
    b = reads_of(targets, k, 70 + k, piece)
    x, want_x = index_of(ctx, targets, k, canonical)
    per = {}
    with x:
        for max_occ in (1, 2, REPEAT - 2, REPEAT - 1, REPEAT, 1 << 20):
            lst, cnt, off, tot, err = run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, max_occ)
            assert err is None and tot[2] > 0
            per[max_occ] = int(cnt[-1])
            if k >= 14 and canonical:
                both = np.frombuffer(lst, P.SEED)["strand"]
                assert 0 < both.sum() < len(both)                          # seeds of either strand
    if k >= 14:                                                            # the piece's codes occur REPEAT times (folded), or REPEAT - 1 and once
        occ = REPEAT if canonical else REPEAT - 1
        assert per[occ - 1] < per[occ] == per[1 << 20] and per[occ] >= occ * (len(piece) - k + 1)


def test_counting_alone_a_list_one_short_and_no_arrays(ctx):
    k = 15
    targets, _ = reference(3)
    b = reads_of(targets, k, 4)
    x, want_x = index_of(ctx, targets, k, True)
    with x:
        full = run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, 8)
        total = int(full[3][2])
        assert full[4] is None and total > 1000
        assert run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, 8, cap=0)[4] is None                # counted only: totals, counts, places
        short = run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, 8, cap=total - 1)
        assert short[4] is not None and short[4].code == E_NOMEM and int(short[3][2]) == total           # nothing written, total set
        assert run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, 8, with_count=False, with_off=False)[0] == full[0]
        assert run(ctx, x, want_x, b.packed(), b.boff, None, b.ln, 8)[4] is None                          # whole reads without d_beg
        again = run(ctx, x, want_x, b.packed(), b.boff, b.beg, b.ln, 8)
        assert again[0] == full[0] and again[2].tobytes() == full[2].tobytes()                             # the same bytes on two calls
        lst, cnt, off, tot, err = run(ctx, x, want_x, b.packed(), [], [], [], 8)                          # n = 0: off[0] = 0 alone
        assert err is None and off.tolist() == [0] and tot.tolist() == [0, 0, 0, 0]


def test_a_bad_unit_in_the_middle_and_units_that_overlap_and_repeat(ctx):
    k = 21
    targets, piece = reference(8)
    b = P.Buffer()
    for s in (targets[0][100:400], targets[1][0:64], targets[2][:1200], targets[0][2400:2490], piece):
        b.add(s, beg=2, guard=6, tail=6)
    nbytes = len(b.packed())
    x, want_x = index_of(ctx, targets, k, True)
    with x:
        for j, (at, ln) in ((2, (nbytes + 1, 50)), (1, (nbytes - 10, 100)), (3, (0, 0x80000000))):
            boff, lens = list(b.boff), list(b.ln)
            boff[j], lens[j] = at, ln
            lst, cnt, off, tot, err = run(ctx, x, want_x, b.packed(), boff, b.beg, lens, REPEAT)
            assert err is not None and err.code == E_FORMAT and err.bad_unit == j and cnt[j] == 0 and tot[2] > 0
        # the same read four times, and pieces of it that overlap each other
        boff = [b.boff[2]] * 7
        beg = [2, 2, 2, 2, 2 + 100, 2 + 131, 2 + 500]
        lens = [1200, 1200, 1200, 1200, 600, 333, 700]
        lst, cnt, off, tot, err = run(ctx, x, want_x, b.packed(), boff, beg, lens, REPEAT)
        assert err is None and cnt[0] == cnt[1] == cnt[3] > 0 and cnt[4] > 0


def test_an_empty_index_and_the_refusals(ctx):
    targets, _ = reference(1)
    b = reads_of(targets, 21, 2)
    with ctx.kmer_index_from_letters([], 21, canonical=True) as x:
        lst, cnt, off, tot, err = run(ctx, x, P.Index([], 21, True), b.packed(), b.boff, b.beg, b.ln, 4)
        assert err is None and tot[2] == 0 and tot[0] > 0 and not cnt.any()
    d = ctx.alloc(256).zero()
    tot = (api.C.c_uint64 * 4)(7, 7, 7, 7)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_seeds(d, d, None, d, None, in_bytes=16, n=1)                                  # no index
        assert e.value.code == E_ARG and "index" in str(e.value)
        with ctx.kmer_index_from_letters(["ACGTACGTTGCA"], 5) as x:
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_seeds(d, d, None, d, x, max_occ=0, in_bytes=16, n=1)
            assert e.value.code == E_ARG and "max_occ" in str(e.value)
            for args in ((None, d, d), (d, None, d), (d, d, None)):                                       # the buffer, the offsets, the lengths
                with pytest.raises(L.DexGPUError) as e:
                    ctx.code_kmer_seeds(args[0], args[1], None, args[2], x, in_bytes=16, n=1)
                assert e.value.code == E_ARG
            f = ctx.lib.dx_code_kmer_seeds
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, x.h, 1, None, None, None, 0, None, None) == E_ARG            # no totals
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, x.h, 1, None, None, None, 8, api.C.byref(tot), None) == E_ARG   # a list, and nowhere
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, x.h, 1, None, d.ptr + 4, None, 0, api.C.byref(tot), None) == E_ARG
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, x.h, 1, None, None, None, 0, api.C.byref(tot), None) == E_ARG
            assert list(tot) == [0, 0, 0, 0]
    finally:
        d.free()
