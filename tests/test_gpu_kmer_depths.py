"""Context.code_kmer_depths (dx_code_kmer_depths) on the GPU against its numpy statement (tests/_depth.py): the WHOLE uint16 profile
is compared, and the units' places -- on the buffer of tests/test_gpu_kmer_screen.py: every unit length around k, a chunk and the cuts
between the kernel's three paths, every phase of a unit's start and every residue of its byte offset; everything that is NOT a unit is
filled with Ts, and the set holds the codes that windows reaching past either end of a unit would have.  The counts are drawn from the
values around the two clamps.  Behind the last depth stand guard words.  No expected value comes from the library."""
import numpy as np
import pytest

import _depth as D
import _find as F
import _kmers_wide as W
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

CHUNK = 64            # KC_CHUNK (csrc/kmers/dx_kmer_windows.hpp)
KS = [1, 2, 14, 15, 16, 17, 31, 32]
COUNTS = [1, 2, 255, 256, 65534, 65535, 65536, 2 ** 32 - 1]
E_ARG, E_FORMAT, E_NOMEM = -1, -3, -6
T, U = 3, np.uint64
GUARD = 64            # words behind the last depth
MARK = 0xC0DE
PAD = 8               # bytes of Ts in front of and behind every unit


def lengths(k):
    return sorted({0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 4 * CHUNK - 1, 4 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1, 5003})


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def every_length(k, seed):
    """every length at all four phases of d_beg, the byte offsets going through every residue mod 16"""
    rng, b, j = np.random.default_rng(seed), D.Buffer(), 0
    for n in lengths(k):
        for beg in range(4):
            b.add(rng.integers(0, 4, n), phase=(5 * j) % 16, beg=beg + 4 * (j % 3), guard=PAD, tail=PAD)
            j += 1
    assert {o % 16 for o in b.boff} == set(range(16))
    return b


def reach_codes(s, k, canonical):
    """the codes of the windows that reach 1 .. k - 1 symbols past either end of the unit into the Ts around it"""
    ext = np.concatenate([np.full(k - 1, T, np.uint8), np.asarray(s, np.uint8), np.full(k - 1, T, np.uint8)])
    c = W.unit_codes(ext, k, canonical)
    return np.concatenate([c[:k - 1], c[len(c) - (k - 1):]]) if k > 1 and len(c) else np.zeros(0, U)


def mixed_pairs(units, k, canonical, seed):
    """(code, count) pairs: a random half of the units' own codes, some absent codes, and the codes of the windows that leave a unit;
    the counts from the values around the clamps"""
    rng = np.random.default_rng(seed)
    own = np.unique(W.all_codes(units, k, canonical))
    half = own[rng.integers(0, 2, len(own)) == 1]
    absent = rng.integers(0, 2 ** 63, 200, dtype=np.uint64) & U(4 ** k - 1 if k < 32 else 2 ** 64 - 1)
    if canonical:
        absent = np.minimum(absent, W.rc(absent, k))
    absent = absent[~np.isin(absent, own)]
    reach = np.concatenate([reach_codes(s, k, canonical) for s in units] + [np.zeros(0, U)])
    codes = rng.permutation(np.unique(np.concatenate([half, absent, reach])))
    return [(int(c), int(x)) for c, x in zip(codes, rng.choice(COUNTS, len(codes)))]


def run(ctx, kset, codes, counts, packed, boff, beg, ln, k, canonical=False, in_bytes=None, cap=None, with_off=True):
    """one call against the statement: (the profile, the places, the windows, the error or None)"""
    want, woff, bad = D.packed_profile(packed, boff, beg, ln, k, canonical, codes, counts, in_bytes)
    nbytes = len(packed) if in_bytes is None else in_bytes
    n, windows = len(ln), len(want)
    cap = windows if cap is None else cap
    d_in = ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16)
    d_boff, d_len = ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(ln, np.uint32))
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    d_depth = ctx.alloc(2 * (windows + GUARD)).upload(np.full(windows + GUARD, MARK, np.uint16))
    d_off = ctx.alloc(8 * (n + 1 + 2)).upload(np.full(n + 3, 2 ** 64 - 1, np.uint64))
    err, got_windows = None, None
    try:
        try:
            got_windows = ctx.code_kmer_depths(d_in, d_boff, d_beg, d_len, kset, cap=cap, depth=d_depth, off=d_off if with_off else None,
                                               in_bytes=nbytes, n=n)[1]
        except L.DexGPUError as e:
            err, got_windows = e, e.windows
        raw, off = d_depth.download(np.uint16, windows + GUARD), d_off.download(np.uint64, n + 3)
    finally:
        for x in (d_in, d_boff, d_len, d_beg, d_depth, d_off):
            if x is not None:
                x.free()
    assert (raw[windows:] == MARK).all(), "a word behind the last depth was written"
    assert (off[n + 1:] == U(2 ** 64 - 1)).all() and got_windows == windows
    if err is not None and err.code == E_NOMEM:
        assert (raw == MARK).all() and (off == U(2 ** 64 - 1)).all(), "DX_E_NOMEM, and something was written"
        return raw[:windows], off[:n + 1], got_windows, err
    diff = np.flatnonzero(raw[:windows] != want)
    assert len(diff) == 0, (k, canonical, [(int(i), int(raw[i]), int(want[i]), int(np.searchsorted(woff, i, "right")) - 1) for i in diff[:8]])
    assert np.array_equal(off[:n + 1], woff) if with_off else (off == U(2 ** 64 - 1)).all()
    assert (bad is None) == (err is None) and (err is None or (err.code == E_FORMAT and err.bad_unit == bad))
    return raw[:windows], off[:n + 1], got_windows, err


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_every_length_phase_and_offset(ctx, k, canonical):
    b = every_length(k, 300 + k)
    pairs = mixed_pairs(b.units, k, canonical, k)
    codes, counts = D.from_kmers(pairs, k, canonical)
    packed = b.packed()
    d = [ctx.to_device(np.asarray(a, t)) for a, t in ((np.frombuffer(packed, np.uint8), np.uint8), (b.boff, np.uint64), (b.beg, np.uint32),
                                                       (b.ln, np.uint32))]
    n = len(b.ln)
    d_scr = ctx.alloc(16 * n)
    try:
        with ctx.kmer_set_from_kmers(pairs, k, canonical) as s, ctx.kmer_set_from_codes(codes, k, canonical) as plain:
            assert np.array_equal(s.codes(), codes) and np.array_equal(s.counts(), counts)
            prof, off, windows, err = run(ctx, s, codes, counts, packed, b.boff, b.beg, b.ln, k, canonical)
            assert err is None and windows == sum(max(0, x - k + 1) for x in b.ln)
            if k > 2:                                                # (at k <= 2 the few codes there are may all be in the set, or none)
                assert 0 < np.count_nonzero(prof) < windows
                assert {int(x) for x in np.unique(prof)} >= {0, 1, 2, 255, 256, 65534, 65535}       # both sides of the clamp are there
            # the non-zero depths of a unit are the screen's hits
            tot = ctx.code_kmer_screen(d[0], d[1], d[2], d[3], s, out=d_scr, n=n)
            hits = d_scr.download(np.uint32, 4 * n)[0::4]
            assert [int(np.count_nonzero(prof[int(off[j]):int(off[j + 1])])) for j in range(n)] == hits.tolist() and tot[1] == hits.sum()
            # an uncounted set gives 0 / 1: the membership
            member = run(ctx, plain, codes, None, packed, b.boff, b.beg, b.ln, k, canonical)[0]
            assert np.array_equal(member, (prof != 0).astype(np.uint16)) and set(np.unique(member).tolist()) <= {0, 1}
    finally:
        for x in d + [d_scr]:
            x.free()


def some_units(seed, k):
    rng, b = np.random.default_rng(seed), D.Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, k - 1, 257, 64, 2000]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=j % 4, guard=PAD, tail=PAD)
    return b


@pytest.mark.parametrize("k", [15, 32])
def test_too_little_room_no_units_and_no_places(ctx, k):
    b = some_units(k, k)
    pairs = mixed_pairs(b.units, k, True, 3)
    codes, counts = D.from_kmers(pairs, k, True)
    with ctx.kmer_set_from_kmers(pairs, k, canonical=True) as s:
        windows = sum(max(0, x - k + 1) for x in b.ln)
        prof, off, got, err = run(ctx, s, codes, counts, b.packed(), b.boff, b.beg, b.ln, k, True, cap=windows - 1)
        assert err is not None and err.code == E_NOMEM and got == windows                    # nothing written, the windows set
        assert run(ctx, s, codes, counts, b.packed(), b.boff, b.beg, b.ln, k, True, with_off=False)[3] is None
        assert run(ctx, s, codes, counts, b.packed(), b.boff, None, b.ln, k, True)[3] is None   # whole reads without d_beg
        prof, off, got, err = run(ctx, s, codes, counts, b.packed(), [], [], [], k, True)     # n = 0: off[0] = 0 alone
        assert err is None and got == 0 and off.tolist() == [0]
        empty = D.Buffer()
        for n in (0, k - 1, 3):
            empty.add(np.zeros(n, np.uint8), guard=PAD, tail=PAD)
        prof, off, got, err = run(ctx, s, codes, counts, empty.packed(), empty.boff, empty.beg, empty.ln, k, True)   # units, and no window
        assert err is None and got == 0 and off.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("k", [15, 32])
def test_a_bad_unit_in_the_middle(ctx, k):
    rng, b = np.random.default_rng(k), D.Buffer()
    for n in (300, 64, 5003, 90, 700):
        b.add(rng.integers(0, 4, n), beg=2, guard=PAD, tail=PAD)
    own = np.unique(W.all_codes(b.units, k))[::2]
    pairs = [(int(c), int(x)) for c, x in zip(own, rng.choice(COUNTS, len(own)))]
    codes, counts = D.from_kmers(pairs, k)
    nbytes = len(b.packed())
    with ctx.kmer_set_from_kmers(pairs, k) as s:
        for j, (at, ln) in ((2, (nbytes + 1, 50)), (1, (nbytes - 10, 100)), (3, (0, 0x80000000))):
            boff, lens = list(b.boff), list(b.ln)
            boff[j], lens[j] = at, ln
            prof, off, got, err = run(ctx, s, codes, counts, b.packed(), boff, b.beg, lens, k)     # (run holds the other units' depths against the statement)
            assert err is not None and err.code == E_FORMAT and err.bad_unit == j and off[j] == off[j + 1] and np.count_nonzero(prof) > 0
        boff = list(b.boff)
        boff[1] = boff[4] = nbytes + 5
        assert run(ctx, s, codes, counts, b.packed(), boff, b.beg, b.ln, k)[3].bad_unit == 1


def test_the_buffers_end_and_two_calls_give_the_same_bytes(ctx):
    k = 21
    rng = np.random.default_rng(40)
    for n in (k, 37, 61, 64, 129, 1030):                          # the unit ends in the buffer's last byte; 37, 61: fewer than 16 bytes
        sym = rng.integers(0, 4, n)
        packed = F.pack(sym, pad=0xff)
        for beg in range(4):
            unit = sym[beg:]
            pairs = [(int(c), 7) for c in np.unique(np.concatenate([W.unit_codes(unit, k, True)[::2], reach_codes(unit, k, True)]))]
            codes, counts = D.from_kmers(pairs, k, True)
            with ctx.kmer_set_from_kmers(pairs, k, canonical=True) as s:
                assert run(ctx, s, codes, counts, packed, [0], [beg], [n - beg], k, True)[3] is None
    b = some_units(3, k)
    pairs = mixed_pairs(b.units, k, True, 8)
    codes, counts = D.from_kmers(pairs, k, True)
    with ctx.kmer_set_from_kmers(pairs, k, canonical=True) as s:
        a = run(ctx, s, codes, counts, b.packed(), b.boff, b.beg, b.ln, k, True)
        c = run(ctx, s, codes, counts, b.packed(), b.boff, b.beg, b.ln, k, True)
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    win = api.C.c_uint64(7)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_depths(d, d, None, d, None, cap=8, depth=d, in_bytes=16, n=1)          # no set
        assert e.value.code == E_ARG and "set" in str(e.value)
        with ctx.kmer_set_from_kmers([(1, 1), (2, 5)], 21) as s:
            for args in ((None, d, d), (d, None, d), (d, d, None)):                               # the buffer, the offsets, the lengths
                with pytest.raises(L.DexGPUError) as e:
                    ctx.code_kmer_depths(args[0], args[1], None, args[2], s, cap=8, depth=d, in_bytes=16, n=1)
                assert e.value.code == E_ARG
            assert ctx.lib.dx_code_kmer_depths(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, d.ptr, 8, None, None, None) == E_ARG
            assert ctx.lib.dx_code_kmer_depths(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, 8, None, api.C.byref(win), None) == E_ARG
            assert ctx.lib.dx_code_kmer_depths(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, d.ptr + 1, 8, None, api.C.byref(win), None) == E_ARG
            assert ctx.lib.dx_code_kmer_depths(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, s.h, d.ptr, 8, None, api.C.byref(win), None) == E_ARG
            assert win.value == 0
    finally:
        d.free()
