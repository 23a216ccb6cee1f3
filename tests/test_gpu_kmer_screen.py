"""Context.code_kmer_screen (dx_code_kmer_screen) on the GPU against its numpy statement (tests/_screen.py): the WHOLE array of
entries is compared and the totals with it -- every unit length around k, a chunk and the cuts between the kernel's three paths, every
phase of a unit's start and every residue of its byte offset.  Everything that is NOT a unit (the guard bytes around it, the symbols in
front of d_beg, the pad bits of its last byte) is filled with Ts, and the set holds the codes that windows reaching past either end of
a unit into the Ts would have: a window that leaves its unit hits where the statement does not.  Behind the last entry stand guard
entries.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_wide as W
import _screen as S
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# csrc/kmers/dx_kmer_windows.hpp
CHUNK = 64            # KC_CHUNK: positions of one 16-byte chunk, which stands on a 16-byte boundary of the BUFFER
KS = [1, 2, 14, 15, 16, 17, 31, 32]
E_ARG, E_FORMAT = -1, -3
T, U = S.T, np.uint64
GUARD = 4             # entries behind the last unit's
MARK = 0xC0DEC0DE
PAD = 8               # bytes of Ts in front of and behind every unit: 64 symbols between two units, more than any window reaches


def lengths(k):
    return sorted({0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 4 * CHUNK - 1, 4 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1, 5003})


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def run(ctx, kset, codes, packed, boff, beg, ln, k, canonical=False, in_bytes=None, with_out=True):
    """one call against the statement: (the entries, the totals, the error or None)"""
    want, tot, bad = S.packed_screen(packed, boff, beg, ln, k, canonical, codes, in_bytes)
    nbytes = len(packed) if in_bytes is None else in_bytes
    n = len(ln)
    d_in = ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16)
    d_boff, d_len = ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(ln, np.uint32))
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    d_out = ctx.alloc(16 * (n + GUARD)).upload(np.full(4 * (n + GUARD), MARK, np.uint32))
    err = None
    try:
        try:
            totals = ctx.code_kmer_screen(d_in, d_boff, d_beg, d_len, kset, out=d_out if with_out else None, in_bytes=nbytes, n=n)
        except L.DexGPUError as e:
            err, totals = e, e.totals
        raw = d_out.download(np.uint32, 4 * (n + GUARD))
    finally:
        for x in (d_in, d_boff, d_len, d_beg, d_out):
            if x is not None:
                x.free()
    got = raw[:4 * n].view(S.SCREEN)
    assert (raw[4 * n:] == MARK).all(), "an entry behind the last unit's was written"
    if with_out:
        diff = np.flatnonzero(got != want)
        assert len(diff) == 0, (k, canonical, [(int(j), int(ln[j]), tuple(got[j]), tuple(want[j])) for j in diff[:5]])
    else:
        assert (raw == MARK).all()
    assert totals.tolist() == tot.tolist(), (totals, tot)
    assert (bad is None) == (err is None) and (err is None or (err.code == E_FORMAT and err.bad_unit == bad))
    return got, totals, err


def reach_codes(s, k, canonical):
    """the codes of the windows that reach 1 .. k - 1 symbols past either end of the unit into the Ts around it"""
    ext = np.concatenate([np.full(k - 1, T, np.uint8), np.asarray(s, np.uint8), np.full(k - 1, T, np.uint8)])
    c = W.unit_codes(ext, k, canonical)
    return np.concatenate([c[:k - 1], c[len(c) - (k - 1):]]) if k > 1 and len(c) else np.zeros(0, U)


def mixed_set(units, k, canonical, seed):
    """a random half of the units' own codes, some absent codes, and the codes of the windows that leave a unit"""
    rng = np.random.default_rng(seed)
    own = np.unique(W.all_codes(units, k, canonical))
    half = own[rng.integers(0, 2, len(own)) == 1]
    absent = rng.integers(0, 2 ** 63, 200, dtype=np.uint64) & U(4 ** k - 1 if k < 32 else 2 ** 64 - 1)
    if canonical:
        absent = np.minimum(absent, W.rc(absent, k))
    absent = absent[~np.isin(absent, own)]
    reach = np.concatenate([reach_codes(s, k, canonical) for s in units] + [np.zeros(0, U)])
    return np.unique(np.concatenate([half, absent, reach]))


def every_length(k, seed):
    """every length at all four phases of d_beg, the byte offsets going through every residue mod 16"""
    rng, b, j = np.random.default_rng(seed), S.Buffer(), 0
    for n in lengths(k):
        for beg in range(4):
            b.add(rng.integers(0, 4, n), phase=(5 * j) % 16, beg=beg + 4 * (j % 3), guard=PAD, tail=PAD)
            j += 1
    assert {o % 16 for o in b.boff} == set(range(16))
    return b


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_every_length_phase_and_offset(ctx, k, canonical):
    b = every_length(k, 300 + k)
    codes = mixed_set(b.units, k, canonical, k)
    with ctx.kmer_set_from_codes(codes, k, canonical) as s:
        got, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
    assert err is None and totals[0] == sum(max(0, n - k + 1) for n in b.ln) and 0 < totals[1] < totals[0]
    if k > 4:                                                        # (at k <= 2 every code of the Ts is a code of the units too)
        # the Ts around a unit make codes that ARE in the set: a kernel that looked past a unit's end would have counted them
        lone = S.Buffer().add(b.units[-1], phase=3, beg=1, guard=PAD, tail=PAD)
        ext = F.symbols(lone.packed(), lone.boff[0] - PAD, 0, 4 * PAD + lone.beg[0] + lone.ln[0] + k - 1)[4 * PAD + lone.beg[0] - (k - 1):]
        assert len(ext) == lone.ln[0] + 2 * (k - 1) and (ext[:k - 1] == T).all() and (ext[-(k - 1):] == T).all()
        assert S.unit_screen(ext, k, canonical, codes)[0] > S.unit_screen(b.units[-1], k, canonical, codes)[0]


# ---- the coverage's seams --------------------------------------------------------------------------------------------------------------
def seam_positions(S0, n, k, long):
    """window positions of a unit of n symbols whose first is symbol S0 of the buffer: the last position of a chunk, of a wave step,
    pairs k - 1, k and k + 1 apart, the first and the last window"""
    last = n - k
    at_chunk_end = (63 - S0) % 64 + 64                                # ... of the unit's second chunk
    pos = {0, last, at_chunk_end}
    if long:
        pos.add(64 * (S0 // 64 + 64) - 1 - S0)                         # lane 63 of the wave's first step: its cover is the carry
        pos.add(64 * (S0 // 64 + 128) - 1 - S0)                        # ... and of the second
        pos.add(64 * (S0 // 64 + 64) - 1 - S0 + k - 1)                 # a window in lane 0 of the next step that overlaps the carried one
    q = at_chunk_end + (70 if long else k + 5)
    for gap in (k - 1, k, k + 1):
        pos |= {q, q + gap}
        q += 2 * k + 9
    assert q < last or not long
    return sorted(p for p in pos if 0 <= p <= last)


@pytest.mark.parametrize("k", [15, 32])
@pytest.mark.parametrize("n", [3 * 4096 + 200, 300, 100], ids=["wave", "sixteen", "lane"])
def test_coverage_seams(ctx, k, n):
    rng = np.random.default_rng(n + k)
    b = S.Buffer().add(rng.integers(0, 4, n), phase=5, beg=2, guard=PAD, tail=PAD)
    S0 = 4 * b.boff[0] + b.beg[0]
    chunks = (S0 + n - 1) // 64 - S0 // 64 + 1
    assert (chunks > 16) if n > 4096 else (4 < chunks <= 16) if n == 300 else chunks <= 4      # the path the unit takes
    pos = seam_positions(S0, n, k, n > 4096) if n > 100 else sorted(p for p in {0, n - k, (63 - S0) % 64, (63 - S0) % 64 + k - 1} if p <= n - k)
    assert any((S0 + p) % 64 == 63 for p in pos)
    for canonical in (False, True):
        all_codes = W.unit_codes(b.units[0], k, canonical)
        codes = np.unique(all_codes[pos])
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        assert err is None and int(got[0]["hits"]) >= len(pos) and int(got[0]["first"]) == 0 and int(got[0]["last"]) == n - k
        assert int(got[0]["covered"]) < n


# ---- the set's extremes ----------------------------------------------------------------------------------------------------------------
def some_units(seed, k):
    rng, b = np.random.default_rng(seed), S.Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, k - 1, 257, 64, 2000]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=j % 4, guard=PAD, tail=PAD)
    return b


@pytest.mark.parametrize("k", [15, 32])
def test_the_empty_set_and_the_set_of_all_codes(ctx, k):
    b = some_units(k, k)
    with ctx.kmer_set_from_codes([], k) as s:
        got, totals, err = run(ctx, s, np.zeros(0, U), b.packed(), b.boff, b.beg, b.ln, k)
    assert err is None and totals.tolist()[1:] == [0, 0, 0] and totals[0] > 0
    assert (got["hits"] == 0).all() and (got["covered"] == 0).all() and (got["first"] == S.NONE).all() and (got["last"] == S.NONE).all()
    for canonical in (False, True):
        codes = np.unique(W.all_codes(b.units, k, canonical))
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        ln = np.array(b.ln)
        assert err is None and totals[1] == totals[0] == got["hits"].sum()
        assert (got["covered"] == np.where(ln >= k, ln, 0)).all() and (got["hits"] == np.maximum(ln - k + 1, 0)).all()


@pytest.mark.parametrize("bits,extra", [(1, 5000), (24, 0), (None, 200000)], ids=["bits1_5000", "bits24_10", "natural_200000"])
def test_narrow_wide_and_natural_index(ctx, monkeypatch, bits, extra):
    k = 21
    b = some_units(77, k)
    rng = np.random.default_rng(extra + 1)
    own = np.unique(W.all_codes(b.units, k, True))
    planted = own[rng.integers(0, 2, len(own)) == 1] if extra else own[rng.choice(len(own), 10, replace=False)]
    more = rng.integers(0, 4 ** k, extra, dtype=np.uint64)
    more = np.minimum(more, W.rc(more, k))
    codes = np.unique(np.concatenate([planted, more[~np.isin(more, own)]]))
    if bits is not None:
        set_flag(monkeypatch, "set_bits", bits)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        info = s.info
        got, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
    assert err is None and totals[1] >= len(planted) and info["codes"] == len(codes) >= (extra or 10)
    assert info["index_bits"] == (bits if bits is not None else 19)                 # 2^19 >= 2 x (200000 + the planted) > 2^18
    if bits == 1:
        assert len(codes) >= 5000                                    # buckets of thousands of codes: the bisection


# ---- the strands -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 32])
def test_a_unit_and_its_reverse_complement_under_a_canonical_set(ctx, k):
    rng, b = np.random.default_rng(k), S.Buffer()
    fwd = [rng.integers(0, 4, n).astype(np.uint8) for n in (k, 90, 300, 1500, 5003)]
    for j, s in enumerate(fwd):
        b.add(s, phase=(7 * j) % 16, beg=j % 4, guard=PAD, tail=PAD)
        b.add((3 - s[::-1]).astype(np.uint8), phase=(7 * j + 3) % 16, beg=(j + 1) % 4, guard=PAD, tail=PAD)
    own = np.unique(W.all_codes(fwd, k, True))
    codes = own[rng.integers(0, 3, len(own)) == 0]
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        got, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
    a, r, ln = got[0::2], got[1::2], np.array(b.ln[0::2])
    assert err is None and (a["hits"] == r["hits"]).all() and (a["covered"] == r["covered"]).all() and a["hits"].sum() > 0
    hit = a["hits"] > 0
    assert (r["first"][hit] == ln[hit] - k - a["last"][hit]).all() and (r["last"][hit] == ln[hit] - k - a["first"][hit]).all()


# ---- the rest --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 32])
def test_whole_reads_without_d_beg(ctx, k):
    rng, b = np.random.default_rng(k), S.Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, k - 1]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=0, guard=PAD, tail=PAD)
    codes = mixed_set(b.units, k, True, 5)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        assert run(ctx, s, codes, b.packed(), b.boff, None, b.ln, k, True)[2] is None


def test_units_that_overlap_and_repeat_no_units_and_totals_alone(ctx):
    rng = np.random.default_rng(9)
    sym = rng.integers(0, 4, 4000)
    packed = F.pack(sym)
    boff = [0, 0, 10, 10, 500, 0, 999, 17, 0]
    beg = [0, 5, 3, 3, 0, 0, 0, 2, 3999]
    ln = [4000, 100, 0, 700, 20, 4000, 4, 2000, 1]
    for k in (1, 16, 21, 32):
        own = np.unique(W.unit_codes(sym, k, k == 21))
        codes = own[::3]
        with ctx.kmer_set_from_codes(codes, k, canonical=k == 21) as s:
            got, totals, err = run(ctx, s, codes, packed, boff, beg, ln, k, canonical=k == 21)
            assert err is None and totals[0] == sum(max(0, n - k + 1) for n in ln) and tuple(got[0]) == tuple(got[5])
            run(ctx, s, codes, packed, boff, beg, ln, k, canonical=k == 21, with_out=False)       # d_out NULL: the totals alone
            got, totals, err = run(ctx, s, codes, packed, [], [], [], k, canonical=k == 21)
            assert err is None and totals.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("k", [2, 21, 32])
def test_the_buffers_end_and_a_buffer_shorter_than_a_load(ctx, k):
    rng = np.random.default_rng(40 + k)
    for n in (k, 37, 61, 64, 129, 1030):                          # the unit ends in the buffer's last byte; 37, 61: fewer than 16 bytes
        sym = rng.integers(0, 4, n)
        packed = F.pack(sym, pad=0xff)
        for beg in range(4):
            if n - beg < k:
                continue
            unit = sym[beg:]
            codes = np.unique(np.concatenate([W.unit_codes(unit, k, k != 21)[::2], reach_codes(unit, k, k != 21)]))
            with ctx.kmer_set_from_codes(codes, k, canonical=k != 21) as s:
                got, totals, err = run(ctx, s, codes, packed, [0], [beg], [n - beg], k, k != 21)
            assert err is None and totals[0] == n - beg - k + 1 and totals[1] > 0
    sym = rng.integers(0, 4, 300)
    packed = F.pack(np.concatenate([np.full(13, T, np.uint8), sym]), pad=0xff)       # ... and begins at an odd byte of it
    codes = np.unique(np.concatenate([W.unit_codes(sym, k)[::2], reach_codes(sym, k, False)]))
    with ctx.kmer_set_from_codes(codes, k) as s:
        assert run(ctx, s, codes, packed, [3], [1], [300], k)[2] is None


@pytest.mark.parametrize("k", [15, 32])
def test_a_bad_unit_in_the_middle(ctx, k):
    rng, b = np.random.default_rng(k), S.Buffer()
    for n in (300, 64, 5003, 90, 700):
        b.add(rng.integers(0, 4, n), beg=2, guard=PAD, tail=PAD)
    codes = np.unique(W.all_codes(b.units, k))[::2]
    nbytes = len(b.packed())
    with ctx.kmer_set_from_codes(codes, k) as s:
        for j, (at, ln) in ((2, (nbytes + 1, 50)), (1, (nbytes - 10, 100)), (3, (0, 0x80000000))):
            boff, lens = list(b.boff), list(b.ln)
            boff[j], lens[j] = at, ln
            got, totals, err = run(ctx, s, codes, b.packed(), boff, b.beg, lens, k)        # (run holds every entry and the totals against the statement)
            assert err is not None and err.code == E_FORMAT and err.bad_unit == j
            assert tuple(int(v) for v in got[j]) == (0, 0, S.NONE, S.NONE) and totals[3] == 4
        boff = list(b.boff)
        boff[1] = boff[4] = nbytes + 5
        assert run(ctx, s, codes, b.packed(), boff, b.beg, b.ln, k)[2].bad_unit == 1


def test_two_calls_give_the_same_bytes(ctx):
    k, b = 21, some_units(3, 21)
    codes = mixed_set(b.units, k, True, 8)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        a = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
        c = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
    assert a[0].tobytes() == c[0].tobytes() and a[1].tolist() == c[1].tolist()


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    tot = (api.C.c_uint64 * 4)(7, 7, 7, 7)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_screen(d, d, None, d, None, out=d, in_bytes=16, n=1)                # no set
        assert e.value.code == E_ARG and "set" in str(e.value)
        with ctx.kmer_set_from_codes([1, 2, 3], 21) as s:
            for args in ((None, d, d), (d, None, d), (d, d, None)):                           # the buffer, the offsets, the lengths
                with pytest.raises(L.DexGPUError) as e:
                    ctx.code_kmer_screen(args[0], args[1], None, args[2], s, out=d, in_bytes=16, n=1)
                assert e.value.code == E_ARG
            assert ctx.lib.dx_code_kmer_screen(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, d.ptr, None, None) == E_ARG
            assert ctx.lib.dx_code_kmer_screen(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, s.h, d.ptr, api.C.byref(tot), None) == E_ARG
            assert list(tot) == [0, 0, 0, 0]
    finally:
        d.free()
