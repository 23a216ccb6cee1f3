"""dx_reads_unpack_lines (k_reads_unpack_lines) on the GPU (needs an MI355X): intervals of packed reads, at any byte offset and any
phase, as the lines undexta prints for them.  Expected bytes are numpy's (tests/_lines.py: unpack_lines_ref), laid into a buffer of
guard bytes.  Bar: bit-exact, and not a byte written outside a unit's text."""
import functools

import numpy as np
import pytest

import _lines as LN
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

GUARD_BYTE, GUARD = 0xA5, 64
LENGTHS = [*range(0, 6), *range(13, 18), 31, 32, 33, 63, 64, 65, 79, 80, 81, 159, 160, 161, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20001]
BEGS = [0, 1, 2, 3, 5, 1022]
WIDTHS = [1, 2, 3, 5, 15, 16, 17, 60, 80, 2 ** 31]
LETTER_SETS = [L.DX_LETTERS_LOWER, L.DX_LETTERS_UPPER, L.DX_LETTERS_ARROW]
NBUF = 5400                                                  # packed bytes: room for the longest unit at the largest beg and any offset


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def packed():
    """one random packed buffer for every test of this file: computed once, never changed"""
    buf = np.random.Generator(np.random.PCG64(20261019)).integers(0, 256, NBUF, dtype=np.uint8)
    buf.setflags(write=False)
    return buf


def place(lens, width, order, gaps):
    """where the units' texts go: in `order`, `gaps[k]` guard bytes in front of the k-th placed, GUARD around all -> (out_off, out_bytes)"""
    out_off = np.zeros(len(lens), np.uint64)
    at = GUARD
    for k, j in enumerate(order):
        at += int(gaps[k])
        out_off[j] = at
        at += LN.text_len(int(lens[j]), width)
    return out_off, at + GUARD


def expected(buf, boff, beg, lens, width, letters, out_off, out_bytes):
    want = np.full(out_bytes, GUARD_BYTE, np.uint8)
    for o, t in zip(out_off.tolist(), LN.unpack_lines_ref(buf, boff, beg, lens, width, letters)):
        assert (want[o: o + len(t)] == GUARD_BYTE).all()             # (the outputs are disjoint)
        want[o: o + len(t)] = np.frombuffer(t, np.uint8)
    return want


def run(ctx, letters, buf, boff, beg, lens, width, out_off, out_bytes, in_bytes=None):
    """dx_reads_unpack_lines into a buffer of out_bytes guard bytes -> that buffer"""
    bufs = [ctx.to_device(np.asarray(buf, np.uint8)) if len(buf) else ctx.alloc(16), ctx.to_device(np.asarray(boff, np.uint64)),
            ctx.to_device(np.asarray(lens, np.uint32)), ctx.to_device(np.asarray(out_off, np.uint64)),
            ctx.to_device(np.full(out_bytes, GUARD_BYTE, np.uint8))]
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    try:
        ctx.reads_unpack_lines(letters, bufs[0], len(buf) if in_bytes is None else in_bytes, bufs[1], d_beg, bufs[2], len(lens), width, bufs[4], bufs[3])
        return bufs[4].download(np.uint8, out_bytes)
    finally:
        for d in bufs + ([d_beg] if d_beg else []):
            d.free()


def check(got, want, out_off, beg, lens):
    if not np.array_equal(got, want):
        diff = np.nonzero(got != want)[0]
        order = np.argsort(out_off)
        unit = order[np.searchsorted(out_off[order], diff[:5], side="right") - 1]
        pytest.fail(f"{len(diff)} bytes differ, first at {diff[:5]} (units {unit}: beg {np.asarray(beg)[unit]}, len {np.asarray(lens)[unit]}, at {out_off[unit]})")


# ---- 1. every length at every phase, every width, every letter set ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid():
    """One unit a (length, beg): starts at every byte residue mod 16 of the buffer, overlapping and repeating there; the longest unit at
    the largest beg ends with the buffer's last byte.  Computed once, never changed."""
    rng = np.random.Generator(np.random.PCG64(1))
    lens = np.array([n for n in LENGTHS for _ in BEGS], np.uint32)
    beg = np.array(BEGS * len(LENGTHS), np.uint32)
    boff = (np.arange(len(lens)) % 16 + 16 * rng.integers(0, 4, len(lens))).astype(np.uint64)
    last = len(lens) - 1
    assert lens[last] == 20001 and beg[last] == 1022
    boff[last] = NBUF - ((int(beg[last]) + int(lens[last]) + 3) >> 2)
    assert ((boff.astype(np.int64) + ((beg.astype(np.int64) + lens + 3) >> 2)) <= NBUF).all()
    assert int(boff[last]) + ((int(beg[last]) + int(lens[last]) - 1) >> 2) == NBUF - 1
    assert set((boff % 16).tolist()) == set(range(16))
    order = rng.permutation(len(lens))
    for a in (lens, beg, boff, order):
        a.setflags(write=False)
    return lens, beg, boff, order


@pytest.mark.parametrize("width", WIDTHS, ids=[f"w{w}" for w in WIDTHS])
def test_every_length_phase_and_letter_set(ctx, width):
    lens, beg, boff, order = grid()
    rng = np.random.Generator(np.random.PCG64(width % 1000))
    back_to_back = place(lens, width, order, np.zeros(len(lens), np.int64))
    guarded = place(lens, width, order, rng.integers(1, 19, len(lens)))
    assert set((guarded[0] % 16).tolist()) == set(range(16))
    assert set((back_to_back[0] % 16).tolist()) == set(range(0, 16, 2 if width == 1 else 1))       # (in lines of 1 every text is even)
    assert (np.diff(back_to_back[0].astype(np.int64)) < 0).any()        # (the outputs are not in unit order)
    for letters in LETTER_SETS:
        for out_off, out_bytes in (back_to_back, guarded):
            want = expected(packed(), boff, beg, lens, width, letters, out_off, out_bytes)
            check(run(ctx, letters, packed(), boff, beg, lens, width, out_off, out_bytes), want, out_off, beg, lens)


# ---- 2. buffers shorter than the kernel's loads ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 5, 7])
def test_buffers_of_a_few_bytes(ctx, nbytes):
    buf = packed()[100: 100 + nbytes]
    units = [(o, b, n) for o in range(nbytes) for b in range(0, 4 * (nbytes - o)) for n in range(0, 4 * (nbytes - o) - b + 1)]
    units.append((nbytes, 0, 0))                                        # (an empty unit at the buffer's end lies inside it)
    boff, beg, lens = (np.array(c, t) for c, t in zip(zip(*units), (np.uint64, np.uint32, np.uint32)))
    for k, width in enumerate((1, 3, 16, 80)):
        letters = LETTER_SETS[k % 3]
        out_off, out_bytes = place(lens, width, np.arange(len(lens)), np.full(len(lens), 1 + k))
        want = expected(buf, boff, beg, lens, width, letters, out_off, out_bytes)
        check(run(ctx, letters, buf, boff, beg, lens, width, out_off, out_bytes), want, out_off, beg, lens)


# ---- 3. unit counts: the four-a-step path and the ticket edges --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 5000])
def test_unit_counts(ctx, n):
    rng = np.random.Generator(np.random.PCG64(n))
    if n == 5000:
        lens = rng.integers(0, 41, n).astype(np.uint32)
    else:                                                               # short ones and long ones side by side in a round
        lens = np.where(rng.random(n) < 0.7, rng.integers(0, 200, n), rng.integers(200, 3000, n)).astype(np.uint32)
    beg = rng.integers(0, 64, n).astype(np.uint32)
    boff = rng.integers(0, NBUF - 800, n).astype(np.uint64)
    boff[n // 2] = boff[0]                                              # (units repeat and overlap in the input)
    order = rng.permutation(n)
    for width, letters in ((3, L.DX_LETTERS_ARROW), (60, L.DX_LETTERS_LOWER)):
        out_off, out_bytes = place(lens, width, order, rng.integers(0, 3, n))
        want = expected(packed(), boff, beg, lens, width, letters, out_off, out_bytes)
        check(run(ctx, letters, packed(), boff, beg, lens, width, out_off, out_bytes), want, out_off, beg, lens)


# ---- 4. whole reads at phase 0 are k_pack2_decode's text ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", [5, 16, 80])
def test_whole_reads_are_pack2_decodes_text(ctx, width):
    rng = np.random.Generator(np.random.PCG64(77 + width))
    lens = np.array(LENGTHS + rng.integers(0, 3000, 40).tolist(), np.uint32)
    boff = np.concatenate([[3], 3 + np.cumsum((lens.astype(np.int64) + 3) // 4 + rng.integers(0, 3, len(lens)))[:-1]]).astype(np.uint64)
    assert int(boff[-1]) + (int(lens[-1]) + 3) // 4 <= 8 * NBUF
    buf = np.concatenate([packed()] * 8)
    out_off, out_bytes = place(lens, width, np.arange(len(lens)), rng.integers(0, 5, len(lens)))
    for letters in LETTER_SETS:
        got = run(ctx, letters, buf, boff, None, lens, width, out_off, out_bytes)            # (d_beg NULL: all 0)
        bufs = [ctx.to_device(buf), ctx.to_device(boff), ctx.to_device(lens), ctx.to_device(out_off), ctx.to_device(np.full(out_bytes, GUARD_BYTE, np.uint8))]
        try:
            ctx.pack2_decode(letters, bufs[0], bufs[1], bufs[2], len(lens), width, bufs[4], bufs[3])
            other = bufs[4].download(np.uint8, out_bytes)
        finally:
            for d in bufs:
                d.free()
        for o, n in zip(out_off.tolist(), lens.tolist()):
            t = LN.text_len(n, width)
            assert np.array_equal(got[o: o + t], other[o: o + t]), (n, o)
        check(got, expected(buf, boff, np.zeros(len(lens), np.uint32), lens, width, letters, out_off, out_bytes), out_off, np.zeros(len(lens)), lens)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    buf = packed()[:64]
    lens = np.full(10, 16, np.uint32)
    boff = np.arange(10, dtype=np.uint64)
    out_off, out_bytes = place(lens, 80, np.arange(10), np.zeros(10, np.int64))
    for letters, width in ((L.DX_LETTERS_NUMBERS, 80), (L.DX_LETTERS_LOWER, 0)):
        with pytest.raises(L.DexGPUError) as e:
            run(ctx, letters, buf, boff, None, lens, width, out_off, out_bytes)
        assert L.ERR_NAMES[e.value.code] == "DX_E_ARG", str(e.value)
    bad = boff.copy()
    bad[7], bad[3] = 61, 65                                             # unit 7 ends a byte behind the buffer, unit 3 begins behind it
    with pytest.raises(L.DexGPUError) as e:
        run(ctx, L.DX_LETTERS_LOWER, buf, bad, None, lens, 80, out_off, out_bytes)
    assert L.ERR_NAMES[e.value.code] == "DX_E_FORMAT" and e.value.bad_unit == 3, str(e.value)
    with pytest.raises(L.DexGPUError) as e:                             # ... and as many packed bytes as the caller says, not as there are
        run(ctx, L.DX_LETTERS_LOWER, buf, boff, None, lens, 80, out_off, out_bytes, in_bytes=12)
    assert L.ERR_NAMES[e.value.code] == "DX_E_FORMAT" and e.value.bad_unit == 9, str(e.value)
    d = ctx.alloc(16)
    try:
        ctx.reads_unpack_lines(L.DX_LETTERS_LOWER, d, 16, d, None, d, 0, 80, d, d)           # n == 0 is fine
    finally:
        d.free()
