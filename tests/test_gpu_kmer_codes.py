"""Context.code_kmer_codes (dx_code_kmer_codes) on the GPU against its numpy statement (tests/_kmers_wide.py): the WHOLE output array
is compared, place by place -- every unit length around k, a chunk and the cuts between the kernel's three paths, every phase of a
unit's start and every residue of its byte offset; and everything that is NOT a unit (the guard bytes around it, the symbols in front
of d_beg, the pad bits of its last byte) is filled with Ts, so that a window that reaches outside its unit has a code the statement
does not have.  Behind the last window stand guard words.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_wide as W
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# csrc/kmers/dx_kmer_codes.hip
CHUNK = 64            # KC_CHUNK: positions of one 16-byte chunk, which stands on a 16-byte boundary of the BUFFER
KS = [1, 2, 14, 15, 16, 17, 31, 32]
E_ARG, E_FORMAT, E_NOMEM = -1, -3, -6          # DX_E_*
T = 3                 # the foreign symbol
GUARD = 8             # words behind the last window
MARK = np.uint64(0xC0DEC0DEC0DEC0DE)


def lengths(k):
    return sorted({0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 4 * CHUNK - 1, 4 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1, 5003})


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


class Buffer:
    """a packed buffer that grows unit by unit; around a unit everything is T, the pad bits too"""
    def __init__(self):
        self.sym, self.boff, self.beg, self.ln, self.n = [], [], [], [], 0       # n: symbols so far (4 a byte)

    def add(self, codes, phase=None, beg=0, guard=2, tail=2):
        """the unit's symbols; phase: (byte offset of its read) mod 16, beg: the symbols of its read in front of it"""
        at = self.n // 4 + guard
        if phase is not None:
            at += (phase - at) % 16
        front = 4 * (at - self.n // 4) + beg
        codes = np.asarray(codes, np.uint8)
        end = self.n + front + len(codes)
        self.sym += [np.full(front, T, np.uint8), codes, np.full((-end) % 4 + 4 * tail, T, np.uint8)]
        self.boff.append(at); self.beg.append(beg); self.ln.append(len(codes))
        self.n = end + (-end) % 4 + 4 * tail
        return self

    def packed(self):
        return F.pack(np.concatenate(self.sym), pad=0xff) if self.sym else b""


def run(ctx, packed, boff, beg, ln, k, canonical=False, short=0, in_bytes=None):
    """one call against the statement: (the array as the device left it without its guard, the windows, the error or None); the
    codes get `short` words less than the windows need"""
    want, bad = W.packed_codes(packed, boff, beg, ln, k, canonical, in_bytes)
    nbytes = len(packed) if in_bytes is None else in_bytes
    d_in = ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16)
    d_boff, d_len = ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(ln, np.uint32))
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    cap = len(want) - short
    d_codes = ctx.alloc(8 * (len(want) + GUARD)).upload(np.full(len(want) + GUARD, MARK))
    err = None
    try:
        try:
            _, windows = ctx.code_kmer_codes(d_in, d_boff, d_beg, d_len, k, canonical, cap=cap, codes=d_codes, in_bytes=nbytes, n=len(ln))
        except L.DexGPUError as e:
            err, windows = e, e.windows
        got = d_codes.download(np.uint64, len(want) + GUARD)
    finally:
        for x in (d_in, d_boff, d_len, d_beg, d_codes):
            if x is not None:
                x.free()
    assert windows == len(want)
    assert (got[len(want):] == MARK).all(), "a word behind the last window was written"
    if err is None or err.code == E_FORMAT:
        assert np.array_equal(got[:len(want)], want), (k, canonical, np.flatnonzero(got[:len(want)] != want)[:5])
        assert bad is None if err is None else err.bad_unit == bad
    return got[:len(want)], windows, err


def every_length(k, seed):
    """every length at all four phases of d_beg, the byte offsets going through every residue mod 16"""
    rng, b, j = np.random.default_rng(seed), Buffer(), 0
    for n in lengths(k):
        for beg in range(4):
            b.add(rng.integers(0, 4, n), phase=(5 * j) % 16, beg=beg + 4 * (j % 3))
            j += 1
    assert {o % 16 for o in b.boff} == set(range(16))
    return b


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_every_length_phase_and_offset(ctx, k, canonical):
    b = every_length(k, 200 + k)
    got, windows, err = run(ctx, b.packed(), b.boff, b.beg, b.ln, k, canonical)
    assert err is None and windows == sum(max(0, n - k + 1) for n in b.ln) > 0
    if k < 32:
        assert int(got.max()) < 4 ** k                             # the bits above the code are zero


@pytest.mark.parametrize("k", [15, 32])
def test_whole_reads_without_d_beg(ctx, k):
    rng, b = np.random.default_rng(k), Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, k - 1]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=0)
    assert run(ctx, b.packed(), b.boff, None, b.ln, k, True)[2] is None


@pytest.mark.parametrize("k", [2, 21, 32])
def test_the_buffers_end_and_a_buffer_shorter_than_a_load(ctx, k):
    rng = np.random.default_rng(40 + k)
    for n in (k, 37, 61, 64, 129, 1030):                          # the unit ends in the buffer's last byte; 37, 61: fewer than 16 bytes
        for beg in range(4):
            if n - beg < k:
                continue
            packed = F.pack(rng.integers(0, 4, n), pad=0xff)
            got, windows, err = run(ctx, packed, [0], [beg], [n - beg], k, k != 21)
            assert err is None and windows == n - beg - k + 1
    packed = F.pack(np.concatenate([np.full(13, T, np.uint8), rng.integers(0, 4, 300)]), pad=0xff)       # ... and begins at an odd byte of it
    assert run(ctx, packed, [3], [1], [300], k)[2] is None


def test_empty_units_and_units_that_overlap_and_repeat(ctx):
    rng = np.random.default_rng(9)
    packed = F.pack(rng.integers(0, 4, 4000))
    boff = [0, 0, 10, 10, 500, 0, 999, 17, 0]
    beg = [0, 5, 3, 3, 0, 0, 0, 2, 3999]
    ln = [4000, 100, 0, 700, 20, 4000, 4, 2000, 1]
    for k in (1, 16, 21, 32):
        got, windows, err = run(ctx, packed, boff, beg, ln, k, canonical=k == 21)
        assert err is None and windows == sum(max(0, n - k + 1) for n in ln)
    got, windows, err = run(ctx, packed, [], [], [], 21)
    assert err is None and windows == 0


@pytest.mark.parametrize("k", [2, 16, 31, 32])
def test_canonical_at_the_edges_of_the_code(ctx, k):
    """poly-T is the top code (2^64 - 1 at k = 32) before the minimum and 0 after it, poly-A is 0, and a window that is its own
    reverse complement (even k) stays what it is"""
    own = np.array(([0, 1, 2, 3] * 8)[:k] if k % 4 == 0 else ([0, 3] * 16)[:k], np.uint8)          # ACGT.., or AT..: both their own
    if k % 2 == 0:
        assert (own == 3 - own[::-1]).all()
    rng = np.random.default_rng(k)
    s = np.concatenate([np.full(100, 3), rng.integers(0, 4, 33), own, rng.integers(0, 4, 29), np.full(100, 0), own, np.full(70, 3)]).astype(np.uint8)
    b = Buffer().add(s, phase=7, beg=1).add(np.full(k, 3), phase=0, beg=2).add(own, phase=15, beg=3)
    plain, _, _ = run(ctx, b.packed(), b.boff, b.beg, b.ln, k, False)
    canon, _, _ = run(ctx, b.packed(), b.boff, b.beg, b.ln, k, True)
    top = 2 ** (2 * k) - 1
    assert int(plain[0]) == top and int(canon[0]) == 0 and int(plain[len(s) - k + 1]) == top and int(canon[len(s) - k + 1]) == 0
    if k % 2 == 0:
        code = int(W.codes(own, k)[0])
        assert int(canon[-1]) == code == int(plain[-1]) and code in canon[:len(s) - k + 1].tolist()


def test_a_list_one_word_short_is_nomem_and_nothing_is_written(ctx):
    rng, b = np.random.default_rng(3), Buffer()
    for n in (100, 40, 2000):
        b.add(rng.integers(0, 4, n), beg=1)
    got, windows, err = run(ctx, b.packed(), b.boff, b.beg, b.ln, 21, short=1)
    assert err is not None and err.code == E_NOMEM and windows == 80 + 20 + 1980 and "2080" in str(err)
    assert (got == MARK).all()


@pytest.mark.parametrize("k", [15, 32])
def test_a_bad_unit_in_the_middle(ctx, k):
    rng, b = np.random.default_rng(k), Buffer()
    for n in (300, 64, 5003, 90, 700):
        b.add(rng.integers(0, 4, n), beg=2)
    nbytes = len(b.packed())
    for j, (at, ln) in ((2, (nbytes + 1, 50)), (1, (nbytes - 10, 100)), (3, (0, 0x80000000))):
        boff, lens = list(b.boff), list(b.ln)
        boff[j], lens[j] = at, ln
        got, windows, err = run(ctx, b.packed(), boff, b.beg, lens, k)            # (run holds the good units' codes against the statement)
        assert err is not None and err.code == E_FORMAT and err.bad_unit == j
    boff = list(b.boff)
    boff[1] = boff[4] = nbytes + 5
    assert run(ctx, b.packed(), boff, b.beg, b.ln, k)[2].bad_unit == 1


def test_the_method_makes_an_array_of_the_right_size_itself(ctx):
    rng, b = np.random.default_rng(12), Buffer()
    for n in (500, 20, 0, 1300):
        b.add(rng.integers(0, 4, n), beg=2)
    packed = b.packed()
    want, _ = W.packed_codes(packed, b.boff, b.beg, b.ln, 21, True)
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array(b.boff, np.uint64)),
            ctx.to_device(np.array(b.beg, np.uint32)), ctx.to_device(np.array(b.ln, np.uint32))]
    codes = None
    try:
        codes, windows = ctx.code_kmer_codes(bufs[0], bufs[1], bufs[2], bufs[3], 21, canonical=True)
        assert windows == len(want) == 480 + 1280 and codes.nbytes >= 8 * windows
        assert np.array_equal(codes.download(np.uint64, windows), want)
    finally:
        for x in bufs + [codes]:
            if x is not None:
                x.free()


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    try:
        for k in (0, 33):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_codes(d, d, None, d, k, codes=d, cap=4, in_bytes=16, n=1)
            assert e.value.code == E_ARG and "k = %d" % k in str(e.value)
        for args in ((None, d, d), (d, None, d), (d, d, None)):                       # the buffer, the offsets, the lengths
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_kmer_codes(args[0], args[1], None, args[2], 21, codes=d, cap=4, in_bytes=16, n=1)
            assert e.value.code == E_ARG
        win = api.C.c_uint64()
        assert ctx.lib.dx_code_kmer_codes(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, None, 4, api.C.byref(win), None) == E_ARG
        assert ctx.lib.dx_code_kmer_codes(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, 21, 0, d.ptr, 4, None, None) == E_ARG
        assert ctx.lib.dx_code_kmer_codes(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, 21, 0, d.ptr, 4, api.C.byref(win), None) == E_ARG
    finally:
        d.free()
