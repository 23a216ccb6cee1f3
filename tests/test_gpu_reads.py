"""The .bps / .arw read side on the GPU (needs an MI355X): dx_reads_unpack (k_reads_unpack) and dx_reads_uncompress --
Load_Read / Load_Subread / Load_All_Reads / Load_Arrow (DB.c:1232-1441, 1508-1548) for a selection at once.  Inputs are the
oracle's Compress_Read bytes and the reference's own golden images, outputs plain slices of the source symbols.  Bar: bit-exact,
and not a byte written outside a unit's len + 1."""
import functools
import struct

import numpy as np
import pytest

from _flags import set_flag

import _oracle as O
from _pack2_cases import LETTERS, NUMBER_ARROW, NUMBER_READ
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

DELIM = {L.DX_LETTERS_LOWER: 0, L.DX_LETTERS_UPPER: 0, L.DX_LETTERS_ARROW: 0, L.DX_LETTERS_NUMBERS: 4}   # DB.c:367-389, DB.c:362
ALL_LETTERS = sorted(LETTERS)
FILL, GUARD = 0xEE, 64
TRANSPORTS = ["reads_packed", "reads_whole"]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def letters_of(sym, letters):
    """symbols 0..3 (uint8 array) as the bytes of a letter set"""
    return np.frombuffer(LETTERS[letters], np.uint8)[sym].tobytes()


def pack(syms, arrow=False, lead=b""):
    """The reads' Compress_Read bytes one behind the other, as .bps / .arw hold them, `lead` bytes in front: (payload, boff)"""
    src = LETTERS[L.DX_LETTERS_ARROW if arrow else L.DX_LETTERS_LOWER]
    parts = [O.compress_read(np.frombuffer(src, np.uint8)[s].tobytes(), arrow) for s in syms]
    boff = len(lead) + np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]]).astype(np.uint64)
    return lead + b"".join(parts), boff.astype(np.uint64)


def device_unpack(ctx, letters, payload, boff, beg, lens, out_off, out_bytes, in_bytes=None):
    """dx_reads_unpack into a buffer of out_bytes pre-filled with FILL -> that buffer"""
    bufs = [ctx.to_device(np.frombuffer(payload, np.uint8)) if len(payload) else ctx.alloc(16),
            ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(lens, np.uint32)),
            ctx.to_device(np.asarray(out_off, np.uint64)), ctx.to_device(np.full(out_bytes, FILL, np.uint8))]
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    try:
        ctx.reads_unpack(letters, bufs[0], len(payload) if in_bytes is None else in_bytes, bufs[1], d_beg, bufs[2], len(lens), bufs[4], bufs[3])
        return bufs[4].download(np.uint8, out_bytes).tobytes()
    finally:
        for d in bufs + ([d_beg] if d_beg else []):
            d.free()


def units_of(text, toff, lens, letters):
    """Load_All_Reads' layout, checked: a delimiter in front, toff as the lengths say, a delimiter behind every unit -> the units"""
    d = DELIM[letters]
    assert len(toff) == len(lens) + 1 and int(toff[0]) == 1 and int(toff[-1]) == len(text) and text[0] == d
    assert (np.diff(toff.astype(np.int64)) == np.asarray(lens, np.int64) + 1).all()
    assert all(text[int(t) - 1] == d for t in toff)
    return [text[int(toff[j]): int(toff[j]) + int(lens[j])] for j in range(len(lens))]


# ---- 1. every small shape ---------------------------------------------------------------------------------------------------

SHAPE_LENGTHS = list(range(71)) + [1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049, 4099, 70000]


@functools.lru_cache(maxsize=None)
def shapes():
    """One read a unit: every length at every phase of beg, the reads back to back behind one odd byte; the outputs with a byte
    between two of them and GUARD bytes around all.  Computed once, never changed."""
    rng = np.random.Generator(np.random.PCG64(20261018))
    beg = np.array([p for p in range(4) for _ in SHAPE_LENGTHS], np.uint32)
    lens = np.array(SHAPE_LENGTHS * 4, np.uint32)
    syms = [rng.integers(0, 4, int(b + n + rng.integers(0, 6)), dtype=np.uint8) for b, n in zip(beg, lens)]
    payload, boff = pack(syms, lead=b"\xa5")
    out_off = (GUARD + 1 + np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 2)[:-1]])).astype(np.uint64)
    out_bytes = int(out_off[-1]) + int(lens[-1]) + 1 + GUARD
    assert set(int(x) & 15 for x in out_off) == set(range(16))         # (device buffers stand on 256-byte boundaries)
    assert len(set(int(x) & 3 for x in boff)) == 4 and any(int(x) & 1 for x in boff)
    for a in (beg, lens, boff, out_off):
        a.setflags(write=False)
    return syms, payload, boff, beg, lens, out_off, out_bytes


@pytest.mark.parametrize("letters", ALL_LETTERS, ids=["lower", "upper", "arrow", "numbers"])
def test_every_small_shape(ctx, letters):
    syms, payload, boff, beg, lens, out_off, out_bytes = shapes()
    want = bytearray([FILL]) * out_bytes
    for s, b, n, o in zip(syms, beg, lens, out_off):
        b, n, o = int(b), int(n), int(o)
        want[o: o + n] = letters_of(s[b: b + n], letters)
        want[o + n] = DELIM[letters]
    got = device_unpack(ctx, letters, payload, boff, beg, lens, out_off, out_bytes)
    if got != bytes(want):
        diff = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(bytes(want), np.uint8))[0]
        unit = np.searchsorted(out_off, diff[:5], side="right") - 1
        pytest.fail(f"{len(diff)} bytes differ, first at {diff[:5]} (units {unit}: beg {beg[unit]}, len {lens[unit]})")
    assert got[:GUARD] == bytes([FILL]) * GUARD and got[-GUARD:] == bytes([FILL]) * GUARD


# ---- 2. the reference's bytes ---------------------------------------------------------------------------------------------------

def bare_payloads(name):
    """The packed payloads of a reference-made .dexta / .dexar, framing cut away, one behind the other as
    .bps / .arw hold them: (payload, boff, rlen)"""
    arrow = name.endswith(".dexar")
    img = O.golden(name)
    key, plen = struct.unpack_from("<Hi", img, 0)
    assert key == 0x55aa
    at, parts, rlen = 6 + plen, [], []
    while at < len(img):
        while img[at] == 0xff:                             # the well delta: a 0xff for every whole 255, then a byte
            at += 1
        beg, end = struct.unpack_from("<ii", img, at + 1)
        at += 1 + 8 + (8 if arrow else 4)                  # ... beg, end, and the quality value or the four channel SNRs
        n = end - beg
        parts.append(img[at: at + (n + 3) // 4])
        rlen.append(n)
        at += (n + 3) // 4
    assert at == len(img) and len(parts) > 3
    boff = np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]]).astype(np.uint64)
    return b"".join(parts), boff, np.array(rlen, np.uint32)


def sequences(text):
    """per record of a .fasta / .arrow text its sequence lines, joined"""
    recs = []
    for ln in text.split(b"\n")[:-1]:
        if ln[:1] == b">":
            recs.append(b"")
        else:
            recs[-1] += ln
    return recs


@pytest.mark.parametrize("img,rt", [("ta_edge.dexta", "ta_edge.rt.fasta"), ("ta_small.dexta", "ta_small.fasta"),
                                    ("ar_edge.dexar", "ar_edge.rt.arrow")], ids=["ta_edge", "ta_small", "ar_edge"])
def test_reference_bytes_back_to_reference_letters(ctx, img, rt):
    """(ta_small's round trip IS its input: tests/golden/cases.json)"""
    payload, boff, rlen = bare_payloads(img)
    seqs = sequences(O.golden(rt))
    assert [len(s) for s in seqs] == rlen.tolist()
    if img.endswith(".dexar"):
        cases = [(L.DX_LETTERS_ARROW, seqs), (L.DX_LETTERS_NUMBERS, [s.translate(NUMBER_ARROW) for s in seqs])]
    else:
        cases = [(L.DX_LETTERS_LOWER, [s.lower() for s in seqs]), (L.DX_LETTERS_UPPER, [s.upper() for s in seqs]),
                 (L.DX_LETTERS_NUMBERS, [s.translate(NUMBER_READ) for s in seqs])]
    for letters, want in cases:
        text, toff = ctx.reads_uncompress(payload, boff, rlen, letters=letters)
        assert units_of(text, toff, rlen, letters) == want, (img, letters)


# ---- 3. subreads at every phase of both ends ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_long_read():
    rng = np.random.Generator(np.random.PCG64(4099))
    syms = [rng.integers(0, 4, 37, dtype=np.uint8), rng.integers(0, 4, 4099, dtype=np.uint8)]
    payload, boff = pack(syms)
    assert int(boff[1]) + (4099 + 3) // 4 == len(payload)          # the long read's last byte is the buffer's last
    return syms, payload, boff, np.array([37, 4099], np.uint32)


@pytest.mark.parametrize("transport", TRANSPORTS)
def test_subreads_at_every_phase_of_both_ends(ctx, transport, monkeypatch):
    syms, payload, boff, rlen = one_long_read()
    pairs = [(b, b + d) for b in list(range(10)) + list(range(1020, 1031)) for d in (0, 1, 2, 3, 4, 5, 15, 16, 17, 64, 1024) if b + d <= 4099]
    pairs += [(4099 - d, 4099) for d in (0, 1, 2, 3, 4, 5, 15, 16, 17, 64, 1024, 4099)]   # ... that end in the buffer's last byte
    beg, end = np.array(pairs, np.uint32).T
    ids = np.ones(len(pairs), np.uint64)
    set_flag(monkeypatch, transport)
    for letters in (L.DX_LETTERS_NUMBERS, L.DX_LETTERS_UPPER):
        text, toff = ctx.reads_uncompress(payload, boff, rlen, ids=ids, beg=beg, end=end, letters=letters)
        got = units_of(text, toff, end - beg, letters)
        want = [letters_of(syms[1][b:e], letters) for b, e in pairs]
        assert got == want, [pairs[k] for k in range(len(pairs)) if got[k] != want[k]][:8]


# ---- 4. selection and order -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def payload200():
    rng = np.random.Generator(np.random.PCG64(200))
    syms = [rng.integers(0, 4, int(n), dtype=np.uint8) for n in rng.integers(1, 9001, 200)]
    payload, boff = pack(syms)
    return syms, payload, boff, np.array([len(s) for s in syms], np.uint32)


@functools.lru_cache(maxsize=None)
def all_reads200():
    """every read as numbers, from the source symbols"""
    return [s.tobytes() for s in payload200()[0]]


def test_selection_and_order(ctx, monkeypatch):
    syms, payload, boff, rlen = payload200()
    text, toff = ctx.reads_uncompress(payload, boff, rlen)
    every = units_of(text, toff, rlen, L.DX_LETTERS_NUMBERS)
    assert every == all_reads200()
    repeats = np.random.Generator(np.random.PCG64(7)).integers(0, 200, 300)
    assert len(set(repeats.tolist())) < 300
    for ids in (np.arange(200)[::-1], repeats):
        t, o = ctx.reads_uncompress(payload, boff, rlen, ids=ids)
        assert units_of(t, o, rlen[ids], L.DX_LETTERS_NUMBERS) == [every[int(i)] for i in ids]
    t, o = ctx.reads_uncompress(payload, boff, rlen, ids=[])
    assert t == b"\x04" and o.tolist() == [1]
    t, o = ctx.reads_uncompress(payload, boff, rlen, ids=[], letters=L.DX_LETTERS_LOWER)
    assert t == b"\x00" and o.tolist() == [1]
    sparse = np.array([150, 3, 199, 77, 3])
    for transport in TRANSPORTS:
        set_flag(monkeypatch, transport)
        t, o = ctx.reads_uncompress(payload, boff, rlen, ids=sparse)
        assert units_of(t, o, rlen[sparse], L.DX_LETTERS_NUMBERS) == [every[int(i)] for i in sparse], transport
        set_flag(monkeypatch, transport, None)


# ---- 5. slices ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transport", TRANSPORTS)
def test_slices_give_the_same_bytes(ctx, transport, monkeypatch):
    syms, payload, boff, rlen = payload200()
    ids = np.concatenate([np.arange(200)[::-1], np.arange(0, 200, 7)])
    want = ctx.reads_uncompress(payload, boff, rlen, ids=ids)
    assert units_of(want[0], want[1], rlen[ids], L.DX_LETTERS_NUMBERS) == [all_reads200()[int(i)] for i in ids]
    budget = 200000
    assert len(want[0]) > 3 * budget                       # at least four slices
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
    set_flag(monkeypatch, transport)
    got = ctx.reads_uncompress(payload, boff, rlen, ids=ids)
    assert got[0] == want[0] and (got[1] == want[1]).all()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

# budget: the selection in slices (test_slices_give_the_same_bytes' figure), every read in order, so that the cut one lies in the last
# slice and its place there is not its place in the selection
@pytest.mark.parametrize("transport, budget", [(t, 0) for t in TRANSPORTS] + [(t, 200000) for t in TRANSPORTS],
                         ids=TRANSPORTS + [f"sliced_{t}" for t in TRANSPORTS])
def test_a_payload_cut_short_names_the_callers_read(ctx, transport, budget, monkeypatch):
    syms, payload, boff, rlen = payload200()
    n, cut = 200, payload[:-1]
    set_flag(monkeypatch, transport)
    selections = (None, np.array([3, n - 1, 7]), np.arange(n)[::-1])
    if budget:
        assert int(rlen[: n - 1].sum()) + n - 1 > budget           # the last read begins behind the first slice
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
        selections = (np.arange(n),)
    for ids in selections:
        with pytest.raises(L.DexGPUError) as e:
            ctx.reads_uncompress(cut, boff, rlen, ids=ids)
        assert e.value.code == -3 and f"entry {n - 1}," in str(e.value), str(e.value)
    # the error came from the library, not from the device: the same context decodes the reads in front of the cut
    ids = np.arange(n - 1)[::-1]
    t, o = ctx.reads_uncompress(cut, boff, rlen, ids=ids)
    assert units_of(t, o, rlen[ids], L.DX_LETTERS_NUMBERS) == [all_reads200()[int(i)] for i in ids]


def test_unpack_reports_the_smallest_bad_unit(ctx):
    sym = np.arange(40, dtype=np.uint8) & 3
    payload, _ = pack([sym])
    assert len(payload) == 10
    #            good     one symbol too many   good, at the end   starts behind the end   nothing, at the end
    boff = [0,       0,                    9,                 11,                     10]
    beg  = [0,       1,                    0,                 0,                      3]
    lens = [40,      40,                   4,                 0,                      0]
    out_off = [16, 80, 144, 160, 176]
    with pytest.raises(L.DexGPUError) as e:
        device_unpack(ctx, L.DX_LETTERS_NUMBERS, payload, boff, beg, lens, out_off, 256)
    assert e.value.code == -3 and e.value.bad_unit == 1
    with pytest.raises(L.DexGPUError) as e:
        device_unpack(ctx, L.DX_LETTERS_NUMBERS, payload, boff[2:], beg[2:], lens[2:], out_off[2:], 256)
    assert e.value.code == -3 and e.value.bad_unit == 1
    # without the two, all is well: a unit of no symbols at boff == in_bytes is its delimiter
    keep = [0, 2, 4]
    got = device_unpack(ctx, L.DX_LETTERS_NUMBERS, payload, [boff[k] for k in keep], [beg[k] for k in keep], [lens[k] for k in keep],
                        [out_off[k] for k in keep], 256)
    want = bytearray([FILL]) * 256
    want[16:57] = sym.tobytes() + b"\x04"
    want[144:149] = sym[36:].tobytes() + b"\x04"
    want[176] = 4
    assert got == bytes(want)
    # ... and the bound is the buffer's, not the allocation's: the same units with one byte fewer
    with pytest.raises(L.DexGPUError) as e:
        device_unpack(ctx, L.DX_LETTERS_NUMBERS, payload, [0, 9], None, [36, 4], [16, 80], 256, in_bytes=9)
    assert e.value.code == -3 and e.value.bad_unit == 1


# ---- 7. round trip with the encoder ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arrow", [False, True], ids=["bps", "arw"])
def test_round_trip_with_the_encoder(ctx, arrow):
    """dx_pack2_encode with d_hdr == NULL (what dex2DB writes to .bps / .arw), then dx_reads_unpack on the device buffer it left"""
    rng = np.random.Generator(np.random.PCG64(91 + arrow))
    lens = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4099, 20000, 0, 7] + [int(x) for x in rng.integers(1, 9000, 60)]
    alpha = np.frombuffer(b"1234G05" if arrow else b"ACGTacgtNn", np.uint8)
    reads = [alpha[rng.integers(0, len(alpha), n)].tobytes() for n in lens]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    nsym = np.array(lens, np.uint32)
    boff = np.concatenate([[0], np.cumsum((nsym + 3) // 4)]).astype(np.uint64)
    total = int(boff[-1])
    letters = L.DX_LETTERS_ARROW if arrow else L.DX_LETTERS_NUMBERS
    want = [letters_of(np.frombuffer(r.translate(NUMBER_ARROW if arrow else NUMBER_READ), np.uint8), letters) for r in reads]
    out_off = (1 + np.concatenate([[0], np.cumsum(nsym.astype(np.int64) + 1)])).astype(np.uint64)
    bufs = [ctx.to_device(np.frombuffer(b"".join(reads) + b"\0" * 16, np.uint8)), ctx.to_device(off), ctx.to_device(nsym), ctx.to_device(boff),
            ctx.to_device(np.full(total + 64, FILL, np.uint8)), ctx.to_device(out_off), ctx.to_device(np.full(int(out_off[-1]), FILL, np.uint8))]
    d_text, d_off, d_n, d_boff, d_packed, d_oo, d_out = bufs
    try:
        ctx.pack2_encode(L.DX_ALPHA_ARROW if arrow else L.DX_ALPHA_BASES, d_text, d_off, d_n, d_n, len(lens), None, None, d_packed, d_boff)
        ctx.reads_unpack(letters, d_packed, total, d_boff, None, d_n, len(lens), d_out, d_oo)
        got = d_out.download(np.uint8, int(out_off[-1])).tobytes()
    finally:
        for d in bufs:
            d.free()
    assert got[0] == FILL
    assert [got[int(o): int(o) + n] for o, n in zip(out_off, lens)] == want
    assert all(got[int(o) + n] == DELIM[letters] for o, n in zip(out_off, lens))
