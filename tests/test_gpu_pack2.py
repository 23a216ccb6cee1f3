"""k_pack2_encode and k_pack2_decode on the GPU (needs an MI355X), through dx_pack2_encode / dx_pack2_decode alone: the case sets of
_pack2_cases.py -- every small shape at every address, texts that end around each 1 KiB step so that the decoder's three-ahead loop
is left through every slot, input bits and bytes that are no read's, narrow and blank lines, framing bytes, texts that end with the
buffer -- against that module's numpy references.  Bar: bit-exact over the WHOLE output buffer, which is pre-filled with FILL, has a
byte or more between two outputs and GUARD bytes around all: a byte written anywhere else fails."""
import numpy as np
import pytest

import _pack2_cases as P
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

DX_E_MISMATCH = -7


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def freed(bufs):
    for d in bufs:
        if d is not None:
            d.free()


def device_decode(ctx, letters, width, packed, in_off, nsym, out_off, out_bytes):
    """dx_pack2_decode into a buffer of out_bytes pre-filled with FILL -> that buffer"""
    bufs = [ctx.to_device(packed), ctx.to_device(np.asarray(in_off, np.uint64)), ctx.to_device(np.asarray(nsym, np.uint32)),
            ctx.to_device(np.asarray(out_off, np.uint64)), ctx.to_device(np.full(out_bytes, P.FILL, np.uint8))]
    try:
        ctx.pack2_decode(letters, bufs[0], bufs[1], bufs[2], len(nsym), width, bufs[4], bufs[3])
        return bufs[4].download(np.uint8, out_bytes)
    finally:
        freed(bufs)


def device_encode(ctx, c, nsym=None):
    """dx_pack2_encode of an EncodeCall into a buffer pre-filled with FILL -> that buffer"""
    bufs = [ctx.to_device(np.frombuffer(c.text, np.uint8)), ctx.to_device(c.off), ctx.to_device(c.tlen),
            ctx.to_device(c.nsym if nsym is None else nsym), ctx.to_device(c.out_off), ctx.to_device(np.full(c.out_bytes, P.FILL, np.uint8)),
            ctx.to_device(c.hdr) if c.hdr is not None else None,
            ctx.to_device(c.hdr_off) if c.hdr is not None else None]
    try:
        ctx.pack2_encode(c.alphabet, bufs[0], bufs[1], bufs[2], bufs[3], len(c.off), bufs[6], bufs[7], bufs[5], bufs[4])
        return bufs[5].download(np.uint8, c.out_bytes)
    finally:
        freed(bufs)


def where_they_differ(got, want, out_off, describe):
    """None, or the first few differing offsets with the units they lie in or behind"""
    if got.tobytes() == want.tobytes():
        return None
    diff = np.flatnonzero(got != want)
    unit = np.maximum(np.searchsorted(np.asarray(out_off, np.int64), diff[:5], side="right") - 1, 0)
    return f"{len(diff)} bytes differ, first at {diff[:5].tolist()}: " + "; ".join(
        f"{int(d)} = unit {int(u)} + {int(d) - int(out_off[u])} ({describe(int(u))}) got {int(got[d])} want {int(want[d])}" for d, u in zip(diff[:5], unit))


def assert_guards(got):
    assert (got[:P.GUARD] == P.FILL).all() and (got[-P.GUARD:] == P.FILL).all()


# ---- 1. the decode grid ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,letters", P.decode_params(), ids=P.decode_ids())
def test_decode_every_shape(ctx, width, letters):
    c = P.decode_case(width)
    want = P.decode_want(c, letters)
    got = device_decode(ctx, letters, width, c.packed, c.in_off, c.nsym, c.out_off, c.out_bytes)
    bad = where_they_differ(got, want, c.out_off, lambda u: f"width {width}, L {int(c.nsym[u])}, adj {int(c.adj[u])}, part {c.part[u]}")
    assert bad is None, bad
    assert_guards(got)


def some_reads(case, pick):
    """the reads `pick` of a decode case as a call of their own, laid out again: (packed, in_off, nsym, out_off, out_bytes, want)"""
    rng = np.random.Generator(np.random.PCG64(len(pick)))
    syms = [case.sym[int(case.sym_off[r]): int(case.sym_off[r + 1])] for r in pick]
    parts, in_off, out_off, o = [rng.integers(0, 256, 3, dtype=np.uint8)], [], [], P.GUARD
    for r, s in zip(pick, syms):
        in_off.append(sum(len(p) for p in parts))
        p = P.pack_ref(s).copy()
        if len(s) & 3:
            p[-1] |= rng.integers(0, 256, dtype=np.uint8) & ((1 << (2 * (-len(s) % 4))) - 1)
        parts += [p, rng.integers(0, 256, 2, dtype=np.uint8)]
        o += 1 + (int(case.adj[r]) - o - 1) % 16
        out_off.append(o)
        o += P.text_len(len(s), case.width)
    return np.concatenate(parts), in_off, [len(s) for s in syms], out_off, o + P.GUARD, syms


@pytest.mark.parametrize("n", [1, 17])
def test_decode_calls_of_one_and_of_seventeen_reads(ctx, n):
    """(the waves draw sixteen reads a ticket: seventeen are a ticket and a read)"""
    for width, letters in ((80, L.DX_LETTERS_UPPER), (17, L.DX_LETTERS_ARROW), (3, L.DX_LETTERS_NUMBERS)):
        case = P.decode_case(width)
        longs = [r for r in range(len(case.nsym)) if case.part[r] == "b"]
        pick = [longs[5 * 64 + 7]] if n == 1 else longs[3::41][:12] + [5, 140, 1000, 2000, 0]
        assert len(pick) == n
        packed, in_off, nsym, out_off, out_bytes, syms = some_reads(case, pick)
        want = np.full(out_bytes, P.FILL, np.uint8)
        for o, s in zip(out_off, syms):
            want[o: o + P.text_len(len(s), width)] = P.decode_ref(s, letters, width)
        got = device_decode(ctx, letters, width, packed, in_off, nsym, out_off, out_bytes)
        bad = where_they_differ(got, want, out_off, lambda u: f"width {width}, L {nsym[u]}, adj {out_off[u] & 15}")
        assert bad is None, bad


def test_decode_a_batch_of_empty_reads_writes_nothing(ctx):
    rng = np.random.Generator(np.random.PCG64(40))
    packed = rng.integers(0, 256, 256, dtype=np.uint8)
    in_off, out_off = np.arange(40) * 3 + 1, P.GUARD + np.arange(40) * 5
    for width in (1, 80):
        got = device_decode(ctx, L.DX_LETTERS_LOWER, width, packed, in_off, np.zeros(40, np.uint32), out_off, 512)
        assert (got == P.FILL).all()


# ---- 2. the encode grid ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(P.ALPHABETS))
def test_encode_every_shape(ctx, kind):
    for c in P.encode_calls(kind):
        got = device_encode(ctx, c)
        hl = np.diff(c.hdr_off.astype(np.int64)) if c.hdr is not None else np.zeros(len(c.off), np.int64)
        bad = where_they_differ(got, c.want, c.out_off, lambda u: f"{c.name}, text of {int(c.tlen[u])} bytes at {int(c.off[u])} (mod 16: "
                                f"{int(c.off[u]) & 15}), {int(c.nsym[u])} symbols, {int(hl[u])} framing bytes, "
                                f"{len(c.text) - int(c.off[u]) - int(c.tlen[u])} bytes behind it")
        assert bad is None, bad
        assert_guards(got)


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------

def test_encode_says_when_a_count_is_wrong_and_forgets_it(ctx):
    c = P.contract_call()
    mid = len(c.off) // 2
    for delta in (1, -1):
        nsym = c.nsym.copy()
        nsym[mid] = int(nsym[mid]) + delta
        with pytest.raises(L.DexGPUError) as e:
            device_encode(ctx, c, nsym)
        assert e.value.code == DX_E_MISMATCH and L.ERR_NAMES[e.value.code] == "DX_E_MISMATCH", str(e.value)
        got = device_encode(ctx, c)                            # DX_OK (anything else raises): the status word does not stick
        bad = where_they_differ(got, c.want, c.out_off, lambda u: f"{int(c.nsym[u])} symbols")
        assert bad is None, bad


@pytest.mark.parametrize("width", P.WIDTHS)
def test_decode_then_encode_gives_the_packed_bytes_back(ctx, width):
    """The grid's reads decoded, and the texts encoded where they stand in the decoder's output buffer, in one context: the packed
    bytes again, each read's where it came from, the pad bits 0 and not a byte more"""
    c, letters = P.decode_case(width), P.letters_at(width)
    n = len(c.nsym)
    tlen = np.array([P.text_len(int(x), width) for x in c.nsym], np.uint32)
    bufs = [ctx.to_device(c.packed), ctx.to_device(c.in_off), ctx.to_device(c.nsym), ctx.to_device(c.out_off),
            ctx.to_device(np.full(c.out_bytes, P.FILL, np.uint8)), ctx.to_device(tlen), ctx.to_device(np.full(c.in_bytes, P.FILL, np.uint8))]
    d_packed, d_in_off, d_nsym, d_out_off, d_text, d_tlen, d_again = bufs
    try:
        ctx.pack2_decode(letters, d_packed, d_in_off, d_nsym, n, width, d_text, d_out_off)
        ctx.pack2_encode(P.ALPHA_OF_LETTERS[letters], d_text, d_out_off, d_tlen, d_nsym, n, None, None, d_again, d_in_off)
        got = d_again.download(np.uint8, c.in_bytes)
    finally:
        freed(bufs)
    bad = where_they_differ(got, P.packed_want(c), c.in_off, lambda u: f"width {width}, L {int(c.nsym[u])}, adj {int(c.adj[u])}")
    assert bad is None, bad
