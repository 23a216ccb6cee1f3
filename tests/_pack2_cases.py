"""Case sets and plain numpy references for the tests of the 2-bit kernels (csrc/dx_pack2.hip: k_pack2_encode, k_pack2_decode), built
around the numbers those kernels are written on: the decoder's 16 text bytes a lane and 1 KiB a step, its output frame shifted by the
output address mod 16, its requests three steps ahead with four ways out of the loop, the 8 packed bytes a chunk is made from; the
encoder's 2 KiB of text a step, its window drained at 4096 symbols, its masked load within 16 bytes of the text's end, its framing
copy 64 bytes a turn.  No GPU and no library here: every generator is a pure function of fixed seeds, the references are the
operations' definitions written out, and tests/test_pack2_cases_host.py checks both against the oracle and that the case sets
reach what they were built to reach."""
import functools
from collections import namedtuple

import numpy as np

LETTERS_LOWER, LETTERS_UPPER, LETTERS_ARROW, LETTERS_NUMBERS = range(4)                  # DX_LETTERS_* (include/dexgpu.h)
ALPHA_BASES, ALPHA_ARROW, ALPHA_NUMBERS = range(3)                                       # DX_ALPHA_*
LETTERS = {LETTERS_LOWER: b"acgt", LETTERS_UPPER: b"ACGT", LETTERS_ARROW: b"1234", LETTERS_NUMBERS: bytes(range(4))}
ALL_LETTERS = sorted(LETTERS)
LETTER_NAMES = ["lower", "upper", "arrow", "numbers"]
NUMBER_READ = bytes(1 if chr(c) in "cC" else 2 if chr(c) in "gG" else 3 if chr(c) in "tT" else 0 for c in range(256))    # DB.c:393-416
NUMBER_ARROW = bytes(0 if chr(c) == "1" else 1 if chr(c) == "2" else 2 if chr(c) in "3G" else 3 for c in range(256))     # DB.c:418-441
CODES = {ALPHA_BASES: NUMBER_READ, ALPHA_ARROW: NUMBER_ARROW, ALPHA_NUMBERS: bytes(c & 3 for c in range(256))}
ALPHA_OF_LETTERS = {LETTERS_LOWER: ALPHA_BASES, LETTERS_UPPER: ALPHA_BASES, LETTERS_ARROW: ALPHA_ARROW, LETTERS_NUMBERS: ALPHA_NUMBERS}
FILL, GUARD = 0xEE, 64
STEP = 1024                                              # DX_STEP: text bytes a wave decodes in one step


# ---- the references ------------------------------------------------------------------------------------------------------------

def text_len(L, width):
    """bytes of L symbols in lines of `width`, a line end behind every line"""
    return L + (L + width - 1) // width


def decode_ref(sym, letters, width):
    """symbols 0..3 -> uint8 [text_len]: the letters, a line end behind every `width` of them and behind the last"""
    sym = np.asarray(sym, np.uint8)
    body = np.full(text_len(len(sym), width), 10, np.uint8)
    i = np.arange(len(sym))
    body[i + i // width] = np.frombuffer(LETTERS[letters], np.uint8)[sym]
    return body


def pack_ref(sym):
    """symbols 0..3 -> uint8 [(n + 3) >> 2]: four a byte, the first in the top two bits, missing ones 0"""
    sym = np.asarray(sym, np.uint8)
    q = np.zeros((len(sym) + 3) // 4 * 4, np.uint8)
    q[: len(sym)] = sym
    q = q.reshape(-1, 4)
    return (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]


def symbols_of(text, alphabet):
    """every byte of the text that is no line end, through the alphabet's table"""
    t = np.frombuffer(bytes(text), np.uint8)
    return np.frombuffer(CODES[alphabet], np.uint8)[t[t != 10]]


def encode_ref(text, alphabet):
    return pack_ref(symbols_of(text, alphabet))


# ---- the decode grid -----------------------------------------------------------------------------------------------------------

WIDTHS = (1, 2, 3, 7, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 80, 1007, 1008, 1009, 1022, 1023, 1024, 1025, 100000)
ALL_LETTER_WIDTHS = (1, 16, 80)
LARGE_WIDTHS = (1, 80, 100000)
SMALL_MAX, LARGE = 130, 70000
LONG_K, LONG_D = tuple(range(1, 11)), (-1, 0, 1, 16)


def letters_at(width):
    """the letter set a width runs with (they rotate over the widths)"""
    return ALL_LETTERS[WIDTHS.index(width) % 4]


def decode_params():
    """(width, letters) of every decode call: one a width, all four letter sets at ALL_LETTER_WIDTHS"""
    return [(w, s) for w in WIDTHS for s in (ALL_LETTERS if w in ALL_LETTER_WIDTHS else [letters_at(w)])]


def decode_ids():
    return [f"w{w}-{LETTER_NAMES[s]}" for w, s in decode_params()]


def long_read_symbols(width, target):
    """-> L whose text is the shortest of at least `target` bytes (no text has 1 byte more than whole lines)"""
    T = target + (target % (width + 1) == 1)
    q, r = divmod(T, width + 1)
    return q * width + (r - 1 if r else 0)


def loop_turns(L, width, adj):
    """k_pack2_decode's three-ahead loop for one read, from P2D_ALLFAST and P2D_TURN: None when the read never enters it, else the
    turns it takes before it leaves.  Turn j is one of the lead-in (j < 3: s_waitcnt vmcnt 3, 4, 5) or a steady one (vmcnt 6), and
    the loop is left through slot j % 4."""
    if width < 16:
        return None
    TS, clen = text_len(L, width) + adj, (L + 3) >> 2

    def all_fast(B):
        return B + STEP < TS and ((B + STEP - 16) >> 2) + 8 <= clen
    if not (all_fast(0) and all_fast(STEP) and all_fast(2 * STEP)):
        return None
    j = 0
    while all_fast((j + 3) * STEP):
        j += 1
    return j


# part: "a" every small length at every address, "b" texts that end around the 1 KiB steps, "c" one large read.  key: L for "a", (k, d)
# for "b".  sym: all reads' symbols, one behind the other (read r: sym[sym_off[r]: sym_off[r + 1]]).  packed: the input image.
DecodeCase = namedtuple("DecodeCase", "width part key adj nsym sym sym_off packed data in_off in_bytes out_off out_bytes")


@functools.lru_cache(maxsize=4)
def decode_case(width):
    """One call's reads.  Input: the packed reads behind one odd byte with now and then a byte or two between them, the pad bits of
    every last byte, the bytes between the reads and 64 behind them random.  Output: every text at its chosen address mod 16, at least
    one byte between two texts and GUARD bytes around all.  Computed once, never changed."""
    rng = np.random.Generator(np.random.PCG64(20261019 + width))
    reads = [("a", L, a, L) for a in range(16) for L in range(SMALL_MAX + 1)]
    reads += [("b", (k, d), a, long_read_symbols(width, k * STEP + d - a)) for k in LONG_K for d in LONG_D for a in range(16)]
    if width in LARGE_WIDTHS:
        reads.append(("c", LARGE, 9, LARGE))
    part, key, adj, nsym = ([r[j] for r in reads] for j in range(4))
    nsym, adj = np.array(nsym, np.uint32), np.array(adj, np.uint32)
    n = len(reads)
    sym_off = np.concatenate([[0], np.cumsum(nsym, dtype=np.int64)])
    sym = rng.integers(0, 4, int(sym_off[-1]), dtype=np.uint8)

    clen = (nsym.astype(np.int64) + 3) >> 2
    gaps = rng.choice([0, 0, 0, 1, 2], n)
    in_off = 1 + np.concatenate([[0], np.cumsum(clen + gaps)[:-1]])
    in_bytes = int(in_off[-1] + clen[-1]) + GUARD
    # the packed bytes and the bits that are theirs, without a loop over the reads; everything else stays random
    r_of = np.repeat(np.arange(n), nsym)
    i = np.arange(len(sym)) - sym_off[r_of]
    at, shift = in_off[r_of] + (i >> 2), (6 - 2 * (i & 3)).astype(np.uint8)
    data = np.bincount(at, weights=sym.astype(np.int64) << shift, minlength=in_bytes).astype(np.uint8)
    owned = np.bincount(at, weights=np.int64(3) << shift, minlength=in_bytes).astype(np.uint8)
    packed = (rng.integers(0, 256, in_bytes, dtype=np.uint8) & ~owned) | data

    out_off, o = np.empty(n, np.int64), GUARD
    for r in range(n):
        o += 1
        o += (int(adj[r]) - o) % 16
        out_off[r] = o
        o += text_len(int(nsym[r]), width)
    case = DecodeCase(width, part, key, adj, nsym, sym, sym_off, packed, data, in_off.astype(np.uint64), in_bytes,
                      out_off.astype(np.uint64), o + GUARD)
    for a in (adj, nsym, sym, sym_off, packed, data, case.in_off, case.out_off):
        a.setflags(write=False)
    return case


def decode_want(case, letters):
    """the whole output buffer of a decode call: FILL but for the texts"""
    want = np.full(case.out_bytes, FILL, np.uint8)
    w, out_off = case.width, case.out_off.astype(np.int64)
    for o, L in zip(out_off.tolist(), case.nsym.tolist()):
        want[o: o + text_len(L, w)] = 10
    r_of = np.repeat(np.arange(len(case.nsym)), case.nsym)
    i = np.arange(len(case.sym)) - case.sym_off[r_of]
    want[out_off[r_of] + i + i // w] = np.frombuffer(LETTERS[letters], np.uint8)[case.sym]
    return want


def packed_want(case):
    """the whole buffer an encoder leaves that writes read r's packed bytes at in_off[r]: FILL but for them, pad bits 0"""
    want = np.full(case.in_bytes, FILL, np.uint8)
    for o, L in zip(case.in_off.tolist(), case.nsym.tolist()):
        want[o: o + ((L + 3) >> 2)] = case.data[o: o + ((L + 3) >> 2)]
    return want


# ---- the encode grid -----------------------------------------------------------------------------------------------------------

LINE_WIDTHS = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 80, None)         # None: a read on one line
HDR_LENS = (0, 1, 13, 17, 63, 64, 65, 130)                           # (the framing bytes are copied 64 a turn)
TEXT_LENGTHS = tuple(2048 * k + e for k in (1, 2, 3) for e in (0, 1, 16, 17, 32, 33))        # P2_STEP
SYMBOL_COUNTS = tuple(4096 * k + e for k in (1, 2, 3) for e in (-1, 0, 1, 2, 3, 16))         # P2_FLUSH_BITS / 2
ALPHABETS = {"bases": ALPHA_BASES, "arrow": ALPHA_ARROW, "numbers": ALPHA_NUMBERS, "numbers_any_byte": ALPHA_NUMBERS}
ENCODE_LARGE_AT = 80                                                 # the line width whose call holds the read of LARGE symbols

# text: the call's whole text buffer, read r at off[r] with tlen[r] bytes, nsym[r] symbols.  hdr / hdr_off: the framing bytes (None:
# the call gives none).  want: the whole output buffer, FILL but for the records at out_off.
EncodeCall = namedtuple("EncodeCall", "name alphabet text off tlen nsym hdr hdr_off out_off out_bytes want")


def _any_byte(rng, n):
    """n bytes of any value but 10"""
    v = rng.integers(0, 255, n, dtype=np.uint8)
    return v + (v >= 10)


def _draw(rng, kind, n):
    if kind == "numbers":
        return rng.integers(0, 4, n, dtype=np.uint8)
    if kind == "numbers_any_byte":
        return _any_byte(rng, n)
    own = np.frombuffer(b"ACGTacgt" if kind == "bases" else b"1234G", np.uint8)   # mostly the alphabet's letters: codes of every value
    return np.where(rng.random(n) < 0.85, own[rng.integers(0, len(own), n)], _any_byte(rng, n))


def wrap(body, lw):
    """the bytes in lines of lw (None: one line), a line end behind every line"""
    lw = lw or max(len(body), 1)
    out = np.full(text_len(len(body), lw), 10, np.uint8)
    i = np.arange(len(body))
    out[i + i // lw] = body
    return out.tobytes()


def shaped(rng, kind, lw, n, shape):
    """A read's text of n symbols.  nl: wrapped; nonl: without the last line end; blank: a blank line first and one in the middle."""
    t = wrap(_draw(rng, kind, n), lw)
    if shape == "nonl":
        return t[:-1]
    if shape == "blank":
        mid = t.find(b"\n", len(t) // 2) + 1
        return b"\n" + t[:mid] + b"\n" + t[mid:]
    return t


def _filler(rng, n):
    """header-like bytes between two reads, some of them line ends"""
    f = rng.integers(32, 127, n, dtype=np.uint8)
    f[rng.random(n) < 0.08] = 10
    f[0] = ord(">")
    return f.tobytes()


def make_call(name, kind, texts, rng, gaps=None, hdr_lens=None):
    """Lay the reads out: filler in front of every read (gaps: its lengths, else 1..48 at random), none behind the last, so that it
    ends with the buffer; framing bytes of hdr_lens (None: no framing); records at every address mod 16 with at least a byte between
    two and GUARD around all."""
    alphabet, n = ALPHABETS[kind], len(texts)
    gaps = rng.integers(1, 49, n) if gaps is None else gaps
    parts, off, at = [], np.empty(n, np.uint64), 0
    for r, (t, g) in enumerate(zip(texts, gaps)):
        parts += [_filler(rng, int(g)), t]
        off[r] = at + int(g)
        at += int(g) + len(t)
    tlen = np.array([len(t) for t in texts], np.uint32)
    packed = [encode_ref(t, alphabet) for t in texts]
    nsym = np.array([len(t) - t.count(b"\n") for t in texts], np.uint32)
    hdr = hdr_off = None
    hl = np.zeros(n, np.int64)
    if hdr_lens is not None:
        hl = np.asarray(hdr_lens, np.int64)
        hdr_off = np.concatenate([[0], np.cumsum(hl)]).astype(np.uint64)
        hdr = rng.integers(0, 256, int(hdr_off[-1]), dtype=np.uint8)
    out_off, o = np.empty(n, np.uint64), GUARD
    skip = rng.integers(1, 17, n)
    for r in range(n):
        o += int(skip[r])
        out_off[r] = o
        o += int(hl[r]) + len(packed[r])
    want = np.full(o + GUARD, FILL, np.uint8)
    for r in range(n):
        p = int(out_off[r])
        if hdr is not None:
            want[p: p + hl[r]] = hdr[int(hdr_off[r]): int(hdr_off[r + 1])]
        want[p + hl[r]: p + hl[r] + len(packed[r])] = packed[r]
    call = EncodeCall(name, alphabet, b"".join(parts), off, tlen, nsym, hdr, hdr_off, out_off, o + GUARD, want)
    for a in (off, tlen, nsym, out_off, want) + (() if hdr is None else (hdr, hdr_off)):
        a.setflags(write=False)
    return call


@functools.lru_cache(maxsize=2)
def encode_calls(kind):
    """One call a line width.  Every symbol count 0..SMALL_MAX and around the window drain in three shapes, texts cut at lengths around
    the 2 KiB step (wherever that falls in a line), a read of no byte, reads of line ends only, in a shuffled order; then a read with a
    partial last chunk and the call's last read, with 9, 16, more than 300 and 15 bytes behind the former in turn -- at 16 its last 16-byte
    load ends with the buffer.  Every third call without framing bytes.  Computed once, never changed."""
    calls = []
    for c, lw in enumerate(LINE_WIDTHS):
        rng = np.random.Generator(np.random.PCG64([20261019, c, sorted(ALPHABETS).index(kind)]))
        texts = [shaped(rng, kind, lw, n, s) for s in ("nl", "nonl", "blank") for n in tuple(range(SMALL_MAX + 1)) + SYMBOL_COUNTS]
        texts += [shaped(rng, kind, lw, T, "blank" if j & 1 else "nl")[:T] for j, T in enumerate(TEXT_LENGTHS)]
        texts += [b"", b"\n", b"\n\n\n"]
        if lw == ENCODE_LARGE_AT:
            texts.append(shaped(rng, kind, lw, LARGE, "nl"))
        texts = [texts[j] for j in rng.permutation(len(texts))]
        last_gap, last = [(4, 5), (6, 10), (7, 300), (6, 9)][c % 4]
        texts += [shaped(rng, kind, lw, 100, "nonl"), shaped(rng, kind, None, last, "nonl")]
        gaps = rng.integers(1, 49, len(texts))
        gaps[-1] = last_gap
        hdr_lens = None if c % 3 == 2 else [HDR_LENS[(r + c) % len(HDR_LENS)] for r in range(len(texts))]
        calls.append(make_call(f"{kind}-lw{lw}", kind, texts, rng, gaps, hdr_lens))
    return calls


@functools.lru_cache(maxsize=None)
def contract_call():
    """a few thousand short reads in lines of 60, no framing: the batch of the d_nsym check"""
    rng = np.random.Generator(np.random.PCG64(3001))
    texts = [shaped(rng, "bases", 60, int(n), "nl") for n in rng.integers(0, 400, 3001)]
    return make_call("contract", "bases", texts, rng)
