"""The case sets and references of _pack2_cases.py (tests/test_gpu_pack2.py runs them on the device): the references agree with the
oracle, and the case sets reach what they were built to reach -- every small length at every output address, texts that end at and
next to every 1 KiB step at every address, every way out of the decoder's three-ahead loop, every residue of the input offsets; every
text and record address, every framing length and the edge of the encoder's masked load.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _oracle as O
import _pack2_cases as P
from dextractor_amd import _lib as L
from dextractor_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_librarys():
    assert (P.LETTERS_LOWER, P.LETTERS_UPPER, P.LETTERS_ARROW, P.LETTERS_NUMBERS) == \
           (L.DX_LETTERS_LOWER, L.DX_LETTERS_UPPER, L.DX_LETTERS_ARROW, L.DX_LETTERS_NUMBERS)
    assert (P.ALPHA_BASES, P.ALPHA_ARROW) == (L.DX_ALPHA_BASES, L.DX_ALPHA_ARROW)
    hdr = open(os.path.join(ROOT, "include", "dexgpu.h")).read()
    assert int(re.search(r"\bDX_ALPHA_NUMBERS\s*=\s*(\d+)", hdr).group(1)) == P.ALPHA_NUMBERS


# ---- the references against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bases", "arrow", "numbers"])
def test_encode_reference_is_compress_read(kind):
    """(the oracle's Number_Read / Number_Arrow take any byte; numbers go to its Compress_Read as they are)"""
    rng = np.random.Generator(np.random.PCG64(11))
    lens = list(range(0, 40)) + [127, 128, 129, 130, 4095, 4096, 4097]
    n = 0
    for lw in P.LINE_WIDTHS:
        for shape in ("nl", "nonl", "blank"):
            for k in lens[(len(shape) + (lw or 0)) % 3::3]:
                text = P.shaped(rng, kind, lw, k, shape)
                seq = text.replace(b"\n", b"")
                assert len(seq) == k
                if kind == "numbers":
                    out = C.create_string_buffer((k + 3) // 4 + 4)
                    m = O.lib().ref_compress_read(k, seq, out)
                    want = out.raw[:m]
                else:
                    want = O.compress_read(seq, arrow=kind == "arrow")
                assert P.encode_ref(text, P.ALPHABETS[kind]).tobytes() == want, (lw, shape, k)
                n += 1
    assert n >= 300
    any_byte = P._any_byte(rng, 100000)
    assert set(any_byte.tolist()) == set(range(256)) - {10}
    assert (P.symbols_of(any_byte.tobytes(), P.ALPHA_NUMBERS) == any_byte & 3).all()
    assert not P.symbols_of(bytes(range(128, 256)), P.ALPHA_BASES).any()           # bytes >= 128: 0
    assert (P.symbols_of(bytes(range(128, 256)), P.ALPHA_ARROW) == 3).all()


@pytest.mark.parametrize("kind", ["fasta", "arrow"])
def test_decode_reference_is_undexta_and_undexar(kind):
    """An image made by the oracle's dexta / dexar, written back by its undexta / undexar at every width of the grid: each record is its
    header line and then the decode reference of its symbols"""
    rng = np.random.Generator(np.random.PCG64(12))
    lens = np.concatenate([np.arange(0, 20), rng.integers(20, 131, 8), [1007, 1008, 1009, 1023, 1024, 1025, 2049, 5000]]).astype(np.uint32)
    c = synth.make_seqfile(kind, len(lens), seed=5, lens=lens, width=70)
    img = (O.dexar if kind == "arrow" else O.dexta)(c.text)
    off, tl = c.off.astype(np.int64), c.tlen.astype(np.int64)
    starts = np.concatenate([[0], (off + tl)[:-1]])
    heads = [c.text[s: o] for s, o in zip(starts, off)]
    table = P.NUMBER_ARROW if kind == "arrow" else P.NUMBER_READ
    syms = [np.frombuffer(c.text[o: o + t].replace(b"\n", b"").translate(table), np.uint8) for o, t in zip(off, tl)]
    assert [len(s) for s in syms] == lens.tolist() and all(h[:1] == b">" and h[-1:] == b"\n" for h in heads)
    reads = 0
    for w in P.WIDTHS:
        if kind == "arrow":
            runs = [(P.LETTERS_ARROW, O.undexar(img, width=w))]
        else:
            runs = [(P.LETTERS_LOWER, O.undexta(img, upper=False, width=w)), (P.LETTERS_UPPER, O.undexta(img, upper=True, width=w))]
        for letters, got in runs:
            want = b"".join(h + P.decode_ref(s, letters, w).tobytes() for h, s in zip(heads, syms))
            assert got == want, (w, letters)
            reads += len(syms)
    assert reads >= 300
    assert P.decode_ref(np.arange(7) & 3, P.LETTERS_NUMBERS, 3).tolist() == [0, 1, 2, 10, 3, 0, 1, 10, 2, 10]
    assert len(P.decode_ref([], P.LETTERS_LOWER, 5)) == 0


def test_pack_reference_by_hand():
    assert P.pack_ref([]).tolist() == []
    assert P.pack_ref([3]).tolist() == [0xc0] and P.pack_ref([1, 2, 3, 0, 2]).tolist() == [0x6c, 0x80]
    assert P.encode_ref(b"\nAC\n\ngT\nn", P.ALPHA_BASES).tolist() == [0x1b, 0x00]
    assert P.encode_ref(b"12\n3G4", P.ALPHA_ARROW).tolist() == [0x1a, 0xc0]


# ---- the decode grid ---------------------------------------------------------------------------------------------------------------

def test_decode_calls():
    params = P.decode_params()
    assert [w for w, _ in params if w not in P.ALL_LETTER_WIDTHS] == [w for w in P.WIDTHS if w not in P.ALL_LETTER_WIDTHS]
    for w in P.ALL_LETTER_WIDTHS:
        assert [s for v, s in params if v == w] == P.ALL_LETTERS
    assert {s for w, s in params if w not in P.ALL_LETTER_WIDTHS} == set(P.ALL_LETTERS)
    assert sum(w >= 16 for w in P.WIDTHS) == 18 and len(P.WIDTHS) == 23


def shortest_text(width, least):
    """by search: the shortest text of at least `least` bytes that `width` allows"""
    L = max(0, least * width // (width + 1) - 2)
    while P.text_len(L, width) < least:
        L += 1
    return L


@pytest.mark.parametrize("width", P.WIDTHS)
def test_decode_case_covers_what_it_names(width):
    c = P.decode_case(width)
    n = len(c.nsym)
    T = np.array([P.text_len(int(x), width) for x in c.nsym], np.int64)
    out_off, in_off, clen = c.out_off.astype(np.int64), c.in_off.astype(np.int64), (c.nsym.astype(np.int64) + 3) >> 2
    assert ((out_off & 15) == c.adj).all()
    # (a) every length at every address
    small = {(c.key[r], int(c.adj[r])) for r in range(n) if c.part[r] == "a"}
    assert small == {(L, a) for L in range(131) for a in range(16)} and all(int(c.nsym[r]) == c.key[r] for r in range(n) if c.part[r] == "a")
    # (b) T + adj is the least value >= k 1024 + d the width allows, for every k, d and address
    long_ = {(c.key[r], int(c.adj[r])): r for r in range(n) if c.part[r] == "b"}
    assert set(long_) == {((k, d), a) for k in range(1, 11) for d in (-1, 0, 1, 16) for a in range(16)}
    exact = 0
    for ((k, d), a), r in long_.items():
        target = k * 1024 + d
        assert int(c.nsym[r]) == shortest_text(width, target - a), (k, d, a)
        assert 0 <= T[r] + a - target <= 1 and (T[r] + a == target or (target - a) % (width + 1) == 1), (k, d, a)
        exact += int(T[r] + a == target)
    print(f"width {width}: {exact} of {len(long_)} long reads end exactly at k 1024 + d")
    # (c)
    assert [int(c.nsym[r]) for r in range(n) if c.part[r] == "c"] == ([70000] if width in (1, 80, 100000) else [])
    assert n == 16 * 131 + 640 + (width in (1, 80, 100000))
    # layout: the reads' bytes disjoint and in order, every residue of the input offset, a byte or more between two texts
    assert in_off[0] == 1 and (in_off[1:] >= in_off[:-1] + clen[:-1]).all() and in_off[-1] + clen[-1] + P.GUARD == c.in_bytes
    assert (in_off[1:] > in_off[:-1] + clen[:-1]).any()
    assert {int(x) & 7 for x in in_off[c.nsym >= 32]} == set(range(8))
    assert out_off[0] > P.GUARD and (out_off[1:] > out_off[:-1] + T[:-1]).all() and out_off[-1] + T[-1] + P.GUARD == c.out_bytes
    # the packed image holds the reads' symbols; pad bits and the bytes between are not all zero
    for r in list(range(0, n, 97)) + [n - 1]:
        o, k = int(in_off[r]), int(c.nsym[r])
        s = c.sym[int(c.sym_off[r]): int(c.sym_off[r + 1])]
        got = (c.packed[o + (np.arange(k) >> 2)] >> (6 - 2 * (np.arange(k) & 3))) & 3
        assert (got == s).all() and (c.data[o: o + int(clen[r])] == P.pack_ref(s)).all()
    tails = [int(c.packed[int(o + k - 1)]) & ((1 << (2 * (-int(L_) % 4))) - 1) for o, k, L_ in zip(in_off, clen, c.nsym) if L_ & 3]
    assert len(set(tails)) > 8 and (c.packed != c.data).sum() > 100
    # the whole-buffer reference is the per-read one
    letters = P.letters_at(width)
    want = P.decode_want(c, letters)
    for r in list(range(0, n, 53)) + [n - 1]:
        s = c.sym[int(c.sym_off[r]): int(c.sym_off[r + 1])]
        assert (want[out_off[r]: out_off[r] + T[r]] == P.decode_ref(s, letters, width)).all()
        assert want[out_off[r] - 1] == P.FILL and want[out_off[r] + T[r]] == P.FILL
    assert (want == P.FILL).sum() == c.out_bytes - T.sum()
    pw = P.packed_want(c)
    assert (pw != P.FILL).sum() <= clen.sum() and (pw[int(in_off[-1]): int(in_off[-1] + clen[-1])] == c.data[int(in_off[-1]): int(in_off[-1] + clen[-1])]).all()


@pytest.mark.parametrize("width", [w for w in P.WIDTHS if w >= 16])
def test_long_reads_leave_the_three_ahead_loop_every_way(width):
    """By the model of the loop's entry and exit in _pack2_cases.loop_turns: texts that never enter it, and 0 to 6 turns taken -- 0, 1, 2
    leave from the lead-in turns through slots 0, 1, 2; 3, 4, 5, 6 from the steady turns through slots 3, 0, 1, 2 -- each of them at an
    aligned and at an unaligned output address"""
    c = P.decode_case(width)
    turns = {}
    for r in range(len(c.nsym)):
        if c.part[r] == "b":
            turns.setdefault(P.loop_turns(int(c.nsym[r]), width, int(c.adj[r])), set()).add(int(c.adj[r]))
    print(f"width {width}: turns taken -> addresses mod 16:", {k: len(v) for k, v in sorted(turns.items(), key=str)})
    assert set(turns) >= {None, 0, 1, 2, 3, 4, 5, 6}
    assert all(0 in turns[j] and len(turns[j]) > 1 for j in range(7))
    assert all(P.loop_turns(L_, width, a) is None for L_ in range(131) for a in (0, 15))
    assert all(P.loop_turns(70000, w, 9) is None for w in (1, 15))


# ---- the encode grid ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(P.ALPHABETS))
def test_encode_calls_cover_what_they_name(kind):
    calls = P.encode_calls(kind)
    assert len(calls) == len(P.LINE_WIDTHS) == 12
    hdr_lens, behind, last_tlen, values = set(), set(), set(), set()
    for c, lw in zip(calls, P.LINE_WIDTHS):
        n = len(c.off)
        off, tlen, out_off = c.off.astype(np.int64), c.tlen.astype(np.int64), c.out_off.astype(np.int64)
        texts = [c.text[o: o + t] for o, t in zip(off, tlen)]
        assert (off[1:] > off[:-1] + tlen[:-1]).all() and off[-1] + tlen[-1] == len(c.text)    # filler between, none behind the last
        assert any(b"\n" in c.text[o + t: p] for o, t, p in zip(off[:-1], tlen[:-1], off[1:]))
        assert {int(x) & 15 for x in off} == set(range(16)) and {int(x) & 15 for x in out_off} == set(range(16)), c.name
        assert [len(t) - t.count(b"\n") for t in texts] == c.nsym.tolist()
        counts = set(c.nsym.tolist())
        assert set(range(131)) | set(P.SYMBOL_COUNTS) <= counts and set(P.TEXT_LENGTHS) <= set(tlen.tolist()), c.name
        assert (70000 in counts) == (lw == 80)
        assert b"" in texts and b"\n" in texts and b"\n\n\n" in texts
        long_ = [t for t in texts if len(t) > 40]
        assert any(t[-1:] != b"\n" for t in long_) and any(t[-1:] == b"\n" for t in long_)
        assert any(t[:1] == b"\n" for t in long_) and any(b"\n\n" in t[1:] for t in long_)
        if lw is None:
            assert any(t.count(b"\n") == 1 and len(t) > 12000 for t in texts)
        else:
            assert max(len(ln) for t in texts[:-1] for ln in t.split(b"\n")) == lw      # (the last read is one line)
        # records: disjoint, a FILL byte or more between two and GUARD around all
        hl = np.diff(c.hdr_off.astype(np.int64)) if c.hdr is not None else np.zeros(n, np.int64)
        size = hl + ((c.nsym.astype(np.int64) + 3) >> 2)
        assert out_off[0] > P.GUARD and (out_off[1:] > out_off[:-1] + size[:-1]).all() and out_off[-1] + size[-1] + P.GUARD == c.out_bytes
        assert (c.want == P.FILL).sum() >= c.out_bytes - size.sum()
        r = n // 2
        p = int(out_off[r] + hl[r])
        assert (c.want[p: p + int(size[r] - hl[r])] == P.encode_ref(texts[r], c.alphabet)).all() and c.want[int(out_off[r]) - 1] == P.FILL
        if c.hdr is not None:
            hdr_lens |= set(hl.tolist())
            assert (c.want[int(out_off[r]): p] == c.hdr[int(c.hdr_off[r]): int(c.hdr_off[r + 1])]).all()
        behind.add(int(len(c.text) - off[-2] - tlen[-2]))
        last_tlen.add(int(tlen[-1]))
        assert tlen[-2] % 16 and tlen[-2] >= 100
        values |= set(np.concatenate([np.frombuffer(t, np.uint8) for t in texts]).tolist())
    assert sum(c.hdr is None for c in calls) == 4 and hdr_lens == set(P.HDR_LENS)
    # the edge of the masked load (a read takes it when 16 bytes or more follow its end in the buffer): 15 and 16 behind the last but one
    assert {9, 15, 16} <= behind and max(behind) > 300 and {5, 9, 10} <= last_tlen and max(last_tlen) >= 300
    if kind == "numbers":
        assert values == {0, 1, 2, 3, 10}
    else:
        assert values == set(range(256))


def test_contract_call():
    c = P.contract_call()
    assert len(c.off) == 3001 and c.hdr is None and int(c.nsym[1500]) > 0
