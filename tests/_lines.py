"""What the extract tests share: numpy's statement of dx_reads_unpack_lines, and the selections of dx_file_extract that dx_file_subset
has no use for.  Expected bytes never come from the code under test: they are this reference's, or `_subset.cut` of the oracle's text."""
import struct

import numpy as np

LETTERS = {0: b"acgt", 1: b"ACGT", 2: b"1234"}                       # DX_LETTERS_LOWER, _UPPER, _ARROW (DB.c:367-389)


def text_len(n, width):
    """bytes of n symbols in lines of `width`, a line end behind every line"""
    return n + (n + width - 1) // width


def unpack_lines_ref(buf, boff, beg, ln, width, letters):
    """numpy's statement of dx_reads_unpack_lines: per unit the bytes of symbols [beg, beg + len) of the packed read at buf[boff:] --
    taken as _subset.repack takes them: symbol i in bits 7 - 2 (i & 3), 6 - 2 (i & 3) of byte i >> 2 --, as letters, a line end behind
    every width-th one and behind the last (undexta.c:263-270)"""
    a = np.frombuffer(bytes(buf), np.uint8)
    tab = np.frombuffer(LETTERS[letters], np.uint8)
    out = []
    for o, b, n in zip(boff, beg, ln):
        o, b, n = int(o), int(b), int(n)
        by = a[o + (b >> 2): o + ((b + n + 3) >> 2)]
        sym = np.stack([(by >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[(b & 3): (b & 3) + n]
        text = np.full(text_len(n, width), 10, np.uint8)
        if n:
            k = np.arange(n)
            text[k + k // width] = tab[sym]
        out.append(text.tobytes())
    return out


def two_bit_reads(img, arrow=False):
    """where the packed reads of a .dexta / .dexar image in the native layout stand in it, and their symbols: (boff, rlen)"""
    key, plen = struct.unpack_from("<Hi", img, 0)
    assert key == 0x55aa
    at, boff, rlen = 6 + plen, [], []
    while at < len(img):
        while img[at] == 0xff:                             # the well delta: a 0xff for every whole 255, then a byte
            at += 1
        b, e = struct.unpack_from("<ii", img, at + 1)
        at += 1 + 8 + (8 if arrow else 4)                  # ... beg, end, and the quality value or the four channel SNRs
        boff.append(at)
        rlen.append(e - b)
        at += (e - b + 3) // 4
    assert at == len(img)
    return np.array(boff, np.uint64), np.array(rlen, np.uint32)


def bodies(text, lead=b">"):
    """a .fasta / .arrow text without its header lines, read by read"""
    out = []
    for ln in text.split(b"\n")[:-1]:
        if ln[:1] == lead:
            out.append(b"")
        else:
            out[-1] += ln + b"\n"
    return out


def whole(lens):
    return [(i, None, None) for i in range(len(lens))]


def with_a_final_empty_unit(units, lens):
    """... the selection the reference has no image for (`_subset.one_empty_each`): a text may end with a header line"""
    k = len(lens) // 2
    return list(units) + [(k, lens[k] // 2, lens[k] // 2)]


def shuffled_with_repeats(lens, seed):
    """records in any order, some of them several times, whole and cut"""
    rng = np.random.Generator(np.random.PCG64(seed))
    units = []
    for i in rng.integers(0, len(lens), 2 * len(lens) + 3):
        i = int(i)
        b = int(rng.integers(0, lens[i] + 1))
        units.append((i, 0, lens[i]) if rng.integers(0, 3) == 0 else (i, b, int(rng.integers(b, lens[i] + 1))))
    assert any(units[k][0] > units[k + 1][0] for k in range(len(units) - 1)) and len({u[0] for u in units}) < len(units)
    return units


def header_offsets(kind, text, n):
    """where the n units' header lines begin in a text, and the text's length behind them: n + 1 values"""
    lead = b"@" if kind == "quiva" else b">"
    lines = text.split(b"\n")[:-1]
    at, out = 0, []
    for k, ln in enumerate(lines):
        if (k % 6 == 0) if kind == "quiva" else ln[:1] == lead:
            assert ln[:1] == lead
            out.append(at)
        at += len(ln) + 1
    assert len(out) == n and at == len(text)
    return out + [at]
