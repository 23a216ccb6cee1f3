"""What dx_code_kmer_screen, dx_file_screen and dx_screen_select are to compute, stated in numpy: per unit the codes of its windows
(tests/_kmers_wide.py's unit_codes), np.isin against the set, a boolean array over the unit's symbols for the union of the hit windows,
and first / last read off the hit positions; for the file level the same over the TEXT the oracle prints for the image.  And the packed
buffer the kernel's tests build: around a unit everything is the foreign symbol T, the pad bits too (the Buffer of
tests/test_gpu_kmer_codes.py).  The reference of tests/test_gpu_kmer_set.py, test_gpu_kmer_screen.py and test_gpu_screen_file.py;
tests/test_screen_host.py holds it against Python string slices.  Nothing here calls the library."""
import numpy as np

import _find as F
import _kmers_wide as W

SCREEN = np.dtype([("hits", "<u4"), ("covered", "<u4"), ("first", "<u4"), ("last", "<u4")])          # dx_screen
NONE = 0xFFFFFFFF
T = 3                 # the foreign symbol
U = np.uint64


class Buffer:
    """a packed buffer that grows unit by unit; around a unit everything is T, the pad bits too"""
    def __init__(self):
        self.sym, self.boff, self.beg, self.ln, self.n = [], [], [], [], 0       # n: symbols so far (4 a byte)
        self.units = []

    def add(self, codes, phase=None, beg=0, guard=2, tail=2):
        """the unit's symbols; phase: (byte offset of its read) mod 16, beg: the symbols of its read in front of it"""
        at = self.n // 4 + guard
        if phase is not None:
            at += (phase - at) % 16
        front = 4 * (at - self.n // 4) + beg
        codes = np.asarray(codes, np.uint8)
        end = self.n + front + len(codes)
        self.sym += [np.full(front, T, np.uint8), codes, np.full((-end) % 4 + 4 * tail, T, np.uint8)]
        self.boff.append(at); self.beg.append(beg); self.ln.append(len(codes)); self.units.append(codes)
        self.n = end + (-end) % 4 + 4 * tail
        return self

    def packed(self):
        return F.pack(np.concatenate(self.sym), pad=0xff) if self.sym else b""


def unit_screen(s, k, canonical, codes):
    """one unit's entry against the set `codes` (a uint64 array): (hits, covered, first, last)"""
    c = W.unit_codes(s, k, canonical)
    hit = np.isin(c, np.asarray(codes, U))
    pos = np.flatnonzero(hit)
    cov = np.zeros(len(s), bool)
    for p in pos:
        cov[p:p + k] = True
    return (len(pos), int(cov.sum()), int(pos[0]) if len(pos) else NONE, int(pos[-1]) if len(pos) else NONE)


def screen(units, k, canonical, codes):
    """the entries of all units (None: a unit that does not lie in its buffer) and the totals: windows, hits, covered, units with a hit"""
    out, tot = np.zeros(len(units), SCREEN), np.zeros(4, U)
    for j, s in enumerate(units):
        e = (0, 0, NONE, NONE) if s is None else unit_screen(s, k, canonical, codes)
        out[j] = e
        if s is not None:
            tot += np.array([max(0, len(s) - k + 1), e[0], e[1], 1 if e[0] else 0], U)
    return out, tot


def packed_screen(packed, boff, beg, ln, k, canonical, codes, in_bytes=None):
    """dx_code_kmer_screen on host arrays (beg None: all 0): (entries, totals, the smallest bad unit or None)"""
    in_bytes = len(packed) if in_bytes is None else in_bytes
    units, bad = [], None
    for j in range(len(ln)):
        at, b, n = int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])
        ok = at <= in_bytes and n < 2 ** 31 and (n == 0 or (b + n - 1) // 4 < in_bytes - at)
        if not ok and bad is None:
            bad = j
        units.append(F.symbols(packed, at, b, n) if ok else None)
    return screen(units, k, canonical, codes) + (bad,)


def distinct(units, k, canonical=False, min_count=1):
    """the codes that the units' windows have min_count times at least, ascending"""
    seen, cnt, _ = W.sparse(units, k, canonical)
    return seen[cnt >= U(min_count)]


def file_screen(kind, text, k, canonical, codes):
    """dx_file_screen's answer, as Context.screen returns it, from the TEXT: (report, rec, rec_len)"""
    rs = F.reads(kind, text)
    rec, tot = screen(rs, k, canonical, codes)
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": int(tot[0]), "hits": int(tot[1]),
           "covered": int(tot[2]), "records_hit": int(tot[3]), "k": k}
    return rep, rec, np.array([len(r) for r in rs], np.uint32)


def select(rec, rec_len, min_hits=1, min_permille=0, drop=False):
    """dx_screen_select as a plain loop over Python integers"""
    out = []
    for i in range(len(rec)):
        match = int(rec[i]["hits"]) >= max(int(min_hits), 1) and int(rec[i]["covered"]) * 1000 >= int(min_permille) * int(rec_len[i])
        if match != bool(drop):
            out.append(i)
    return out
