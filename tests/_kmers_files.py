"""What dx_code_kmer_bins, dx_code_kmer_codes_range, dx_kmer_range_plan and dx_files_kmers_wide / dx_files_kmer_set are to compute,
stated on top of tests/_kmers_wide.py: the bins are np.bincount of the codes' top bits, the range filter is a boolean mask, the plan
is a Python loop, and the file level is W.file_kmers_wide over the CONCATENATED texts of the images -- a window never spans two
records, so concatenating is exact.  The reference of the three test_gpu_kmer*bins / range / files files;
tests/test_kmers_files_host.py holds the bins against a dict over string slices.  Nothing here calls the library."""
import numpy as np

import _find as F
import _kmers_wide as W

U = np.uint64
BITS_MAX = 12


def bits_for(k, bits=BITS_MAX):
    """`bits` clamped by the 2 k bits a code has"""
    return min(bits, 2 * k)


def bin_of(codes, k, bits):
    return (np.asarray(codes, U) >> U(2 * k - bits)).astype(np.int64)


def bins(codes, k, bits):
    """dx_code_kmer_bins' counts for an array of codes"""
    return np.bincount(bin_of(codes, k, bits), minlength=1 << bits).astype(U)


def in_range(codes, k, bits, lo, hi):
    """dx_code_kmer_codes_range's filter, as a mask"""
    b = bin_of(codes, k, bits)
    return (b >= lo) & (b < hi)


class BinTooLarge(Exception):
    def __init__(self, b, windows):
        super().__init__(f"bin {b} holds {windows} windows")
        self.bin, self.windows = b, windows


def plan(bins_, room):
    """dx_kmer_range_plan: the cuts [0, ..., len(bins)] -- a range takes bins while its sum stays <= room, an empty bin costs nothing;
    room 0: one range"""
    cut, total = [0], 0
    for b, w in enumerate(int(v) for v in bins_):
        if room and w > room:
            raise BinTooLarge(b, w)
        if room and total + w > room:
            cut.append(b)
            total = 0
        total += w
    return cut + [len(bins_)]


# ---- the units that test_gpu_kmer_bins.py and test_gpu_kmer_codes_range.py share -------------------------------------------------------
T = 3                 # the foreign symbol: everything around a unit is Ts, the pad bits too
CHUNK = 64            # KC_CHUNK: positions of a 16-byte chunk; up to 4 chunks go by a lane, up to 16 by 16 lanes, the rest by the wave
KS = [(1, False), (5, False), (6, False), (7, False), (7, True), (14, False), (21, False), (21, True), (31, False), (32, False), (32, True)]


class Buffer:
    """a packed buffer that grows unit by unit; around a unit everything is T"""
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

    def unit(self, boff, beg, ln):
        """a unit over what is there already: it overlaps or repeats others"""
        self.boff.append(boff); self.beg.append(beg); self.ln.append(ln)
        return self

    def packed(self):
        return F.pack(np.concatenate(self.sym), pad=0xff)


def seam_lengths(k):
    """0, around k, and the seams of the three routes: a chunk, 4 chunks, 16 chunks, one step of the wave (4096 positions), two, three"""
    return [0, k - 1, k, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8200, 12300]


def shapes(k, seed):
    """(packed, boff, beg, ln, bad): the seam lengths; a short unit at every byte offset mod 16 and every phase; units that overlap and
    repeat; a unit of 5000 equal symbols; ONE unit that does not lie inside the buffer, index `bad`, in the middle; and at the end a
    unit that ends in the buffer's last byte"""
    rng, b, j = np.random.default_rng(seed), Buffer(), 0
    for n in seam_lengths(k):
        b.add(rng.integers(0, 4, n), phase=(5 * j) % 16, beg=j % 4 + 4 * (j % 3))
        j += 1
    long_one = len(b.ln) - 1                                       # the 12300
    for phase in range(16):
        for beg in range(4):
            b.add(rng.integers(0, 4, 40 + k + 3 * phase + beg), phase=phase, beg=beg)
    assert {(o % 16, g % 4) for o, g in zip(b.boff, b.beg)} == {(o, g) for o in range(16) for g in range(4)}
    b.unit(b.boff[long_one], b.beg[long_one], b.ln[long_one])      # the long one again
    b.unit(b.boff[long_one] + 100, 3, 5000)                        # ... and a stretch inside it
    b.unit(b.boff[long_one] + 101, 1, 300)
    b.unit(b.boff[3], b.beg[3] + 1, 62)
    bad = len(b.ln)
    b.unit(0, 0, 100)                                              # (its place is set below, when the buffer's size is known)
    b.add(np.full(5000, 2, np.uint8), phase=9, beg=2)              # a homopolymer
    b.add(rng.integers(0, 4, 1026), phase=11, beg=2, tail=0)       # ends in the last byte, no pad bits
    packed = b.packed()
    assert (b.beg[-1] + b.ln[-1]) % 4 == 0 and b.boff[-1] + (b.beg[-1] + b.ln[-1]) // 4 == len(packed)
    b.boff[bad] = len(packed) - 10
    return packed, b.boff, b.beg, b.ln, bad


def text_codes(kind, texts, k, canonical=False):
    """every window's code of the records of the texts, one text behind the other"""
    return W.all_codes([r for t in texts for r in F.reads(kind, t)], k, canonical)


def files_kmers_wide(kind, texts, k, canonical=False, nspec=256, min_count=0, max_list=0):
    """dx_files_kmers_wide's answer without "passes" and "files", as Context.kmers_wide_files returns it, from the TEXTS"""
    return W.file_kmers_wide(kind, b"".join(texts), k, canonical, nspec, min_count, max_list)


def files_of(kind, texts, k):
    """the report's "files": records, symbols and windows an image"""
    out = []
    for t in texts:
        rs = F.reads(kind, t)
        out.append({"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": int(sum(max(0, len(r) - k + 1) for r in rs))})
    return out
