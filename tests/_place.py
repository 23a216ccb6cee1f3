"""What dx_code_kmer_index, dx_code_kmer_seeds, dx_seeds_place, dx_file_place and dx_place_select are to compute, stated in numpy:
the codes of a target's windows (tests/_kmers_wide.py's codes and rc), np.lexsort by (code, position) for the index; np.searchsorted
and np.repeat for a unit's seeds; np.unique over (strand, bin) for the vote; for the file level the same over the TEXT the oracle
prints for the image.  The packed buffers are tests/_screen.py's Buffer, the texts' records tests/_find.py's reads.  The reference of
the four test_gpu_*place* / kmer_index / kmer_seeds files; tests/test_place_host.py holds it against Python string slices, a dict of
positions and a loop over bins.  Nothing here calls the library."""
import numpy as np

import _find as F
import _kmers_wide as W
from _screen import Buffer  # noqa: F401                           (the packed buffers of the kernel's tests)

SEED = np.dtype([("unit", "<u4"), ("pos", "<u4"), ("gpos", "<u4"), ("strand", "<u4")])                             # dx_seed
PLACE = np.dtype([("seeds", "<u4"), ("votes", "<u4"), ("strand", "<u4"), ("diag", "<u4"), ("rbeg", "<u4"), ("rend", "<u4"),
                  ("gbeg", "<u4"), ("gend", "<u4")])                                                                # dx_place
U = np.uint64
NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def windows(s, k, canonical):
    """a sequence's windows: (the codes kept, their flips as uint32)"""
    fwd = W.codes(s, k)
    if not canonical:
        return fwd, np.zeros(len(fwd), np.uint32)
    r = W.rc(fwd, k)
    return np.minimum(fwd, r), (r < fwd).astype(np.uint32)


class Index:
    """the index of `targets` (arrays of codes): codes ascending, counts, start (uint32, codes + 1), pos (uint32: g << 1 | flip,
    ascending in g inside a code), toff (uint64, targets + 1)"""

    def __init__(self, targets, k, canonical=False):
        self.k, self.canonical = k, canonical
        self.toff = np.zeros(len(targets) + 1, U)
        self.toff[1:] = np.cumsum([len(t) for t in targets], dtype=np.int64) if len(targets) else []
        code, word = [np.zeros(0, U)], [np.zeros(0, np.int64)]
        for t, s in enumerate(targets):
            c, f = windows(s, k, canonical)
            g = int(self.toff[t]) + np.arange(len(c), dtype=np.int64)
            code.append(c)
            word.append((g << 1) | f)
        code, word = np.concatenate(code), np.concatenate(word)
        order = np.lexsort((word, code))
        self.codes, cnt = np.unique(code, return_counts=True)
        self.counts = cnt.astype(np.uint32)
        self.start = np.zeros(len(self.codes) + 1, np.uint32)
        self.start[1:] = np.cumsum(cnt)
        self.pos = word[order].astype(np.uint32)
        self.windows = len(code)


def unit_seeds(j, s, x, max_occ):
    """unit j's seeds against the Index x as a SEED array in the order (pos, gpos), and its windows that give one at least"""
    c, f = windows(s, x.k, x.canonical)
    if len(c) == 0 or len(x.codes) == 0:
        return np.zeros(0, SEED), 0
    at = np.minimum(np.searchsorted(x.codes, c), len(x.codes) - 1)
    give = (x.codes[at] == c) & (x.counts[at].astype(np.int64) <= max_occ)
    p = np.flatnonzero(give)
    n = x.counts[at[p]].astype(np.int64)
    out = np.zeros(int(n.sum()), SEED)
    if len(out):
        first = np.repeat(np.cumsum(n) - n, n)                               # where each window's seeds begin in the unit's list
        r = np.repeat(x.start[at[p]].astype(np.int64), n) + (np.arange(len(out)) - first)
        out["unit"], out["pos"] = j, np.repeat(p, n)
        out["gpos"], out["strand"] = x.pos[r] >> 1, (x.pos[r] & 1) ^ np.repeat(f[p], n)
    return out, len(p)


def seeds(units, x, max_occ=1):
    """all units' seeds (None: a unit that does not lie in its buffer): (the list, off: uint64 [n + 1], totals: windows, windows
    with a seed, seeds, units with a seed)"""
    parts, tot = [], [0, 0, 0, 0]
    for j, s in enumerate(units):
        e, w = (np.zeros(0, SEED), 0) if s is None else unit_seeds(j, s, x, max_occ)
        parts.append(e)
        if s is not None:
            tot = [tot[0] + max(0, len(s) - x.k + 1), tot[1] + w, tot[2] + len(e), tot[3] + (1 if len(e) else 0)]
    off = np.zeros(len(units) + 1, U)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.int64) if units else []
    return np.concatenate(parts + [np.zeros(0, SEED)]), off, tot


def packed_units(packed, boff, beg, ln, in_bytes=None):
    """the units of host arrays as dx_code_kmer_codes takes them (beg None: all 0): (units, None where one does not lie inside the
    in_bytes; the smallest such index or None)"""
    in_bytes = len(packed) if in_bytes is None else in_bytes
    units, bad = [], None
    for j in range(len(ln)):
        at, b, n = int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])
        ok = at <= in_bytes and n < 2 ** 31 and (n == 0 or (b + n - 1) // 4 < in_bytes - at)
        if not ok and bad is None:
            bad = j
        units.append(F.symbols(packed, at, b, n) if ok else None)
    return units, bad


def diag(e):
    """the seeds' 32-bit diagonals as int64"""
    p, g = e["pos"].astype(np.int64), e["gpos"].astype(np.int64)
    return np.where(e["strand"] == 1, g + p, g - p + 2 ** 31) & M32


def unit_place(e, k, band_bits):
    """one unit's dx_place from its seeds e, as a tuple of 8"""
    if len(e) == 0:
        return (0, 0, 0, NONE, NONE, NONE, NONE, NONE)
    b = diag(e) >> band_bits
    last = (1 << (32 - band_bits)) - 1
    key = (e["strand"].astype(np.int64) << (32 - band_bits)) | b
    uniq, cnt = np.unique(key, return_counts=True)
    nxt = np.zeros(len(uniq), np.int64)
    if len(uniq) > 1:
        follows = (uniq[1:] == uniq[:-1] + 1) & ((uniq[:-1] & last) != last)   # the run behind is (s, b + 1)
        nxt[:-1] = np.where(follows, cnt[1:], 0)
    votes = cnt + nxt
    best = int(np.argmax(votes))                                             # (the first of the largest: the smaller s, then the smaller b)
    s, bb = int(uniq[best] >> (32 - band_bits)), int(uniq[best] & last)
    voted = (e["strand"] == s) & ((b == bb) | ((b == bb + 1) & (bb != last)))
    v = e[voted]
    return (len(e), int(votes[best]), s, (bb << band_bits) & M32, int(v["pos"].min()), (int(v["pos"].max()) + k) & M32,
            int(v["gpos"].min()), (int(v["gpos"].max()) + k) & M32)


def place(lst, off, k, band_bits):
    """dx_seeds_place on host arrays: (a PLACE array, the totals: seeds, votes, units placed)"""
    n = len(off) - 1
    out, tot = np.zeros(n, PLACE), [0, 0, 0]
    for j in range(n):
        t = unit_place(lst[int(off[j]):int(off[j + 1])], k, band_bits)
        out[j] = t
        tot = [tot[0] + t[0], tot[1] + t[1], tot[2] + (1 if t[0] else 0)]
    return out, tot


def file_place(kind, text, x, max_occ=1, band_bits=8):
    """dx_file_place's answer, as Context.place returns it, from the TEXT: (report without groups, rec, rec_len)"""
    rs = F.reads(kind, text)
    lst, off, st = seeds(rs, x, max_occ)
    rec, pt = place(lst, off, x.k, band_bits)
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": st[0], "hits": st[1], "seeds": st[2], "votes": pt[1],
           "records_placed": pt[2], "k": x.k, "band_bits": band_bits}
    return rep, rec, np.array([len(r) for r in rs], np.uint32)


def where(rec, toff):
    """per record (target, tbeg, tend) by np.searchsorted over toff; NONE x 3 for a record that is not placed"""
    toff = np.asarray(toff, U).astype(np.int64)
    out = []
    for r in rec:
        if int(r["votes"]) == 0 or int(r["gbeg"]) >= int(toff[-1]):
            out.append((NONE, NONE, NONE))
            continue
        t = int(np.searchsorted(toff, int(r["gbeg"]), side="right")) - 1
        out.append((t, int(r["gbeg"]) - int(toff[t]), min(int(r["gend"]), int(toff[t + 1])) - int(toff[t])))
    return out


def select(rec, toff, target=None, lo=0, hi=M32, min_votes=1, strands=3, drop=False):
    """dx_place_select as a plain loop over Python integers"""
    toff = [int(x) for x in toff]
    out = []
    for i in range(len(rec)):
        votes, s, gb, ge = (int(rec[i][f]) for f in ("votes", "strand", "gbeg", "gend"))
        match = False
        if votes >= max(int(min_votes), 1) and s in (0, 1) and (strands >> s) & 1 and gb < toff[-1]:
            t = max(j for j in range(len(toff) - 1) if toff[j] <= gb)
            if target is None or t == target:
                match = gb - toff[t] < hi and lo < min(ge, toff[t + 1]) - toff[t]
        if match != bool(drop):
            out.append(i)
    return out


def planted(targets, n, length, rate, seed):
    """n reads cut from the targets (arrays of codes), alternately of either strand, every symbol replaced by another with
    probability `rate` (substitutions only): (reads, truth: (target, position in it, strand) a read)"""
    rng = np.random.default_rng(seed)
    reads, truth = [], []
    for i in range(n):
        t = int(rng.integers(0, len(targets)))
        while len(targets[t]) < length:
            t = (t + 1) % len(targets)
        p = int(rng.integers(0, len(targets[t]) - length + 1))
        s = np.array(targets[t][p:p + length], np.uint8)
        hit = rng.random(length) < rate
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        if i % 2:
            s = (3 - s)[::-1]
        reads.append(s)
        truth.append((t, p, i % 2))
    return reads, truth


def same_entries(got, want, dtype=PLACE):
    """every field of every entry"""
    assert got.dtype == dtype and len(got) == len(want), (got.dtype, len(got), len(want))
    for f in dtype.names:
        diff = np.flatnonzero(got[f] != want[f])
        assert len(diff) == 0, (f, [(int(j), got[j].tolist(), want[j].tolist()) for j in diff[:5]])
