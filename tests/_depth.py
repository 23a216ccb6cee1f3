"""What the counted sets, dx_code_kmer_depths, dx_depth_stats, dx_file_depth and dx_depth_select are to compute, stated in numpy: the
codes of a unit's windows (tests/_kmers_wide.py's unit_codes), counted with np.unique(..., return_counts=True), looked up with
np.searchsorted, clamped; a stretch's statistics from np.sort; for the file level the same over the TEXT the oracle prints for the
image.  The packed buffers are tests/_screen.py's Buffer.  The reference of the four test_gpu_*depth* / kmer_set_counted files;
tests/test_depth_host.py holds it against Python string slices and a dict of counts.  Nothing here calls the library."""
import numpy as np

import _find as F
import _kmers_wide as W
from _screen import Buffer  # noqa: F401                           (the packed buffers of the kernel's tests)

DEPTH = np.dtype([("windows", "<u4"), ("hits", "<u4"), ("sum", "<u8"), ("min", "<u2"), ("q1", "<u2"), ("median", "<u2"),
                  ("q3", "<u2"), ("max", "<u2"), ("reserved", "<u2", (3,))])                                      # dx_depth
U = np.uint64
COUNT_MAX = 2 ** 32 - 1                                              # where a set's counts saturate
DEPTH_MAX = 65535                                                    # ... and a profile's depths
STATS = ["min", "q1", "median", "q3", "max"]                         # DX_DEPTH_*


def counted(units, k, canonical=False, min_count=1):
    """the counted set of the units' windows: (codes ascending, their counts as uint32, saturated) of the codes seen min_count times"""
    seen, cnt, _ = W.sparse(units, k, canonical)
    keep = cnt >= U(min_count)
    return seen[keep], np.minimum(cnt[keep], U(COUNT_MAX)).astype(np.uint32)


def from_sorted(sorted_codes, min_count=1):
    """dx_kmer_set_from_sorted_counted on a host array: (codes, counts)"""
    seen, cnt = np.unique(np.asarray(sorted_codes, U), return_counts=True)
    keep = cnt >= min_count
    return seen[keep].astype(U), np.minimum(cnt[keep], COUNT_MAX).astype(np.uint32)


def from_kmers(pairs, k, canonical=False):
    """dx_kmer_set_from_kmers of (code, count) pairs: folded, the zero counts dropped, equal codes added with Python integers and
    saturated: (codes, counts)"""
    code = np.array([p[0] for p in pairs], U)
    if canonical and len(code):
        code = np.minimum(code, W.rc(code, k))
    total = {}
    for c, (_, n) in zip(code.tolist(), pairs):
        if int(n):
            total[c] = min(total.get(c, 0) + int(n), COUNT_MAX)
    keys = sorted(total)
    return np.array(keys, U), np.array([total[c] for c in keys], np.uint32)


def unit_depths(s, k, canonical, codes, counts=None):
    """one unit's depths as uint16: min(count, 65535) of every window's code, 0 where the set (codes ascending) does not hold it;
    counts None: an uncounted set, 1 for every code it holds"""
    c = W.unit_codes(s, k, canonical)
    codes = np.asarray(codes, U)
    if len(codes) == 0 or len(c) == 0:
        return np.zeros(len(c), np.uint16)
    at = np.minimum(np.searchsorted(codes, c), len(codes) - 1)
    hit = codes[at] == c
    cnt = np.ones(len(codes), np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    return np.where(hit, np.minimum(cnt[at], DEPTH_MAX), 0).astype(np.uint16)


def profile(units, k, canonical, codes, counts=None):
    """the units' depths one behind the other and their places: (uint16 array, off: uint64 [n + 1]); a unit None has no window"""
    parts = [np.zeros(0, np.uint16) if s is None else unit_depths(s, k, canonical, codes, counts) for s in units]
    off = np.zeros(len(units) + 1, U)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.int64) if units else []
    return np.concatenate(parts + [np.zeros(0, np.uint16)]), off


def packed_profile(packed, boff, beg, ln, k, canonical, codes, counts=None, in_bytes=None):
    """dx_code_kmer_depths on host arrays (beg None: all 0): (the profile, off, the smallest bad unit or None)"""
    in_bytes = len(packed) if in_bytes is None else in_bytes
    units, bad = [], None
    for j in range(len(ln)):
        at, b, n = int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])
        ok = at <= in_bytes and n < 2 ** 31 and (n == 0 or (b + n - 1) // 4 < in_bytes - at)
        if not ok and bad is None:
            bad = j
        units.append(F.symbols(packed, at, b, n) if ok else None)
    return profile(units, k, canonical, codes, counts) + (bad,)


def entry(v):
    """a stretch's dx_depth as a tuple: windows, hits, sum, min, q1, median, q3, max"""
    v = np.asarray(v, np.uint16)
    w = len(v)
    if w == 0:
        return (0, 0, 0, 0, 0, 0, 0, 0)
    s = np.sort(v)
    return (w, int(np.count_nonzero(v)), int(v.astype(U).sum()), int(s[0]), int(s[(w - 1) // 4]), int(s[(2 * (w - 1)) // 4]),
            int(s[(3 * (w - 1)) // 4]), int(s[-1]))


def stats(depth, off):
    """dx_depth_stats on host arrays: (a DEPTH array, the totals: windows, hits, sum, units with a hit)"""
    n = len(off) - 1
    out, tot = np.zeros(n, DEPTH), [0, 0, 0, 0]
    for j in range(n):
        e = entry(depth[int(off[j]):int(off[j + 1])])
        for f, x in zip(DEPTH.names[:8], e):
            out[j][f] = x
        tot = [tot[0] + e[0], tot[1] + e[1], tot[2] + e[2], tot[3] + (1 if e[1] else 0)]
    return out, tot


def file_depth(kind, text, k, canonical, codes, counts=None):
    """dx_file_depth's answer, as Context.depth(profile=True) returns it, from the TEXT: (report, rec, rec_len, profile, rec_off)"""
    rs = F.reads(kind, text)
    prof, off = profile(rs, k, canonical, codes, counts)
    rec, tot = stats(prof, off)
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": tot[0], "hits": tot[1], "sum": tot[2],
           "records_hit": tot[3], "k": k}
    return rep, rec, np.array([len(r) for r in rs], np.uint32), prof, off


def select(rec, stat="median", lo=0, hi=65535, min_windows=1, drop=False):
    """dx_depth_select as a plain loop over Python integers"""
    out = []
    for i in range(len(rec)):
        match = int(rec[i]["windows"]) >= max(int(min_windows), 1) and int(lo) <= int(rec[i][stat]) <= int(hi)
        if match != bool(drop):
            out.append(i)
    return out


def same_entries(got, want):
    """every field of every entry, the reserved words too"""
    assert got.dtype == DEPTH and len(got) == len(want)
    for f in DEPTH.names:
        diff = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert len(diff) == 0, (f, [(int(j), got[j].tolist(), want[j].tolist()) for j in diff[:5]])
