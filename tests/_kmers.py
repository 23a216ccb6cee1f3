"""What dx_code_kmers, dx_kmer_spectrum, dx_kmer_list and dx_file_kmers are to compute, stated in numpy: the sliding codes of arrays of
symbols, counted with bincount; and for the file level the same over the TEXT -- the letters of each record as the oracle's
undexta -U / undexar prints them (tests/_find.py's text_of and reads).  The reference of tests/test_gpu_code_kmers.py and
tests/test_gpu_kmers_file.py; tests/test_kmers_host.py holds it against a dict over string slices.  Nothing here calls the library."""
import numpy as np

import _find as F

KMER = np.dtype([("count", "<u8"), ("code", "<u4"), ("reserved", "<u4")])      # dx_kmer
DENSE = 10            # up to this k file_kmers counts with bincount into the whole table; beyond it keeps the cells in use (4^14 are 2 GiB)


def codes(s, k):
    """the codes of the windows of k symbols of the array of codes s, the first symbol on top: sum s[p + i] 4^(k - 1 - i)"""
    s = np.asarray(s, np.int64)
    if len(s) < k:
        return np.zeros(0, np.int64)
    w = np.lib.stride_tricks.sliding_window_view(s, k)
    return w @ (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))


def rc(code, k):
    """the code of the reverse complement: the symbols 3 - c in reverse order"""
    code = np.asarray(code, np.int64)
    out = np.zeros_like(code)
    for i in range(k):
        out = out * 4 + (3 - (code >> (2 * i)) % 4)               # (the lowest symbol first: it becomes the top one)
    return out


def table(units, k, canonical=False):
    """units: arrays of codes -> (the 4^k counts as uint64, the windows)"""
    t, windows = np.zeros(4 ** k, np.int64), 0
    for s in units:
        c = codes(s, k)
        if canonical:
            c = np.minimum(c, rc(c, k))
        t += np.bincount(c, minlength=4 ** k)
        windows += len(c)
    return t.astype(np.uint64), windows


def sparse(units, k, canonical=False):
    """the same without the table, for a k whose 4^k cells nobody wants on the host: (the codes seen, ascending; their counts; the windows)"""
    c = np.concatenate([codes(s, k) for s in units] + [np.zeros(0, np.int64)])
    if canonical:
        c = np.minimum(c, rc(c, k))
    seen, cnt = np.unique(c, return_counts=True)
    return seen.astype(np.uint32), cnt.astype(np.uint64), len(c)


def spectrum(t, nspec):
    """dx_kmer_spectrum's answer for a table: {"spectrum", "distinct", "max_count", "max_code"}"""
    t = np.asarray(t, np.uint64)
    seen = t[t > 0]
    spec = np.bincount(np.minimum(seen, np.uint64(nspec - 1)).astype(np.int64), minlength=nspec).astype(np.uint64)
    assert spec[0] == 0
    m = int(t.max()) if len(seen) else 0
    return {"spectrum": spec, "distinct": len(seen), "max_count": m, "max_code": int(np.flatnonzero(t == m)[0]) if m else 0}


def listing(t, min_count, cap):
    """dx_kmer_list's answer: (found, the first cap entries in ascending code order as a KMER array)"""
    t = np.asarray(t, np.uint64)
    at = np.flatnonzero(t >= np.uint64(min_count))
    out = np.zeros(min(len(at), cap), KMER)
    out["code"], out["count"] = at[:cap], t[at[:cap]]
    return len(at), out


def packed_table(packed, boff, beg, ln, k, canonical=False):
    """dx_code_kmers on host arrays (beg None: all 0)"""
    return table([F.symbols(packed, int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])) for j in range(len(ln))], k, canonical)


def letters_of(kind, code, k):
    return bytes((b"ACGT" if kind == "fasta" else b"1234")[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def file_kmers(kind, text, k, canonical=False, nspec=256, min_count=0, max_list=0):
    """dx_file_kmers' answer, as Context.kmers returns it, from the TEXT: (report, spectrum, list of (count, code, letters), table)"""
    rs = F.reads(kind, text)
    if k <= DENSE:
        t, windows = table(rs, k, canonical)
        sp = spectrum(t, nspec)
        found, lst = listing(t, min_count, max_list) if min_count else (0, np.zeros(0, KMER))
    else:                                                          # (the same figures from the cells in use: no table)
        t, (seen, cnt, windows) = None, sparse(rs, k, canonical)
        sp = spectrum(cnt, nspec)
        sp["max_code"] = int(seen[sp["max_code"]]) if len(seen) else 0
        keep = np.flatnonzero(cnt >= np.uint64(max(min_count, 1)))[:max_list if min_count else 0]
        lst = np.zeros(len(keep), KMER)
        lst["code"], lst["count"] = seen[keep], cnt[keep]
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": windows, "distinct": sp["distinct"],
           "max_count": sp["max_count"], "max_code": sp["max_code"], "k": k, "listed": len(lst)}
    return rep, sp["spectrum"], [(int(e["count"]), int(e["code"]), letters_of(kind, int(e["code"]), k)) for e in lst], t
