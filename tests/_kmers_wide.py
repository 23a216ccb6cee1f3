"""What dx_code_kmer_codes, dx_kmer_runs and dx_file_kmers_wide are to compute, stated in numpy for 1 <= k <= 32: the sliding codes of
arrays of symbols as uint64, counted with np.unique; and for the file level the same over the TEXT -- the letters of each record as
the oracle's undexta -U / undexar prints them (tests/_find.py's text_of and reads).  The reference of the four test_gpu_*wide* /
sort / runs files; tests/test_kmers_wide_host.py holds it against a dict over string slices with Python integers.  Nothing here calls
the library."""
import numpy as np

import _find as F

KMER64 = np.dtype([("code", "<u8"), ("count", "<u8")])          # dx_kmer64
U = np.uint64


def codes(s, k):
    """the codes of the windows of k symbols of the array of codes s, the first symbol on top, as uint64 (k <= 32: 2 k bits)"""
    s = np.asarray(s).astype(U)
    if len(s) < k:
        return np.zeros(0, U)
    n = len(s) - k + 1
    out = np.zeros(n, U)
    for i in range(k):                                            # (shifts and ors: no product that could leave 64 bits)
        out = (out << U(2)) | s[i:i + n]
    return out


def rc(code, k):
    """the code of the reverse complement: the symbols 3 - c in reverse order"""
    code = np.asarray(code, U)
    out = np.zeros_like(code)
    for i in range(k):
        out = (out << U(2)) | (U(3) - ((code >> U(2 * i)) & U(3)))    # (the lowest symbol first: it becomes the top one)
    return out


def unit_codes(s, k, canonical=False):
    c = codes(s, k)
    return np.minimum(c, rc(c, k)) if canonical else c


def all_codes(units, k, canonical=False):
    """every unit's codes one behind the other: dx_code_kmer_codes' array"""
    return np.concatenate([unit_codes(s, k, canonical) for s in units] + [np.zeros(0, U)])


def sparse(units, k, canonical=False):
    """(the codes seen, ascending; their counts; the windows)"""
    c = all_codes(units, k, canonical)
    seen, cnt = np.unique(c, return_counts=True)
    return seen.astype(U), cnt.astype(U), len(c)


def spectrum(seen, cnt, nspec):
    """dx_kmer_runs' figures for (codes, counts): {"spectrum", "distinct", "max_count", "max_code"}"""
    cnt = np.asarray(cnt, U)
    spec = np.bincount(np.minimum(cnt, U(nspec - 1)).astype(np.int64), minlength=nspec).astype(U)
    assert spec[0] == 0
    m = int(cnt.max()) if len(cnt) else 0
    return {"spectrum": spec, "distinct": len(cnt), "max_count": m, "max_code": int(seen[np.flatnonzero(cnt == U(m))[0]]) if m else 0}


def listing(seen, cnt, min_count, cap):
    """dx_kmer_runs' list: (found, the first cap entries in ascending code order as a KMER64 array)"""
    at = np.flatnonzero(np.asarray(cnt, U) >= U(min_count))
    out = np.zeros(min(len(at), cap), KMER64)
    out["code"], out["count"] = seen[at[:cap]], cnt[at[:cap]]
    return len(at), out


def runs(sorted_codes, min_count, cap, nspec):
    """dx_kmer_runs on a host array: (found, list, figures)"""
    seen, cnt = np.unique(np.asarray(sorted_codes, U), return_counts=True)
    found, lst = listing(seen, cnt.astype(U), min_count, cap)
    return found, lst, spectrum(seen, cnt, nspec)


def packed_codes(packed, boff, beg, ln, k, canonical=False, in_bytes=None):
    """dx_code_kmer_codes on host arrays (beg None: all 0): (the whole array, the smallest bad unit or None).  A unit that does not
    lie inside the in_bytes has no window."""
    in_bytes = len(packed) if in_bytes is None else in_bytes
    units, bad = [], None
    for j in range(len(ln)):
        at, b, n = int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])
        ok = at <= in_bytes and (n == 0 or (b + n - 1) // 4 < in_bytes - at)
        if not ok and bad is None:
            bad = j
        units.append(F.symbols(packed, at, b, n) if ok else np.zeros(0, np.uint8))
    return all_codes(units, k, canonical), bad


def letters_of(kind, code, k):
    return bytes((b"ACGT" if kind == "fasta" else b"1234")[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def file_kmers_wide(kind, text, k, canonical=False, nspec=256, min_count=0, max_list=0):
    """dx_file_kmers_wide's answer, as Context.kmers_wide returns it, from the TEXT: (report, spectrum, list of (count, code, letters))"""
    rs = F.reads(kind, text)
    seen, cnt, windows = sparse(rs, k, canonical)
    sp = spectrum(seen, cnt, nspec)
    lst = listing(seen, cnt, min_count, max_list)[1] if min_count else np.zeros(0, KMER64)
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "windows": windows, "distinct": sp["distinct"],
           "max_count": sp["max_count"], "max_code": sp["max_code"], "k": k, "listed": len(lst)}
    return rep, sp["spectrum"], [(int(e["count"]), int(e["code"]), letters_of(kind, int(e["code"]), k)) for e in lst]
