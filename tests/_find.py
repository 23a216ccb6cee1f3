"""What dx_code_find and dx_file_find are to compute, stated in numpy: a naive sliding compare over arrays of codes, and for the
file level over the TEXT -- the letters of each record as the oracle's undexta -U / undexar prints them.  The reference of
tests/test_gpu_find.py and tests/test_gpu_find_file.py.  Nothing here calls the library."""
import numpy as np

import _oracle as O

HIT = np.dtype([("record", "<u8"), ("pos", "<u4"), ("query", "<u2"), ("strand", "u1"), ("mis", "u1")])      # dx_hit
SAT32 = 0xFFFFFFFF


def symbols(packed, at, beg, n):
    """symbols [beg, beg + n) of the packed read at byte `at` (DB.c:319-338: four a byte, the first in the top two bits)"""
    raw = np.frombuffer(bytes(packed), np.uint8)[at:at + (beg + n + 3) // 4]
    assert len(raw) == (beg + n + 3) // 4, "a reference read outside its buffer"
    return np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[beg:beg + n]


def pack(codes, pad=0):
    """codes -> packed bytes; the pad bits of the last byte are the low bits of `pad`"""
    c = np.asarray(codes, np.uint8)
    n = len(c)
    full = np.concatenate([c, np.zeros((-n) % 4, np.uint8)]).reshape(-1, 4)
    out = ((full[:, 0] << 6) | (full[:, 1] << 4) | (full[:, 2] << 2) | full[:, 3]).astype(np.uint8)
    if n & 3:
        out[-1] |= pad & ((1 << (8 - 2 * (n & 3))) - 1)
    return out.tobytes()


def query(codes, max_mis=0):
    """codes of 1 to 32 symbols -> the (code, len, max_mis) of a dx_query: the first symbol on top"""
    code = 0
    for c in codes:
        code = (code << 2) | int(c)
    return code, len(codes), int(max_mis)


def windows(s, q, max_mis):
    """the positions at which the codes q lie in the codes s with at most max_mis differing places -> (positions, distances)"""
    s, q = np.asarray(s, np.uint8), np.asarray(q, np.uint8)
    if len(s) < len(q):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    mis = np.zeros(len(s) - len(q) + 1, np.int64)
    for i, c in enumerate(q):                                     # the naive compare, a query symbol at a time
        mis += s[i:i + len(mis)] != c
    pos = np.flatnonzero(mis <= max_mis)
    return pos, mis[pos]


def search(units, queries):
    """units: arrays of codes; queries: (codes, max_mis) -> every hit in the order (unit, pos, query) as a HIT array (strand 0), the
    hits a unit, the hits a query"""
    rows, per_unit, per_query = [], np.zeros(len(units), np.uint64), np.zeros(len(queries), np.uint64)
    for j, s in enumerate(units):
        mine = []
        for k, (q, mm) in enumerate(queries):
            pos, mis = windows(s, q, mm)
            per_query[k] += len(pos)
            mine += [(int(p), k, int(d)) for p, d in zip(pos, mis)]
        per_unit[j] = len(mine)
        rows += [(j, p, k, 0, d) for p, k, d in sorted(mine)]
    return np.array(rows, HIT) if rows else np.zeros(0, HIT), per_unit, per_query


def code_find(packed, boff, beg, ln, queries, cap=0):
    """dx_code_find on host arrays; beg None: all 0 -> {"hits", "total" (a query), "count" (a unit, saturated), "list" (the first cap)}"""
    units = [symbols(packed, int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])) for j in range(len(ln))]
    lst, per_unit, per_query = search(units, queries)
    return {"hits": int(per_query.sum()), "total": per_query, "count": np.minimum(per_unit, SAT32).astype(np.uint32), "list": lst[:cap]}


# ---- the file level, from the text ---------------------------------------------------------------------------------------------------
def text_of(kind, img):
    """the text the ORACLE prints for an image: undexta -U / undexar"""
    return O.undexta(img, upper=True) if kind == "fasta" else O.undexar(img)


def reads(kind, text):
    """a text -> the letters of every record, line breaks taken out, as arrays of codes"""
    letters = b"ACGT" if kind == "fasta" else b"1234"
    lut = np.full(256, 255, np.uint8)
    for c, l in enumerate(letters):
        lut[l] = c
    lines = text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n")
    starts = [i for i, l in enumerate(lines) if l.startswith(b">")] + [len(lines)]
    out = []
    for s, e in zip(starts, starts[1:]):
        codes = lut[np.frombuffer(b"".join(lines[s + 1:e]), np.uint8)]
        assert (codes != 255).all(), "a letter the decoder never prints"
        out.append(codes)
    return out


def pattern_codes(kind, p):
    return [(b"acgt" if kind == "fasta" else b"1234").index(c) for c in (p.lower().encode() if isinstance(p, str) else p.lower())]


def file_find(kind, text, patterns, max_mis=0, both_strands=False, max_hits=1 << 20):
    """dx_file_find's answer, as Context.find(per_record=True) returns it, from the TEXT: (report, the first max_hits hits in the order
    (record, pos, pattern, strand)).  The reverse complement of a pattern is searched as a pattern of its own, strand 1, unless it is
    the pattern itself (a palindrome reports strand 0 only)."""
    rs = reads(kind, text)
    qs, name = [], []
    for p, pat in enumerate(patterns):
        c = pattern_codes(kind, pat)
        qs.append((c, max_mis)); name.append((p, 0))
        rc = [3 - v for v in reversed(c)]
        if both_strands and rc != c:
            qs.append((rc, max_mis)); name.append((p, 1))
    lst, per_unit, per_query = search(rs, qs)                      # (queries in the order (pattern, strand): so is the list)
    per = np.zeros((len(patterns), 2), np.uint64)
    for k, (p, s) in enumerate(name):
        per[p, s] += per_query[k]
    k = lst["query"].astype(np.int64)
    lst["query"], lst["strand"] = np.array(name, np.int64)[k, 0], np.array(name, np.int64)[k, 1]
    hits = int(per_query.sum())
    rep = {"records": len(rs), "records_hit": int((per_unit != 0).sum()), "hits": hits, "listed": min(hits, max_hits),
           "per_pattern": per, "rec_hits": np.minimum(per_unit, SAT32).astype(np.uint32)}
    return rep, lst[:max_hits]


def assert_same_find(got, want):
    (g, gl), (w, wl) = got, want
    for f in ("records", "records_hit", "hits", "listed"):
        assert g[f] == w[f], (f, g[f], w[f])
    assert np.array_equal(g["per_pattern"], w["per_pattern"]), (g["per_pattern"], w["per_pattern"])
    if "rec_hits" in g:
        assert np.array_equal(g["rec_hits"], w["rec_hits"])
    assert len(gl) == len(wl) and (gl == wl).all(), [(a, b) for a, b in zip(gl, wl) if a != b][:5]
