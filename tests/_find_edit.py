"""What dx_code_find_edit and dx_file_find_edit are to compute, stated in numpy and plain Python: the semi-global edit distance D by
the plain DP column, the valley rule over it, and for the file level the same over the TEXT -- the letters of each record as the
oracle's undexta -U / undexar prints them.  An independent bit-vector implementation (Myers 1999) on Python ints stands beside the
DP, and the same recurrence on numpy words a query, for the cases where the DP would take too long.  The reference of
tests/test_find_edit_host.py, tests/test_gpu_find_edit.py and tests/test_gpu_find_edit_file.py.  Nothing here calls the library.

The contract.  Unit U has L symbols, query P has m (1..64) and an error bound k, 0 <= k < m.
    D(e) = min over 0 <= s <= e of Levenshtein(P, U[s, e)) for 1 <= e <= L (substitution, insertion, deletion cost one each);
    c(e) = min(D(e), k + 1), c(0) = c(L + 1) = k + 1.
A hit is an end e with c(e) <= k, c(e) < c(e - 1) and c(e) <= c(e + 1): one for each valley of the distance, at the leftmost end of
its floor; pos = e (the exclusive end of the occurrence), mis = D(e)."""
import numpy as np

import _find as F

HIT, SAT32 = F.HIT, F.SAT32


# ---- the distance ----------------------------------------------------------------------------------------------------------------------
def dp(s, qs):
    """D for the codes s against every query of qs (arrays of codes, all of one length m), by the plain DP column -> int64 [len(qs),
    len(s)]: entry [j, e - 1] = D(e) of query j.  Row 0 of the matrix is 0 all along: the start in the read is free."""
    s, qs = np.asarray(s, np.uint8), np.asarray(qs, np.uint8).reshape(len(qs), -1)
    nq, m = qs.shape
    idx = np.arange(m + 1, dtype=np.int64)
    col = np.tile(idx, (nq, 1))                                   # column 0: D[i][0] = i
    out = np.zeros((nq, len(s)), np.int64)
    for e, c in enumerate(s):
        t = np.empty_like(col)
        t[:, 0] = 0
        t[:, 1:] = np.minimum(col[:, :-1] + (qs != c), col[:, 1:] + 1)      # a substitution or a match; the text's symbol left out
        col = np.minimum.accumulate(t - idx, axis=1) + idx       # ... and the query's symbols left out, from above
        out[:, e] = col[:, m]
    return out


def bitvector(s, q):
    """D for the codes s against the one query q, by the bit-vector recurrence on Python ints (semi-global: no carry of 1 into the
    horizontal shift) -> list of len(s) distances"""
    m = len(q)
    full, top = (1 << m) - 1, 1 << (m - 1)
    peq = [0, 0, 0, 0]
    for i, c in enumerate(q):
        peq[int(c)] |= 1 << i
    pv, mv, score, out = full, 0, m, []
    for c in s:
        eq = peq[int(c)]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & full
        ph = (mv | ~(xh | pv)) & full
        mh = pv & xh
        score += 1 if ph & top else 0
        score -= 1 if mh & top else 0
        ph, mh = (ph << 1) & full, (mh << 1) & full
        pv = (mh | ~(xv | ph)) & full
        mv = ph & xv
        out.append(score)
    return out


def bitvector_many(s, qs):
    """... and for many queries of any lengths at once, a numpy word a query -> int64 [len(qs), len(s)]"""
    nq = len(qs)
    m = np.array([len(q) for q in qs], np.uint64)
    peq = np.zeros((4, nq), np.uint64)
    for j, q in enumerate(qs):
        for i, c in enumerate(q):
            peq[int(c), j] |= np.uint64(1 << i)
    one, sh = np.uint64(1), m - np.uint64(1)
    pv, mv = np.full(nq, ~np.uint64(0)), np.zeros(nq, np.uint64)
    score, out = m.astype(np.int64), np.zeros((nq, len(s)), np.int64)
    for e, c in enumerate(np.asarray(s, np.uint8)):
        eq = peq[int(c)]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | ~(xh | pv)
        mh = pv & xh
        score = score + ((ph >> sh) & one).astype(np.int64) - ((mh >> sh) & one).astype(np.int64)
        ph, mh = ph << one, mh << one
        pv = mh | ~(xv | ph)
        mv = ph & xv
        out[:, e] = score
    return out


def valleys(D, k):
    """the valley rule over D(1 .. L) -> (the ends, the distances there)"""
    D = np.asarray(D, np.int64)
    c = np.concatenate([[k + 1], np.minimum(D, k + 1), [k + 1]])                 # c(0) .. c(L + 1)
    e = 1 + np.flatnonzero((c[1:-1] <= k) & (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:]))
    return e, c[e]


# ---- the search ------------------------------------------------------------------------------------------------------------------------
def dp_units(units, qs):
    """dp for many units at once (the same column, an axis more): a list of [len(qs), len(unit)] arrays.  The units are padded to the
    longest with code 0; what the DP makes of the pad lies behind every unit's own ends and is cut off."""
    qs = np.asarray(qs, np.uint8).reshape(len(qs), -1)
    nq, m = qs.shape
    most = max((len(u) for u in units), default=0)
    text = np.zeros((len(units), most), np.uint8)
    for j, u in enumerate(units):
        text[j, :len(u)] = u
    idx = np.arange(m + 1, dtype=np.int8)
    col = np.tile(idx, (len(units), nq, 1))
    out = np.zeros((len(units), nq, most), np.int8)
    for e in range(most):
        t = np.empty_like(col)
        t[:, :, 0] = 0
        t[:, :, 1:] = np.minimum(col[:, :, :-1] + (qs[None, :, :] != text[:, e, None, None]).astype(np.int8), col[:, :, 1:] + 1)
        col = np.minimum.accumulate(t - idx, axis=2) + idx
        out[:, :, e] = col[:, :, m]
    return [out[j, :, :len(u)].astype(np.int64) for j, u in enumerate(units)]


def distances(units, queries, fast=False):
    """D of every query (codes, k) over every unit: a list (a unit) of int64 [queries, len(unit)].  fast: by the bit-vector words, else
    by the DP"""
    if fast and len(queries) <= 4:                                # (a few queries: Python ints are quicker than numpy words of one element)
        return [np.array([bitvector(s, q) for q, _ in queries], np.int64).reshape(len(queries), len(s)) for s in units]
    if fast:
        return [bitvector_many(s, [q for q, _ in queries]) for s in units]
    out = [np.zeros((len(queries), len(s)), np.int64) for s in units]
    for m in sorted({len(q) for q, _ in queries}):
        js = [j for j, (q, _) in enumerate(queries) if len(q) == m]
        for u, d in enumerate(dp_units(units, [queries[j][0] for j in js])):
            out[u][js] = d
    return out


def unit_hits(D, errs):
    """the valley rule for all queries of a unit at once: D [queries, L], errs [queries] -> (pos, query, mis) in the order (pos, query);
    tests/test_find_edit_host.py holds it against valleys()"""
    errs = np.asarray(errs, np.int64)[:, None]
    c = np.concatenate([errs + 1, np.minimum(D, errs + 1), errs + 1], axis=1)                 # c(0) .. c(L + 1), a row a query
    hit = (c[:, 1:-1] <= errs) & (c[:, 1:-1] < c[:, :-2]) & (c[:, 1:-1] <= c[:, 2:])
    pos, k = np.nonzero(hit.T)                                    # (row-major over (end, query): the list's order)
    return pos + 1, k, c[k, pos + 1]


def search(units, queries, fast=False):
    """units: arrays of codes; queries: (codes, k) -> every hit in the order (unit, pos, query) as a HIT array (strand 0), the hits a
    unit, the hits a query"""
    parts, per_unit, per_query = [], np.zeros(len(units), np.uint64), np.zeros(len(queries), np.uint64)
    errs = [k for _, k in queries]
    for j, D in enumerate(distances(units, queries, fast)):
        pos, k, mis = unit_hits(D, errs)
        rows = np.zeros(len(pos), HIT)
        rows["record"], rows["pos"], rows["query"], rows["mis"] = j, pos, k, mis
        parts.append(rows)
        per_unit[j] = len(pos)
        per_query += np.bincount(k, minlength=len(queries)).astype(np.uint64)
    return np.concatenate(parts) if parts else np.zeros(0, HIT), per_unit, per_query


def code_find_edit(packed, boff, beg, ln, queries, cap=0, fast=False):
    """dx_code_find_edit on host arrays; beg None: all 0 -> {"hits", "total" (a query), "count" (a unit, saturated), "list" (the first cap)}"""
    units = [F.symbols(packed, int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])) for j in range(len(ln))]
    lst, per_unit, per_query = search(units, queries, fast)
    return {"hits": int(per_query.sum()), "total": per_query, "count": np.minimum(per_unit, SAT32).astype(np.uint32), "list": lst[:cap]}


def file_find_edit(kind, text, patterns, max_err=0, both_strands=False, max_hits=1 << 20, fast=False):
    """dx_file_find_edit's answer, as Context.find_edit(per_record=True) returns it, from the TEXT: (report, the first max_hits hits in
    the order (record, pos, pattern, strand)).  The reverse complement of a pattern is searched as a pattern of its own, strand 1,
    unless it is the pattern itself; its pos is the end of the reverse complement's occurrence on the read as stored."""
    rs = F.reads(kind, text)
    qs, name = [], []
    for p, pat in enumerate(patterns):
        c = F.pattern_codes(kind, pat)
        qs.append((c, max_err)); name.append((p, 0))
        rc = [3 - v for v in reversed(c)]
        if both_strands and rc != c:
            qs.append((rc, max_err)); name.append((p, 1))
    lst, per_unit, per_query = search(rs, qs, fast)
    per = np.zeros((len(patterns), 2), np.uint64)
    for k, (p, s) in enumerate(name):
        per[p, s] += per_query[k]
    k = lst["query"].astype(np.int64)
    lst["query"], lst["strand"] = np.array(name, np.int64)[k, 0], np.array(name, np.int64)[k, 1]
    hits = int(per_query.sum())
    rep = {"records": len(rs), "records_hit": int((per_unit != 0).sum()), "hits": hits, "listed": min(hits, max_hits),
           "per_pattern": per, "rec_hits": np.minimum(per_unit, SAT32).astype(np.uint32)}
    return rep, lst[:max_hits]
