"""What dx_code_hit_starts, dx_file_find_edit_spans, dx_hits_cut_plan and dx_file_cut are to compute, stated in numpy and plain Python.
The reference of tests/test_find_span_host.py, tests/test_gpu_hit_starts.py and tests/test_gpu_cut_file.py.  Nothing here calls the
library.

The start.  A hit of dx_code_find_edit (tests/_find_edit.py) is (unit U, end e, query P of m symbols, distance d = D(e)).  Its start is
    the LARGEST s, 0 <= s <= e, with Levenshtein(P, U[s, e)) == d
found here by the plain DP: the Levenshtein distance of P against U[s, e) for EVERY s in [e - m - d, e - m + d] clipped to the unit
(|(e - s) - m| <= d for any stretch d edits from P), the largest s that reaches d taken.

The plan.  Within a record the spans [start, pos) of all hits are united (spans that overlap or touch become one); the pieces are what
lies between the united spans, in front of the first and behind the last, and a piece has one symbol at least.  split: every piece of
at least min_len symbols, in order; longest: the longest such piece, on a tie the first; drop: nothing of a record with a hit.  A record
without a hit is kept whole in every mode.

The file.  The cut image is the oracle's dexta / dexar / dexqv of the text -- the oracle's undexta -U / undexar / undexqv of the image --
with every record cut as the plan says and its header rewritten to well/(B + beg)_(B + end) (tests/_subset.py: cut)."""
import numpy as np

import _find as F
import _find_edit as E
import _subset as S

NONE = 0xFFFFFFFF


# ---- the start -------------------------------------------------------------------------------------------------------------------------
def levenshtein(p, texts):
    """the Levenshtein distance of the codes p against each of `texts` (arrays of codes), by the plain DP: one column a text symbol,
    all texts side by side, each read off at its own length"""
    p = np.asarray(p, np.int64)
    m, n = len(p), len(texts)
    most = max((len(t) for t in texts), default=0)
    pad = np.full((n, most), -1, np.int64)
    for j, t in enumerate(texts):
        pad[j, :len(t)] = t
    idx = np.arange(m + 1, dtype=np.int64)
    col = np.tile(idx, (n, 1))                                    # column 0: the distance of p[:i] from the empty text is i
    out = np.full(n, -1, np.int64)
    for j, t in enumerate(texts):
        if len(t) == 0:
            out[j] = m
    for c in range(most):
        new = np.empty_like(col)
        new[:, 0] = c + 1                                         # (the empty pattern against c + 1 symbols)
        new[:, 1:] = np.minimum(col[:, :-1] + (p[None, :] != pad[:, c, None]), col[:, 1:] + 1)
        col = np.minimum.accumulate(new - idx, axis=1) + idx
        for j, t in enumerate(texts):
            if len(t) == c + 1:
                out[j] = col[j, m]
    return out


def reaching(u, e, p, d):
    """every s in the window with Levenshtein(p, u[s:e]) == d, ascending"""
    m = len(p)
    lo, hi = max(0, e - m - d), min(e, e - m + d)
    if hi < lo:
        return []
    ss = list(range(lo, hi + 1))
    dist = levenshtein(p, [np.asarray(u[s:e]) for s in ss])
    return [s for s, x in zip(ss, dist) if x == d]


def start_of(u, e, p, d):
    """the start of the hit (e, p, d) in the unit u, or NONE when no stretch that ends at e lies d from p"""
    r = reaching(u, e, p, d)
    return r[-1] if r else NONE


def backward_bitvector(u, e, p, d):
    """a second, independent formulation: the bit-vector recurrence on Python ints with the query REVERSED and a carry of 1 into the
    horizontal deltas (the start is anchored at e), stepped backwards from symbol e - 1, the score beginning at m; the first step t
    at which the score is d gives e - t"""
    m = len(p)
    full, top = (1 << m) - 1, 1 << (m - 1)
    peq = [0, 0, 0, 0]
    for i, c in enumerate(reversed([int(c) for c in p])):
        peq[c] |= 1 << i
    pv, mv, score = full, 0, m
    for t in range(1, min(e, m + d) + 1):
        eq = peq[int(u[e - t])]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & full
        ph = (mv | ~(xh | pv)) & full
        mh = pv & xh
        score += (1 if ph & top else 0) - (1 if mh & top else 0)
        ph, mh = ((ph << 1) | 1) & full, (mh << 1) & full
        pv = (mh | ~(xv | ph)) & full
        mv = ph & xv
        if score == d:
            return e - t
    return NONE


def code_hit_starts(packed, boff, beg, ln, queries, hits):
    """dx_code_hit_starts on host arrays for a list of GOOD hits (a HIT array: record, pos, query, mis) -> uint32 starts"""
    units = {}
    out = np.zeros(len(hits), np.uint32)
    for i, h in enumerate(hits):
        j = int(h["record"])
        if j not in units:
            units[j] = F.symbols(packed, int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j]))
        out[i] = start_of(units[j], int(h["pos"]), queries[int(h["query"])][0], int(h["mis"]))
    return out


# ---- the file level, from the text -----------------------------------------------------------------------------------------------------
def file_find_spans(kind, text, patterns, max_err=0, both_strands=False, max_hits=1 << 20):
    """dx_file_find_edit_spans' answer, as Context.find_spans(per_record=True) returns it, from the TEXT: tests/_find_edit.py's report and
    list, and for every listed hit the start of its occurrence on the read as stored -- a strand-1 hit is a hit of the pattern's
    reverse complement"""
    rep, lst = E.file_find_edit(kind, text, patterns, max_err, both_strands, max_hits)
    rs = F.reads(kind, text)
    st = np.zeros(len(lst), np.uint32)
    for i, h in enumerate(lst):
        c = F.pattern_codes(kind, patterns[int(h["query"])])
        if h["strand"]:
            c = [3 - v for v in reversed(c)]
        st[i] = start_of(rs[int(h["record"])], int(h["pos"]), c, int(h["mis"]))
    rep = dict(rep, start=st, rec_len=np.array([len(r) for r in rs], np.uint32))
    return rep, lst


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def plan(records, pos, starts, rec_len, min_len=0, mode="split"):
    """hits (records[i], starts[i], pos[i]) in any order -> (units [(id, beg, end)], report)"""
    per = {}
    for r, s, e in zip(records, starts, pos):
        r, s, e = int(r), int(s), int(e)
        assert 0 <= r < len(rec_len) and 0 <= s <= e <= int(rec_len[r])
        per.setdefault(r, []).append((s, e))
    units, rep = [], dict(records_in=len(rec_len), records_cut=0, records_dropped=0, pieces=0, symbols_in=0, symbols_kept=0, spans=0)
    for r, n in enumerate(int(x) for x in rec_len):
        rep["symbols_in"] += n
        if r not in per:
            units.append((r, 0, n))
            continue
        united = []
        for s, e in sorted(per[r]):
            if united and s <= united[-1][1]:
                united[-1][1] = max(united[-1][1], e)
            else:
                united.append([s, e])
        rep["spans"] += len(united)
        edges = [0] + [x for s, e in united for x in (s, e)] + [n]
        pieces = [(b, e) for b, e in zip(edges[0::2], edges[1::2]) if e - b >= max(min_len, 1)]
        if mode == "longest":
            pieces = [max(pieces, key=lambda p: (p[1] - p[0], -p[0]))] if pieces else []
        elif mode == "drop":
            pieces = []
        else:
            assert mode == "split"
        units += [(r, b, e) for b, e in pieces]
        rep["records_cut" if pieces else "records_dropped"] += 1
    rep["pieces"] = len(units)
    rep["symbols_kept"] = sum(e - b for _, b, e in units)
    return units, rep


def cut_text(kind, text, units):
    """the text with every record cut as the units say, headers rewritten"""
    return S.cut(kind, text, units)


def cut_image(kind, img, units, lossy=False):
    """the oracle's encoding of the oracle's text of img, cut"""
    text = cut_text(kind, S.DECODE[kind](img), units)
    return S.ENCODE[kind](text, lossy) if kind == "quiva" else S.ENCODE[kind](text)
