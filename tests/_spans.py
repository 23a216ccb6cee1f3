"""What dx_code_kmer_spans, dx_spans_join, dx_spans_cut_plan and dx_file_screen_spans are to compute, stated in numpy and plain
Python: a unit's raw spans read off the boolean cover array that tests/_screen.py's unit_screen builds (the union of the hit windows
[p, p + k)), the join and the filter as a plain loop, the plan as a plain loop over Python integers, and for the file level the same
over the TEXT the oracle prints for the image.  The reference of tests/test_gpu_kmer_spans.py, test_gpu_spans_join.py and
test_gpu_screen_spans_file.py; tests/test_spans_host.py holds it against cases written by hand.  Nothing here calls the library."""
import numpy as np

import _find as F
import _kmers_wide as W

SPAN = np.dtype([("record", "<u8"), ("beg", "<u4"), ("end", "<u4")])          # dx_span
U = np.uint64


def cover(s, k, canonical, codes):
    """the unit's symbols that lie in a window whose code is in the set, as a boolean array (unit_screen's)"""
    c = W.unit_codes(s, k, canonical)
    cov = np.zeros(len(s), bool)
    for p in np.flatnonzero(np.isin(c, np.asarray(codes, U))):
        cov[p:p + k] = True
    return cov


def runs(cov):
    """the maximal runs of True as [(beg, end)]"""
    out, beg = [], None
    for i, v in enumerate(list(cov) + [False]):
        if v and beg is None:
            beg = i
        elif not v and beg is not None:
            out.append((beg, i))
            beg = None
    return out


def unit_spans(s, k, canonical, codes):
    return runs(cover(s, k, canonical, codes))


def as_spans(triples):
    a = np.zeros(len(triples), SPAN)
    for i, (r, b, e) in enumerate(triples):
        a[i] = (r, b, e)
    return a


def spans(units, k, canonical, codes):
    """the list of all units (None: a unit that does not lie in its buffer) in the order (unit, beg), every unit's count, and the totals:
    spans, covered symbols, units with a span"""
    lst, cnt = [], np.zeros(len(units), np.uint32)
    tot = [0, 0, 0]
    for j, s in enumerate(units):
        if s is None:
            continue
        sp = unit_spans(s, k, canonical, codes)
        cnt[j] = len(sp)
        lst += [(j, b, e) for b, e in sp]
        tot[0] += len(sp); tot[1] += sum(e - b for b, e in sp); tot[2] += 1 if sp else 0
    return as_spans(lst), cnt, np.array(tot, U)


def packed_spans(packed, boff, beg, ln, k, canonical, codes, in_bytes=None):
    """dx_code_kmer_spans on host arrays (beg None: all 0): (list, counts, totals, the smallest bad unit or None)"""
    in_bytes = len(packed) if in_bytes is None else in_bytes
    units, bad = [], None
    for j in range(len(ln)):
        at, b, n = int(boff[j]), 0 if beg is None else int(beg[j]), int(ln[j])
        ok = at <= in_bytes and n < 2 ** 31 and (n == 0 or (b + n - 1) // 4 < in_bytes - at)
        if not ok and bad is None:
            bad = j
        units.append(F.symbols(packed, at, b, n) if ok else None)
    return spans(units, k, canonical, codes) + (bad,)


def first_bad(lst):
    """the smallest index of a list that breaks dx_spans_join's input order, or None"""
    for i in range(len(lst)):
        r, b, e = (int(lst[i][f]) for f in ("record", "beg", "end"))
        if not b < e:
            return i
        if i:
            pr, pe = int(lst[i - 1]["record"]), int(lst[i - 1]["end"])
            if r < pr or (r == pr and b < pe):
                return i
    return None


def join(lst, max_gap, min_span):
    """the join, then the filter: (the kept spans as a SPAN array, [kept, their symbols])"""
    joined = []
    for i in range(len(lst)):
        r, b, e = (int(lst[i][f]) for f in ("record", "beg", "end"))
        if joined and joined[-1][0] == r and b - joined[-1][2] <= max_gap:
            joined[-1][2] = e
        else:
            joined.append([r, b, e])
    kept = [tuple(x) for x in joined if x[2] - x[1] >= min_span]
    return as_spans(kept), [len(kept), sum(e - b for _, b, e in kept)]


def plan(triples, rec_len, min_len=0, mode="split"):
    """spans (record, beg, end) in any order -> (units [(id, beg, end)], report): dx_spans_cut_plan over Python integers"""
    per = {}
    for r, s, e in triples:
        r, s, e = int(r), int(s), int(e)
        assert 0 <= r < len(rec_len) and 0 <= s <= e <= int(rec_len[r])
        per.setdefault(r, []).append((s, e))
    units, rep = [], dict(records_in=len(rec_len), records_cut=0, records_dropped=0, pieces=0, symbols_in=0, symbols_kept=0, spans=0)
    for r in range(len(rec_len)):
        n = int(rec_len[r])
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
        pieces, at = [], 0
        for s, e in united + [[n, n]]:
            if s - at >= max(min_len, 1):
                pieces.append((at, s))
            at = e
        if mode == "longest":
            best = None
            for p in pieces:
                if best is None or p[1] - p[0] > best[1] - best[0]:
                    best = p
            pieces = [best] if best else []
        elif mode == "drop":
            pieces = []
        else:
            assert mode == "split"
        units += [(r, b, e) for b, e in pieces]
        rep["records_cut" if pieces else "records_dropped"] += 1
    rep["pieces"] = len(units)
    rep["symbols_kept"] = sum(e - b for _, b, e in units)
    return units, rep


def file_spans(kind, text, k, canonical, codes, max_gap=0, min_span=0, max_spans=1 << 20):
    """dx_file_screen_spans's answer, as Context.screen_spans returns it, from the TEXT: (report, spans, rec_spans, rec_len)"""
    rs = F.reads(kind, text)
    raw, cnt, tot = spans(rs, k, canonical, codes)
    kept, jt = join(raw, max_gap, min_span)
    rec = np.zeros(len(rs), np.uint32)
    for r in kept["record"]:
        rec[int(r)] += 1
    n = min(len(kept), max_spans)
    rep = {"records": len(rs), "symbols": int(sum(len(r) for r in rs)), "covered": int(tot[1]), "records_hit": int(tot[2]),
           "raw_spans": int(tot[0]), "spans": jt[0], "span_symbols": jt[1], "listed": n, "k": k}
    return rep, kept[:n], rec, np.array([len(r) for r in rs], np.uint32)
