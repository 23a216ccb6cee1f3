"""The host side of the screen spans, no GPU: the new symbols are exported, declared and bound, the structures have the C sizes;
tests/_spans.py (the statement the GPU tests hold the kernels against) against cases written by hand; and dx_spans_cut_plan against the
statement's plan and against dx_hits_cut_plan over the same triples.  No expected value comes from the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find_span as P
import _oracle as O
import _spans as SP
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_kmer_spans", "dx_spans_join", "dx_file_screen_spans", "dx_spans_cut_plan", "dx_file_screen_cut"]
E_ARG = -1
MODES = ("split", "longest", "drop")


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("code_kmer_spans", "spans_join", "screen_spans", "screen_cut"):
        assert callable(getattr(api.Context, m))
    assert callable(api.spans_cut_plan)
    assert C.sizeof(L.Span) == 16 == api.SPAN_DTYPE.itemsize == SP.SPAN.itemsize
    assert [f for f, _ in L.Span._fields_] == ["record", "beg", "end"] == list(api.SPAN_DTYPE.names)
    assert [api.SPAN_DTYPE.fields[f][1] for f in api.SPAN_DTYPE.names] == [L.Span.record.offset, L.Span.beg.offset, L.Span.end.offset] == [0, 8, 12]
    assert C.sizeof(L.SpansReport) == 72
    assert [f for f, _ in L.SpansReport._fields_] == ["records", "symbols", "covered", "records_hit", "raw_spans", "spans", "span_symbols",
                                                      "listed", "k", "reserved"]
    assert re.search(r"typedef struct \{ uint64_t record; uint32_t beg, end; \} dx_span;", hdr)


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    tot, rp = (C.c_uint64 * 3)(), L.SpansReport()
    out, ln = C.c_void_p(), C.c_size_t()
    assert lib.dx_code_kmer_spans(None, None, 0, None, None, None, 0, None, None, None, 0, C.byref(tot), None) == E_ARG
    assert lib.dx_spans_join(None, None, 0, 0, 0, None, 0, C.cast(tot, C.POINTER(C.c_uint64 * 2)), None) == E_ARG
    assert lib.dx_file_screen_spans(None, L.DX_KIND_FASTA, img, len(img), None, 0, 0, 0, C.byref(rp), None, None, None) == E_ARG
    assert lib.dx_file_screen_cut(None, L.DX_KIND_FASTA, img, len(img), None, 0, 0, 0, 0, C.byref(out), C.byref(ln), None, None, None,
                                  None, None) == E_ARG
    assert lib.dx_spans_cut_plan(None, 0, None, 0, 0, 0, None, None, None, None, None) == E_ARG


# ---- the statement, by hand ------------------------------------------------------------------------------------------------------------
def test_runs_and_unit_spans_by_hand():
    assert SP.runs([]) == [] and SP.runs([False, False]) == []
    assert SP.runs([True, True, False, True]) == [(0, 2), (3, 4)]
    assert SP.runs([False, True, True, True]) == [(1, 4)]
    # acgtacgtaa, k = 3: acg at 0 and 4, cgt at 1 and 5, gta at 2 and 6, tac at 3, taa at 7
    s = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 0], np.uint8)
    code = lambda w: sum("acgt".index(c) << (2 * (len(w) - 1 - i)) for i, c in enumerate(w))
    assert SP.unit_spans(s, 3, False, [code("acg")]) == [(0, 3), (4, 7)]                       # hit windows k + 1 apart: a gap of one symbol
    assert SP.unit_spans(s, 3, False, [code("acg"), code("tac")]) == [(0, 7)]                  # ... closed by a window between them
    assert SP.unit_spans(s, 3, False, [code("taa")]) == [(7, 10)]                              # a span that ends at the unit's end
    assert SP.unit_spans(s, 3, False, [code("ccc")]) == [] and SP.unit_spans(s[:2], 3, False, [code("acg")]) == []
    assert SP.unit_spans(s, 3, True, [min(code("tta"), code("taa"))]) == [(7, 10)]              # canonical: either strand's code
    lst, cnt, tot = SP.spans([s, None, s[:2], s], 3, False, [code("acg")])
    assert [tuple(int(v) for v in x) for x in lst] == [(0, 0, 3), (0, 4, 7), (3, 0, 3), (3, 4, 7)]
    assert cnt.tolist() == [2, 0, 0, 2] and tot.tolist() == [4, 12, 2]


def test_join_and_filter_by_hand():
    lst = SP.as_spans([(0, 0, 5), (0, 7, 9), (0, 12, 20), (1, 21, 25), (1, 25, 30), (3, 4, 5)])
    same = lambda got, want: [tuple(int(v) for v in x) for x in got[0]] == want and got[1] == [len(want), sum(e - b for _, b, e in want)]
    assert same(SP.join(lst, 0, 0), [(0, 0, 5), (0, 7, 9), (0, 12, 20), (1, 21, 30), (3, 4, 5)])           # (spans that touch: a gap of 0)
    assert same(SP.join(lst, 1, 0), [(0, 0, 5), (0, 7, 9), (0, 12, 20), (1, 21, 30), (3, 4, 5)])
    assert same(SP.join(lst, 2, 0), [(0, 0, 9), (0, 12, 20), (1, 21, 30), (3, 4, 5)])                      # a gap exactly at max_gap
    assert same(SP.join(lst, 3, 0), [(0, 0, 20), (1, 21, 30), (3, 4, 5)])                                 # (20 -> 21 is a record change)
    assert same(SP.join(lst, 2 ** 32 - 1, 0), [(0, 0, 20), (1, 21, 30), (3, 4, 5)])                       # one span a record
    assert same(SP.join(lst, 2, 9), [(0, 0, 9), (1, 21, 30)])                                             # the filter comes after the join
    assert same(SP.join(lst, 2, 10), []) and same(SP.join(lst[:0], 5, 0), [])
    assert SP.first_bad(lst) is None and SP.first_bad(lst[:0]) is None
    # no symbol; begins inside its predecessor (twice); beg beyond end; a record that decreases
    for i, entry in ((2, (0, 12, 12)), (3, (0, 19, 25)), (1, (0, 4, 9)), (5, (3, 9, 5)), (4, (0, 25, 30))):
        bad = lst.copy()
        bad[i] = entry
        assert SP.first_bad(bad) == i, (i, entry)
    ok = lst.copy()
    ok[3] = (0, 21, 25)                                          # (record 0 goes on behind 20, record 1 follows: in order)
    assert SP.first_bad(ok) is None


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def units_of(sel):
    return list(zip(sel["ids"].tolist(), sel["beg"].tolist(), sel["end"].tolist()))


def same_plan(triples, rec_len, min_len, mode):
    """dx_spans_cut_plan against the statement, and against dx_hits_cut_plan over the same triples as hits and starts"""
    want_units, want_rep = SP.plan(triples, rec_len, min_len, mode)
    sel, rep = api.spans_cut_plan(SP.as_spans(triples), rec_len, min_len, mode)
    assert units_of(sel) == want_units, (mode, min_len, units_of(sel)[:6], want_units[:6])
    assert rep == want_rep, (rep, want_rep)
    hits = np.zeros(len(triples), api.HIT_DTYPE)
    hits["record"], hits["pos"] = [t[0] for t in triples], [t[2] for t in triples]
    hsel, hrep = api.cut_plan(hits, np.array([t[1] for t in triples], np.uint32), rec_len, min_len, mode)
    assert units_of(hsel) == want_units and hrep == want_rep
    assert (want_units, want_rep) == P.plan([t[0] for t in triples], [t[2] for t in triples], [t[1] for t in triples], rec_len, min_len, mode)
    return want_units, want_rep


def test_the_plan_on_cases_made_by_hand():
    rec_len = [30, 0, 12, 40, 7, 20]
    # record 0: two spans that touch, one nested, one apart; 2: a span over the whole record; 3: overlapping spans out of order;
    # 4, 1 (of length 0): none; 5: spans at 0 and at the record's end
    tr = [(0, 2, 8), (0, 8, 12), (0, 3, 5), (0, 20, 25), (2, 0, 12), (3, 18, 22), (3, 5, 23), (3, 30, 31), (3, 10, 31), (5, 0, 4), (5, 15, 20)]
    units, rep = same_plan(tr, rec_len, 0, "split")
    assert units == [(0, 0, 2), (0, 12, 20), (0, 25, 30), (1, 0, 0), (3, 0, 5), (3, 31, 40), (4, 0, 7), (5, 4, 15)]
    assert rep == dict(records_in=6, records_cut=3, records_dropped=1, pieces=8, symbols_in=109, symbols_kept=47, spans=6)
    assert same_plan(tr, rec_len, 1, "split")[0] == units                              # (a piece has one symbol at least: 0 and 1 are one)
    assert same_plan(tr, rec_len, 6, "split")[0] == [(0, 12, 20), (1, 0, 0), (3, 31, 40), (4, 0, 7), (5, 4, 15)]
    assert same_plan(tr, rec_len, 0, "longest")[0] == [(0, 12, 20), (1, 0, 0), (3, 31, 40), (4, 0, 7), (5, 4, 15)]
    assert same_plan(tr, rec_len, 1000, "longest")[0] == [(1, 0, 0), (4, 0, 7)]
    units, rep = same_plan(tr, rec_len, 0, "drop")
    assert units == [(1, 0, 0), (4, 0, 7)] and rep == dict(records_in=6, records_cut=0, records_dropped=4, pieces=2, symbols_in=109,
                                                           symbols_kept=7, spans=6)
    # an empty span cuts nothing out and parts the record where it stands; at 0 and at the end it parts nothing off
    assert same_plan([(0, 4, 4)], [10], 0, "split")[0] == [(0, 0, 4), (0, 4, 10)]
    assert same_plan([(0, 0, 0), (0, 10, 10)], [10], 0, "split")[0] == [(0, 0, 10)]
    assert same_plan([(0, 0, 0)], [0], 0, "split") == ([], dict(records_in=1, records_cut=0, records_dropped=1, pieces=0, symbols_in=0,
                                                              symbols_kept=0, spans=1))
    assert same_plan([(0, 5, 7), (0, 12, 20)], [25], 0, "longest")[0] == [(0, 0, 5)]   # the first of two pieces of one length
    assert same_plan([], [3, 0, 9], 5, "split")[0] == [(0, 0, 3), (1, 0, 0), (2, 0, 9)]
    assert same_plan([], [], 0, "longest")[0] == []


@pytest.mark.parametrize("mode", MODES)
def test_the_plan_on_random_cases(mode):
    rng = np.random.default_rng(47)
    for trial in range(120):
        n = int(rng.integers(1, 12))
        rec_len = rng.integers(0, 60, n)
        tr = []
        for _ in range(int(rng.integers(0, 40))):
            r = int(rng.integers(0, n))
            e = int(rng.integers(0, rec_len[r] + 1))
            tr.append((r, int(rng.integers(max(0, e - 9), e + 1)), e))
        for min_len in (0, 1, int(rng.integers(2, 12)), 1000):
            same_plan(sorted(tr), rec_len, min_len, mode)
        same_plan(tr, rec_len, 3, mode)                              # ... and any order


def test_the_plan_refuses():
    api.spans_cut_plan(SP.as_spans([(0, 2, 5), (1, 3, 8)]), [10, 8])
    for tr, rec_len, mode in (([(0, 6, 5)], [10], "split"),           # beg > end
                              ([(0, 2, 5), (1, 3, 9)], [10, 8], "split"),      # end beyond the record
                              ([(0, 2, 5), (1, 3, 6)], [10], "split"),         # a record that is not there
                              ([(0, 2, 5)], [10], 3), ([(0, 2, 5)], [10], -1)):
        with pytest.raises(L.DexGPUError) as e:
            api.spans_cut_plan(SP.as_spans(tr), rec_len, 0, mode)
        assert e.value.code == E_ARG, (tr, rec_len, mode)
    lib, n, sel = L.load(), C.c_uint64(7), [C.c_void_p() for _ in range(3)]
    one = SP.as_spans([(0, 2, 5)])
    rl = np.array([10], np.uint32)
    assert lib.dx_spans_cut_plan(None, 1, rl.ctypes.data, 1, 0, 0, *[C.byref(a) for a in sel], C.byref(n), None) == E_ARG and n.value == 0
    assert lib.dx_spans_cut_plan(one.ctypes.data, 1, None, 1, 0, 0, *[C.byref(a) for a in sel], C.byref(n), None) == E_ARG
    assert lib.dx_spans_cut_plan(one.ctypes.data, 1, rl.ctypes.data, 1, 0, 0, None, C.byref(sel[1]), C.byref(sel[2]), C.byref(n), None) == E_ARG
    assert all(a.value is None for a in sel)
