"""The host side of dx_code_hit_starts, dx_file_find_edit_spans, dx_hits_cut_plan and dx_file_cut (no GPU): the four entry points are
declared, exported and bound; calls without a context are argument errors; the statement of the GPU tests -- tests/_find_span.py: the
start by the plain DP over every s of the window -- is held against a second, independent formulation, the backward bit-vector scan on
Python ints; dx_hits_cut_plan is held against the plan in plain Python; and both find in ta_edge and ta_small what was counted by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _find_edit as E
import _find_span as P
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_hit_starts", "dx_file_find_edit_spans", "dx_hits_cut_plan", "dx_file_cut"]
E_ARG = -1


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("code_hit_starts", "find_spans", "cut"):
        assert callable(getattr(api.Context, m))
    assert callable(api.cut_plan)
    assert C.sizeof(L.Cut) == 56 and [f for f, _ in L.Cut._fields_] == ["records_in", "records_cut", "records_dropped", "pieces",
                                                                        "symbols_in", "symbols_kept", "spans"]
    for name, v in (("DX_CUT_SPLIT", 0), ("DX_CUT_LONGEST", 1), ("DX_CUT_DROP", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == v == getattr(L, name)


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    q, fd, bad = (L.EQuery * 1)(api.equery([0], 0)), L.Find(), C.c_uint64()
    pats = (C.c_char_p * 1)(b"ACGT")
    lst, st, out, ln = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert lib.dx_code_hit_starts(None, None, 0, None, None, None, 0, q, 1, None, 0, None, C.byref(bad)) == E_ARG
    assert lib.dx_file_find_edit_spans(None, L.DX_KIND_FASTA, img, len(img), pats, 1, 0, 0, 0, C.byref(fd), C.byref(lst), None,
                                       C.byref(st), None) == E_ARG
    assert lib.dx_file_cut(None, L.DX_KIND_FASTA, img, len(img), pats, 1, 0, 0, 0, 0, C.byref(out), C.byref(ln), None, None, None, None,
                           None) == E_ARG
    assert lib.dx_hits_cut_plan(None, None, 0, None, 0, 0, 0, None, None, None, None, None) == E_ARG


# ---- the start: the statement against the backward bit-vector --------------------------------------------------------------------------
def mutated(rng, q, edits):
    w = [int(c) for c in q]
    for _ in range(edits):
        op, i = int(rng.integers(3)), int(rng.integers(len(w)))
        if op == 0:
            w[i] = (w[i] + 1 + int(rng.integers(3))) % 4
        elif op == 1:
            w.insert(i, int(rng.integers(4)))
        elif len(w) > 1:
            del w[i]
    return w


def planted_cases():
    """(unit, query, k): a copy of the query under up to k random edits in a short random unit -- at its very start in one case of four,
    at its very end in another --, m around the word sizes and small"""
    rng = np.random.default_rng(41)
    for trial in range(400):
        m = (1, 2, 3, 5, 8, 20, 32, 33, 45, 64)[trial % 10]
        k = int(rng.integers(0, min(m - 1, 11) + 1))
        q = rng.integers(0, 4, m).astype(np.uint8)
        # (a low-entropy query now and then: runs make several s reach the distance)
        if trial % 7 == 0:
            q = rng.integers(0, 2, m).astype(np.uint8) * 3
        u = rng.integers(0, 4, int(rng.integers(m + 12, m + 90))).astype(np.uint8)      # (room for the copy with up to 11 insertions)
        w = mutated(rng, q, int(rng.integers(0, k + 1)))
        at = {0: 0, 1: max(0, len(u) - len(w))}.get(trial % 4, int(rng.integers(0, len(u) - len(w) + 1)))
        u[at:at + len(w)] = w[:len(u) - at]
        yield u, q, k


def test_the_statement_equals_the_backward_bit_vector():
    """every hit of every planted case: the largest s of the plain DP is the first step of the backward scan that scores d.  The case
    set, BY THE STATEMENT ALONE, holds hits with several s that reach d, hits whose length is not m, and hits with s = 0."""
    hits = several = other_len = at_zero = wide = 0
    for u, q, k in planted_cases():
        e, mis = E.valleys(E.dp(u, [q])[0], k)
        for end, d in zip(e.tolist(), mis.tolist()):
            r = P.reaching(u, end, q, d)
            assert r, "D(e) is the minimum over s: some s reaches it"
            s = P.start_of(u, end, q, d)
            assert s == r[-1] and abs((end - s) - len(q)) <= d
            assert P.backward_bitvector(u, end, q, d) == s, (len(q), k, end, d, r)
            hits += 1; several += len(r) > 1; other_len += end - s != len(q); at_zero += s == 0; wide += end - s > 64
    assert hits >= 400 and several >= 20 and other_len >= 20 and at_zero >= 20 and wide >= 1, (hits, several, other_len, at_zero, wide)


def test_the_tie_counted_by_hand():
    """P = GAC, U = TTAC, e = 4, d = 1: TAC (s = 1, a substitution) and AC (s = 2, a deletion) both lie 1 from GAC; TTAC lies 2.  The
    answer is the shortest stretch: s = 2."""
    u, p = F.pattern_codes("fasta", "TTAC"), F.pattern_codes("fasta", "GAC")
    assert E.dp(u, [p])[0].tolist()[-1] == 1
    assert P.levenshtein(p, [u[0:], u[1:], u[2:], u[3:], u[4:]]).tolist() == [2, 1, 1, 2, 3]
    assert P.reaching(u, 4, p, 1) == [1, 2] and P.start_of(u, 4, p, 1) == 2 == P.backward_bitvector(u, 4, p, 1)
    assert P.start_of(u, 4, p, 0) == P.NONE == P.backward_bitvector(u, 4, p, 0)       # (a distance that no stretch has)


def test_levenshtein_on_known_pairs():
    c = lambda s: F.pattern_codes("fasta", s)
    assert P.levenshtein(c("ACGT"), [c("ACGT"), c("AGT"), c("ACGGT"), c("TGCA"), [], c("A")]).tolist() == [0, 1, 1, 4, 4, 3]
    assert P.levenshtein(c("GATTACA"), [c("GCATGC")]).tolist() == [4]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
MODES = ("split", "longest", "drop")


def same_plan(records, pos, starts, rec_len, min_len, mode):
    want_units, want_rep = P.plan(records, pos, starts, rec_len, min_len, mode)
    hits = np.zeros(len(pos), api.HIT_DTYPE)
    hits["record"], hits["pos"] = records, pos
    sel, rep = api.cut_plan(hits, starts, rec_len, min_len, mode)
    got = list(zip(sel["ids"].tolist(), sel["beg"].tolist(), sel["end"].tolist()))
    assert got == want_units, (mode, min_len, got[:6], want_units[:6])
    assert rep == want_rep, (rep, want_rep)
    assert all(a <= b for a, b in zip(sel["ids"][:-1].tolist(), sel["ids"][1:].tolist()))
    return want_units, want_rep


def test_the_plan_on_cases_made_by_hand():
    rec_len = [30, 0, 12, 40, 7, 20]
    #          record 0: two spans that touch, one nested in the first, one apart; 2: a span over the whole record; 3: hits of two
    #          patterns interleaved, given by pos (not by start); 4, 1: none; 5: spans at both ends
    hits = [(0, 2, 8), (0, 8, 12), (0, 3, 5), (0, 20, 25), (2, 0, 12), (3, 18, 22), (3, 5, 23), (3, 30, 31), (3, 10, 31), (5, 0, 4), (5, 15, 20)]
    r, s, e = (np.array(x) for x in zip(*hits))
    units, rep = same_plan(r, e, s, rec_len, 0, "split")
    assert units == [(0, 0, 2), (0, 12, 20), (0, 25, 30), (1, 0, 0), (3, 0, 5), (3, 31, 40), (4, 0, 7), (5, 4, 15)]
    assert rep == dict(records_in=6, records_cut=3, records_dropped=1, pieces=8, symbols_in=109, symbols_kept=47, spans=6)
    assert same_plan(r, e, s, rec_len, 1, "split")[0] == units                      # (a piece has one symbol at least: 0 and 1 are one)
    units, rep = same_plan(r, e, s, rec_len, 6, "split")
    assert units == [(0, 12, 20), (1, 0, 0), (3, 31, 40), (4, 0, 7), (5, 4, 15)] and rep["records_dropped"] == 1 and rep["records_cut"] == 3
    units, rep = same_plan(r, e, s, rec_len, 0, "longest")
    assert units == [(0, 12, 20), (1, 0, 0), (3, 31, 40), (4, 0, 7), (5, 4, 15)]
    units, rep = same_plan(r, e, s, rec_len, 1000, "longest")
    assert units == [(1, 0, 0), (4, 0, 7)] and rep["records_dropped"] == 4            # (a record without a hit: whole, whatever min_len is)
    units, rep = same_plan(r, e, s, rec_len, 0, "drop")
    assert units == [(1, 0, 0), (4, 0, 7)] and rep == dict(records_in=6, records_cut=0, records_dropped=4, pieces=2, symbols_in=109,
                                                           symbols_kept=7, spans=6)
    # the first of two pieces of one length
    assert same_plan([0, 0], [7, 20], [5, 12], [25], 0, "longest")[0] == [(0, 0, 5)]
    assert same_plan([0, 0], [7, 20], [5, 12], [25], 0, "split")[0] == [(0, 0, 5), (0, 7, 12), (0, 20, 25)]
    # no hits at all, no records at all
    assert same_plan([], [], [], [3, 0, 9], 5, "split")[0] == [(0, 0, 3), (1, 0, 0), (2, 0, 9)]
    assert same_plan([], [], [], [], 0, "longest")[0] == []


@pytest.mark.parametrize("mode", MODES)
def test_the_plan_on_random_cases(mode):
    rng = np.random.default_rng(43)
    for trial in range(120):
        n = int(rng.integers(1, 12))
        rec_len = rng.integers(0, 60, n)
        nh = int(rng.integers(0, 40))
        r = rng.integers(0, n, nh)
        e = np.array([int(rng.integers(0, rec_len[j] + 1)) for j in r], np.int64)
        s = np.array([int(rng.integers(max(0, x - 9), x + 1)) for x in e], np.int64)
        order = np.lexsort((e, r))                                  # the list's order: (record, pos)
        for min_len in (0, 1, int(rng.integers(2, 12)), 1000):
            same_plan(r[order], e[order], s[order], rec_len, min_len, mode)
        same_plan(r, e, s, rec_len, 3, mode)                        # ... and any order


def test_the_plan_refuses():
    hits = np.zeros(2, api.HIT_DTYPE)
    hits["record"], hits["pos"] = [0, 1], [5, 6]
    ok = ([2, 3], [10, 8])
    api.cut_plan(hits, *ok)
    for start, rec_len, mode in (([6, 3], [10, 8], "split"),        # start > pos
                                 ([2, P.NONE], [10, 8], "split"),   # a bad hit's start
                                 ([2, 3], [10, 5], "split"),        # pos beyond the record
                                 ([2, 3], [10], "split"),           # a record that is not there
                                 ([2, 3], [10, 8], 3), ([2, 3], [10, 8], -1)):
        with pytest.raises(L.DexGPUError) as e:
            api.cut_plan(hits, start, rec_len, 0, mode)
        assert e.value.code == E_ARG, (start, rec_len, mode)


# ---- the goldens, counted by hand ------------------------------------------------------------------------------------------------------
def test_ta_edge_counted_by_hand():
    """ta_edge's reads: ACGTA, none, ACGTACG, GT, TTTT, C, AAAAAA, ACGT x 43 + G (173), T x 80; tests/test_find_edit_host.py counts the
    hits of ACGTAC and TTTT in them.  k = 0: a hit's occurrence is the m symbols in front of its end.  Read 2: [0, 6) of 7.  Read 4:
    [0, 4), the whole read.  Read 7: ends 6, 10 .. 170, the spans [0, 6), [4, 10) .. [164, 170) overlap into ONE, [0, 170) of 173.
    Read 8: one valley, [0, 4) of 80."""
    text = F.text_of("fasta", O.golden("ta_edge.dexta"))
    rep, lst = P.file_find_spans("fasta", text, ["ACGTAC", "TTTT"])
    assert rep["hits"] == 45 and rep["rec_len"].tolist() == [5, 0, 7, 2, 4, 1, 6, 173, 80]
    assert (rep["start"] == lst["pos"] - np.where(lst["query"] == 0, 6, 4)).all()
    units, cut = same_plan(lst["record"], lst["pos"], rep["start"], rep["rec_len"], 0, "split")
    assert units == [(0, 0, 5), (1, 0, 0), (2, 6, 7), (3, 0, 2), (5, 0, 1), (6, 0, 6), (7, 170, 173), (8, 4, 80)]
    assert cut == dict(records_in=9, records_cut=3, records_dropped=1, pieces=8, symbols_in=278, symbols_kept=94, spans=4)
    assert same_plan(lst["record"], lst["pos"], rep["start"], rep["rec_len"], 2, "split")[0] == \
        [(0, 0, 5), (1, 0, 0), (3, 0, 2), (5, 0, 1), (6, 0, 6), (7, 170, 173), (8, 4, 80)]
    assert same_plan(lst["record"], lst["pos"], rep["start"], rep["rec_len"], 0, "drop")[0] == [(0, 0, 5), (1, 0, 0), (3, 0, 2), (5, 0, 1), (6, 0, 6)]
    # k = 1: read 0, ACGTA, is the pattern less its last letter, end 5, distance 1: CGTA is 2 away, so the occurrence is the whole read
    rep, lst = P.file_find_spans("fasta", text, ["ACGTAC", "TTTT"], max_err=1)
    assert tuple(int(v) for v in lst[0]) == (0, 5, 0, 0, 1) and rep["start"][0] == 0 and rep["hits"] == 46
    units, cut = same_plan(lst["record"], lst["pos"], rep["start"], rep["rec_len"], 0, "split")
    assert units[0] == (1, 0, 0) and cut["records_dropped"] == 2


def test_ta_small_counted():
    """GATC 34 and ACGTT 8 exact hits (tests/test_find_edit_host.py, tests/test_find_host.py): with no error allowed a start is its end
    less the pattern's length, two hits never touch here, and record 10 has none"""
    text = F.text_of("fasta", O.golden("ta_small.dexta"))
    rep, lst = P.file_find_spans("fasta", text, ["GATC", "ACGTT"])
    assert rep["hits"] == 42 and (rep["start"] == lst["pos"] - np.where(lst["query"] == 0, 4, 5)).all()
    units, cut = same_plan(lst["record"], lst["pos"], rep["start"], rep["rec_len"], 0, "split")
    assert cut["spans"] == 42 and cut["records_cut"] == 11 and cut["records_dropped"] == 0 and cut["records_in"] == 12
    assert cut["symbols_kept"] == cut["symbols_in"] - 34 * 4 - 8 * 5 and (10, 0, int(rep["rec_len"][10])) in units
    assert units[:2] == [(0, 0, 46), (0, 50, 74)]                  # (the first hits end at 50 and 78)
