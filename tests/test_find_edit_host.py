"""dx_file_find_edit's host side (no GPU): the two new entry points are declared, exported and bound; calls without a context are
argument errors; and the oracle of the GPU tests -- tests/_find_edit.py: the plain DP column, the valley rule, and an independent
bit-vector implementation -- is valid on its own: the DP equals the bit-vector, a column restarted m + k symbols in front of an end
has min(D, k + 1) there (what the kernel's stretches rest on), and it finds in ta_edge and ta_small what was counted by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _find as F
import _find_edit as E
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_code_find_edit", "dx_file_find_edit"]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("code_find_edit", "find_edit"):
        assert callable(getattr(api.Context, m))
    assert C.sizeof(L.EQuery) == 24 and [getattr(L.EQuery, f).offset for f in ("code", "len", "max_err")] == [0, 16, 20]
    assert int(re.search(r"#define\s+DX_FIND_EDIT_STRETCH\s+(\d+)u", hdr).group(1)) == 128


def test_no_context_is_an_argument_error():
    lib = L.load()
    img = O.golden("ta_small.dexta")
    q, fd, hits, bad = (L.EQuery * 1)(api.equery([0], 0)), L.Find(), C.c_uint64(), C.c_uint64()
    pats = (C.c_char_p * 1)(b"ACGT")
    assert lib.dx_code_find_edit(None, None, 0, None, None, None, 0, q, 1, None, None, 0, None, C.byref(hits), C.byref(bad)) == -1
    assert lib.dx_file_find_edit(None, L.DX_KIND_FASTA, img, len(img), pats, 1, 0, 0, 0, C.byref(fd), None, None) == -1


def test_the_query_layout():
    """the first symbol on top of code[0], symbol 32 on top of code[1], unused bits 0"""
    q = api.equery([1, 2, 3], 1)
    assert (q.code[0], q.code[1], q.len, q.max_err) == (0b011011 << 58, 0, 3, 1)
    q = api.equery([3] * 32 + [2, 1], 5)
    assert (q.code[0], q.code[1], q.len, q.max_err) == ((1 << 64) - 1, 0b1001 << 60, 34, 5)


# ---- the statement against itself ------------------------------------------------------------------------------------------------------
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


def some_text(rng, L, q):
    """L random codes, in two of three cases with a copy of q under up to three edits somewhere"""
    s = rng.integers(0, 4, L).astype(np.uint8)
    if rng.integers(3) and L:
        w = mutated(rng, q, int(rng.integers(4)))
        at = int(rng.integers(0, L))
        s[at:at + len(w)] = w[:L - at]
    return s


def test_the_dp_equals_the_bit_vector():
    """m 1 .. 64, L 0 .. 300: the DP column, the recurrence on Python ints and the same on numpy words give one D"""
    rng = np.random.default_rng(1)
    for trial in range(320):
        m = trial % 64 + 1
        q = rng.integers(0, 4, m).astype(np.uint8)
        s = some_text(rng, int(rng.integers(0, 301)), q)
        d = E.dp(s, [q])[0]
        assert d.tolist() == E.bitvector(s, q)
        assert (E.bitvector_many(s, [q, q[:(m + 1) // 2]]) == np.stack([d, E.dp(s, [q[:(m + 1) // 2]])[0]])).all()


def test_every_bound_for_small_patterns():
    """m 1 .. 6 and every k < m: the hits of the valley rule are the same from either D, and obey the rule's three clauses"""
    rng = np.random.default_rng(2)
    for m in range(1, 7):
        q = rng.integers(0, 4, m).astype(np.uint8)
        s = some_text(rng, 200, q)
        d = E.dp(s, [q])[0]
        for k in range(m):
            e, mis = E.valleys(d, k)
            e2, mis2 = E.valleys(E.bitvector(s, q), k)
            assert e.tolist() == e2.tolist() and mis.tolist() == mis2.tolist()
            pos, _, mis3 = E.unit_hits(np.stack([d, d]), [k, k])                    # (the rule for many queries at once, as search() applies it)
            assert pos.tolist() == np.repeat(e, 2).tolist() and mis3.tolist() == np.repeat(mis, 2).tolist()
            c = [k + 1] + [min(int(x), k + 1) for x in d] + [k + 1]
            assert e.tolist() == [i for i in range(1, 201) if c[i] <= k and c[i] < c[i - 1] and c[i] <= c[i + 1]]
            assert len(e) == 0 or e.min() >= m - k                # (D(e) >= m - e: a unit shorter than m - k has no hit)


def stretch_hits(s, q, k, S):
    """the hits as a kernel finds them that cuts the ends into stretches [e0, e1) of S: a standard column begun at symbol
    max(0, e0 - 1 - (m + k)), stepped through symbol e1 (none behind the unit's end), only the ends of the stretch classified"""
    m, L, out = len(q), len(s), []
    for e0 in range(1, L + 1, S):
        e1 = min(e0 + S, L + 1)
        st, t = max(0, e0 - 1 - (m + k)), min(e1, L)
        d = E.bitvector(s[st:t], q)
        c = lambda e: k + 1 if e <= st or e == L + 1 else min(d[e - st - 1], k + 1)       # (e <= st is asked for e = 0 alone)
        out += [(e, c(e)) for e in range(e0, e1) if c(e) <= k and c(e) < c(e - 1) and c(e) <= c(e + 1)]
    return out


def test_the_restart_property():
    """DP against restarted DP: for every end e, a column begun m + k symbols in front of it has min(D, k + 1) at e; and the stretches
    built on it give the hits of the whole scan for any stretch size, the kernel's among them"""
    rng = np.random.default_rng(3)
    for trial in range(300):
        m = int(rng.integers(1, 24))
        k = int(rng.integers(0, m))
        q = rng.integers(0, 4, m).astype(np.uint8)
        s = some_text(rng, int(rng.integers(0, 400)), q)
        d = E.dp(s, [q])[0]
        for e in rng.integers(1, len(s) + 1, 8 if len(s) else 0):
            st = max(0, int(e) - (m + k))
            assert min(E.dp(s[st:e], [q])[0][-1], k + 1) == min(d[e - 1], k + 1)
        e, mis = E.valleys(d, k)
        for S in (1, 7, 128):
            assert stretch_hits(s, q, k, S) == list(zip(e.tolist(), mis.tolist())), (trial, m, k, S)


# ---- the goldens, counted by hand ------------------------------------------------------------------------------------------------------
def test_the_reference_finds_what_was_counted_by_hand_in_ta_edge():
    """ta_edge's reads as undexta -U prints them: ACGTA, none, ACGTACG, GT, TTTT, C, AAAAAA, ACGT x 43 + G (173), T x 80.
    k = 0.  ACGTAC: read 2 ends at 6; read 7 at 6, 10 .. 170 (a copy begins at 4 j and needs 4 j + 6 <= 172): 42.  TTTT: read 4 ends at
      4; in read 8 D is 0 at every end from 4 on, which is ONE valley, reported at the leftmost end of its floor: 4.
    k = 1.  ACGTAC: read 0, ACGTA, is the pattern less its last letter: end 5, distance 1 (end 4, ACGT, is 2 away).  Read 2: D(5) = 1,
      D(6) = 0, D(7) = 1: one valley, at 6.  Read 7: D runs 0, 1, 2, 1 with period 4, the valleys where it did for k = 0; behind 170
      come 1, 2 and (ACGTG) 2.  TTTT: read 4: D(3) = 1 > D(4) = 0: the valley is at 4; read 8 again 4; GT and C are 3 away."""
    text = F.text_of("fasta", O.golden("ta_edge.dexta"))
    rep, lst = E.file_find_edit("fasta", text, ["ACGTAC", "TTTT"])
    assert (rep["records"], rep["records_hit"], rep["hits"], rep["listed"]) == (9, 4, 45, 45)
    assert rep["per_pattern"].tolist() == [[43, 0], [2, 0]] and rep["rec_hits"].tolist() == [0, 0, 1, 0, 1, 0, 0, 42, 1]
    assert [tuple(int(v) for v in h) for h in lst[:4]] == [(2, 6, 0, 0, 0), (4, 4, 1, 0, 0), (7, 6, 0, 0, 0), (7, 10, 0, 0, 0)]
    assert tuple(int(v) for v in lst[-1]) == (8, 4, 1, 0, 0) and tuple(int(v) for v in lst[-2]) == (7, 170, 0, 0, 0)
    rep, lst = E.file_find_edit("fasta", text, ["ACGTAC", "TTTT"], max_err=1)
    assert rep["per_pattern"].tolist() == [[44, 0], [2, 0]] and rep["rec_hits"].tolist() == [1, 0, 1, 0, 1, 0, 0, 42, 1]
    assert [tuple(int(v) for v in h) for h in lst[:4]] == [(0, 5, 0, 0, 1), (2, 6, 0, 0, 0), (4, 4, 1, 0, 0), (7, 6, 0, 0, 0)]
    rep, lst = E.file_find_edit("fasta", text, ["GATC", "ACGTT"], max_err=1)      # ACGT + one letter missing: ends 4, 8 .. in every ACGT run
    assert rep["per_pattern"].tolist() == [[0, 0], [45, 0]] and rep["rec_hits"].tolist() == [1, 0, 1, 0, 0, 0, 0, 43, 0]
    assert E.file_find_edit("fasta", text, ["GATC", "ACGTT"])[0]["hits"] == 0
    rep, lst = E.file_find_edit("fasta", text, ["ACGTAC"], max_hits=5)
    assert (rep["hits"], rep["listed"], len(lst)) == (43, 5, 5) and [int(h["pos"]) for h in lst] == [6, 6, 10, 14, 18]


def test_the_reference_finds_what_was_counted_in_ta_small():
    """derived once with the DP from ta_small's text, record by record, and written down; for k = 0 the counts are those of a text
    search (tests/test_find_host.py has GATC 34, ACGTT 8)"""
    text = F.text_of("fasta", O.golden("ta_small.dexta"))
    rep, lst = E.file_find_edit("fasta", text, ["GATC", "ACGTT"])
    assert rep["per_pattern"][:, 0].tolist() == [34, 8] and rep["rec_hits"].tolist() == [4, 1, 4, 2, 7, 4, 4, 2, 5, 4, 0, 5]
    assert [(int(h["record"]), int(h["pos"])) for h in lst[:5]] == [(0, 50), (0, 78), (0, 241), (0, 783), (1, 84)]
    rep, lst = E.file_find_edit("fasta", text, ["GATC", "ACGTT"], max_err=1)
    assert rep["per_pattern"][:, 0].tolist() == [780, 221] and rep["hits"] == 1001 and rep["records_hit"] == 12
    assert rep["rec_hits"].tolist() == [109, 65, 68, 54, 107, 91, 86, 53, 123, 75, 70, 100]
    assert [(int(h["pos"]), int(h["mis"])) for h in lst[:7]] == [(10, 1), (15, 1), (31, 1), (50, 0), (53, 1), (67, 1), (78, 0)]
    rep, _ = E.file_find_edit("fasta", text, ["ACGTAC", "TTTT"])
    assert rep["per_pattern"][:, 0].tolist() == [4, 25] and rep["rec_hits"].tolist() == [4, 3, 3, 1, 4, 3, 2, 2, 2, 2, 0, 3]
    rep, _ = E.file_find_edit("fasta", text, ["ACGTAC", "TTTT"], max_err=1)
    assert rep["per_pattern"][:, 0].tolist() == [91, 299] and rep["rec_hits"].tolist() == [33, 23, 27, 15, 37, 36, 29, 21, 56, 38, 32, 43]


@pytest.mark.parametrize("name", ["ta_edge", "ta_small"])
def test_with_no_error_allowed_the_hits_are_finds_moved_by_m(name):
    """k = 0: c is 0 or 1, and two ends in a row with D = 0 would make the pattern its own shift by one, a single letter repeated.  So
    for every other pattern -- those that overlap themselves at a longer period too, ACGTACGT among them -- each end with D = 0 is
    its own valley, and the hits are exactly find's exact hits with pos_edit = pos_find + m.  A run of one letter is ONE valley: of
    find's hits of TTTT in it only the first is reported."""
    text = F.text_of("fasta", O.golden(name + ".dexta"))
    pats = ["GATC", "ACGT", "ACGTACGT", "TTTTCC", "CAAAC", "TA", "GGCC"]
    for both in (False, True):
        want, wl = F.file_find("fasta", text, pats, both_strands=both)
        got, gl = E.file_find_edit("fasta", text, pats, both_strands=both)
        assert want["hits"] == got["hits"] > 0 and (want["per_pattern"] == got["per_pattern"]).all() and (want["rec_hits"] == got["rec_hits"]).all()
        moved = wl.copy()
        moved["pos"] += np.array([len(pats[q]) for q in wl["query"]], np.uint32)
        key = lambda a: sorted(tuple(int(v) for v in h) for h in a)
        assert key(moved) == key(gl)
    runs, _ = F.file_find("fasta", text, ["TTTT"])
    once, ol = E.file_find_edit("fasta", text, ["TTTT"])
    assert 0 < once["hits"] <= runs["hits"] and (name != "ta_edge" or (once["hits"], runs["hits"]) == (2, 78))
