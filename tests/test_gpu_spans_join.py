"""Context.spans_join (dx_spans_join) on the GPU against the plain loop of tests/_spans.py, on synthetic lists: gaps at and one beyond
max_gap, min_span at and one beyond a joined length, runs that cross a tile's seam, one joined span of 10^5 entries, records of one
span each, a record change with a small numeric gap, the cap, every kind of bad list, and the same bytes on two calls.  Behind the
output stand guard entries.  No expected value comes from the library."""
import numpy as np
import pytest

import _spans as SP
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3
TILE = 2048           # SJ_TILE of csrc/screen/dx_screen_spans.hip: entries a workgroup
GUARD = 4
MARK = 0xC0DEC0DE
ALL = 2 ** 32 - 1


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def run(ctx, lst, max_gap, min_span, cap=None):
    """one call against the loop: the kept spans as far as they were listed, and the totals"""
    want, tot = SP.join(lst, max_gap, min_span)
    assert SP.first_bad(lst) is None
    cap = len(lst) if cap is None else cap
    d_in = ctx.to_device(lst) if len(lst) else None
    d_out = ctx.alloc(16 * (cap + GUARD)).upload(np.full(4 * (cap + GUARD), MARK, np.uint32))
    try:
        totals, got = ctx.spans_join(d_in, max_gap, min_span, cap=cap, n=len(lst), out=d_out if cap else None)
        raw = d_out.download(np.uint32, 4 * (cap + GUARD))
    finally:
        for x in (d_in, d_out):
            if x is not None:
                x.free()
    listed = min(cap, len(want))
    assert totals.tolist() == tot, (totals, tot, max_gap, min_span)
    assert (raw[4 * listed:] == MARK).all(), "a span was written at cap or beyond, or behind the last"
    assert len(got) == listed and got.tobytes() == raw[:4 * listed].tobytes()
    diff = np.flatnonzero(got != want[:listed])
    assert len(diff) == 0, (max_gap, min_span, cap, [(int(j), tuple(got[j]), tuple(want[j])) for j in diff[:5]])
    return got, totals


def random_list(seed, n, records, gaps=(1, 2, 3, 5, 9, 40)):
    """n spans over about `records` records, in order: lengths 1 to 60, gaps from the given few values, so that many lie at a bound"""
    rng = np.random.default_rng(seed)
    rec = np.sort(rng.integers(0, records, n)).astype(np.uint64) * 3          # (not every record number occurs)
    ln = rng.integers(1, 61, n)
    gap = rng.choice(gaps, n)
    out = np.zeros(n, SP.SPAN)
    at, last = 0, None
    for i in range(n):
        if rec[i] != last:
            at, last = int(rng.integers(0, 4)), rec[i]                         # (a record's first beg is small: less than the end before it)
        else:
            at += int(gap[i])
        out[i] = (rec[i], at, at + int(ln[i]))
        at += int(ln[i])
    return out


def test_gaps_at_and_beyond_max_gap_and_min_span_at_and_beyond_a_length(ctx):
    lst = random_list(1, 5000, 300)
    assert len(lst) > 2 * TILE
    for max_gap in (0, 1, 2, 3, 4, 5, 8, 9, 39, 40, ALL):
        got, totals = run(ctx, lst, max_gap, 0)
    assert len(got) == len(np.unique(lst["record"]))                          # max_gap UINT32_MAX: one span a record
    assert len(run(ctx, lst, 0, 0)[0]) == len(lst)                            # (no gap is 0: nothing joins)
    joined = SP.join(lst, 5, 0)[0]
    ln = int(np.median(joined["end"].astype(np.int64) - joined["beg"]))
    a, b = run(ctx, lst, 5, ln)[1], run(ctx, lst, 5, ln + 1)[1]
    assert a[0] > b[0] > 0                                                    # a joined span of exactly ln symbols stays, then goes
    run(ctx, lst, 5, ALL)
    # touching spans: a gap of 0 joins under every max_gap
    touch = SP.as_spans([(7, 0, 5), (7, 5, 9), (7, 10, 12)])
    assert [tuple(int(v) for v in x) for x in run(ctx, touch, 0, 0)[0]] == [(7, 0, 9), (7, 10, 12)]


def test_runs_that_cross_a_tile_seam_and_records_of_one_span(ctx):
    # runs of 3 to 700 entries with gaps of 1, apart by gaps of 50: heads at irregular places of every tile, runs across every seam
    rng = np.random.default_rng(5)
    tr, at = [], 0
    while len(tr) < 4 * TILE + 100:
        for _ in range(int(rng.integers(3, 700))):
            tr.append((2, at, at + 3))
            at += 4
        at += 49
    lst = SP.as_spans(tr)
    assert any(lst["beg"][t * TILE] - lst["end"][t * TILE - 1] == 1 for t in range(1, 4))       # a run goes on across a seam
    got, totals = run(ctx, lst, 1, 0)
    assert 10 < len(got) < len(lst) // 3
    run(ctx, lst, 1, 500)
    run(ctx, lst, 0, 0)
    one_each = SP.as_spans([(r, 5, 30) for r in range(3 * TILE + 7)])
    assert len(run(ctx, one_each, ALL, 0)[0]) == len(one_each)
    assert len(run(ctx, one_each, ALL, 26)[0]) == 0
    # a head exactly at a tile's first and last place
    i = np.arange(2 * TILE + 5, dtype=np.int64)
    edge = np.zeros(len(i), SP.SPAN)
    edge["beg"] = 4 * i + 50 * ((i >= TILE - 1).astype(np.int64) + (i >= TILE) + (i >= 2 * TILE))
    edge["end"] = edge["beg"] + 3
    assert [int(x["beg"]) for x in run(ctx, edge, 1, 0)[0]] == [0, 4 * (TILE - 1) + 50, 4 * TILE + 100, 8 * TILE + 150]


def test_one_joined_span_of_100000_entries(ctx):
    n = 100000
    i = np.arange(n, dtype=np.int64)
    lst = np.zeros(n + 2, SP.SPAN)
    lst["record"][:n + 1], lst["beg"][1:n + 1], lst["end"][1:n + 1] = 4, 100 + 10 * i, 108 + 10 * i
    lst[0] = (4, 0, 50)                                                        # 50 symbols in front: a span of its own
    lst[n + 1] = (5, 3, 9)                                                     # ... and the next record
    assert n // TILE >= 48
    got, totals = run(ctx, lst, 2, 0)
    assert [tuple(int(v) for v in x) for x in got] == [(4, 0, 50), (4, 100, 10 * n + 98), (5, 3, 9)]
    assert len(run(ctx, lst, 2, 51)[0]) == 1


def test_one_joined_span_whose_end_lies_more_than_256_tiles_away(ctx):
    """the search of the tiles that follow takes 256 of them a step: this span's next head is found in its second step"""
    n, pre = 257 * TILE + 3, TILE // 2 + 5                                     # (the span begins in the middle of a tile)
    i = np.arange(n, dtype=np.int64)
    lst = np.zeros(pre + n + 3, SP.SPAN)
    lst["record"][:pre], lst["beg"][:pre], lst["end"][:pre] = 3, 20 * np.arange(pre), 20 * np.arange(pre) + 7     # gaps of 13: none joins
    lst["record"][pre:pre + n], lst["beg"][pre:pre + n], lst["end"][pre:pre + n] = 4, 100 + 6 * i, 104 + 6 * i    # gaps of 2: all join
    lst[pre + n:] = [(5, 3, 9), (5, 12, 20), (5, 30, 32)]
    got, totals = run(ctx, lst, 2, 0)
    assert len(got) == pre + 4 and tuple(int(v) for v in got[pre]) == (4, 100, 6 * n + 98)
    assert [tuple(int(v) for v in x) for x in got[pre + 1:]] == [(5, 3, 9), (5, 12, 20), (5, 30, 32)]


def test_a_record_change_with_a_small_numeric_gap_does_not_join(ctx):
    lst = SP.as_spans([(0, 0, 10), (1, 11, 20), (1, 21, 30), (2, 0, 5), (2 ** 40, 6, 8), (2 ** 40 + 1, 9, 10)])
    got, _ = run(ctx, lst, 5, 0)
    assert [tuple(int(v) for v in x) for x in got] == [(0, 0, 10), (1, 11, 30), (2, 0, 5), (2 ** 40, 6, 8), (2 ** 40 + 1, 9, 10)]
    got, _ = run(ctx, lst, ALL, 0)
    assert len(got) == 5


def test_the_cap_and_no_spans(ctx):
    lst = random_list(3, 3 * TILE + 11, 40)
    kept = len(SP.join(lst, 3, 4)[0])
    assert kept > TILE
    for cap in (0, 1, kept // 2, TILE, kept - 1, kept, kept + 3):
        got, totals = run(ctx, lst, 3, 4, cap=cap)
        assert totals[0] == kept and len(got) == min(cap, kept)
    got, totals = run(ctx, lst[:0], 3, 4, cap=5)
    assert len(got) == 0 and totals.tolist() == [0, 0]
    totals, got = ctx.spans_join(lst, 3, 4)                                    # a host array: uploaded there, room for all
    assert totals[0] == kept == len(got) and got.tobytes() == SP.join(lst, 3, 4)[0].tobytes()


def test_every_kind_of_bad_list_with_its_index(ctx):
    lst = random_list(4, 2 * TILE + 50, 30)
    same = np.flatnonzero(lst["record"][1:] == lst["record"][:-1]) + 1         # entries that follow one of their record
    for i in (0, 1, int(same[same > TILE][0]), 2 * TILE, len(lst) - 1):
        bad = lst.copy()
        bad["end"][i] = bad["beg"][i]                                          # no symbol
        assert SP.first_bad(bad) == i
        with pytest.raises(L.DexGPUError) as e:
            ctx.spans_join(bad, 3, 0)
        assert e.value.code == E_FORMAT and e.value.bad_unit == i
    for i in (int(same[0]), int(same[same > TILE][3]), int(same[-1])):
        bad = lst.copy()
        bad["beg"][i] = bad["end"][i - 1] - 1                                  # it begins inside the span in front of it
        assert SP.first_bad(bad) == i
        with pytest.raises(L.DexGPUError) as e:
            ctx.spans_join(bad, 3, 0, cap=0)
        assert e.value.code == E_FORMAT and e.value.bad_unit == i
    change = np.flatnonzero(lst["record"][1:] != lst["record"][:-1]) + 1
    for i in (int(change[1]), int(change[-1])):
        bad = lst.copy()
        bad["record"][i:] = np.where(bad["record"][i:] == bad["record"][i], bad["record"][i - 1] - 1, bad["record"][i:])     # the records decrease
        assert SP.first_bad(bad) == i
        with pytest.raises(L.DexGPUError) as e:
            ctx.spans_join(bad, 3, 0)
        assert e.value.code == E_FORMAT and e.value.bad_unit == i
    bad = lst.copy()
    bad["end"][77] = bad["beg"][77]
    bad["end"][TILE + 9] = 0
    with pytest.raises(L.DexGPUError) as e:
        ctx.spans_join(bad, 3, 0)
    assert e.value.bad_unit == 77                                              # the smallest of two


def test_two_calls_give_the_same_bytes_and_the_refusals(ctx):
    lst = random_list(6, 3 * TILE, 100)
    a, b = run(ctx, lst, 3, 10), run(ctx, lst, 3, 10)
    assert len(a[0]) > 100 and a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()
    d = ctx.alloc(4096).zero()
    tot = (api.C.c_uint64 * 2)(7, 7)
    f = ctx.lib.dx_spans_join
    try:
        assert f(ctx.h, d.ptr, 4, 0, 0, d.ptr + 1024, 4, None, None) == E_ARG                              # no totals
        assert f(ctx.h, None, 4, 0, 0, d.ptr + 1024, 4, api.C.byref(tot), None) == E_ARG and list(tot) == [0, 0]
        assert f(ctx.h, d.ptr, 4, 0, 0, None, 4, api.C.byref(tot), None) == E_ARG                           # a cap and no list
        assert f(ctx.h, d.ptr, 4, 0, 0, d.ptr + 32, 4, api.C.byref(tot), None) == E_ARG                     # d_out overlaps d_in
        assert f(ctx.h, d.ptr, 4, 0, 0, d.ptr + 1024, 1 << 32, api.C.byref(tot), None) == E_ARG
        assert f(ctx.h, d.ptr, 1 << 36, 0, 0, d.ptr + 1024, 4, api.C.byref(tot), None) == E_ARG
        assert f(ctx.h, d.ptr + 4, 4, 0, 0, d.ptr + 1024, 4, api.C.byref(tot), None) == E_ARG               # not aligned
        assert f(ctx.h, None, 0, 0, 0, None, 0, api.C.byref(tot), None) == 0                                # no spans: nothing to do
    finally:
        d.free()
