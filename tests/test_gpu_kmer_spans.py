"""Context.code_kmer_spans (dx_code_kmer_spans) on the GPU against its numpy statement (tests/_spans.py): the WHOLE list is compared,
every unit's count and the totals with it, and on the same call arguments the invariants against Context.code_kmer_screen -- a unit's
lengths sum to `covered`, its first beg is `first`, its last end `last` + k.  The buffers are tests/_screen.py's: everything that is not a
unit is filled with Ts.  The sets are made of codes taken from chosen positions of the units themselves, so that spans begin at symbol
0, end at the unit's end, end and begin at a chunk's edge and cross the seams of the kernel's three paths.  Behind the list and behind
the counts stand guard entries.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_wide as W
import _screen as S
import _spans as SP
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

KS = [2, 15, 21, 32]
E_ARG, E_FORMAT = -1, -3
T, U = S.T, np.uint64
GUARD = 4             # entries behind the list and behind the counts
MARK = 0xC0DEC0DE
PAD = 8               # bytes of Ts in front of and behind every unit
PATHS = {"lane": 100, "sixteen": 300, "wave": 3 * 4096 + 200}


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def tuples(a):
    return [tuple(int(v) for v in x) for x in a]


def run(ctx, kset, codes, packed, boff, beg, ln, k, canonical=False, in_bytes=None, cap=None, with_count=True, screen=True):
    """one call against the statement: (the list as far as it was made, the counts, the totals, the error or None); cap None: room
    for every span"""
    want, cnt, tot, bad = SP.packed_spans(packed, boff, beg, ln, k, canonical, codes, in_bytes)
    nbytes = len(packed) if in_bytes is None else in_bytes
    n = len(ln)
    cap = len(want) if cap is None else cap
    d_in = ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16)
    d_boff, d_len = ctx.to_device(np.asarray(boff, np.uint64)), ctx.to_device(np.asarray(ln, np.uint32))
    d_beg = ctx.to_device(np.asarray(beg, np.uint32)) if beg is not None else None
    d_cnt = ctx.alloc(4 * (n + GUARD)).upload(np.full(n + GUARD, MARK, np.uint32))
    d_sp = ctx.alloc(16 * (cap + GUARD)).upload(np.full(4 * (cap + GUARD), MARK, np.uint32))
    d_scr = ctx.alloc(16 * (n + 1))
    err = None
    try:
        try:
            totals, lst = ctx.code_kmer_spans(d_in, d_boff, d_beg, d_len, kset, count=d_cnt if with_count else None, cap=cap,
                                              spans=d_sp if cap else None, in_bytes=nbytes, n=n)
        except L.DexGPUError as e:
            err, totals, lst = e, e.totals, None
        raw = d_sp.download(np.uint32, 4 * (cap + GUARD))
        counts = d_cnt.download(np.uint32, n + GUARD)
        scr = None
        if screen and n:
            try:
                stot = ctx.code_kmer_screen(d_in, d_boff, d_beg, d_len, kset, out=d_scr, in_bytes=nbytes, n=n)
            except L.DexGPUError as e:
                stot = e.totals
            scr = d_scr.download(np.uint32, 4 * n).view(S.SCREEN)
    finally:
        for x in (d_in, d_boff, d_len, d_beg, d_cnt, d_sp, d_scr):
            if x is not None:
                x.free()
    listed = min(cap, len(want))
    got = raw[:4 * listed].view(np.uint8).view(SP.SPAN)
    assert (raw[4 * listed:] == MARK).all(), "a span was written at cap or beyond, or behind the last"
    diff = np.flatnonzero(got != want[:listed])
    assert len(diff) == 0, (k, canonical, cap, [(int(j), tuple(got[j]), tuple(want[j])) for j in diff[:5]])
    assert lst is None or (len(lst) == listed and lst.tobytes() == got.tobytes())
    if with_count:
        assert (counts[n:] == MARK).all() and counts[:n].tolist() == cnt.tolist(), (counts[:n].tolist()[:20], cnt.tolist()[:20])
    else:
        assert (counts == MARK).all()
    assert totals.tolist() == tot.tolist(), (totals, tot)                     # (total[0]: every span, listed or not)
    assert (bad is None) == (err is None) and (err is None or (err.code == E_FORMAT and err.bad_unit == bad))
    if scr is not None:
        # the invariants against dx_code_kmer_screen, from the statement's list (which the kernel's was just held against)
        assert int(stot[2]) == int(tot[1]) and int(stot[3]) == int(tot[2])
        for j in range(n):
            mine = want[want["record"] == j]
            assert int(scr[j]["covered"]) == int((mine["end"].astype(np.int64) - mine["beg"]).sum()), j
            if len(mine):
                assert int(scr[j]["first"]) == int(mine["beg"][0]) and int(scr[j]["last"]) + k == int(mine["end"][-1]), j
                assert (mine["end"].astype(np.int64) - mine["beg"] >= k).all() and (mine["beg"][1:] > mine["end"][:-1]).all()
            else:
                assert int(scr[j]["hits"]) == 0
    return got, counts[:n], totals, err


def codes_at(units, pos, k, canonical):
    """the set of the codes of the windows at the chosen positions pos[j] of unit j"""
    out = [W.unit_codes(s, k, canonical)[[p for p in ps if 0 <= p <= len(s) - k]] for s, ps in zip(units, pos) if len(s) >= k]
    return np.unique(np.concatenate(out + [np.zeros(0, U)]))


# ---- every length, phase and d_beg ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_every_length_phase_and_offset(ctx, k, canonical):
    rng, b = np.random.default_rng(500 + k), S.Buffer()
    for n in range(0, 201):
        b.add(rng.integers(0, 4, n), phase=n % 16, beg=(n // 16) % 4, guard=PAD, tail=PAD)
    assert {(o % 16, g) for o, g in zip(b.boff, b.beg)} == {(p, g) for p in range(16) for g in range(4)}
    assert {k - 1, k, k + 1} <= set(b.ln)
    # the first window, the last, one in the middle, and two k + 1 apart
    pos = [[0, len(s) - k, len(s) // 2, len(s) // 3, len(s) // 3 + k + 1] if j % 3 else [len(s) // 2] for j, s in enumerate(b.units)]
    codes = codes_at(b.units, pos, k, canonical)
    with ctx.kmer_set_from_codes(codes, k, canonical) as s:
        got, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
    assert err is None and totals[0] > 100 and (counts[:k] == 0).all()
    if k >= 15:
        assert counts.max() >= 3 and (got["beg"] == 0).sum() > 50 and (got["end"] == np.array(b.ln)[got["record"].astype(int)]).sum() > 50


# ---- the three paths and their seams ---------------------------------------------------------------------------------------------------
def seam_windows(S0, n, k, path):
    """window positions of three units of n symbols whose first is symbol S0[j] of the buffer, by what their spans do at the seams:
    unit 0 has spans that begin at 0, end at len and CROSS a seam, unit 1 spans that END at a chunk's (a step's) last position, unit 2
    spans that BEGIN at a chunk's (a step's) first"""
    c = [64 * (x // 64 + 1) - x for x in S0]                        # the first position of the unit's second chunk
    w = [4096 * (x // 4096 + 1) - x for x in S0]                    # ... of the wave path's second step
    pos = [[0, n - k, c[0] - k // 2], [c[1] - k], [c[2]]]
    if path != "lane":
        pos[0].append(c[0] + 128 - k // 2); pos[1].append(c[1] + 192 - k); pos[2].append(c[2] + 128)
    if path == "wave":
        pos[0] += [w[0] - k // 2, w[0] + 4096 - 1]                   # (a window whose first symbol alone is the step's)
        pos[1] += [w[1] - k, w[1] + 4096 - k]
        pos[2] += [w[2], w[2] + 4096]
    assert all(0 <= p <= n - k for ps in pos for p in ps)
    return pos


@pytest.mark.parametrize("k", [15, 21, 32])
@pytest.mark.parametrize("path", list(PATHS))
def test_spans_at_the_seams_of_every_path(ctx, path, k):
    n = PATHS[path]
    rng, b = np.random.default_rng(n + k), S.Buffer()
    for j in range(3):
        b.add(rng.integers(0, 4, n), phase=5, beg=2, guard=PAD, tail=PAD)
    S0 = [4 * o + g for o, g in zip(b.boff, b.beg)]
    for x in S0:
        chunks = (x + n - 1) // 64 - x // 64 + 1
        assert (chunks > 16) if path == "wave" else (4 < chunks <= 16) if path == "sixteen" else 1 < chunks <= 4      # the path the unit takes
    pos = seam_windows(S0, n, k, path)
    for canonical in (False, True):
        codes = codes_at(b.units, pos, k, canonical)
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        assert err is None
        spans = [[(int(x["beg"]), int(x["end"])) for x in got[got["record"] == j]] for j in range(3)]
        assert all(set(pos[j]) <= {b_ for b_, e_ in spans[j]} for j in (1, 2))         # (every planted window begins a span of its own)
        assert spans[0][0][0] == 0 and spans[0][-1][1] == n
        assert any((S0[0] + b_) % 64 > (S0[0] + e_ - 1) % 64 for b_, e_ in spans[0])       # across a chunk seam
        assert any((S0[1] + e_) % 64 == 0 for b_, e_ in spans[1]) and any((S0[2] + b_) % 64 == 0 for b_, e_ in spans[2])
        if path == "wave":
            assert sum((S0[0] + b_) % 4096 > (S0[0] + e_ - 1) % 4096 for b_, e_ in spans[0]) >= 2       # across a wave-step seam
            assert sum((S0[1] + e_) % 4096 == 0 for b_, e_ in spans[1]) >= 2 and sum((S0[2] + b_) % 4096 == 0 for b_, e_ in spans[2]) >= 2


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("path", list(PATHS))
def test_one_span_over_the_whole_unit_and_the_most_spans_a_unit_can_have(ctx, path, k):
    n = PATHS[path]
    rng = np.random.default_rng(7 * n + k)
    b = S.Buffer().add(rng.integers(0, 4, n), phase=11, beg=1, guard=PAD, tail=PAD)
    for canonical in (False, True):
        codes = np.unique(W.unit_codes(b.units[0], k, canonical))
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        assert err is None and tuples(got) == [(0, 0, n)] and totals.tolist() == [1, n, 1]
        # hit windows k + 1 apart: every gap is one symbol
        at = list(range(0, n - k + 1, k + 1))
        codes = codes_at(b.units, [at], k, canonical)
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        assert err is None and len(got) <= n // (k + 1) + 1
        if np.isin(W.unit_codes(b.units[0], k, canonical), codes).sum() == len(at):           # (no chosen code stands twice in the unit)
            assert tuples(got) == [(0, p, p + k) for p in at] and len(got) == (n - k) // (k + 1) + 1
        else:
            assert k < 21                                             # (k = 2 always; k = 15 by chance in the longest unit)


# ---- the cap ---------------------------------------------------------------------------------------------------------------------------
def some_units(seed, k):
    rng, b = np.random.default_rng(seed), S.Buffer()
    for j, n in enumerate([k, 70, 300, 0, 1100, 5003, k - 1, 257, 64, 2000]):
        b.add(rng.integers(0, 4, n), phase=(3 * j) % 16, beg=j % 4, guard=PAD, tail=PAD)
    return b


def sparse_set(b, k, canonical, every=40):
    """windows `every` apart, and one pair k + 1 apart in every unit that has room"""
    return codes_at(b.units, [list(range(0, len(s), every)) + [len(s) - k, 5, 5 + k + 1] for s in b.units], k, canonical)


@pytest.mark.parametrize("k", [15, 32])
def test_the_cap(ctx, k):
    b = some_units(k, k)
    codes = sparse_set(b, k, True)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        full, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
        total = int(totals[0])
        assert err is None and total == len(full) > 150 and counts[5] > 100
        first5 = int(counts[:5].sum())
        for cap in (0, 1, first5 + int(counts[5]) // 2, first5 + int(counts[5]) // 2 + 1, first5, total - 1, total, total + 5):
            # (in the middle of the wave-path unit's spans, at a unit's edge, exactly the count, beyond it; run holds the sentinels)
            got, _, tt, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True, cap=cap, screen=False)
            assert err is None and int(tt[0]) == total and len(got) == min(cap, total)
        run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True, cap=total // 2, with_count=False, screen=False)     # d_count NULL
        run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True, cap=0, with_count=False, screen=False)


def test_a_cap_that_ends_inside_an_open_span_of_the_wave_path(ctx):
    """spans of the wave path that are open at a step's seam, and caps at them: the span below cap gets its end from the next step"""
    k, n = 21, 3 * 4096 + 200
    rng = np.random.default_rng(77)
    b = S.Buffer().add(rng.integers(0, 4, n), phase=0, beg=0, guard=PAD, tail=PAD)
    S0 = 4 * b.boff[0]
    w1 = 4096 * (S0 // 4096 + 1) - S0
    at = [100, w1 - 10, w1 + 4096 - 5, n - k]
    codes = codes_at(b.units, [at], k, False)
    with ctx.kmer_set_from_codes(codes, k) as s:
        full = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k)[0]
        assert tuples(full) == [(0, p, p + k) for p in at]
        for cap in (1, 2, 3, 4):
            run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, cap=cap, screen=False)


# ---- the set's extremes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 32])
def test_the_empty_set_and_the_set_of_all_codes(ctx, k):
    b = some_units(k + 1, k)
    with ctx.kmer_set_from_codes([], k) as s:
        got, counts, totals, err = run(ctx, s, np.zeros(0, U), b.packed(), b.boff, b.beg, b.ln, k, cap=8)
    assert err is None and totals.tolist() == [0, 0, 0] and len(got) == 0 and (counts == 0).all()
    for canonical in (False, True):
        codes = np.unique(W.all_codes(b.units, k, canonical))
        with ctx.kmer_set_from_codes(codes, k, canonical) as s:
            got, counts, totals, err = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, canonical)
        assert err is None and tuples(got) == [(j, 0, n) for j, n in enumerate(b.ln) if n >= k]
        assert counts.tolist() == [int(n >= k) for n in b.ln]


# ---- the rest --------------------------------------------------------------------------------------------------------------------------
def test_units_that_overlap_and_repeat_no_units_and_whole_reads(ctx):
    rng = np.random.default_rng(9)
    sym = rng.integers(0, 4, 4000)
    packed = F.pack(sym)
    boff = [0, 0, 10, 10, 500, 0, 999, 17, 0]
    beg = [0, 5, 3, 3, 0, 0, 0, 2, 3999]
    ln = [4000, 100, 0, 700, 20, 4000, 4, 2000, 1]
    for k in (2, 16, 21, 32):
        own = W.unit_codes(sym, k, k == 21)
        codes = np.unique(own[::37] if k > 2 else own[:1])
        with ctx.kmer_set_from_codes(codes, k, canonical=k == 21) as s:
            got, counts, totals, err = run(ctx, s, codes, packed, boff, beg, ln, k, canonical=k == 21)
            assert err is None and counts[0] == counts[5] > 0
            a, c = got[got["record"] == 0], got[got["record"] == 5]
            assert a["beg"].tolist() == c["beg"].tolist() and a["end"].tolist() == c["end"].tolist()
            got, counts, totals, err = run(ctx, s, codes, packed, [], [], [], k, canonical=k == 21, cap=4)
            assert err is None and totals.tolist() == [0, 0, 0] and len(got) == 0
            assert run(ctx, s, codes, packed, [0, 10, 500], None, [4000, 0, 900], k, canonical=k == 21)[3] is None      # d_beg NULL


@pytest.mark.parametrize("k", [2, 21, 32])
def test_the_buffers_end_and_a_buffer_shorter_than_a_load(ctx, k):
    rng = np.random.default_rng(40 + k)
    for n in (k, 37, 61, 64, 129, 1030):                          # the unit ends in the buffer's last byte; 37, 61: fewer than 16 bytes
        sym = rng.integers(0, 4, n)
        packed = F.pack(sym, pad=0xff)
        for beg in range(4):
            if n - beg < k:
                continue
            unit = sym[beg:]
            codes = codes_at([unit], [[0, len(unit) - k, len(unit) // 2]], k, k != 21)
            with ctx.kmer_set_from_codes(codes, k, canonical=k != 21) as s:
                got, counts, totals, err = run(ctx, s, codes, packed, [0], [beg], [n - beg], k, k != 21)
            assert err is None and got[0]["beg"] == 0 and got[-1]["end"] == n - beg


@pytest.mark.parametrize("k", [15, 32])
def test_a_bad_unit_in_the_middle(ctx, k):
    rng, b = np.random.default_rng(k), S.Buffer()
    for n in (300, 64, 5003, 90, 700):
        b.add(rng.integers(0, 4, n), beg=2, guard=PAD, tail=PAD)
    codes = sparse_set(b, k, False, every=50)
    nbytes = len(b.packed())
    with ctx.kmer_set_from_codes(codes, k) as s:
        for j, (at, ln) in ((2, (nbytes + 1, 50)), (1, (nbytes - 10, 100)), (3, (0, 0x80000000))):
            boff, lens = list(b.boff), list(b.ln)
            boff[j], lens[j] = at, ln
            got, counts, totals, err = run(ctx, s, codes, b.packed(), boff, b.beg, lens, k)     # (run holds the list, the counts and the totals)
            assert err is not None and err.code == E_FORMAT and err.bad_unit == j
            assert counts[j] == 0 and not (got["record"] == j).any() and totals[2] == 4 and len(got) > 4
        boff = list(b.boff)
        boff[1] = boff[4] = nbytes + 5
        assert run(ctx, s, codes, b.packed(), boff, b.beg, b.ln, k)[3].bad_unit == 1


def test_two_calls_give_the_same_bytes(ctx):
    k, b = 21, some_units(3, 21)
    codes = sparse_set(b, k, True, every=30)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        a = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
        c = run(ctx, s, codes, b.packed(), b.boff, b.beg, b.ln, k, True)
    assert len(a[0]) > 100 and a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes() and a[2].tolist() == c[2].tolist()


def test_refusals(ctx):
    d = ctx.alloc(256).zero()
    tot = (api.C.c_uint64 * 3)(7, 7, 7)
    f = ctx.lib.dx_code_kmer_spans
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_spans(d, d, None, d, None, cap=1, spans=d, in_bytes=16, n=1)                 # no set
        assert e.value.code == E_ARG and "set" in str(e.value)
        with ctx.kmer_set_from_codes([1, 2, 3], 21) as s:
            for args in ((None, d, d), (d, None, d), (d, d, None)):                                   # the buffer, the offsets, the lengths
                with pytest.raises(L.DexGPUError) as e:
                    ctx.code_kmer_spans(args[0], args[1], None, args[2], s, cap=1, spans=d, in_bytes=16, n=1)
                assert e.value.code == E_ARG
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, d.ptr, 1, None, None) == E_ARG            # no totals
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, None, 1, api.C.byref(tot), None) == E_ARG   # a cap and no list
            assert list(tot) == [0, 0, 0]
            tot[0] = 7
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1 << 31, s.h, None, d.ptr, 1, api.C.byref(tot), None) == E_ARG
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, d.ptr, 1 << 32, api.C.byref(tot), None) == E_ARG
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, d.ptr + 4, 1, api.C.byref(tot), None) == E_ARG
            assert list(tot) == [0, 0, 0]
            assert f(ctx.h, d.ptr, 16, d.ptr, None, d.ptr, 1, s.h, None, d.ptr + 64, 1, api.C.byref(tot), None) == 0    # (a unit of length 0)
    finally:
        d.free()
