"""dx_code_find_edit followed by dx_code_hit_starts on the GPU against the statement (tests/_find_span.py: the plain DP over every s of
the window, the largest s that reaches the distance): patterns around the two word sizes with every bound up to 12, every phase of a
unit's first symbol, units that are the buffer's first and last bytes, hits at a unit's first and last symbols, the pattern's missing
prefix planted just in front of d_beg, overlapping and repeated units, duplicate queries, ends across the search kernel's stretches, an
empty list, and every kind of bad hit.  Everything that is NOT a unit (the bytes around it, the pad bits of its last byte) is 0xFF unless a
test plants something there.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_edit as E
import _find_span as P
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

STRETCH = 128                     # include/dexgpu.h: DX_FIND_EDIT_STRETCH (tests/test_find_edit_host.py asserts the figure)
E_ARG, E_FORMAT = -1, -3          # DX_E_*
GUARD = 0xA5A5A5A5                # the word behind d_start[n_hits]
NONE = P.NONE


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


class Buffer:
    """a packed buffer that grows unit by unit.  add(codes, phase, front): the unit's read begins at a byte offset = phase (mod 4) and
    has the codes `front` in front of the unit (d_beg = len(front)); around a read every bit is 1 (guard bytes of 0xFF; none: 0)"""
    def __init__(self):
        self.raw, self.boff, self.beg, self.ln = bytearray(), [], [], []

    def add(self, codes, phase=0, front=(), guard=3):
        self.raw += b"\xff" * guard
        if guard:
            self.raw += b"\xff" * ((phase - len(self.raw)) % 4)
        self.boff.append(len(self.raw)); self.beg.append(len(front)); self.ln.append(len(codes))
        self.raw += F.pack(np.concatenate([np.asarray(front, np.uint8), np.asarray(codes, np.uint8)]).astype(np.uint8), pad=0xFF)

    def packed(self, guard=3):
        return bytes(self.raw) + b"\xff" * guard


def mutate(rng, q, edits):
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


def hit_bytes(lst):
    return np.ascontiguousarray(lst, dtype=api.HIT_DTYPE).view(np.uint8)


def starts_of(ctx, packed, boff, beg, ln, queries, d_list, n_hits):
    """dx_code_hit_starts over hits that stand on the device -> (the starts or the error, the word behind them)"""
    n = len(ln)
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array(boff, np.uint64)),
            ctx.to_device(np.array(beg if beg is not None else [0] * n, np.uint32)), ctx.to_device(np.array(ln, np.uint32)),
            ctx.to_device(np.full(n_hits + 1, GUARD, np.uint32))]
    try:
        try:
            got = ctx.code_hit_starts(bufs[0], len(packed), bufs[1], bufs[2] if beg is not None else None, bufs[3], n, queries,
                                      d_list, n_hits, d_start=bufs[4])
        except L.DexGPUError as e:
            got = e
        raw = bufs[4].download(np.uint32, n_hits + 1)
    finally:
        for x in bufs:
            x.free()
    assert raw[n_hits] == GUARD, "the word behind the last start is written"
    if not isinstance(got, Exception):
        assert np.array_equal(got, raw[:n_hits])
    return got, raw[:n_hits]


def run(ctx, packed, boff, beg, ln, queries):
    """dx_code_find_edit, then dx_code_hit_starts on the list as it stands on the device, both against the statement"""
    n = len(ln)
    want = E.code_find_edit(packed, boff, beg, ln, queries, cap=1 << 40, fast=True)["list"]
    cap = len(want) + 3
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array(boff, np.uint64)),
            ctx.to_device(np.array(beg if beg is not None else [0] * n, np.uint32)), ctx.to_device(np.array(ln, np.uint32)),
            ctx.to_device(np.full(16 * (cap + 2), 0xEE, np.uint8))]
    try:
        rep, lst = ctx.code_find_edit(bufs[0], len(packed), bufs[1], bufs[2] if beg is not None else None, bufs[3], n, queries,
                                      cap=cap, d_hits=bufs[4])
        assert rep["hits"] == len(want) == len(lst) and (lst == want).all()
        got, _ = starts_of(ctx, packed, boff, beg, ln, queries, bufs[4], len(lst))
    finally:
        for x in bufs:
            x.free()
    assert not isinstance(got, Exception), got
    ref = P.code_hit_starts(packed, boff, beg, ln, queries, want)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, [(tuple(int(v) for v in want[i]), int(got[i]), int(ref[i])) for i in bad[:8]]
    return want, ref


# ---- patterns around the word sizes, every bound -----------------------------------------------------------------------------------------
def planted(m, k, seed):
    """Twelve units and the query.  Copies of the query under up to k random edits: in the middle of units at every phase of d_boff
    (odd bytes among them) and of d_beg; at a unit's very first symbols, with the query's missing head planted in the symbols in front
    of d_beg; at a unit's very last symbols; in a unit that is the buffer's first bytes and one that is its last (no guard bytes)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 4, m).astype(np.uint8)
    b = Buffer()

    def text(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    def plant(x, at, w):
        w = w[:len(x) - at]
        x[at:at + len(w)] = w
        return x

    x = plant(text(m + 40), 3, mutate(rng, q, k))                  # the buffer's first bytes: reads backwards reach byte 0
    b.add(x, guard=0)
    for phase in range(4):
        for nb in range(2):
            front = text(4 * nb + (phase + nb) % 4 + 1)             # d_beg = 1 .. 8: every d_beg mod 4, at every phase of d_boff
            x = plant(text(2 * m + 70 + phase), int(rng.integers(m + 12, m + 40)), mutate(rng, q, int(rng.integers(0, k + 1))))
            b.add(x, phase=phase, front=front)
    # the query's tail at the unit's first symbols, its head just in front of d_beg: a scan that ignored the unit's start would
    # find the whole query there
    cut = max(1, min(k, m - 1))
    x = plant(text(m + 30), 0, list(q[cut:]) if m > 1 else list(q))
    b.add(x, phase=1, front=list(text(5)) + list(q[:cut]))
    x = text(m + 50)
    w = mutate(rng, q, k // 2)
    b.add(plant(x, len(x) - len(w), w), phase=3, front=text(2))    # at the unit's very last symbols: e = L
    x = plant(text(m + 45), 30, mutate(rng, q, k))                 # the buffer's last bytes: the query itself at their end, and in
    x = plant(x, len(x) - m, list(q))                              # front of it a symbol that lets no copy end one symbol earlier
    x[len(x) - m - 1] = (int(q[0]) + 1) % 4
    b.add(x, phase=2)
    return b, q


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 63, 64])
def test_every_bound_at_every_phase(ctx, m):
    seen = set()
    for k in range(0, min(m - 1, 12) + 1):
        b, q = planted(m, k, 100 * m + k)
        assert {o % 4 for o in b.boff} == {0, 1, 2, 3} and {g % 4 for g in b.beg} == {0, 1, 2, 3} and b.boff[0] == 0
        packed = b.packed(guard=0)
        assert b.boff[-1] + (b.beg[-1] + b.ln[-1] + 3) // 4 == len(packed)          # the last unit is the buffer's last bytes
        want, ref = run(ctx, packed, b.boff, b.beg, b.ln, [(q, k)])
        by_unit = {}
        for h, s in zip(want, ref):
            by_unit.setdefault(int(h["record"]), []).append((int(s), int(h["pos"]), int(h["mis"])))
        assert set(by_unit) >= set(range(len(b.ln))) - ({9} if k == 0 and m > 1 else set()), sorted(by_unit)
        assert (b.ln[11] - m, b.ln[11], 0) in by_unit[11]           # e = L
        if m >= 31 and k >= 1:                                      # the tail alone, from the unit's first symbol: e < m, s = 0
            cut = max(1, min(k, m - 1))
            assert (0, m - cut, cut) in by_unit[9], by_unit[9][:4]
        seen |= {("s0", s == 0) for v in by_unit.values() for s, _, _ in v} | {("len", e - s != m) for v in by_unit.values() for s, e, _ in v}
    assert ("s0", True) in seen and (m == 1 or ("len", True) in seen)


def test_a_window_wider_than_a_word(ctx):
    """m = 64, k = 24: a copy with 22 letters inserted is an occurrence of more than 64 symbols, d >= 20"""
    rng = np.random.default_rng(64024)
    q = rng.integers(0, 4, 64).astype(np.uint8)
    w = [int(c) for c in q]
    for i in sorted(rng.choice(63, 22, replace=False).tolist(), reverse=True):
        w.insert(i + 1, (w[i] + 2) % 4)
    b = Buffer()
    for phase, at in ((1, 40), (2, 7), (0, 0)):
        x = rng.integers(0, 4, 220).astype(np.uint8)
        x[at:at + len(w)] = w
        b.add(x, phase=phase, front=rng.integers(0, 4, phase + 2))
    want, ref = run(ctx, b.packed(), b.boff, b.beg, b.ln, [(q, 24), (q[:40], 11)])
    wide = [(int(h["pos"]) - int(s), int(h["mis"])) for h, s in zip(want, ref) if h["query"] == 0]
    assert any(n > 64 and d >= 20 for n, d in wide), wide


def test_mixed_lengths_duplicates_and_overlapping_units(ctx):
    """queries of both word sizes in one list (a wave runs both instances), duplicates among them; the whole read twice, parts of it that
    overlap, from symbols in its middle"""
    rng = np.random.default_rng(77)
    qs = [(rng.integers(0, 4, m).astype(np.uint8), k) for m, k in ((4, 1), (8, 2), (32, 6), (33, 6), (45, 9), (64, 12), (5, 0))]
    qs += [qs[1], qs[4], qs[1]]
    x = rng.integers(0, 4, 1500).astype(np.uint8)
    for i, (q, k) in enumerate(qs[:7]):
        for j in range(3):
            w = mutate(rng, q, int(rng.integers(0, k + 1)))
            at = 40 + 200 * i + 66 * j
            x[at:at + len(w)] = w
    b = Buffer()
    b.add(x, phase=1)
    at = b.boff[0]
    boff, beg, ln = [at, at, at + 10, at, at + 100, at], [0, 0, 3, 500, 1, 0], [1500, 1500, 900, 1000, 1099, 1500]
    want, ref = run(ctx, b.packed(), boff, beg, ln, qs)
    per = np.bincount(want["query"], minlength=len(qs))
    assert (per[:7] > 0).all() and per[1] == per[7] == per[9] and per[4] == per[8]
    first = [s for h, s in zip(want, ref) if h["record"] == 0]
    assert first == [s for h, s in zip(want, ref) if h["record"] == 1] == [s for h, s in zip(want, ref) if h["record"] == 5]


def test_ends_across_the_search_kernels_stretches(ctx):
    """a long unit with a copy ending at every end from 2 STRETCH - 3 to 2 STRETCH + 3 (one a unit) and copies that straddle 3, 4 and 5
    STRETCH in one unit: the list is the search kernel's, whose lanes meet at those ends"""
    rng = np.random.default_rng(78)
    q = rng.integers(0, 4, 20).astype(np.uint8)
    b = Buffer()
    for d in range(-3, 4):
        x = rng.integers(0, 4, 3 * STRETCH + 11).astype(np.uint8)
        w = mutate(rng, q, 2)
        end = 2 * STRETCH + d
        x[end - len(w):end] = w
        b.add(x, phase=d % 4, front=rng.integers(0, 4, d % 3))
    x = rng.integers(0, 4, 6 * STRETCH).astype(np.uint8)
    for mult in (3, 4, 5):
        w = mutate(rng, q, 3)
        x[mult * STRETCH - 9:mult * STRETCH - 9 + len(w)] = w
    b.add(x, phase=3, front=[1])
    want, ref = run(ctx, b.packed(), b.boff, b.beg, b.ln, [(q, 4)])
    ends = {(int(h["record"]), int(h["pos"])) for h in want}
    assert len({e for _, e in ends if abs(e - 2 * STRETCH) <= 5}) >= 5 and sum(r == 7 for r, _ in ends) >= 3


# ---- the list --------------------------------------------------------------------------------------------------------------------------
def some_units(seed=79):
    rng = np.random.default_rng(seed)
    qs = [(rng.integers(0, 4, 5).astype(np.uint8), 1), (rng.integers(0, 4, 40).astype(np.uint8), 5)]
    b = Buffer()
    for n in (90, 300, 0, 140, 61):
        x = rng.integers(0, 4, n).astype(np.uint8)
        if n > 80:
            w = mutate(rng, qs[1][0], 3)
            x[20:20 + len(w)] = w
        b.add(x, phase=int(rng.integers(4)), front=rng.integers(0, 4, int(rng.integers(5))))
    return b, qs


def test_no_hits_launches_nothing(ctx):
    b, qs = some_units()
    d = ctx.to_device(np.zeros(64, np.uint8))
    try:
        got, _ = starts_of(ctx, b.packed(), b.boff, b.beg, b.ln, qs, d, 0)
        assert not isinstance(got, Exception) and len(got) == 0
        assert len(ctx.code_hit_starts(None, 0, None, None, None, 0, qs, None, 0)) == 0
    finally:
        d.free()


def test_bad_hits(ctx):
    """each kind of bad hit among good ones: DX_E_FORMAT, the smallest index, UINT32_MAX in its place, the neighbours' starts right"""
    b, qs = some_units()
    packed = b.packed()
    good = E.code_find_edit(packed, b.boff, b.beg, b.ln, qs, cap=1 << 40)["list"]
    ref = P.code_hit_starts(packed, b.boff, b.beg, b.ln, qs, good)
    assert len(good) >= 12 and (ref != NONE).all()
    long_hit = int(np.flatnonzero(good["query"] == 1)[0])

    def check(lst, boff, bad):
        d = ctx.to_device(hit_bytes(lst))
        try:
            got, raw = starts_of(ctx, packed, boff, b.beg, b.ln, qs, d, len(lst))
        finally:
            d.free()
        want = ref.copy()
        want[bad] = NONE
        if not bad:
            assert not isinstance(got, Exception) and np.array_equal(got, want)
            return
        assert isinstance(got, L.DexGPUError) and got.code == E_FORMAT and got.bad_unit == min(bad), got
        assert np.array_equal(raw, want) and np.array_equal(got.starts, want)

    check(good, b.boff, [])
    for field, value, at in (("record", len(b.ln), 4), ("record", 1 << 40, 4), ("pos", 0, 5), ("pos", None, 2), ("query", len(qs), 7),
                             ("query", 0xFFFF, 7), ("mis", 2, 1), ("mis", 6, long_hit), ("mis", 255, 3)):
        lst = good.copy()
        if field == "pos" and value is None:
            value = b.ln[int(lst[at]["record"])] + 1
        if field == "mis" and value == 2:
            at = int(np.flatnonzero(good["query"] == 0)[1])
        lst[field][at] = value
        check(lst, b.boff, [at])
    # a distance the data does not have at that end: no stretch reaches it
    lst = good.copy()
    at = int(np.flatnonzero((good["query"] == 0) & (good["mis"] == 1))[0])
    lst["mis"][at] = 0
    check(lst, b.boff, [at])
    lst = good.copy()
    lst["pos"][long_hit] -= 17
    lst["mis"][long_hit] = 0
    check(lst, b.boff, [long_hit])
    # several at once: the smallest index is reported
    lst = good.copy()
    lst["pos"][9], lst["query"][3], lst["record"][6] = 0, 99, 1 << 33
    check(lst, b.boff, [3, 6, 9])
    # a unit that does not lie inside the bytes: its hits are bad, and it is not read
    boff = list(b.boff)
    boff[1] = len(packed) - 3
    check(good, boff, np.flatnonzero(good["record"] == 1).tolist())
    boff[1] = len(packed) + 1
    check(good, boff, np.flatnonzero(good["record"] == 1).tolist())


def test_refused_arguments(ctx):
    d = ctx.to_device(np.zeros(64, np.uint8))
    ok = ([0, 1], 1)
    try:
        for qs in ([], [ok] * 65, [([], 0)], [(0, 0, 65, 0)], [([0, 1], 2)], [(1 << 59, 0, 2, 0)], [(0, 1, 32, 0)]):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_hit_starts(d, 16, d, None, d, 1, qs, d, 1, d_start=d)
            assert e.value.code == E_ARG, qs
        for args in ((d, 16, None, None, d, 1, [ok], d, 1), (d, 16, d, None, None, 1, [ok], d, 1), (None, 16, d, None, d, 1, [ok], d, 1),
                     (d, 16, d, None, d, 1, [ok], None, 1), (d, 16, d, None, d, 1 << 31, [ok], d, 1), (d, 16, d, None, d, 1, [ok], d, 1 << 32)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_hit_starts(*args, d_start=d)
            assert e.value.code == E_ARG, args[1:]
    finally:
        d.free()
