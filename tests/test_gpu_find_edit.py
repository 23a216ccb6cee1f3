"""dx_code_find_edit on the GPU against its statement (tests/_find_edit.py: the plain DP column and the valley rule; for the long units
the independent bit-vector words), the whole ordered list compared: every unit length from 0 to 700 at every phase of its start with
64 queries that hit everywhere, long units that the wave takes in several steps, long patterns planted under random edits with their
ends on every offset of three of the kernel's stretches, every cap, overlapping and repeated units, duplicate queries, and the
refusals.  Everything that is NOT a unit (the bytes around it, the symbols in front of d_beg, the pad bits of its last byte) is 0xFF.
No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_edit as E
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# include/dexgpu.h: #define DX_FIND_EDIT_STRETCH 128u -- the documented #define is MIRRORED here (tests/test_find_edit_host.py reads the
# header and asserts the figure); csrc/find/dx_find_edit.hip: FE_LANE 4, FE_GROUP 16 stretches, the wave's step 64
STRETCH = 128
LANE, GROUP, STEP = 4 * STRETCH, 16 * STRETCH, 64 * STRETCH
E_ARG, E_FORMAT = -1, -3          # DX_E_*
GUARD = 3                         # bytes of 0xFF around every unit


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


class Buffer:
    """a packed buffer that grows unit by unit; around a unit, in front of its d_beg and in its last byte's pad bits every bit is 1"""
    def __init__(self):
        self.raw, self.boff, self.beg, self.ln = bytearray(), [], [], []

    def add(self, codes, phase=0, beg=0, guard=GUARD):
        """the unit's symbols; phase: (byte offset of its read) mod 4, beg: the symbols of its read in front of it"""
        self.raw += b"\xff" * guard
        self.raw += b"\xff" * ((phase - len(self.raw)) % 4)
        self.boff.append(len(self.raw)); self.beg.append(beg); self.ln.append(len(codes))
        self.raw += F.pack(np.concatenate([np.full(beg, 3, np.uint8), np.asarray(codes, np.uint8)]), pad=0xFF)

    def packed(self):
        return bytes(self.raw) + b"\xff" * GUARD


def run(ctx, packed, boff, beg, ln, queries, cap=None, fast=False, want=None):
    """the call against the reference: every unit's count, the totals, and the list (cap None: room for all and three more)"""
    n = len(ln)
    if want is None:
        want = E.code_find_edit(packed, boff, beg, ln, queries, cap=1 << 40, fast=fast)
    cap = want["hits"] + 3 if cap is None else cap
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array(boff, np.uint64)),
            ctx.to_device(np.array(beg if beg is not None else [0] * n, np.uint32)), ctx.to_device(np.array(ln, np.uint32)), ctx.alloc(4 * n + 4),
            ctx.to_device(np.full(16 * (cap + 2), 0xEE, np.uint8))]
    try:
        rep, lst = ctx.code_find_edit(bufs[0], len(packed), bufs[1], bufs[2] if beg is not None else None, bufs[3], n, queries,
                                      d_count=bufs[4], cap=cap, d_hits=bufs[5])
        count, raw = bufs[4].download(np.uint32, n), bufs[5].download(np.uint8)
        none, _ = ctx.code_find_edit(bufs[0], len(packed), bufs[1], bufs[2] if beg is not None else None, bufs[3], n, queries)
    finally:
        for x in bufs:
            x.free()
    bad = np.flatnonzero(count != want["count"])
    assert len(bad) == 0, [(int(j), ln[j], boff[j] % 4, int(count[j]), int(want["count"][j])) for j in bad[:8]]
    assert rep["hits"] == want["hits"] == none["hits"] and np.array_equal(rep["total"], want["total"]) and np.array_equal(none["total"], want["total"])
    k = min(cap, want["hits"])
    assert len(lst) == k and (lst == want["list"][:k]).all(), [(a, w) for a, w in zip(lst, want["list"]) if a != w][:5]
    assert (raw[16 * k:] == 0xEE).all(), "a byte behind the list's end is written"
    return want


def queries_8_3(rng, nq=64):
    return [(rng.integers(0, 4, 8).astype(np.uint8), 3) for _ in range(nq)]


# ---- every small shape -----------------------------------------------------------------------------------------------------------------
def test_every_small_shape(ctx):
    """every unit length 0 .. 700 (a lane's unit up to 512, a group's beyond, stretch ends at 128, 256 ...), all four phases of d_boff
    and d_beg 0 .. 5 among them, 64 queries of m = 8, k = 3 at once: hits on every position, so on every stretch and class boundary"""
    rng = np.random.default_rng(11)
    b = Buffer()
    for n in range(701):
        b.add(rng.integers(0, 4, n), phase=n % 4, beg=(n // 4 + n // 24) % 6)
    assert {(o % 4, g) for o, g in zip(b.boff, b.beg)} == {(p, g) for p in range(4) for g in range(6)}
    want = run(ctx, b.packed(), b.boff, b.beg, b.ln, queries_8_3(rng))
    assert want["hits"] > 64 * sum(b.ln) // 30 and len(set(want["list"]["pos"].tolist())) >= 690     # (about every end from 5 on carries a hit somewhere)


def test_without_d_beg_and_a_buffer_of_fewer_than_16_bytes(ctx):
    rng = np.random.default_rng(12)
    b = Buffer()
    for n in (0, 1, 5, 127, 128, 129, 700):
        b.add(rng.integers(0, 4, n), phase=int(rng.integers(4)))
    run(ctx, b.packed(), b.boff, None, b.ln, queries_8_3(rng, 5))
    for n in (1, 4, 5, 13, 30):                                   # the whole buffer is the unit: nothing around it
        s = rng.integers(0, 4, n).astype(np.uint8)
        q = [(s[:min(n, 3)].copy(), 0), (np.array([1, 2], np.uint8), 1)]
        want = run(ctx, F.pack(s, pad=0xFF), [0], None, [n], q)
        assert want["total"][0] >= 1


# ---- long units ------------------------------------------------------------------------------------------------------------------------
def test_long_units(ctx):
    """two random units of about 40 000 and 70 000 symbols: the wave class takes 5 and 9 steps; the same 64 queries, the full list
    (the reference by the bit-vector words)"""
    rng = np.random.default_rng(13)
    b = Buffer()
    b.add(rng.integers(0, 4, 5 * STEP - 1000 + 3), phase=1, beg=2)
    b.add(rng.integers(0, 4, 40), phase=3)
    b.add(rng.integers(0, 4, 8 * STEP + 4537), phase=2, beg=5)
    want = run(ctx, b.packed(), b.boff, b.beg, b.ln, queries_8_3(rng), fast=True)
    assert want["hits"] > 64 * 100000 // 20


# ---- long patterns ---------------------------------------------------------------------------------------------------------------------
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


def planted(m, k):
    """copies of a pattern of m symbols under up to k random edits, far enough apart not to disturb each other (more than 2 (m + k)):
    in one long unit (the wave's, 13 steps) their ends at 1000 + 257 i, i < 3 x STRETCH -- 257 = 2 STRETCH + 1: every offset of a
    stretch three times over, on 384 different stretches --, one more copy at the unit's very first and one at its very last symbols;
    and one copy a unit with its end on every offset of a stretch in STRETCH units of the group's class and STRETCH of a lane's
    -> (the buffer, the query, the (unit, end) of every copy)"""
    rng = np.random.default_rng(1000 * m + k)
    q = rng.integers(0, 4, m).astype(np.uint8)
    b, ends = Buffer(), []

    def plant(x, end):
        w = mutate(rng, q, int(rng.integers(0, k + 1)))
        x[end - len(w):end] = w
        ends.append((len(b.ln), end))

    x = rng.integers(0, 4, 1000 + 257 * 3 * STRETCH + 333).astype(np.uint8)
    for i in range(3 * STRETCH):
        plant(x, 1000 + 257 * i)
    w = mutate(rng, q, min(k, 1))
    x[:len(w)] = w
    plant(x, len(x))
    b.add(x, phase=3, beg=1)
    for i in range(STRETCH):
        x = rng.integers(0, 4, LANE + 2 * STRETCH + 50 + i % 7).astype(np.uint8)        # the group's: its end in the unit's fourth stretch
        plant(x, 3 * STRETCH + 7 + i)
        b.add(x, phase=i % 4, beg=i % 6)
        x = rng.integers(0, 4, 2 * STRETCH + 40 + i).astype(np.uint8)                   # a lane's: in its first and second
        plant(x, STRETCH - 40 + i)
        b.add(x, phase=(i + 1) % 4, beg=(i + 2) % 6)
    return b, q, ends


def check_planted(want, ends, k):
    """a planted copy is within k of the pattern, so c <= k at its end: a valley's floor lies there or close by"""
    found = {}
    for h in want["list"]:
        found.setdefault(int(h["record"]), []).append(int(h["pos"]))
    lost = [(j, end) for j, end in ends if not any(abs(p - end) <= 2 * k + 1 for p in found.get(j, []))]
    assert not lost, lost[:5]
    assert {e % STRETCH for j, e in ends if j == 0} == set(range(STRETCH)) == {e % STRETCH for j, e in ends if j and j % 2}
    assert min(found[0]) <= 64 + 16 + 1 and want["hits"] >= len(ends) + 1       # (the copy at the unit's first symbols ends within m + k of them)


@pytest.mark.parametrize("m", [31, 32, 33, 45, 63, 64])
def test_long_patterns_planted(ctx, m):
    """m around the word sizes, k = 0, 1, 5 and m / 4 (random text has no such hits: they are planted, see planted()); the reference
    by the bit-vector on Python ints"""
    for k in sorted({0, 1, 5, m // 4}):
        b, q, ends = planted(m, k)
        assert b.ln[0] > 12 * STEP and LANE < b.ln[1] <= GROUP and b.ln[2] <= LANE
        want = run(ctx, b.packed(), b.boff, b.beg, b.ln, [(q, k)], fast=True)
        check_planted(want, ends, k)


def test_mixed_lengths_in_one_call(ctx):
    """queries of both word sizes side by side, 1 to 64 symbols, bounds from 0 to m - 1"""
    rng = np.random.default_rng(14)
    qs = [(rng.integers(0, 4, m).astype(np.uint8), k) for m, k in ((1, 0), (2, 1), (5, 4), (16, 2), (32, 3), (33, 3), (45, 9), (64, 16), (64, 63), (7, 0))]
    b = Buffer()
    for n in (3, 60, LANE + 9, GROUP + 200):
        x = rng.integers(0, 4, n).astype(np.uint8)
        for q, k in qs[3:8]:
            if n > 2 * len(q):
                w = mutate(rng, q, k // 2)
                at = int(rng.integers(0, n - len(w)))
                x[at:at + len(w)] = w
        b.add(x, phase=int(rng.integers(4)), beg=int(rng.integers(6)))
    want = run(ctx, b.packed(), b.boff, b.beg, b.ln, qs, fast=True)
    assert (want["total"][[0, 3, 4, 5, 6, 7]] > 0).all()


# ---- the list --------------------------------------------------------------------------------------------------------------------------
def test_the_cap_and_the_sentinel(ctx):
    """cap 0, 1, a few in the middle of a unit, hits - 1, hits, hits + 1: the first cap hits, element for element, and not a byte behind
    them -- with many hits in every class (a lane's unit, a group's, the wave's over two steps)"""
    rng = np.random.default_rng(15)
    b = Buffer()
    for n in (40, 0, 7 * STRETCH + 3, STEP + 300, 9, 3 * STRETCH):
        b.add(rng.integers(0, 4, n), phase=int(rng.integers(4)), beg=int(rng.integers(6)))
    qs = queries_8_3(rng, 6)
    want = run(ctx, b.packed(), b.boff, b.beg, b.ln, qs, fast=True)
    hits = want["hits"]
    assert hits > 3000
    for cap in (0, 1, 30, hits // 2, hits - 1, hits, hits + 1):
        run(ctx, b.packed(), b.boff, b.beg, b.ln, qs, cap=cap, want=want)


# ---- units and queries -----------------------------------------------------------------------------------------------------------------
def test_overlapping_and_repeated_units_and_duplicate_queries(ctx):
    rng = np.random.default_rng(16)
    b = Buffer()
    b.add(rng.integers(0, 4, 3000), phase=2)
    at = b.boff[0]
    boff = [at, at, at + 10, at, at + 100, at]                    # the whole read twice, parts of it that overlap, the whole again
    beg = [0, 0, 3, 500, 1, 0]
    ln = [3000, 3000, 900, 2500, 2599, 3000]
    qs = queries_8_3(rng, 4)
    qs += [qs[0], qs[2], qs[0]]
    want = run(ctx, b.packed(), boff, beg, ln, qs)
    assert want["total"][0] == want["total"][4] == want["total"][6] > 0 and want["count"][0] == want["count"][1] == want["count"][5]


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_units_and_no_units(ctx):
    """units that do not lie inside the buffer are refused by the bounds check: DX_E_FORMAT with the smallest of them, no hits of
    their own, the others searched"""
    rng = np.random.default_rng(17)
    b = Buffer()
    for n in (50, 300, 5000, 20, 70):
        b.add(rng.integers(0, 4, n), phase=int(rng.integers(4)))
    packed, n = b.packed(), len(b.ln)
    qs = queries_8_3(rng, 3)
    good = E.code_find_edit(packed, b.boff, None, b.ln, qs)["count"]
    boff, ln = np.array(b.boff, np.uint64), np.array(b.ln, np.uint32)
    boff[3] = len(packed) + 1                                      # begins behind the buffer
    ln[1] = 4 * (len(packed) - b.boff[1]) + 1                      # ends one symbol behind it
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(boff), ctx.to_device(ln), ctx.to_device(np.full(n, 77, np.uint32))]
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_find_edit(bufs[0], len(packed), bufs[1], None, bufs[2], n, qs, d_count=bufs[3], cap=100)
        assert e.value.code == E_FORMAT and e.value.bad_unit == 1
        assert bufs[3].download(np.uint32, n).tolist() == [good[0], 0, good[2], 0, good[4]] and good[2] > 0
        rep, lst = ctx.code_find_edit(bufs[0], len(packed), bufs[1], None, bufs[2], 0, qs, d_count=bufs[3], cap=100)
        assert rep["hits"] == 0 and rep["total"].tolist() == [0, 0, 0] and len(lst) == 0
    finally:
        for x in bufs:
            x.free()


def test_refused_arguments(ctx):
    d = ctx.to_device(np.zeros(64, np.uint8))
    ok = ([0, 1], 1)
    try:
        for qs in ([], [ok] * 65, [([], 0)], [(0, 0, 65, 0)], [([0, 1], 2)], [([0], 1)], [(1 << 59, 0, 2, 0)], [(0, 1, 32, 0)],
                   [((1 << 64) - 1, 1 << 61, 33, 0)], [(0, 3, 63, 0)]):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_find_edit(d, 16, d, None, d, 1, qs)
            assert e.value.code == E_ARG, qs
        for args, kw in (((d, 16, None, None, d, 1, [ok]), {}), ((d, 16, d, None, None, 1, [ok]), {}), ((None, 16, d, None, d, 1, [ok]), {}),
                         ((d, 16, d, None, d, 1 << 31, [ok]), {}), ((d, 16, d, None, d, 1, [ok]), {"cap": 1 << 32, "d_hits": d})):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_find_edit(*args, **kw)
            assert e.value.code == E_ARG, (args[1:], kw)
        assert ctx.code_find_edit(d, 16, d, None, d, 1, [((1 << 64) - 1, (1 << 64) - 1, 64, 0)])[0]["hits"] == 0      # (all bits used: 64 t)
    finally:
        d.free()
