"""dx_code_find on the GPU against its numpy statement (tests/_find.py), on the smallest shapes that can go wrong: every query length
around the one-word cut, every unit length around a chunk, the wave's step and the cuts between the kernel's three paths, every
phase of a unit's start, its first symbol and its end, windows planted on both sides of every chunk and step boundary -- and
everything that is NOT a unit (the guard bytes around it, the symbols in front of d_beg, the pad bits of its last byte) filled with
the query itself, laid so that a window that reaches outside the unit completes a match and shows as a wrong count.  No expected
value comes from the library."""
import numpy as np
import pytest

import _find as F
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# csrc/find/dx_find.hip
CHUNK = 64            # FD_CHUNK: positions of one 16-byte chunk, which stands on a 16-byte boundary of the BUFFER
LANE = 4 * CHUNK      # FD_LANE: a unit of up to four chunks is its lane's, chunk after chunk
GROUP = 16 * CHUNK    # FD_GROUP: up to 16 chunks 16 lanes take the unit, beyond the wave
STEP = 64 * CHUNK     # FD_STEP: what the wave takes of a long unit a step
NARROW = 16           # FD_NARROW: a query up to here is decided by the window's upper word
QLENS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32]
CUTS = [CHUNK, LANE, GROUP, STEP, 2 * STEP]
LENGTHS = sorted({c + d for c in CUTS for d in (-1, 0, 1)})       # (at phase 0 a unit of c symbols ends with the chunk, the group, the step)
assert all({c - 1, c, c + 1} <= set(LENGTHS) for c in CUTS) and {NARROW - 1, NARROW, NARROW + 1} <= set(QLENS)
E_ARG, E_FORMAT = -1, -3          # DX_E_*
GUARD = 9             # bytes around every unit: more than the 31 symbols a window can reach beyond its first


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def some_query(rng, m):
    """m codes that are no repetition of a shorter word (so that only whole, planted copies match exactly), or one code for m == 1"""
    while True:
        q = rng.integers(0, 4, m).astype(np.uint8)
        if m == 1 or not any(np.array_equal(q, np.roll(q, s)) for s in range(1, m)):
            return q


class Buffer:
    """a packed buffer that grows unit by unit.  Around a unit everything is `fill`, the query, repeated: in front of the unit so that
    the repetition's symbol 0 is the LAST symbol in front of it, behind it so that it goes on with the query's last symbol -- a unit
    that begins with fill[1:] or ends with fill[:-1] has a match that reaches outside by one symbol, on either side."""
    def __init__(self, fill):
        self.fill, self.sym, self.boff, self.beg, self.ln = np.asarray(fill, np.uint8), [], [], [], []
        self.n = 0                                                 # symbols so far (4 a byte)

    def _front(self, k):
        m = len(self.fill)
        return self.fill[(np.arange(-k, 0) + 1) % m]

    def _tail(self, k):
        m = len(self.fill)
        return self.fill[(np.arange(k) + m - 1) % m]

    def add(self, codes, phase=None, beg=0, guard=GUARD, tail=GUARD):
        """the unit's symbols; phase: (byte offset of its read) mod 16, beg: the symbols of its read in front of it"""
        assert self.n % 4 == 0
        at = self.n // 4 + guard
        if phase is not None:
            at += (phase - at) % 16
        front = 4 * (at - self.n // 4) + beg
        codes = np.asarray(codes, np.uint8)
        end = self.n + front + len(codes)
        self.sym += [self._front(front), codes, self._tail((-end) % 4 + 4 * tail)]
        self.boff.append(at); self.beg.append(beg); self.ln.append(len(codes))
        self.n = end + (-end) % 4 + 4 * tail

    def packed(self):
        return F.pack(np.concatenate(self.sym)) if self.sym else b""


def unit(rng, n, q, how):
    """n random codes with the query planted: "first", "last", "every" (the query repeated; for one symbol every position hits),
    "over" (the unit begins with q[1:] and ends with q[:-1]: with the fill around it two matches that reach outside)"""
    m, x = len(q), rng.integers(0, 4, n).astype(np.uint8)
    if how == "first" and n >= m:
        x[:m] = q
    if how == "last" and n >= m:
        x[n - m:] = q
    if how == "every":
        x = np.resize(q, n) if n else x
    if how == "over" and n >= m - 1 and m > 1:
        x[n - (m - 1):] = q[:-1]
        x[:m - 1] = q[1:]
    return x


def run(ctx, b, queries, cap=None, beg=True):
    """the call against the reference: every unit's count, the totals, and the list (cap None: room for all and three more)"""
    packed, n = b.packed(), len(b.ln)
    want = F.code_find(packed, b.boff, b.beg if beg else None, b.ln, queries, cap=1 << 40)
    cap = want["hits"] + 3 if cap is None else cap
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(np.array(b.boff, np.uint64)),
            ctx.to_device(np.array(b.beg, np.uint32)), ctx.to_device(np.array(b.ln, np.uint32)), ctx.alloc(4 * n + 4),
            ctx.to_device(np.full(16 * (cap + 2), 0xEE, np.uint8))]
    try:
        rep, lst = ctx.code_find(bufs[0], len(packed), bufs[1], bufs[2] if beg else None, bufs[3], n, [F.query(q, mm) for q, mm in queries],
                                 d_count=bufs[4], cap=cap, d_hits=bufs[5])
        count, raw = bufs[4].download(np.uint32, n), bufs[5].download(np.uint8)
        none, _ = ctx.code_find(bufs[0], len(packed), bufs[1], bufs[2] if beg else None, bufs[3], n, [F.query(q, mm) for q, mm in queries])
    finally:
        for x in bufs:
            x.free()
    bad = np.flatnonzero(count != want["count"])
    assert len(bad) == 0, [(int(j), b.ln[j], b.boff[j] % 16, b.beg[j], int(count[j]), int(want["count"][j])) for j in bad[:8]]
    assert rep["hits"] == want["hits"] == none["hits"] and np.array_equal(rep["total"], want["total"]) and np.array_equal(none["total"], want["total"])
    k = min(cap, want["hits"])
    assert len(lst) == k and (lst == want["list"][:k]).all(), [(a, w) for a, w in zip(lst, want["list"]) if a != w][:5]
    assert (raw[16 * k:] == 0xEE).all(), "a byte behind the list's end is written"
    return want


# ---- lengths, paths, plants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", QLENS)
def test_lengths_and_planted_hits(ctx, m):
    """every length around every cut, at phase 0 (where the cuts are exact) and at a random phase; 0, m - 1, m, m + 1; a unit at the
    buffer's first byte and one that ends with its last byte; nothing, the first window, the last, every window, and windows that
    would match if they reached outside"""
    rng = np.random.default_rng(m)
    q = some_query(rng, m)
    for how in ("none", "first", "last", "every", "over"):
        b = Buffer(q)
        b.add(unit(rng, 70, q, how), guard=0)                     # begins with the buffer
        for n in [0, m - 1, m, m + 1] + LENGTHS:
            b.add(unit(rng, n, q, how), phase=0)
            b.add(unit(rng, n, q, how), phase=int(rng.integers(16)), beg=int(rng.integers(8)))
        b.add(unit(rng, 4 * 40 + 1, q, how), tail=0)              # ends in the buffer's last byte: only its pad bits follow
        assert b.boff[0] == 0 and b.boff[-1] + 41 == len(b.packed())
        want = run(ctx, b, [(q, 0)])
        if how == "every" and m == 1:
            assert want["hits"] == sum(b.ln)                      # (a homopolymer read against a homopolymer query)
        if how in ("first", "last"):
            assert want["hits"] >= sum(n >= m for n in b.ln)


@pytest.mark.parametrize("n", [37, 1100])
def test_all_phases(ctx, n):
    """every d_boff mod 16, every d_beg mod 4 (and beyond a byte), every end mod 4: a lane's or a group's unit, and the wave's"""
    rng = np.random.default_rng(n)
    q = some_query(rng, 17)
    b = Buffer(q)
    for phase in range(16):
        for beg in (0, 1, 2, 3, 6):
            for extra in range(4):
                b.add(unit(rng, n + extra, q, ("first", "last", "over", "every")[extra]), phase=phase, beg=beg)
    assert {x % 16 for x in b.boff} == set(range(16)) and {(s + t) % 4 for s, t in zip(b.beg, b.ln)} == set(range(4))
    run(ctx, b, [(q, 0)])
    if n == 37:
        run(ctx, b, [(q, 0)], beg=False)                          # (d_beg == NULL: the reads from their first symbol)


@pytest.mark.parametrize("m", QLENS)
def test_windows_across_chunk_and_step_boundaries(ctx, m):
    """a window that begins at each of k - m + 1 .. k for the boundary k between two chunks of a lane's unit, of a group's and of
    the wave's, and between two of the wave's steps"""
    rng = np.random.default_rng(100 + m)
    q = some_query(rng, m)
    b, plants = Buffer(q), 0
    for d in range(m):
        x = rng.integers(0, 4, 3 * CHUNK).astype(np.uint8)        # phase 0: chunk boundaries at 64, 128; the lane's
        x[CHUNK - d:CHUNK - d + m] = q
        b.add(x, phase=0)
        g = rng.integers(0, 4, LANE + 3 * CHUNK).astype(np.uint8)  # ... the group's
        for k in (CHUNK, LANE + CHUNK):
            g[k - d:k - d + m] = q
        b.add(g, phase=0)
        y = rng.integers(0, 4, STEP + 5 * CHUNK).astype(np.uint8)
        for k in (3 * CHUNK, STEP, STEP + CHUNK):
            y[k - d:k - d + m] = q
        b.add(y, phase=0)
        z = rng.integers(0, 4, STEP + 5 * CHUNK).astype(np.uint8)  # ... and where the unit begins in the middle of a chunk
        for k in (3 * CHUNK - 23, STEP - 23):
            z[k - d:k - d + m] = q
        b.add(z, phase=5, beg=3)
        plants += 8
    assert run(ctx, b, [(q, 0)])["hits"] >= plants


# ---- mismatches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 16, 17, 32])
def test_mismatches(ctx, m):
    """0, 1, 2 and m - 1 mismatches allowed: windows planted at exactly that distance hit, at one more they do not"""
    rng = np.random.default_rng(200 + m)
    q = some_query(rng, m)
    for mm in sorted({0, 1, 2, m - 1}):
        b, exact, over = Buffer(q), [], []
        for n in (CHUNK - 4 if m <= NARROW else 3 * CHUNK - 4, LANE + 2 * CHUNK, STEP + 3 * CHUNK):       # (three plants side by side need 3 m symbols)
            x = rng.integers(0, 4, n).astype(np.uint8)
            for at, miss, where in ((0, mm, exact), (n - m, mm + 1, over), (n // 2 - m // 2, mm, exact)):
                w = q.copy()
                k = rng.choice(m, miss, replace=False)
                w[k] = (w[k] + rng.integers(1, 4, miss)) % 4
                x[at:at + m] = w
                where.append((len(b.ln), at))
            b.add(x, phase=int(rng.integers(16)), beg=int(rng.integers(4)))
        want = run(ctx, b, [(q, mm)])
        got = {(int(h["record"]), int(h["pos"])): int(h["mis"]) for h in want["list"]}
        assert all(got.get(p) == mm for p in exact)
        assert all(p not in got for p in over)


# ---- several queries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 64])
def test_queries(ctx, nq):
    """1, 2 and 64 queries of every length, duplicates among them, with and without mismatches: every hit of every one, in order"""
    rng = np.random.default_rng(300 + nq)
    qs = [(some_query(rng, QLENS[k % len(QLENS)]), (0, 1)[k % 3 == 2 and QLENS[k % len(QLENS)] > 1]) for k in range(nq)]
    if nq > 1:
        qs[-1] = qs[0]                                             # (a duplicate reports on its own)
    b = Buffer(qs[0][0])
    for n in (0, 3, CHUNK - 1, 3 * CHUNK, LANE + 3 * CHUNK, GROUP + 7, STEP + 2 * CHUNK + 1):
        x = rng.integers(0, 4, n).astype(np.uint8)
        for q, _ in qs:                                            # a copy of every query somewhere in every unit that has room
            if n >= len(q):
                at = int(rng.integers(0, n - len(q) + 1))
                x[at:at + len(q)] = q
        b.add(x, phase=int(rng.integers(16)), beg=int(rng.integers(4)))
    want = run(ctx, b, qs)
    if nq > 1:
        assert want["total"][0] == want["total"][-1] > 0


# ---- the list --------------------------------------------------------------------------------------------------------------------------
def test_the_cap_and_the_canary(ctx):
    """cap 0, one below the hits, the hits, one above, and a few in the middle of a unit: the first cap hits, element for element,
    and not a byte behind them -- with many hits in every path (a lane's unit, a group's, the wave's over two steps)"""
    rng = np.random.default_rng(5)
    q1, q2 = np.array([2], np.uint8), np.array([2, 2, 2], np.uint8)
    b = Buffer(q1)
    for n in (40, 0, 7 * CHUNK + 3, 2 * STEP + 100, 9, 3 * CHUNK):
        x = rng.integers(0, 4, n).astype(np.uint8)
        x[n // 3:2 * n // 3] = 2
        b.add(x, phase=int(rng.integers(16)), beg=int(rng.integers(4)))
    hits = run(ctx, b, [(q1, 0), (q2, 1)])["hits"]
    assert hits > 2 * STEP // 3
    for cap in (0, 1, 30, hits // 2, hits - 1, hits, hits + 1):
        run(ctx, b, [(q1, 0), (q2, 1)], cap=cap)


# ---- what is no unit -------------------------------------------------------------------------------------------------------------------
def test_a_buffer_of_fewer_than_16_bytes(ctx):
    q = np.array([1, 3, 0], np.uint8)
    for n in (1, 3, 4, 5, 11, 12, 13, 30):
        b = Buffer(q)
        b.add(unit(np.random.default_rng(n), n, q, "last"), guard=0, tail=0)
        assert len(b.packed()) == (n + 3) // 4 < 16
        assert run(ctx, b, [(q, 0), (q[:1], 0)])["total"][0] >= (n >= 3)


def test_bad_units_and_no_units(ctx):
    """units that do not lie inside the buffer: DX_E_FORMAT with the smallest of them, no hits of their own, the others searched"""
    rng = np.random.default_rng(9)
    q = np.array([0, 0], np.uint8)
    b = Buffer(q)
    for n in (50, 300, 5000, 20, 70):
        b.add(unit(rng, n, q, "every"), phase=int(rng.integers(16)))
    packed, n = b.packed(), len(b.ln)
    boff, ln = np.array(b.boff, np.uint64), np.array(b.ln, np.uint32)
    boff[3] = len(packed) + 1                                      # begins behind the buffer
    ln[1] = 4 * (len(packed) - b.boff[1]) + 1                      # ends one symbol behind it
    bufs = [ctx.to_device(np.frombuffer(packed, np.uint8)), ctx.to_device(boff), ctx.to_device(ln), ctx.to_device(np.full(n, 77, np.uint32))]
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_find(bufs[0], len(packed), bufs[1], None, bufs[2], n, [F.query(q)], d_count=bufs[3], cap=100)
        assert e.value.code == E_FORMAT and e.value.bad_unit == 1
        assert bufs[3].download(np.uint32, n).tolist() == [49, 0, 4999, 0, 69]
        rep, lst = ctx.code_find(bufs[0], len(packed), bufs[1], None, bufs[2], 0, [F.query(q)], d_count=bufs[3], cap=100)
        assert rep["hits"] == 0 and rep["total"].tolist() == [0] and len(lst) == 0
    finally:
        for x in bufs:
            x.free()


def test_refused_arguments(ctx):
    d = ctx.to_device(np.zeros(64, np.uint8))
    try:
        for qs in ([], [(0, 1, 0)] * 65, [(0, 0, 0)], [(0, 33, 0)], [(4, 1, 0)], [(1 << 62, 31, 0)]):
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_find(d, 16, d, None, d, 1, qs)
            assert e.value.code == E_ARG, qs
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_find(d, 16, None, None, d, 1, [(0, 1, 0)])
        assert e.value.code == E_ARG
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_find(d, 16, d, None, d, 1 << 31, [(0, 1, 0)])
        assert e.value.code == E_ARG
        assert ctx.code_find(d, 16, d, None, d, 1, [((1 << 64) - 1, 32, 0)])[0]["hits"] == 0
    finally:
        d.free()
