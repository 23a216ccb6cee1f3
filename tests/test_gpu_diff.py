"""dx_diff_ranges and dx_code_diff on the GPU against their numpy statements (tests/_diff.py), on the smallest shapes that can go
wrong: every length around a chunk, a step and the cuts between the kernel's three paths; every pair of phases; differences
planted on both sides of every edge; and guard bytes around every range that DIFFER between the two sides, so that a read outside
a range shows as a wrong count.  No expected value comes from the library."""
import numpy as np
import pytest

import _diff as D
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# csrc/compare/dx_diff.hip
SHORT = 16        # DF_SHORT: units below go byte by byte, a lane each
GROUP = 256       # 16 lanes x 16 bytes: what the four-a-step path takes of a unit a step
STEP = 1024       # DX_STEP: what the wave takes of a long unit a step
LONG = 2048       # DF_LONG: units from here on take the whole wave
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65537]
assert all(c + 1 in LENGTHS for c in (SHORT, GROUP, STEP, LONG))    # (one unit just over every cut)
SYMBOLS = (list(range(18)) + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537] +
           [4 * c + d for c in (GROUP, STEP, LONG) for d in (-3, -1, 0, 1, 4, 5)])           # ... in bytes, and in symbols of the last byte
PLANTS = ["none", "first", "last", "edges", "every"]
FILL_A, FILL_B = 0xA5, 0x5A                                         # whatever is no unit: differs between the sides


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def planted(n, how):
    """the places of a unit of n bytes (symbols) that are made to differ"""
    if how == "none" or n == 0:
        return []
    if how == "first":
        return [0]
    if how == "last":
        return [n - 1]
    if how == "every":
        return list(range(n))
    edges = {k for e in (16, 32, 256, 1024, 2048, 4096, n - 16, n - n % 16, n - n % 1024) for k in (e - 1, e)}
    return sorted(k for k in edges if 0 <= k < n)


class Sides:
    """two buffers that grow unit by unit: a unit's bytes stand at a chosen phase on either side, a guard byte at least between two
    units, and everything that is no unit is FILL_A on one side and FILL_B on the other"""
    def __init__(self):
        self.a, self.b, self.a_off, self.b_off, self.ln = bytearray(), bytearray(), [], [], []

    def add(self, xa, xb, pa=None, pb=None, units=None, guard=True):
        for buf, x, ph, fill, off in ((self.a, xa, pa, FILL_A, self.a_off), (self.b, xb, pb, FILL_B, self.b_off)):
            if guard and len(buf):
                buf.append(fill)
            if ph is not None:
                buf.extend([fill] * ((ph - len(buf)) % 16))
            off.append(len(buf))
            buf.extend(x)
        self.ln.append(len(xa) if units is None else units)

    def device(self, ctx, extra=()):
        arrs = [np.frombuffer(bytes(self.a), np.uint8), np.array(self.a_off, np.uint64), np.frombuffer(bytes(self.b), np.uint8),
                np.array(self.b_off, np.uint64), np.array(self.ln, np.uint32)] + [np.asarray(e) for e in extra]
        return [ctx.to_device(x) for x in arrs]


def byte_unit(rng, n, how, mask=0xFF):
    """n bytes for side a, and for side b the same under the mask but for the planted places"""
    xa = rng.integers(0, 256, n, dtype=np.uint8)
    xb = xa & mask
    for k in planted(n, how):
        xb[k] ^= rng.integers(1, 256)
    return xa.tobytes(), xb.tobytes()


def run_ranges(ctx, s, kind=None, nkinds=1, a_and=None):
    n = len(s.ln)
    bufs = s.device(ctx, [np.asarray(kind, np.uint8)] if kind is not None else [])
    d_differ, d_first = ctx.alloc(4 * n + 4), ctx.alloc(4 * n + 4)
    try:
        got = ctx.diff_ranges(bufs[0], len(s.a), bufs[1], bufs[2], len(s.b), bufs[3], bufs[4], n, d_kind=bufs[5] if kind is not None else None,
                              nkinds=nkinds, a_and=a_and, d_differ=d_differ, d_first=d_first)
        got["rec_differ"], got["rec_first"] = d_differ.download(np.uint32, n), d_first.download(np.uint32, n)
        plain = ctx.diff_ranges(bufs[0], len(s.a), bufs[1], bufs[2], len(s.b), bufs[3], bufs[4], n, d_kind=bufs[5] if kind is not None else None,
                                nkinds=nkinds, a_and=a_and)       # (no per-unit arrays: the same tallies)
        assert all(np.array_equal(plain[k], got[k]) for k in ("differ", "units", "sum_abs", "max_abs")) and plain["first"] == got["first"]
    finally:
        for b in bufs + [d_differ, d_first]:
            b.free()
    want = D.diff_ranges(s.a, s.a_off, s.b, s.b_off, s.ln, kind=kind, nkinds=nkinds, a_and=a_and)
    bad = np.flatnonzero((got["rec_differ"] != want["rec_differ"]) | (got["rec_first"] != want["rec_first"]))
    assert len(bad) == 0, [(int(j), s.ln[j], s.a_off[j] % 16, s.b_off[j] % 16, int(got["rec_differ"][j]), int(want["rec_differ"][j]),
                            int(got["rec_first"][j]), int(want["rec_first"][j])) for j in bad[:8]]
    D.assert_same_report(got, want)
    return want


# ---- dx_diff_ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", PLANTS)
def test_diff_ranges_lengths_and_planted_differences(ctx, how):
    """every length, twice at random phases; units of fewer than 16 bytes at the very start and the very end of both buffers"""
    rng = np.random.default_rng(PLANTS.index(how))
    s = Sides()
    s.add(*byte_unit(rng, 5, how), guard=False)                   # at byte 0 of both sides
    for n in LENGTHS + LENGTHS:
        s.add(*byte_unit(rng, n, how), pa=int(rng.integers(16)), pb=int(rng.integers(16)))
    s.add(*byte_unit(rng, 7, how))                                # ends with both buffers
    assert s.a_off[0] == s.b_off[0] == 0 and s.a_off[-1] + 7 == len(s.a) and s.b_off[-1] + 7 == len(s.b)
    want = run_ranges(ctx, s)
    assert int(want["differ"][0]) == sum(len(planted(n, how)) for n in s.ln)      # (the guards differ and are not in it)


@pytest.mark.parametrize("n", [37, 1030])
def test_diff_ranges_all_phases(ctx, n):
    rng = np.random.default_rng(n)
    s = Sides()
    for pa in range(16):
        for pb in range(16):
            s.add(*byte_unit(rng, n, "edges"), pa=pa, pb=pb)
    assert sorted({(a % 16, b % 16) for a, b in zip(s.a_off, s.b_off)}) == [(p, q) for p in range(16) for q in range(16)]
    run_ranges(ctx, s)


@pytest.mark.parametrize("nkinds", [1, 5, 8])
def test_diff_ranges_kinds_masks_and_repeated_units(ctx, nkinds):
    """a mask on one kind only (its units differ from b only where the mask says so, or not at all); units that repeat and overlap"""
    rng = np.random.default_rng(40 + nkinds)
    masked = nkinds - 1
    a_and = [0xFF] * nkinds
    a_and[masked] = 0xFC
    s, kind = Sides(), []
    for n in [3, 16, 40, 300, 1500, 2500, 5000] * 3:
        k = int(rng.integers(nkinds))
        s.add(*byte_unit(rng, n, "edges" if rng.random() < 0.7 else "none", mask=a_and[k]), pa=int(rng.integers(16)), pb=int(rng.integers(16)))
        kind.append(k)
    for j, cut in ((4, 0), (4, 0), (5, 100), (6, 1), (3, 17)):      # unit j again, from byte `cut` of it on
        s.a_off.append(s.a_off[j] + cut); s.b_off.append(s.b_off[j] + cut); s.ln.append(s.ln[j] - cut); kind.append(kind[j])
    want = run_ranges(ctx, s, kind=kind, nkinds=nkinds, a_and=a_and)
    assert int(want["units"].sum()) > 0 and int(want["max_abs"].max()) > 3
    if nkinds > 1:                                                # without the mask that kind's units differ in more places
        loose = D.diff_ranges(s.a, s.a_off, s.b, s.b_off, s.ln, kind=kind, nkinds=nkinds)
        assert int(loose["differ"][masked]) > int(want["differ"][masked])


def test_diff_ranges_no_units(ctx):
    got = ctx.diff_ranges(None, 0, None, None, 0, None, None, 0, nkinds=5)
    assert got["first"] is None and all(int(got[k].sum()) == 0 and len(got[k]) == 5 for k in ("differ", "units", "sum_abs", "max_abs"))
    with pytest.raises(L.DexGPUError) as e:
        ctx.diff_ranges(None, 0, None, None, 0, None, None, 0, nkinds=9)
    assert e.value.code == -1


def test_diff_ranges_refuses_the_smallest_bad_unit(ctx):
    a = np.arange(4096, dtype=np.uint8); b = np.arange(4000, dtype=np.uint8)
    cases = [  # (a_off, b_off, len, kind) per unit, nkinds, the index refused
        ([(0, 0, 4000, 0), (96, 0, 4000, 0), (97, 0, 4000, 0), (4096, 0, 1, 0)], 1, 2),            # one byte past a
        ([(0, 0, 4000, 0), (0, 1, 4000, 0), (5000, 0, 0, 0)], 1, 1),                              # one byte past b
        ([(0, 0, 10, 4), (0, 0, 10, 5), (0, 0, 10, 200), (0, 3999, 2, 0)], 5, 1),                 # a kind equal to nkinds
        ([(4096, 4000, 0, 0), (4097, 0, 0, 0)], 1, 1)]                                            # an empty unit behind the end
    for units, nkinds, bad in cases:
        u = np.array(units, np.uint64)
        bufs = [ctx.to_device(x) for x in (a, u[:, 0].copy(), b, u[:, 1].copy(), u[:, 2].astype(np.uint32), u[:, 3].astype(np.uint8))]
        try:
            with pytest.raises(L.DexGPUError) as e:
                ctx.diff_ranges(bufs[0], len(a), bufs[1], bufs[2], len(b), bufs[3], bufs[4], len(u), d_kind=bufs[5], nkinds=nkinds)
            assert e.value.code == -3 and e.value.bad_unit == bad, (units, e.value.bad_unit)
            got = ctx.diff_ranges(bufs[0], len(a), bufs[1], bufs[2], len(b), bufs[3], bufs[4], bad, d_kind=bufs[5], nkinds=nkinds)
            want = D.diff_ranges(a, u[:bad, 0], b, u[:bad, 1], u[:bad, 2], kind=u[:bad, 3], nkinds=nkinds)     # (the units in front of it, on their own)
            assert got["first"] == want["first"] and np.array_equal(got["differ"], want["differ"])
        finally:
            for x in bufs:
                x.free()


# ---- dx_code_diff ------------------------------------------------------------------------------------------------------------------
def code_unit(rng, n, how, pad_ones=True):
    """a packed read of n symbols for side a and for side b: the planted symbols differ, and so do all pad bits of the last byte"""
    nb = (n + 3) // 4
    xa = rng.integers(0, 256, nb, dtype=np.uint8)
    xb = xa.copy()
    for i in planted(n, how):
        xb[i >> 2] ^= int(rng.integers(1, 4)) << (6 - 2 * (i & 3))
    if n & 3 and pad_ones:
        pad = (1 << (8 - 2 * (n & 3))) - 1
        xa[-1] &= ~pad & 0xFF
        xb[-1] |= pad
    return xa.tobytes(), xb.tobytes()


def run_codes(ctx, s):
    n = len(s.ln)
    bufs = s.device(ctx)
    d_differ, d_first = ctx.alloc(4 * n + 4), ctx.alloc(4 * n + 4)
    try:
        got = ctx.code_diff(bufs[0], len(s.a), bufs[1], bufs[2], len(s.b), bufs[3], bufs[4], n, d_differ=d_differ, d_first=d_first)
        got["rec_differ"], got["rec_first"] = d_differ.download(np.uint32, n), d_first.download(np.uint32, n)
    finally:
        for b in bufs + [d_differ, d_first]:
            b.free()
    want = D.code_diff(s.a, s.a_off, s.b, s.b_off, s.ln)
    bad = np.flatnonzero((got["rec_differ"] != want["rec_differ"]) | (got["rec_first"] != want["rec_first"]))
    assert len(bad) == 0, [(int(j), s.ln[j], s.a_off[j] % 16, s.b_off[j] % 16, int(got["rec_differ"][j]), int(want["rec_differ"][j]),
                            int(got["rec_first"][j]), int(want["rec_first"][j])) for j in bad[:8]]
    D.assert_same_report(got, want)
    return want


@pytest.mark.parametrize("how", PLANTS)
def test_code_diff_lengths_and_planted_differences(ctx, how):
    """every length at every byte phase of either side in turn; pad bits all ones on side b only; the byte behind a read differs"""
    rng = np.random.default_rng(70 + PLANTS.index(how))
    s = Sides()
    xa, xb = code_unit(rng, 9, how)
    s.add(xa, xb, units=9, guard=False)
    for k, n in enumerate(SYMBOLS + SYMBOLS):
        xa, xb = code_unit(rng, n, how)
        s.add(xa, xb, pa=k % 16, pb=(5 * k + k // 16) % 16, units=n)
    xa, xb = code_unit(rng, 30, how)
    s.add(xa, xb, units=30)
    assert s.a_off[0] == s.b_off[0] == 0 and s.a_off[-1] + 8 == len(s.a) and s.b_off[-1] + 8 == len(s.b)
    assert {o % 16 for o in s.a_off} == set(range(16)) == {o % 16 for o in s.b_off}
    want = run_codes(ctx, s)
    assert want["symbols"] == sum(len(planted(n, how)) for n in s.ln)              # (pad bits and guards are not in it)


def test_code_diff_every_place_in_a_byte_and_the_first_is_msb_first(ctx):
    """one symbol planted at each of the four places of a byte, at the front, in the middle and at the end of reads of every len % 4"""
    rng = np.random.default_rng(9)
    s, where = Sides(), []
    for n in (21, 22, 23, 24, 2500 * 4 + 1, 2500 * 4 + 2):
        for i in sorted({0, 1, 2, 3, n // 2, n // 2 + 1, n // 2 + 2, n // 2 + 3, n - 4, n - 3, n - 2, n - 1}):
            xa, _ = code_unit(rng, n, "none", pad_ones=False)
            xb = bytearray(xa)
            xb[i >> 2] ^= 1 << (6 - 2 * (i & 3))
            xb[-1] ^= (1 << (8 - 2 * (n & 3))) - 1 if n & 3 else 0
            s.add(xa, bytes(xb), pa=int(rng.integers(16)), pb=int(rng.integers(16)), units=n)
            where.append(i)
    want = run_codes(ctx, s)
    assert list(want["rec_first"]) == where and (want["rec_differ"] == 1).all()
    # two in one byte: the one nearer the top bits is the first
    s = Sides()
    s.add(bytes([0b00011011] * 5), bytes([0b00101010, 0b00011011, 0b00011011, 0b00011011, 0b00011000]), units=20)
    assert list(run_codes(ctx, s)["rec_first"]) == [1]


def test_code_diff_all_phases(ctx):
    rng = np.random.default_rng(12)
    s = Sides()
    for n in (69, 9001):
        for pa in range(16):
            for pb in range(16):
                xa, xb = code_unit(rng, n, "edges")
                s.add(xa, xb, pa=pa, pb=pb, units=n)
    run_codes(ctx, s)


def test_code_diff_refusals_are_packed_unit_oks(ctx):
    assert ctx.code_diff(None, 0, None, None, 0, None, None, 0) == {"symbols": 0, "units": 0, "first": None}
    a = np.zeros(100, np.uint8); b = np.zeros(90, np.uint8)
    cases = [([(0, 0, 360), (10, 0, 360), (10, 0, 361), (0, 0, 400)], 2),      # the last symbol's byte is one past a
             ([(0, 0, 360), (0, 1, 356), (0, 89, 5)], 2),                     # ... past b
             ([(100, 90, 0), (0, 91, 0)], 1),                                  # a read that starts behind the end
             ([(0, 0, 0), (0, 0, 0x80000000)], 1)]                             # more symbols than a read has (UNITS_LEN_MAX)
    for units, bad in cases:
        u = np.array(units, np.uint64)
        bufs = [ctx.to_device(x) for x in (a, u[:, 0].copy(), b, u[:, 1].copy(), u[:, 2].astype(np.uint32))]
        try:
            with pytest.raises(L.DexGPUError) as e:
                ctx.code_diff(bufs[0], len(a), bufs[1], bufs[2], len(b), bufs[3], bufs[4], len(u))
            assert e.value.code == -3 and e.value.bad_unit == bad, (units, e.value.bad_unit)
            assert ctx.code_diff(bufs[0], len(a), bufs[1], bufs[2], len(b), bufs[3], bufs[4], bad)["first"] is None
        finally:
            for x in bufs:
                x.free()
