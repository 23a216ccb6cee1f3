"""Context.depth_stats (dx_depth_stats) on the GPU against numpy (tests/_depth.py: np.sort(v)[(t * (w - 1)) // 4]), fed from uploaded
arrays: stretches of every length around a lane's four values, a wave's step of 256 and beyond, in one call and in shuffled order;
contents that put all values into one bin of the high byte, into one bin of the low byte, at the two ends of the range, and the rank
exactly at the change between two values.  Every field of every entry and the four totals are compared; behind the last entry stand
guard entries.  No expected value comes from the library."""
import numpy as np
import pytest

import _depth as D
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 70001]
GUARD = 3             # entries behind the last
MARK = 0xC0DEC0DE
U = np.uint64


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def contents(kind, w, rng):
    if kind == "equal":
        return np.full(w, 0x1234, np.uint16)
    if kind == "descending":                                         # strictly, while the range lasts
        return (65535 - np.arange(w) % 65536).astype(np.uint16)
    if kind == "low_byte":                                           # one bin of the high byte
        return (0x4200 + rng.integers(0, 256, w)).astype(np.uint16)
    if kind == "high_byte":                                          # values that differ only in the high byte
        return (rng.integers(0, 256, w) * 256 + 0x5a).astype(np.uint16)
    if kind == "ends":
        return (rng.integers(0, 2, w) * 65535).astype(np.uint16)
    if kind == "change":                                             # two values, and a rank exactly at the change: the first
        a = np.full(w, 300, np.uint16)                               # (w - 1) // 4 + 1 sorted values are 299, so q1 is the last 299
        a[:(w - 1) // 4 + 1] = 299                                   # and the next rank the first 300
        return rng.permutation(a)
    if kind == "change_median":
        a = np.full(w, 0x0100, np.uint16)                            # ... across a change of the high byte, at the median
        a[:(2 * (w - 1)) // 4] = 0x00ff
        return rng.permutation(a)
    return rng.integers(0, 65536, w).astype(np.uint16)


KINDS = ["equal", "descending", "low_byte", "high_byte", "ends", "change", "change_median", "random"]


def run(ctx, depth, off, with_out=True):
    """one call against the statement: (the entries, the totals)"""
    n = len(off) - 1
    want, wtot = D.stats(depth, off)
    d_depth = ctx.alloc(2 * len(depth) + 16).upload(np.asarray(depth, np.uint16)) if len(depth) else ctx.alloc(16)
    d_off = ctx.to_device(np.asarray(off, np.uint64))
    d_out = ctx.alloc(32 * (n + GUARD)).upload(np.full(8 * (n + GUARD), MARK, np.uint32))
    try:
        totals = ctx.depth_stats(d_depth, d_off, n, out=d_out if with_out else None)
        raw = d_out.download(np.uint32, 8 * (n + GUARD))
    finally:
        for x in (d_depth, d_off, d_out):
            x.free()
    assert (raw[8 * n:] == MARK).all(), "an entry behind the last was written"
    assert totals.tolist() == wtot, (totals, wtot)
    if not with_out:
        assert (raw == MARK).all()
        return None, totals
    got = raw[:8 * n].view(D.DEPTH)
    D.same_entries(got, want)
    return got, totals


@pytest.mark.parametrize("kind", KINDS)
def test_every_length_in_one_call_and_shuffled(ctx, kind):
    rng = np.random.default_rng(KINDS.index(kind))
    parts = [contents(kind, w, rng) for w in LENGTHS]
    got = {}
    for order in (list(range(len(LENGTHS))), rng.permutation(len(LENGTHS)).tolist()):
        depth = np.concatenate([parts[i] for i in order])
        off = np.concatenate([[0], np.cumsum([LENGTHS[i] for i in order])]).astype(U)
        e, tot = run(ctx, depth, off)
        assert tot[0] == sum(LENGTHS)
        for j, i in enumerate(order):                                # a stretch's entry does not depend on where it stands
            assert got.setdefault(i, e[j].tobytes()) == e[j].tobytes()
    run(ctx, depth, off, with_out=False)                             # d_out NULL: the totals alone


def test_stretches_that_leave_gaps_overlap_and_begin_at_odd_words(ctx):
    """off need not be sums of the lengths: it must not decrease, and a stretch may begin at any word"""
    rng = np.random.default_rng(3)
    depth = rng.integers(0, 700, 9000).astype(np.uint16)
    depth[rng.integers(0, 3, 9000) == 0] = 0
    for start in (0, 1, 2, 3, 5):
        run(ctx, depth[start:], np.array([0, 0, 1, 6, 263, 263, 1290, 8000, 9000 - start], U))
    got, tot = run(ctx, np.zeros(500, np.uint16), np.array([0, 100, 500], U))        # no hit at all
    assert tot.tolist() == [500, 0, 0, 0] and (got["max"] == 0).all()


def test_no_units_refusals_and_a_decreasing_offset(ctx):
    tot = (api.C.c_uint64 * 4)(7, 7, 7, 7)
    d = ctx.alloc(256).zero()
    try:
        assert ctx.depth_stats(d, d, 0).tolist() == [0, 0, 0, 0]
        assert ctx.lib.dx_depth_stats(ctx.h, d.ptr, d.ptr, 1, d.ptr, None) == E_ARG
        for args in ((None, d.ptr), (d.ptr, None)):
            assert ctx.lib.dx_depth_stats(ctx.h, args[0], args[1], 1, d.ptr, api.C.byref(tot)) == E_ARG and list(tot) == [0, 0, 0, 0]
        assert ctx.lib.dx_depth_stats(ctx.h, d.ptr, d.ptr, 1 << 31, d.ptr, api.C.byref(tot)) == E_ARG
        assert ctx.lib.dx_depth_stats(ctx.h, d.ptr + 1, d.ptr, 1, d.ptr, api.C.byref(tot)) == E_ARG          # a profile at an odd byte
    finally:
        d.free()
    depth = np.arange(100, dtype=np.uint16) + 1
    d_depth, d_off, d_out = ctx.to_device(depth), ctx.to_device(np.array([0, 10, 40, 30, 60, 50, 100], U)), ctx.alloc(32 * 6).zero()
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.depth_stats(d_depth, d_off, 6, out=d_out)
        assert e.value.code == E_FORMAT and "index 2" in str(e.value)                   # the smallest index
        got = d_out.download(np.uint8, 32 * 6).view(D.DEPTH)
        want, _ = D.stats(depth, [0, 10, 40, 40, 60, 60, 100])                          # the stretches that decrease count nothing
        for j in (0, 1, 3, 5):
            want_j = D.stats(depth, [[0, 10], [10, 40], None, [30, 60], None, [50, 100]][j])[0][0]
            assert got[j].tobytes() == want_j.tobytes()
        assert got[2].tobytes() == got[4].tobytes() == bytes(32)
        assert e.value.totals.tolist() == [10 + 30 + 30 + 50, 10 + 30 + 30 + 50, int(depth[:40].sum() + depth[30:60].sum() + depth[50:].sum()), 4]
    finally:
        for x in (d_depth, d_off, d_out):
            x.free()
