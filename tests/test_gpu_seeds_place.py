"""Context.seeds_place (dx_seeds_place) on the GPU against the numpy statement of tests/_place.py, on hand-made seed lists: one seed;
seeds in bins b and b + 1 against b - 1 and b; a tie between strands and between bins; a unit without seeds between two with seeds;
the last bin, whose neighbour does not exist; diagonals that wrap around 2^32; band_bits of 0, 4, 8, 16 and 31; stretches on both
sides of the cuts between a lane, 16 lanes and the wave; a unit of a few thousand seeds, so that a run crosses a tile of the sort; a
decreasing d_off and a seed that names another unit.  No expected value comes from the library."""
import numpy as np
import pytest

import _place as P
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3
BITS = [0, 4, 8, 16, 31]
VT_LANE, VT_GROUP = 4, 256              # csrc/place/dx_place_vote.hip


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def lists(units):
    """units: lists of (pos, gpos, strand) -> (a SEED array, off)"""
    lst = np.zeros(sum(len(u) for u in units), P.SEED)
    off, at = np.zeros(len(units) + 1, np.uint64), 0
    for j, u in enumerate(units):
        for p, g, s in u:
            lst[at] = (j, p, g, s)
            at += 1
        off[j + 1] = at
    return lst, off


def on(diag_, pos, strand=0):
    """a seed on the diagonal diag_ (as the key holds it) at read position pos"""
    return (pos, (diag_ - pos if strand else diag_ - 2 ** 31 + pos) % 2 ** 32, strand)


def check(ctx, units, k, bits, **kw):
    lst, off = lists(units)
    want, wtot = P.place(lst, off, k, bits)
    tot, got = ctx.seeds_place(lst, off, k, band_bits=bits, **kw)
    P.same_entries(got, want)
    assert tot.tolist() == wtot
    return got


@pytest.mark.parametrize("bits", BITS)
def test_hand_made_lists(ctx, bits):
    w, k = 1 << bits, 21
    mid = 2 ** 31 + 40 * w if bits < 25 else 2 ** 31                     # a bin's first diagonal
    b = mid >> bits
    units = [
        [on(mid + 3 % w, 7)],                                              # one seed
        [on(mid, 1), on(mid + w, 2), on(mid + w, 3), on(mid - w, 4), on(mid - w, 5), on(mid - w, 9)],     # b - 1, b: 4; b, b + 1: 3
        [],                                                                # no seed, between two that have some
        [on(mid, 1), on(mid + w, 2), on(mid + w, 3), on(mid + w, 8), on(mid - w, 4), on(mid - w, 5)],     # b - 1, b: 3; b, b + 1: 4
        [on(mid, 5, 1), on(mid, 6, 0), on(mid, 9, 1), on(mid, 2, 0)],      # a tie between the strands: strand 0
        [on(mid + 5 * w, 1), on(mid + 5 * w, 2), on(mid, 3), on(mid, 4)],  # a tie between two bins: the smaller
        [on(mid, 1), on(mid + 2 * w, 2)],                                  # bins b and b + 2 do not add
        [on(2 ** 32 - 1, 3), on(2 ** 32 - 1, 900), on(0, 4, 1), on(w % 2 ** 32, 5, 1)],                   # the last bin has no neighbour; the first
        [on(2 ** 32 - 1, 3, 1), on(0, 4, 1), on(0, 5, 1)],                 # strand 1's last bin does not run into anything
        [(5, 2, 0), (3, 2 ** 32 - 2, 1), (2 ** 31 - 1, 0, 0)],             # diagonals that wrap around 2^32
    ]
    got = check(ctx, units, k, bits)
    assert list(got[2].tolist()) == [0, 0, 0] + [P.NONE] * 5 and got[0]["votes"] == 1
    if bits < 25:
        assert got[1]["votes"] == 4 and got[1]["diag"] == ((b - 1) << bits) and got[3]["votes"] == 4 and got[3]["diag"] == (b << bits)
        assert got[4]["strand"] == 0 and got[4]["votes"] == 2 and got[5]["diag"] == (b << bits) and got[6]["votes"] == 1
    assert ctx.seeds_place(lists([])[0], np.zeros(1, np.uint64), k)[1].tolist() == []                     # n = 0


@pytest.mark.parametrize("bits", [0, 8, 31])
def test_stretches_around_the_cuts_between_the_paths(ctx, bits):
    rng = np.random.default_rng(bits)
    units = []
    for n in (1, VT_LANE - 1, VT_LANE, VT_LANE + 1, 15, 16, 17, 63, 64, 65, VT_GROUP - 1, VT_GROUP, VT_GROUP + 1, 0, 300, 0, 0, 2, 700):
        # a read of 2000 symbols on one diagonal of either strand, and noise all over the reference
        true = int(rng.integers(10 ** 6, 2 * 10 ** 6))
        u = []
        for i in range(n):
            p = int(rng.integers(0, 2000))
            if rng.random() < 0.6:
                u.append((p, true + p, 0) if n % 2 else (p, true + 2000 - p, 1))
            else:
                u.append((p, int(rng.integers(0, 2 ** 31 - 40)), int(rng.integers(0, 2))))
        units.append(u)
    got = check(ctx, units * 4, 15, bits)                                 # (76 units: more than one round of a wave)
    assert got["votes"].max() > 100


def test_a_unit_of_a_few_thousand_seeds(ctx):
    """one run of 5000 equal keys and one of 3000 in the bin behind it, in the middle of noise: the runs cross tiles of the sort, and
    the vote is the sum of both"""
    rng = np.random.default_rng(77)
    k, bits = 32, 8
    d = 2 ** 31 + 123456 * 256
    u = [on(d + int(rng.integers(0, 256)), int(rng.integers(0, 30000)), 1) for _ in range(5000)]
    u += [on(d + 256 + int(rng.integers(0, 256)), int(rng.integers(0, 30000)), 1) for _ in range(3000)]
    u += [(int(rng.integers(0, 30000)), int(rng.integers(0, 2 ** 31 - 40)), int(rng.integers(0, 2))) for _ in range(4000)]
    rng.shuffle(u)
    noise = [[(int(rng.integers(0, 900)), int(rng.integers(0, 2 ** 20)), int(rng.integers(0, 2))) for _ in range(600)] for _ in range(3)]
    got = check(ctx, [noise[0], u, noise[1], [], noise[2]], k, bits)
    assert got[1]["votes"] == 8000 and got[1]["strand"] == 1 and got[1]["diag"] == d and got[1]["seeds"] == 12000
    lst, off = lists([noise[0], u, noise[1], [], noise[2]])
    a = ctx.seeds_place(lst, off, k, band_bits=bits)[1]
    assert a.tobytes() == got.tobytes()                                    # the same bytes on two calls
    # a list that does not begin at the array's first entry: off[0] > 0
    pad = np.zeros(5, P.SEED)
    pad["unit"] = 99
    moved = ctx.seeds_place(np.concatenate([pad, lst]), off + np.uint64(5), k, band_bits=bits)[1]
    assert moved.tobytes() == got.tobytes()


def test_a_decreasing_off_a_foreign_seed_and_the_refusals(ctx):
    units = [[on(2 ** 31 + 5, 1)], [on(2 ** 31 + 900, 2), on(2 ** 31 + 900, 3)], [on(2 ** 31, 4, 1)]]
    lst, off = lists(units)
    bad = off.copy()
    bad[2] = 0                                                             # off = 0, 1, 0, 4
    with pytest.raises(L.DexGPUError) as e:
        ctx.seeds_place(lst, bad, 21)
    assert e.value.code == E_FORMAT and "index 1" in str(e.value)
    with pytest.raises(L.DexGPUError) as e:
        ctx.seeds_place(lst, off[::-1].copy(), 21)                         # the last place in front of the first
    assert e.value.code == E_FORMAT
    far = off.copy()
    far[1] = 9                                                             # a stretch that ends behind the list
    with pytest.raises(L.DexGPUError) as e:
        ctx.seeds_place(lst, far, 21)
    assert e.value.code == E_FORMAT and "index 0" in str(e.value)
    foreign = lst.copy()
    foreign["unit"][2] = 0
    with pytest.raises(L.DexGPUError) as e:
        ctx.seeds_place(foreign, off, 21)
    assert e.value.code == E_FORMAT and "seed 2" in str(e.value)
    for kw in (dict(k=0), dict(k=33), dict(k=21, band_bits=32)):
        with pytest.raises(L.DexGPUError) as e:
            ctx.seeds_place(lst, off, **kw)
        assert e.value.code == E_ARG
    d = ctx.alloc(256).zero()
    tot = (api.C.c_uint64 * 3)(7, 7, 7)
    try:
        f = ctx.lib.dx_seeds_place
        assert f(ctx.h, d.ptr, d.ptr, 1, 21, 8, d.ptr, None) == E_ARG
        assert f(ctx.h, d.ptr, None, 1, 21, 8, d.ptr, api.C.byref(tot)) == E_ARG and list(tot) == [0, 0, 0]
        assert f(ctx.h, d.ptr, d.ptr, 1, 21, 8, None, api.C.byref(tot)) == E_ARG
        assert f(ctx.h, d.ptr, d.ptr + 4, 1, 21, 8, d.ptr, api.C.byref(tot)) == E_ARG
        assert f(ctx.h, d.ptr, d.ptr, 1 << 31, 21, 8, d.ptr, api.C.byref(tot)) == E_ARG
    finally:
        d.free()
