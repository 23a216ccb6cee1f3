"""dx_code_kmers, dx_kmer_spectrum and dx_kmer_list on the GPU against their numpy statement (tests/_kmers.py), on the smallest shapes
that can go wrong: every unit length around k, a chunk and the cuts between the kernel's three paths, every phase of a unit's start
and every residue of its byte offset, both counting routes and both sides of the cut between them, and everything that is NOT a unit
(the guard bytes around it, the symbols in front of d_beg, the pad bits of its last byte) filled with Ts, so that a window that
reaches outside a unit lands in a cell the statement does not count.  Equality is exact: integer adds have no order.  No expected
value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import _find as F
import _kmers as K
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

# csrc/kmers/dx_kmers.hip
CUT = 7               # KM_LDS_K: up to here the table stands in LDS, beyond the adds are global
CHUNK = 64            # KC_CHUNK: positions of one 16-byte chunk, which stands on a 16-byte boundary of the BUFFER
LANE = 4 * CHUNK      # KC_LANE: a unit of up to four chunks is its lane's
GROUP = 16 * CHUNK    # KC_GROUP: up to 16 chunks 16 lanes take the unit, beyond the wave
STEP = 64 * CHUNK     # what the wave takes of a long unit a step
KS = [1, 2, CUT, CUT + 1, 13, 14]
E_ARG, E_FORMAT = -1, -3          # DX_E_*
T = 3                 # the foreign symbol


def lengths(k):
    return sorted({0, k - 1, k, k + 1, 9000} | {c + d for c in (CHUNK, LANE, GROUP, STEP) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tables(ctx):
    """a zeroed device table of 4^k counters, one allocation a k for the whole module"""
    have = {}

    def fresh(k):
        if k not in have:
            have[k] = ctx.alloc(8 * 4 ** k)
        return have[k].zero()
    yield fresh
    for b in have.values():
        b.free()


class Buffer:
    """a packed buffer that grows unit by unit; around a unit everything is T, the pad bits too"""
    def __init__(self):
        self.sym, self.boff, self.beg, self.ln, self.n = [], [], [], [], 0       # n: symbols so far (4 a byte)

    def add(self, codes, phase=None, beg=0, guard=2, tail=2):
        """the unit's symbols; phase: (byte offset of its read) mod 16, beg: the symbols of its read in front of it"""
        at = self.n // 4 + guard
        if phase is not None:
            at += (phase - at) % 16
        front = 4 * (at - self.n // 4) + beg
        codes = np.asarray(codes, np.uint8)
        end = self.n + front + len(codes)
        self.sym += [np.full(front, T, np.uint8), codes, np.full((-end) % 4 + 4 * tail, T, np.uint8)]
        self.boff.append(at); self.beg.append(beg); self.ln.append(len(codes))
        self.n = end + (-end) % 4 + 4 * tail
        return self

    def packed(self):
        return F.pack(np.concatenate(self.sym)) if self.sym else b""

    def units(self):
        p = self.packed()
        return [F.symbols(p, self.boff[j], self.beg[j], self.ln[j]) for j in range(len(self.ln))]


def upload(ctx, b, sel=None):
    sel = range(len(b.ln)) if sel is None else sel
    packed = b.packed()
    return [ctx.to_device(np.frombuffer(packed, np.uint8)) if packed else ctx.alloc(16), ctx.to_device(np.array([b.boff[j] for j in sel], np.uint64)),
            ctx.to_device(np.array([b.beg[j] for j in sel], np.uint32)), ctx.to_device(np.array([b.ln[j] for j in sel], np.uint32))], len(packed), len(sel)


def fetch(ctx, table, k, room):
    """what the table holds, by dx_kmer_list: (codes, counts)"""
    found, lst = ctx.kmer_list(table, k, 1, room)
    assert found == len(lst), "more cells in use than windows were counted"
    return lst["code"], lst["count"]


def same(got, want, what=""):
    (gc, gn), (wc, wn) = got, want
    assert len(gc) == len(wc) and (gc == wc).all() and (gn == wn).all(), (
        what, len(gc), len(wc), [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(gc, gn, wc, wn) if a != c or b != d][:6])


def run(ctx, tables, b, k, canonical=False, beg=True, nspec=8):
    """one call over all units of the buffer against the statement: the windows, the table (through the list; the whole of it where
    it is small), and the spectrum of it"""
    seen, cnt, windows = K.sparse(b.units(), k, canonical)
    table = tables(k)
    bufs, nbytes, n = upload(ctx, b)
    try:
        _, got = ctx.code_kmers(bufs[0], bufs[1], bufs[2] if beg else None, bufs[3], k, canonical, table, in_bytes=nbytes, n=n)
    finally:
        for x in bufs:
            x.free()
    assert got == windows
    same(fetch(ctx, table, k, windows + 3), (seen, cnt), (k, canonical))
    if k <= CUT + 1:
        dense, w = K.table(b.units(), k, canonical)
        assert np.array_equal(table.download(np.uint64, 4 ** k), dense) and w == windows
    sp, want = ctx.kmer_spectrum(table, k, nspec), K.spectrum(cnt, nspec)
    assert np.array_equal(sp["spectrum"], want["spectrum"]) and sp["distinct"] == len(seen) and sp["max_count"] == want["max_count"]
    assert sp["max_code"] == (int(seen[want["max_code"]]) if len(seen) else 0)
    return seen, cnt, windows


def every_length(k, seed):
    """every length at all four phases of d_beg, the byte offsets going through every residue mod 16"""
    rng, b, j = np.random.default_rng(seed), Buffer(), 0
    for n in lengths(k):
        for beg in range(4):
            b.add(rng.integers(0, 4, n), phase=(5 * j) % 16, beg=beg + 4 * (j % 3))
            j += 1
    assert {o % 16 for o in b.boff} == set(range(16))
    return b


# ---- lengths, phases, routes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_every_length_phase_and_offset(ctx, tables, k, canonical):
    b = every_length(k, 100 + k)
    seen, cnt, windows = run(ctx, tables, b, k, canonical)
    assert windows == sum(max(0, n - k + 1) for n in b.ln) > 0
    if not canonical and k <= 2:
        run(ctx, tables, b, k, beg=True, nspec=2)


@pytest.mark.parametrize("k", [1, 3, CUT, CUT + 1])
def test_d_beg_null_is_all_zero(ctx, tables, k):
    rng, b = np.random.default_rng(7), Buffer()
    for j, n in enumerate([k, 70, 300, 1100, 4200]):
        b.add(rng.integers(0, 4, n), phase=j * 3)
    run(ctx, tables, b, k, beg=False)


@pytest.mark.parametrize("k", [2, CUT, CUT + 1, 14])
@pytest.mark.parametrize("nbytes", [1, 4, 7, 15, 16, 17, 33])
def test_short_buffers_and_a_unit_on_the_last_byte(ctx, tables, k, nbytes):
    """the buffer is the unit's bytes and one in front: nothing behind the unit's last byte belongs to the call"""
    rng = np.random.default_rng(nbytes)
    for cutoff in (0, 1, 3):                                       # (symbols of the last byte that are pad)
        n = 4 * (nbytes - (1 if nbytes > 1 else 0)) - cutoff
        if n < 0:
            continue
        b = Buffer().add(rng.integers(0, 4, n), guard=1 if nbytes > 1 else 0, tail=0)
        assert len(b.packed()) == nbytes
        run(ctx, tables, b, k, k % 2 == 0)


# ---- canonical -------------------------------------------------------------------------------------------------------------------------
def test_self_complementary_kmers_count_once_a_window(ctx, tables):
    """ACGT and GGCC are their own reverse complements: canonical leaves their cells what they are without it, not twice that"""
    rng, b = np.random.default_rng(11), Buffer()
    acgt, ggcc = [0, 1, 2, 3], [2, 2, 1, 1]
    for n, plant in ((40, acgt), (300, ggcc), (1500, acgt), (5000, ggcc)):
        x = rng.integers(0, 4, n)
        for at in (0, n // 2, n - 4):
            x[at:at + 4] = plant
        b.add(x, phase=n % 16, beg=n % 4)
    seen, cnt, _ = run(ctx, tables, b, 4, False)
    plain = dict(zip(seen.tolist(), cnt.tolist()))
    seen, cnt, _ = run(ctx, tables, b, 4, True)
    canon = dict(zip(seen.tolist(), cnt.tolist()))
    for word in (acgt, ggcc):
        code = int(K.codes(word, 4)[0])
        assert int(K.rc(code, 4)) == code and canon[code] == plain[code] >= 6
    tttt, aaaa = 255, 0
    assert canon[aaaa] == plain.get(aaaa, 0) + plain.get(tttt, 0) and tttt not in canon
    run(ctx, tables, b, 5, True)                                   # (an odd k: no k-mer is its own)
    run(ctx, tables, b, 9, True)
    run(ctx, tables, b, 10, True)


# ---- repeats ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, CUT, CUT + 1, 12, 14])
def test_homopolymers_periods_overlaps_and_repeats(ctx, tables, k, monkeypatch):
    rng, b = np.random.default_rng(k), Buffer()
    b.add(np.full(5000, 2), phase=3, beg=1)                        # one cell
    b.add(np.full(5000, 3), phase=9, beg=2)                        # the table's last cell; the Ts around it must stay out
    b.add(np.resize([1, 2], 5000), phase=0, beg=3)                 # two cells
    b.add(np.concatenate([np.full(100, 0), rng.integers(0, 4, 50), np.full(k + 3, 1)]), phase=12)
    seen, cnt, _ = run(ctx, tables, b, k, False)
    assert cnt[seen == K.codes(np.full(k, 2), k)[0]] >= 5000 - k + 1 and cnt[seen == 4 ** k - 1] >= 5000 - k + 1      # (the hot cells)
    run(ctx, tables, b, k, True)
    monkeypatch.setenv("DEXGPU_TEST", "kmer_merge=0")              # (the measurement's switch: every window an add of its own)
    run(ctx, tables, b, k, False)
    monkeypatch.delenv("DEXGPU_TEST")
    # units that overlap, and a unit listed twice: their windows add
    x = rng.integers(0, 4, 3000)
    o = Buffer().add(x, phase=5)
    for beg, n in ((0, 3000), (0, 3000), (17, 900), (500, 2500), (2999, 1), (1000, k)):
        o.boff.append(o.boff[0]); o.beg.append(beg); o.ln.append(n)
    run(ctx, tables, o, k, False)


@pytest.mark.parametrize("k", [1, 3, 6, CUT])
def test_the_lds_cells_swept_early_lose_nothing(ctx, tables, k, monkeypatch):
    """DEXGPU_TEST=kmer_flush=1: a wave empties the workgroup's cells after every round and every step, while the others count"""
    monkeypatch.setenv("DEXGPU_TEST", "kmer_flush=1")
    run(ctx, tables, every_length(k, 5), k, k % 2 == 1)


# ---- accumulation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, CUT, CUT + 1, 13])
def test_two_calls_over_halves_are_one_call_and_the_high_word_carries(ctx, tables, k):
    b = every_length(k, 40 + k)
    seen, cnt, windows = K.sparse(b.units(), k)
    table = tables(k)
    hot = int(seen[np.argmax(cnt)])
    pre = np.array([2 ** 32 - 1], np.uint64)
    ctx._chk(ctx.lib.dx_h2d(ctx.h, table.ptr + 8 * hot, pre.ctypes.data, 8))
    n, got = len(b.ln), 0
    for sel in (range(0, n, 2), range(1, n, 2)):
        bufs, nbytes, m = upload(ctx, b, list(sel))
        try:
            got += ctx.code_kmers(bufs[0], bufs[1], bufs[2], bufs[3], k, False, table, in_bytes=nbytes, n=m)[1]
        finally:
            for x in bufs:
                x.free()
    assert got == windows
    want = cnt.copy()
    want[seen == hot] += np.uint64(2 ** 32 - 1)
    assert int(want[seen == hot][0]) >= 2 ** 32
    same(fetch(ctx, table, k, windows + 3), (seen, want))


TORCH_SIDE = r"""
import sys
import numpy as np
import torch
torch.cuda.init()                                  # (torch first, as in tools/: it does not find the device once the library has it open)
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import _kmers as K
import test_gpu_code_kmers as T
from dextractor_amd import api
b = T.every_length(5, 9)
dense, w = K.table(b.units(), 5, True)
with api.Context(0) as ctx:
    t = [torch.from_numpy(np.frombuffer(b.packed(), np.uint8).copy()).cuda(), torch.from_numpy(np.array(b.boff, np.int64)).cuda(),
         torch.from_numpy(np.array(b.beg, np.int32)).cuda(), torch.from_numpy(np.array(b.ln, np.int32)).cuda()]
    table, windows = ctx.code_kmers(t[0], t[1], t[2], t[3], 5, True)
    assert table.dtype == torch.int64 and tuple(table.shape) == (4 ** 5,) and table.is_cuda and windows == w
    assert np.array_equal(table.cpu().numpy().astype(np.uint64), dense)
    again, w2 = ctx.code_kmers(t[0], t[1], t[2], t[3], 5, True, table)
    assert again is table and w2 == w and np.array_equal(table.cpu().numpy().astype(np.uint64), 2 * dense)
    sp = ctx.kmer_spectrum(table, 5, 32)
    assert sp["distinct"] == int((dense > 0).sum()) and sp["max_count"] == 2 * int(dense.max())
print("torch side ok")
"""


def test_torch_tensors_and_a_table_made_here_when_none_is_given():
    """Context.code_kmers on torch tensors, the table made by it: in a process of its own, which starts torch before the library"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", TORCH_SIDE, os.path.dirname(here), here], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch side ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, CUT + 1])
def test_a_unit_past_the_buffer_is_named_and_adds_nothing(ctx, tables, k):
    rng, b = np.random.default_rng(3), Buffer()
    for j, n in enumerate([100, 20, 700, 64, 2000, 31]):
        b.add(rng.integers(0, 4, n), phase=j)
    nbytes = len(b.packed())
    good = b.units()
    for j, (off, beg, n) in ((4, (nbytes - 3, 0, 13)), (1, (nbytes + 1, 0, 0)), (2, (0, 4 * nbytes - 2, 3))):
        b.boff[j], b.beg[j], b.ln[j] = off, beg, n                 # 4: ends one symbol past the end; 1: begins past it; 2: by d_beg
    bad = {1, 2, 4}
    table = tables(k)
    bufs, _, n = upload(ctx, b)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmers(bufs[0], bufs[1], bufs[2], bufs[3], k, False, table, in_bytes=nbytes, n=n)
    finally:
        for x in bufs:
            x.free()
    assert e.value.code == E_FORMAT and e.value.bad_unit == 1
    seen, cnt, windows = K.sparse([u for j, u in enumerate(good) if j not in bad], k)
    same(fetch(ctx, table, k, windows + 3), (seen, cnt))           # (the other units' counts are there)


def test_no_units_and_the_argument_errors(ctx, tables):
    table = tables(4)
    mark = np.arange(256, dtype=np.uint64)
    table.upload(mark)
    b = Buffer().add(np.arange(40) % 4)
    bufs, nbytes, n = upload(ctx, b)
    win, bad = C.c_uint64(5), C.c_uint64()

    def call(d_in=bufs[0].ptr, boff=bufs[1].ptr, ln=bufs[3].ptr, n=1, k=4, tab=table.ptr):
        return ctx.lib.dx_code_kmers(ctx.h, d_in, nbytes, boff, None, ln, n, k, 0, tab, C.byref(win), C.byref(bad))
    try:
        assert call(n=0) == 0 and win.value == 0 and bad.value == 2 ** 64 - 1
        assert call(d_in=None, boff=None, ln=None, n=0) == 0
        for kw in ({"k": 0}, {"k": 15}, {"tab": None}, {"boff": None}, {"ln": None}, {"d_in": None}, {"n": 2 ** 31}):
            assert call(**kw) == E_ARG, kw
        assert "dx_code_kmers" in (ctx.lib.dx_last_error(ctx.h) or b"").decode()
        assert np.array_equal(table.download(np.uint64, 256), mark)               # (nothing was changed by any of them)
        assert call() == 0 and win.value == 37
    finally:
        for x in bufs:
            x.free()
    found = C.c_uint64()
    assert ctx.lib.dx_kmer_list(ctx.h, table.ptr, 4, 0, None, 0, C.byref(found)) == E_ARG                  # min_count 0
    assert ctx.lib.dx_kmer_list(ctx.h, table.ptr, 4, 1, None, 5, C.byref(found)) == E_ARG                  # room without a place
    assert ctx.lib.dx_kmer_list(ctx.h, None, 4, 1, None, 0, C.byref(found)) == E_ARG
    assert ctx.lib.dx_kmer_list(ctx.h, table.ptr, 15, 1, None, 0, C.byref(found)) == E_ARG
    spec = (C.c_uint64 * 4)()
    assert ctx.lib.dx_kmer_spectrum(ctx.h, table.ptr, 4, spec, 1, None, None, None) == E_ARG               # nspec < 2
    assert ctx.lib.dx_kmer_spectrum(ctx.h, table.ptr, 0, spec, 4, None, None, None) == E_ARG
    assert ctx.lib.dx_kmer_spectrum(ctx.h, None, 4, spec, 4, None, None, None) == E_ARG
    assert ctx.lib.dx_kmer_spectrum(ctx.h, table.ptr, 4, None, 0, None, None, None) == 0                   # (nothing is asked for)


# ---- the spectrum and the list of tables made by hand ----------------------------------------------------------------------------------
def hand_table(k, cells):
    t = np.zeros(4 ** k, np.uint64)
    for code, v in cells.items():
        t[code] = v
    return t


@pytest.mark.parametrize("k,cells", [
    (3, {}),                                                                                   # an empty table
    (1, {0: 1, 3: 1}),
    (3, {0: 15, 5: 16, 9: 14, 63: 2 ** 40, 17: 2 ** 40, 40: 1}),                                # above, at and below nspec - 1 = 15; a tie for the largest
    (6, {c: (c * 7) % 23 for c in range(0, 4096, 3)}),                                          # more than one tile of the list
    (8, {65535: 7, 0: 7, 2048: 7, 2047: 3, 40000: 5000}),                                       # a cell beyond the spectrum's bins in LDS
], ids=["empty", "k1", "ties", "tiles", "wide"])
def test_spectrum_and_list_of_hand_made_tables(ctx, tables, k, cells):
    t = hand_table(k, cells)
    table = tables(k)
    table.upload(t)
    for nspec in (2, 16, 300, 6000):
        sp, want = ctx.kmer_spectrum(table, k, nspec), K.spectrum(t, nspec)
        assert np.array_equal(sp["spectrum"], want["spectrum"]), nspec
        assert (sp["distinct"], sp["max_count"], sp["max_code"]) == (want["distinct"], want["max_count"], want["max_code"])
    none = ctx.kmer_spectrum(table, k, None)
    assert none["spectrum"] is None and none["distinct"] == want["distinct"] and none["max_code"] == want["max_code"]
    top = int(t.max())
    for least in sorted({1, 2, 7, 15, 16, max(top, 1), top + 1}):
        found, _ = K.listing(t, least, 0)
        for cap in sorted({0, max(found - 1, 0), found, found + 1}):
            want_found, want_lst = K.listing(t, least, cap)
            d_out = ctx.to_device(np.full(16 * (cap + 2), 0xEE, np.uint8))
            got = C.c_uint64(99)
            try:
                ctx._chk(ctx.lib.dx_kmer_list(ctx.h, table.ptr, k, least, d_out.ptr if cap else None, cap, C.byref(got)))
                raw = d_out.download(np.uint8)
            finally:
                d_out.free()
            n = min(cap, want_found)
            assert got.value == want_found == found
            assert (raw[:16 * n].view(K.KMER) == want_lst).all(), (least, cap)
            assert (raw[16 * n:] == 0xEE).all(), "a byte behind the list's end is written"
    assert K.listing(t, top + 1, 5)[0] == 0                        # (min_count above the maximum: nothing)
