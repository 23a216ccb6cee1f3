"""Context.code_kmer_index, .kmer_index_from_letters and .kmer_index (dx_code_kmer_index, dx_kmer_index_from_letters,
dx_file_kmer_index) on the GPU against the numpy statement of tests/_place.py: codes, counts, start, pos and toff are compared whole,
for targets of 0, k - 1, k, 70 and 300 symbols, a poly-A target (one code with all positions), a word that is its own reverse
complement, at every k of {1, 5, 14, 21, 32}, canonical and not; the three routes give the same index; the set inside screens as a
set built from the same codes does.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _oracle as O
import _place as P
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3
KS = [1, 5, 14, 21, 32]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def targets_of(k, seed):
    rng = np.random.default_rng(seed)
    t = [rng.integers(0, 4, n).astype(np.uint8) for n in (0, k - 1, k, 70, 300, 1100, 5003)]   # (1100: 17 to 64 chunks; 5003: two pieces, two wave steps)
    t.append(np.zeros(90, np.uint8))                                         # poly-A: one code, every position
    if k % 2 == 0:                                                           # h + rc(h): a k-mer that is its own reverse complement
        h = rng.integers(0, 4, k // 2).astype(np.uint8)
        t.append(np.concatenate([rng.integers(0, 4, 9).astype(np.uint8), h, (3 - h)[::-1], rng.integers(0, 4, 7).astype(np.uint8)]))
    t.append(t[4][40:200].copy())                                            # a repeat: codes with two positions
    t.append((3 - t[4][100:260])[::-1].copy())                              # ... and of the other strand
    return t


def same_index(x, want):
    i = x.info
    assert (i["codes"], i["windows"], i["targets"], i["symbols"]) == (len(want.codes), want.windows, len(want.toff) - 1, int(want.toff[-1]))
    assert (i["k"], bool(i["canonical"])) == (want.k, want.canonical)
    s = x.kset()
    assert s.counted and np.array_equal(s.codes(), want.codes) and np.array_equal(s.counts(), want.counts)
    start, pos = x.positions()
    assert start.dtype == np.uint32 and np.array_equal(start, want.start)
    diff = np.flatnonzero(pos != want.pos)
    assert len(pos) == len(want.pos) and len(diff) == 0, [(int(j), int(pos[j]), int(want.pos[j])) for j in diff[:8]]
    assert x.targets().dtype == np.uint64 and np.array_equal(x.targets(), want.toff)
    return start, pos


def units_index(ctx, targets, k, canonical, arrow=False):
    b = P.Buffer()
    for j, s in enumerate(targets):
        b.add(s, phase=(5 * j) % 16, beg=j % 4 + 4 * (j % 3), guard=6, tail=6)
    d = [ctx.to_device(np.asarray(a, t)) for a, t in ((np.frombuffer(b.packed(), np.uint8), np.uint8), (b.boff, np.uint64), (b.beg, np.uint32),
                                                       (b.ln, np.uint32))]
    try:
        return ctx.code_kmer_index(d[0], d[1], d[2], d[3], k, canonical=canonical, arrow=arrow), b
    finally:
        for v in d:
            v.free()


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", KS)
def test_units_and_letters_give_the_statements_index(ctx, k, canonical):
    targets = targets_of(k, 40 + k)
    want = P.Index(targets, k, canonical)
    if canonical and k % 2 == 0:
        flips = want.pos & 1
        assert 0 < flips.sum() < len(flips)
    x, b = units_index(ctx, targets, k, canonical)
    with x:
        start, pos = same_index(x, want)
        if k >= 14:
            assert int(want.counts.max()) >= 90 - k + 1 and (np.diff(start.astype(np.int64)) >= 1).all()
        # the set inside screens as a set of the same codes does
        d = [ctx.to_device(np.asarray(a, t)) for a, t in ((np.frombuffer(b.packed(), np.uint8), np.uint8), (b.boff, np.uint64),
                                                           (b.beg, np.uint32), (b.ln, np.uint32))]
        outs = [ctx.alloc(16 * len(b.ln)) for _ in range(2)]
        try:
            with ctx.kmer_set_from_codes(want.codes, k, canonical) as plain:
                ta = ctx.code_kmer_screen(d[0], d[1], d[2], d[3], x.kset(), out=outs[0], n=len(b.ln))
                tb = ctx.code_kmer_screen(d[0], d[1], d[2], d[3], plain, out=outs[1], n=len(b.ln))
            assert np.array_equal(ta, tb) and ta[1] == ta[0] == want.windows
            assert outs[0].download(np.uint32, 4 * len(b.ln)).tobytes() == outs[1].download(np.uint32, 4 * len(b.ln)).tobytes()
        finally:
            for v in d + outs:
                v.free()
    with ctx.kmer_index_from_letters(["".join("ACGT"[c] for c in s) for s in targets], k, canonical=canonical) as y:
        s2, p2 = same_index(y, want)
        assert s2.tobytes() == start.tobytes() and p2.tobytes() == pos.tobytes()


@pytest.mark.parametrize("kind,name,k", [("fasta", "ta_small.dexta", 21), ("fasta", "ta_edge.dexta", 5), ("arrow", "ar_small.dexar", 14)])
def test_an_images_records_are_the_targets(ctx, kind, name, k):
    img = O.golden(name)
    rs = F.reads(kind, F.text_of(kind, img))
    canonical = kind == "fasta"
    want = P.Index(rs, k, canonical)
    with ctx.kmer_index(kind, img, k, canonical=canonical) as x:
        same_index(x, want)
        assert bool(x.info["arrow"]) == (kind == "arrow") and x.info["device_bytes"] >= 12 * len(want.codes) + 4 * want.windows
    letters = "ACGT" if kind == "fasta" else "1234"
    with ctx.kmer_index_from_letters(["".join(letters[c] for c in s) for s in rs], k, canonical=canonical, arrow=kind == "arrow") as y:
        same_index(y, want)


def test_no_targets_no_windows_and_the_refusals(ctx):
    with ctx.kmer_index_from_letters([], 21) as x:
        same_index(x, P.Index([], 21))
    with ctx.kmer_index_from_letters(["ACGT", "", "AC"], 5, canonical=True) as x:
        same_index(x, P.Index([np.array([0, 1, 2, 3]), np.zeros(0, int), np.array([0, 1])], 5, True))
    for kw in (dict(k=0), dict(k=33), dict(k=5, canonical=True, arrow=True)):
        seqs = ["1234"] if kw.get("arrow") else ["ACGT"]
        with pytest.raises(L.DexGPUError) as e:
            ctx.kmer_index_from_letters(seqs, **kw)
        assert e.value.code == E_ARG
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_index_from_letters(["ACGT", "ACGNA"], 3)
    assert e.value.code == E_ARG and "target 1" in str(e.value) and "position 3" in str(e.value)
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_index("quiva", O.golden("qv_tiny.dexqv"), 15)
    assert e.value.code == E_ARG
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_index("arrow", O.golden("ar_small.dexar"), 15, canonical=True)
    assert e.value.code == E_ARG
    # a reference of 2^31 symbols or more is refused from the lengths alone, the size named; a target outside the buffer is DX_E_FORMAT
    d = ctx.alloc(64).zero()
    d_len = ctx.to_device(np.array([0x7fffffff, 5], np.uint32))
    d_off = ctx.to_device(np.array([0, 0], np.uint64))
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_index(d, d_off, None, d_len, 21, in_bytes=64, n=2)
        assert e.value.code == E_ARG and "2^31" in str(e.value)
        d_len.upload(np.array([40, 5000], np.uint32))
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_kmer_index(d, d_off, None, d_len, 21, in_bytes=64, n=2)
        assert e.value.code == E_FORMAT
        h = api.C.c_void_p(5)
        assert ctx.lib.dx_code_kmer_index(ctx.h, d.ptr, 64, None, None, d_len.ptr, 2, 21, 0, 0, api.C.byref(h)) == E_ARG and h.value is None
        assert ctx.lib.dx_kmer_index_info(None, api.C.byref(L.IndexInfo())) == E_ARG
        assert ctx.lib.dx_kmer_index_free(ctx.h, None) == 0
    finally:
        for v in (d, d_len, d_off):
            v.free()
