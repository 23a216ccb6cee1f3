"""KmerSet (dx_kmer_set_from_codes, dx_kmer_set_from_sorted, dx_file_kmer_set) on the GPU against tests/_screen.py and
tests/_kmers_wide.py: the codes that come back are np.unique's of what went in, the k-mers of an image those of the oracle's text, with
min_count those counted so often; the info fields; the bucket index forced narrow and wide.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_wide as W
import _oracle as O
import _screen as S
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
U = np.uint64
GOLDEN = [("fasta", "ta_small.dexta"), ("fasta", "ta_edge.dexta"), ("arrow", "ar_small.dexar")]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def natural_bits(n, k):
    p = 1
    while (1 << p) < 2 * n:
        p += 1
    return max(1, min(p, 2 * k, 26))


# ---- from_codes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(1, 40), (8, 3000), (21, 10000), (32, 5000)])
def test_unsorted_codes_with_repeats_come_back_ascending_and_distinct(ctx, k, n):
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * U(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if k < 32:
        codes &= U(4 ** k - 1)
    codes = np.concatenate([codes, codes[: n // 3], codes[:5], codes[:5]])          # repeats, some three times
    rng.shuffle(codes)
    with ctx.kmer_set_from_codes(codes, k) as s:
        got, info = s.codes(), s.info
    want = np.unique(codes)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert info == {"codes": len(want), "device_bytes": 8 * len(want) + 4 * (2 ** info["index_bits"] + 1), "k": k, "canonical": 0, "arrow": 0,
                    "index_bits": natural_bits(len(want), k)}


def test_the_empty_set_and_the_ends_of_the_code_space(ctx):
    with ctx.kmer_set_from_codes([], 21) as s:
        assert s.info["codes"] == 0 and len(s.codes()) == 0 and s.info["index_bits"] == 1 and s.info["k"] == 21
    with ctx.kmer_set_from_codes([2 ** 64 - 1, 0, 2 ** 64 - 1, 0, 2 ** 63], 32) as s:        # compared unsigned
        assert s.codes().tolist() == [0, 2 ** 63, 2 ** 64 - 1]
    with ctx.kmer_set_from_codes([3, 0], 1, arrow=True) as s:
        assert s.codes().tolist() == [0, 3] and s.info["arrow"] == 1 and s.info["index_bits"] == 2


@pytest.mark.parametrize("k", [15, 32])
def test_canonical_folds_both_strands_to_one_code(ctx, k):
    rng = np.random.default_rng(k)
    words = ["".join("ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(200)]
    rev = [w[::-1].translate(str.maketrans("ACGT", "TGCA")) for w in words]
    fwd = np.array([api.kmer_code64(w) for w in words], U)
    bwd = np.array([api.kmer_code64(w) for w in rev], U)
    want = np.unique(np.minimum(fwd, W.rc(fwd, k)))
    assert np.array_equal(np.unique(np.minimum(bwd, W.rc(bwd, k))), want)            # (the statement folds them alike)
    for given in (fwd, bwd, np.concatenate([fwd[:100], bwd[100:], bwd[:7]])):
        with ctx.kmer_set_from_codes(given, k, canonical=True) as s:
            assert np.array_equal(s.codes(), want) and s.info["canonical"] == 1
    with ctx.kmer_set_from_codes(np.concatenate([fwd, bwd]), k) as s:                # not canonical: the two strands stay two codes
        assert np.array_equal(s.codes(), np.unique(np.concatenate([fwd, bwd])))


def test_refusals(ctx):
    for k in (0, 33):
        with pytest.raises(L.DexGPUError) as e:
            ctx.kmer_set_from_codes([1, 2], k)
        assert e.value.code == E_ARG and "k = %d" % k in str(e.value)
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_set_from_codes([1, 2], 15, canonical=True, arrow=True)
    assert e.value.code == E_ARG and "canonical" in str(e.value)
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_set_from_codes([1, 2, 4 ** 15, 3], 15)
    assert e.value.code == E_ARG and "code 2" in str(e.value)
    with ctx.kmer_set_from_codes([4 ** 15 - 1], 15) as s:                           # ... and the largest code of 15 symbols is one
        assert s.codes().tolist() == [4 ** 15 - 1]
    h = api.C.c_void_p(5)
    assert ctx.lib.dx_kmer_set_from_codes(ctx.h, None, 3, 15, 0, 0, api.C.byref(h)) == E_ARG and h.value is None
    assert ctx.lib.dx_kmer_set_from_codes(ctx.h, None, 0, 15, 0, 0, None) == E_ARG
    d = ctx.alloc(64).zero()
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.kmer_set_from_sorted(d, 4, 15, min_count=0)
        assert e.value.code == E_ARG and "min_count" in str(e.value)
        assert ctx.lib.dx_kmer_set_from_sorted(ctx.h, None, 4, 1, 15, 0, 0, api.C.byref(h)) == E_ARG
    finally:
        d.free()
    with ctx.kmer_set_from_codes([1, 2, 3], 15) as s:
        out = np.zeros(2, U)
        assert ctx.lib.dx_kmer_set_codes(ctx.h, s.h, out.ctypes.data, 2) == -6 and b"3 codes" in ctx.lib.dx_last_error(ctx.h)
        assert ctx.lib.dx_kmer_set_codes(ctx.h, None, out.ctypes.data, 2) == E_ARG
    assert ctx.lib.dx_kmer_set_free(ctx.h, None) == 0


# ---- from_sorted -----------------------------------------------------------------------------------------------------------------------
def test_runs_of_min_count_from_a_sorted_array(ctx):
    """runs of every length up to 40 and one of 5000 (longer than a tile of 2048 keys), tiles' edges inside runs"""
    rng = np.random.default_rng(2)
    vals = np.unique(rng.integers(0, 4 ** 21, 3000, dtype=np.uint64))
    cnt = rng.integers(1, 41, len(vals))
    cnt[len(vals) // 2] = 5000
    keys = np.repeat(vals, cnt)
    d = ctx.to_device(keys)
    try:
        for mc in (1, 2, 3, 17, 40, 41, 5000, 5001, len(keys) + 5, 2 ** 64 - 1):
            with ctx.kmer_set_from_sorted(d, len(keys), 21, min_count=mc) as s:
                assert np.array_equal(s.codes(), vals[cnt >= min(mc, 2 ** 62)]), mc
        with ctx.kmer_set_from_sorted(d, 0, 21) as s:
            assert s.info["codes"] == 0
    finally:
        d.free()


# ---- the k-mers of an image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 32])
@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_the_k_mers_of_the_goldens(ctx, monkeypatch, kind, name, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    text = F.text_of(kind, img)
    rs = F.reads(kind, text)
    for canonical in ((False, True) if kind == "fasta" else (False,)):
        for mc in (1, 2):
            want = S.distinct(rs, k, canonical, mc)
            s, rep = ctx.kmer_set(kind, img, k, canonical=canonical, min_count=mc, report=True)
            with s:
                assert np.array_equal(s.codes(), want), (canonical, mc)
                assert s.info["k"] == k and s.info["canonical"] == int(canonical) and s.info["arrow"] == int(kind == "arrow")
                assert s.info["index_bits"] == natural_bits(len(want), k)
            full = W.file_kmers_wide(kind, text, k, canonical)[0]
            assert rep == {f: full[f] for f in rep}                                  # what kmers_wide reports, from the text
    assert len(S.distinct(rs, k, False, 1)) > 0
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    with ctx.kmer_set(kind, img, k) as s:
        assert np.array_equal(s.codes(), S.distinct(rs, k))


def test_image_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    for args, word in ((("quiva", O.golden("qv_tiny.dexqv"), 21), "dexqv"), (("arrow", ar, 21, True), "canonical"), (("fasta", ta, 0), "k = 0"),
                       (("fasta", ta, 33), "k = 33"), (("fasta", ta, 21, False, 0), "min_count")):
        with pytest.raises(L.DexGPUError) as e:
            ctx.kmer_set(*args)
        assert e.value.code == E_ARG and word in str(e.value) and "dx_file_kmer_set" in str(e.value)
    h = api.C.c_void_p()
    assert ctx.lib.dx_file_kmer_set(ctx.h, L.DX_KIND_FASTA, ta, len(ta), 21, 0, 1, api.C.byref(h), None) == 0 and h.value
    assert ctx.lib.dx_kmer_set_free(ctx.h, h) == 0


# ---- the bucket index, forced ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 20])
def test_set_bits_gives_the_same_codes_back(ctx, monkeypatch, bits):
    codes = np.random.default_rng(50).integers(0, 4 ** 21, 50, dtype=np.uint64)
    with ctx.kmer_set_from_codes(codes, 21) as s:
        assert s.info["index_bits"] == natural_bits(50, 21) == 7
    set_flag(monkeypatch, "set_bits", bits)
    with ctx.kmer_set_from_codes(codes, 21) as s:
        assert s.info["index_bits"] == bits and np.array_equal(s.codes(), np.unique(codes))
        assert s.info["device_bytes"] == 8 * 50 + 4 * (2 ** bits + 1)
    with ctx.kmer_set_from_codes([0, 3, 9], 2) as s:                                 # clamped to the code's 2 k bits
        assert s.info["index_bits"] == min(bits, 4) and s.codes().tolist() == [0, 3, 9]
