"""Context.kmers (dx_file_kmers) and Context.kmers_add on the GPU against tests/_kmers.py, which counts the k-mers of the TEXT the
oracle's undexta -U / undexar prints for the image: the goldens and their legacy and byte-swapped variants, images this library
packs from small synthetic texts (empty records, Ns, lower case, a k-mer that lies across two records), the same in slices, two
images counted into one table, the listed k-mers searched again with Context.find, and the refusals.  No expected value comes from
the library."""
import numpy as np
import pytest

import _find as F
import _kmers as K
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
GOLDEN = [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("fasta", "ta_lower_w60.dexta"), ("fasta", "ta_small.legacy.dexta"),
          ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_edge.dexar"),
          ("arrow", "ar_small.dexar"), ("arrow", "ar_small.swapped.dexar")]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def check(ctx, kind, img, k, canonical=False, nspec=256, min_count=0, max_list=0):
    want = K.file_kmers(kind, F.text_of(kind, img), k, canonical, nspec, min_count, max_list)
    rep, spec, lst = ctx.kmers(kind, img, k, canonical, nspec, min_count, max_list)
    assert rep == want[0], (rep, want[0])
    assert np.array_equal(spec, want[1])
    assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in lst] == want[2]
    return want


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8, 14])
@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_goldens(ctx, monkeypatch, kind, name, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    want = check(ctx, kind, img, k, min_count=1, max_list=1 << 20)
    assert want[0]["windows"] > 0 and want[0]["listed"] == want[0]["distinct"]
    check(ctx, kind, img, k, nspec=3, min_count=2, max_list=5)
    if kind == "fasta":
        check(ctx, kind, img, k, canonical=True, nspec=40, min_count=1, max_list=1 << 20)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
    check(ctx, kind, img, k, canonical=kind == "fasta", min_count=1, max_list=7)


def test_the_golden_figures_counted_by_hand(ctx):
    """tests/test_kmers_host.py counts these in ta_edge's text by hand"""
    img = O.golden("ta_edge.dexta")
    rep, spec, lst = ctx.kmers("fasta", img, 2, nspec=64, min_count=1, max_list=100)
    assert (rep["records"], rep["symbols"], rep["windows"], rep["distinct"], rep["max_count"], rep["max_code"]) == (9, 278, 270, 7, 82, 15)
    assert [(bytes(e["letters"]), int(e["count"])) for e in lst] == [(b"AA", 5), (b"AC", 46), (b"CG", 46), (b"GT", 46), (b"TA", 44),
                                                                     (b"TG", 1), (b"TT", 82)]
    assert spec[46] == 3 and spec[63] == 1 and spec.sum() == 7
    rep, spec, lst = ctx.kmers("fasta", img, 4, canonical=True, min_count=1, max_list=100)
    assert [(bytes(e["letters"]), int(e["count"])) for e in lst] == [(b"AAAA", 81), (b"ACGT", 45), (b"CACG", 1), (b"CGTA", 87), (b"GTAC", 43)]
    assert (rep["windows"], rep["max_count"], bytes(api.kmer_letters(rep["max_code"], 4))) == (257, 87, b"CGTA")


# ---- synthetic texts, packed by this library -------------------------------------------------------------------------------------------
PLANT = "GGCCAATTGGCCAT"      # 14 letters; its halves are laid at the end of one record and the start of the next


def synthetic(kind, n=260, seed=7):
    """n records of 0 .. 700 symbols: every seventh empty, Ns and lower case among the letters (fasta), PLANT whole in some, and its
    two halves at the end of one record and the start of the next, where it must not be counted"""
    rng = np.random.default_rng(seed)
    letters = "ACGT" if kind == "fasta" else "1234"
    plant = PLANT if kind == "fasta" else PLANT.translate(str.maketrans("ACGT", "1234"))
    out, seqs, across = [], [], 0
    for i in range(n):
        ln = 0 if i % 7 == 3 else int(rng.integers(1, 701))
        s = "".join(letters[c] for c in rng.integers(0, 4, ln))
        if i % 5 == 0 and ln >= 60:
            s = plant + s[14:ln - 14] + plant
        if i % 11 == 1 and ln >= 30:
            s = s[:-7] + plant[:7]                                  # ... and the next record begins with the other half
        if i % 11 == 2 and ln >= 30 and seqs[-1].endswith(plant[:7]):
            s = plant[7:] + s[7:]
            across += 1
        if kind == "fasta" and i % 4 == 1:
            s = "".join(("N" if rng.integers(20) == 0 else c.lower() if rng.integers(2) else c) for c in s)
        seqs.append(s)
        head = f">syn/{100 + 3 * i}/0_{len(s)} " + ("RQ=0.850" if kind == "fasta" else "SN=6.81,9.99,10.50,4.00")
        out.append(head + "".join("\n" + s[k:k + 70] for k in range(0, len(s), 70)))
    whole = sum(r.upper().replace("N", "A").count(plant) for r in seqs)              # (what undexta -U prints: an N is stored as a)
    assert across >= 5 and whole >= 40
    return ("\n".join(out) + "\n").encode(), plant, whole


@pytest.fixture(scope="module", params=["fasta", "arrow"])
def corpus(request, ctx):
    text, plant, whole = synthetic(request.param)
    img = ctx.dexta(text) if request.param == "fasta" else ctx.dexar(text)
    assert img == (O.dexta(text) if request.param == "fasta" else O.dexar(text))
    return request.param, img, plant, whole


@pytest.mark.parametrize("budget", [None, "4096"], ids=["whole", "slices"])
def test_synthetic_texts(ctx, monkeypatch, corpus, budget):
    kind, img, plant, whole = corpus
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    if budget:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", budget)
        assert len(img) >= 3 * 4096                                # three slices at least
    for k in (1, 5, 7, 8, 11):
        check(ctx, kind, img, k, min_count=3, max_list=40)
        if kind == "fasta":
            check(ctx, kind, img, k, canonical=True, min_count=3, max_list=40)
    want = check(ctx, kind, img, 14, min_count=2, max_list=1000)
    code = api.kmer_code(plant, arrow=kind == "arrow")
    assert (whole, code, plant.encode()) in want[2]                 # the whole copies, and not one that lies across two records
    assert want[0]["records"] == 260


def test_two_images_into_one_table(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, img, plant, whole = corpus
    other = O.golden("ta_small.dexta" if kind == "fasta" else "ar_small.dexar")
    k = 8
    a, b = ctx.kmers(kind, img, k, table=True), ctx.kmers(kind, other, k, table=True)
    assert len(a) == 4 and a[3].dtype == np.uint64 and a[3].shape == (4 ** k,)
    assert np.array_equal(a[3], K.file_kmers(kind, F.text_of(kind, img), k)[3])
    table = ctx.alloc(8 * 4 ** k).zero()
    try:
        ra, rb = ctx.kmers_add(kind, img, k, False, table), ctx.kmers_add(kind, other, k, False, table)
        both = table.download(np.uint64, 4 ** k)
        sp = ctx.kmer_spectrum(table, k, 256)
    finally:
        table.free()
    assert np.array_equal(both, a[3] + b[3])
    assert ra == {f: a[0][f] for f in ("records", "symbols", "windows")} and rb == {f: b[0][f] for f in ("records", "symbols", "windows")}
    want = K.spectrum(a[3] + b[3], 256)
    assert np.array_equal(sp["spectrum"], want["spectrum"]) and sp["distinct"] == want["distinct"] and sp["max_code"] == want["max_code"]


def test_the_listed_kmers_are_found_where_they_were_counted(ctx, monkeypatch):
    """over-represented k-mers -> Context.find: exactly `count` hits each; canonical: both strands together, and a k-mer that is its
    own reverse complement on strand 0 alone"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden("ta_small.dexta")
    rep, _, lst = ctx.kmers("fasta", img, 6, min_count=7, max_list=60)
    assert 5 < len(lst) <= 60
    found, _ = ctx.find("fasta", img, [bytes(e["letters"]).decode() for e in lst], max_hits=0)
    assert found["per_pattern"][:, 0].tolist() == [int(e["count"]) for e in lst] and found["per_pattern"][:, 1].sum() == 0
    rep, _, lst = ctx.kmers("fasta", img, 6, canonical=True, min_count=11, max_list=30)
    own = [e for e in lst if K.rc(int(e["code"]), 6) == int(e["code"])]
    more = ctx.kmers("fasta", img, 4, canonical=True, min_count=1, max_list=256)[2]
    for lst in (lst, more[:32]):
        assert len(lst) > 5
        found, _ = ctx.find("fasta", img, [bytes(e["letters"]).decode() for e in lst], both_strands=True, max_hits=0)
        assert found["per_pattern"].sum(axis=1).tolist() == [int(e["count"]) for e in lst]
        for e, per in zip(lst, found["per_pattern"]):
            if K.rc(int(e["code"]), len(e["letters"])) == int(e["code"]):
                assert per[1] == 0 and per[0] == e["count"]
    assert any(K.rc(int(e["code"]), 4) == int(e["code"]) for e in more[:32]) or own       # (AATT, ACGT ... : some palindrome was looked at)
    ar = O.golden("ar_small.dexar")
    rep, _, lst = ctx.kmers("arrow", ar, 5, min_count=30, max_list=40)
    assert len(lst) > 3
    found, _ = ctx.find("arrow", ar, [bytes(e["letters"]).decode() for e in lst], max_hits=0)
    assert found["per_pattern"][:, 0].tolist() == [int(e["count"]) for e in lst]


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmers(*args, **kw)
    return e.value


def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    e = refused(ctx, "quiva", O.golden("qv_tiny.dexqv"), 8)
    assert e.code == E_ARG and "dexqv" in str(e)
    e = refused(ctx, "arrow", ar, 8, canonical=True)
    assert e.code == E_ARG and "canonical" in str(e)
    for k in (0, 15):
        e = refused(ctx, "fasta", ta, k)
        assert e.code == E_ARG and "k = %d" % k in str(e)
    e = refused(ctx, "fasta", ta, 8, nspec=1)
    assert e.code == E_ARG and "spectrum" in str(e)
    table = ctx.alloc(8 * 4 ** 3).zero()
    try:
        for args in (("quiva", O.golden("qv_tiny.dexqv"), 3, False), ("arrow", ar, 3, True), ("fasta", ta, 0, False), ("fasta", ta, 15, False)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.kmers_add(*args, table)
            assert e.value.code == E_ARG
        assert not table.download(np.uint64, 64).any()
        with pytest.raises(L.DexGPUError) as e:
            ctx.kmers_add("fasta", ta, 3, False, None)
        assert e.value.code == E_ARG
    finally:
        table.free()
    ctx.kmers("arrow", ar, 14)
    ctx.kmers("fasta", ta, 1, canonical=True, nspec=2)


def test_a_truncated_image_is_unpack2s_error(ctx):
    for kind, name in (("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")):
        img = O.golden(name)
        for cut in (len(img) - 1, len(img) - 37):
            with pytest.raises(L.DexGPUError) as want:
                (ctx.undexta if kind == "fasta" else ctx.undexar)(img[:cut])
            assert refused(ctx, kind, img[:cut], 8).code == want.value.code
