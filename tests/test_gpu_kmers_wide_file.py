"""Context.kmers_wide (dx_file_kmers_wide) on the GPU against tests/_kmers_wide.py, which counts the k-mers of the TEXT the oracle's
undexta -U / undexar prints for the image: the goldens and their legacy and byte-swapped variants, images this library packs from
small synthetic texts (empty records, Ns, lower case, a 32-mer that lies across two records), the same in slices, the new route held
against the merged one (Context.kmers) where both exist, a listed 21-mer searched again with Context.find, and the refusals.  No
expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_wide as W
import _oracle as O
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM = -1, -6
GOLDEN = [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("fasta", "ta_lower_w60.dexta"), ("fasta", "ta_small.legacy.dexta"),
          ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_edge.dexar"),
          ("arrow", "ar_small.dexar"), ("arrow", "ar_small.swapped.dexar")]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def texts():
    """the oracle's text of an image, made once a module"""
    have = {}

    def of(kind, img):
        if (kind, img) not in have:
            have[kind, img] = F.text_of(kind, img)
        return have[kind, img]
    return of


def check(ctx, texts, kind, img, k, canonical=False, nspec=256, min_count=0, max_list=0):
    want = W.file_kmers_wide(kind, texts(kind, img), k, canonical, nspec, min_count, max_list)
    rep, spec, lst = ctx.kmers_wide(kind, img, k, canonical, nspec, min_count, max_list)
    assert rep == want[0], (rep, want[0])
    assert np.array_equal(spec, want[1])
    assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in lst] == want[2]
    return want


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 15, 21, 32])
@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_goldens(ctx, texts, monkeypatch, kind, name, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    want = check(ctx, texts, kind, img, k, min_count=1, max_list=1 << 20)
    assert want[0]["windows"] > 0 and want[0]["listed"] == want[0]["distinct"]
    check(ctx, texts, kind, img, k, nspec=3, min_count=2, max_list=5)
    if kind == "fasta":
        check(ctx, texts, kind, img, k, canonical=True, nspec=40, min_count=1, max_list=1 << 20)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
    check(ctx, texts, kind, img, k, canonical=kind == "fasta", min_count=1, max_list=7)


# ---- synthetic texts, packed by this library -------------------------------------------------------------------------------------------
PLANT = "GGCCAATTGGCCATACGGTTAACCGTATGCAT"      # 32 letters; its halves are laid at the end of one record and the start of the next


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
        if i % 5 == 0 and ln >= 100:
            s = plant + s[32:ln - 32] + plant
        if i % 11 == 1 and ln >= 60:
            s = s[:-16] + plant[:16]                                # ... and the next record begins with the other half
        if i % 11 == 2 and ln >= 60 and seqs[-1].endswith(plant[:16]):
            s = plant[16:] + s[16:]
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
def test_synthetic_texts(ctx, texts, monkeypatch, corpus, budget):
    kind, img, plant, whole = corpus
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    if budget:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", budget)
        assert len(img) >= 3 * 4096                                # three slices at least
    for k in (1, 8, 16, 21, 31):
        check(ctx, texts, kind, img, k, min_count=3, max_list=40)
        if kind == "fasta":
            check(ctx, texts, kind, img, k, canonical=True, min_count=3, max_list=40)
    want = check(ctx, texts, kind, img, 32, min_count=2, max_list=1000)
    code = api.kmer_code64(plant, arrow=kind == "arrow")
    assert (whole, code, plant.encode()) in want[2]                 # the whole copies, and not one that lies across two records
    assert want[0]["records"] == 260


# ---- the new route against the merged one ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8, 14])
def test_the_wide_route_is_the_table_route_where_both_exist(ctx, monkeypatch, corpus, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, img, plant, whole = corpus
    for kd, im in ((kind, img), ("fasta", O.golden("ta_small.dexta"))):
        for canonical in ((False, True) if kd == "fasta" else (False,)):
            a = ctx.kmers(kd, im, k, canonical, nspec=64, min_count=2, max_list=500)
            b = ctx.kmers_wide(kd, im, k, canonical, nspec=64, min_count=2, max_list=500)
            assert a[0] == b[0] and list(a[0]) == list(b[0])        # the same keys, the same figures
            assert np.array_equal(a[1], b[1])
            assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in a[2]] == \
                   [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in b[2]]
            assert b[2].dtype == api.KMER64_LIST_DTYPE and (len(b[2]) > 3 or im is not img)      # (the corpus repeats its plant at any k)


def test_a_listed_21_mer_is_found_where_it_was_counted(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, img, plant, whole = corpus
    rep, _, lst = ctx.kmers_wide(kind, img, 21, min_count=2, max_list=60)
    assert 5 < len(lst) <= 60 and all(len(e["letters"]) == 21 for e in lst)
    found, _ = ctx.find(kind, img, [bytes(e["letters"]).decode() for e in lst], max_hits=0)
    assert found["per_pattern"][:, 0].tolist() == [int(e["count"]) for e in lst] and found["per_pattern"][:, 1].sum() == 0


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmers_wide(*args, **kw)
    return e.value


def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    e = refused(ctx, "quiva", O.golden("qv_tiny.dexqv"), 21)
    assert e.code == E_ARG and "dexqv" in str(e)
    e = refused(ctx, "arrow", ar, 21, canonical=True)
    assert e.code == E_ARG and "canonical" in str(e)
    for k in (0, 33):
        e = refused(ctx, "fasta", ta, k)
        assert e.code == E_ARG and "k = %d" % k in str(e)
    e = refused(ctx, "fasta", ta, 21, nspec=1)
    assert e.code == E_ARG and "spectrum" in str(e)
    lib, km, lst, n = ctx.lib, L.Kmers64(), api.C.c_void_p(), api.C.c_uint64()
    km.records = 77
    assert lib.dx_file_kmers_wide(ctx.h, 7, ta, len(ta), 21, 0, 0, 0, api.C.byref(km), None, 0, None, None) == E_ARG
    assert lib.dx_file_kmers_wide(ctx.h, L.DX_KIND_FASTA, ta, len(ta), 21, 0, 1, 5, api.C.byref(km), None, 0, api.C.byref(lst), None) == E_ARG
    assert b"list" in lib.dx_last_error(ctx.h) and km.records == 77
    assert lib.dx_file_kmers_wide(ctx.h, L.DX_KIND_FASTA, ta, len(ta), 21, 0, 0, 0, None, None, 0, None, None) == E_ARG
    assert lib.dx_file_kmers_wide(ctx.h, L.DX_KIND_FASTA, ta, len(ta), 21, 0, 0, 0, api.C.byref(km), None, 0, None, None) == 0
    assert km.records > 0 and km.k == 21
    ctx.kmers_wide("arrow", ar, 32)
    ctx.kmers_wide("fasta", ta, 1, canonical=True, nspec=2)


def test_codes_that_cannot_be_allocated_are_nomem_and_the_report_stays(monkeypatch):
    """DEXGPU_TEST=fail_malloc_over=<bytes>: the image goes up, the array of the codes (8 bytes a window) does not"""
    img = O.golden("ta_small.dexta")
    with api.Context(0) as c:
        windows = c.kmers_wide("fasta", img, 21)[0]["windows"]
        assert 8 * windows > 4 * len(img)
        km, spec = L.Kmers64(), np.full(8, 5, np.uint64)
        km.records = km.windows = 77
        set_flag(monkeypatch, "fail_malloc_over", str(4 * windows))
        rc = c.lib.dx_file_kmers_wide(c.h, L.DX_KIND_FASTA, img, len(img), 21, 0, 0, 0, api.C.byref(km), spec.ctypes.data, 8, None, None)
        set_flag(monkeypatch, "fail_malloc_over", None)
        assert rc == E_NOMEM and str(8 * windows + 64) in c.lib.dx_last_error(c.h).decode()
        assert (km.records, km.windows) == (77, 77) and (spec == 5).all()
        assert c.kmers_wide("fasta", img, 21)[0]["windows"] == windows            # nothing of it is left behind


def test_a_truncated_image_is_unpack2s_error(ctx):
    for kind, name in (("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")):
        img = O.golden(name)
        for cut in (len(img) - 1, len(img) - 37):
            with pytest.raises(L.DexGPUError) as want:
                (ctx.undexta if kind == "fasta" else ctx.undexar)(img[:cut])
            assert refused(ctx, kind, img[:cut], 21).code == want.value.code
