"""Context.screen (dx_file_screen), api.screen_select and Context.subset on the GPU against tests/_screen.py, which works on the TEXT
the oracle prints for an image: every 2-bit golden against the set of its own k-mers and against another image's, the answer in slices
record for record the unsliced one, a set of the wrong kind, and the planted case -- reads cut from a reference on both strands among
random ones, screened, selected and dropped, the image that is left held byte for byte against the oracle's dexta of the others' text.
No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _oracle as O
import _screen as S
import _subset as SUB
import _u2_slices as U2
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


def same(got, want):
    (grep, grec, glen), (wrep, wrec, wlen) = got, want
    assert grep == wrep, (grep, wrep)
    assert grec.dtype == api.SCREEN_DTYPE and np.array_equal(glen, wlen)
    diff = np.flatnonzero(grec != wrec)
    assert len(diff) == 0, [(int(j), tuple(grec[j]), tuple(wrec[j])) for j in diff[:5]]


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 32])
@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_an_image_against_its_own_k_mers_is_covered(ctx, monkeypatch, kind, name, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    lens = np.array([len(r) for r in F.reads(kind, F.text_of(kind, img))], np.int64)
    with ctx.kmer_set(kind, img, k, canonical=kind == "fasta") as s:
        rep, rec, rec_len = ctx.screen(kind, img, s)
    assert np.array_equal(rec_len, lens) and (lens >= k).any()
    assert (rec["covered"] == np.where(lens >= k, lens, 0)).all() and (rec["hits"] == np.maximum(lens - k + 1, 0)).all()
    assert (rec["first"] == np.where(lens >= k, 0, S.NONE)).all() and (rec["last"] == np.where(lens >= k, lens - k, S.NONE)).all()
    assert rep == {"records": len(lens), "symbols": int(lens.sum()), "windows": int(np.maximum(lens - k + 1, 0).sum()),
                   "hits": int(np.maximum(lens - k + 1, 0).sum()), "covered": int(lens[lens >= k].sum()),
                   "records_hit": int((lens >= k).sum()), "k": k}


@pytest.mark.parametrize("kind,name,other,k", [("fasta", "ta_small.dexta", "ta_lower_w60.dexta", 8), ("fasta", "ta_lower_w60.dexta", "ta_small.swapped.dexta", 9),
                                               ("fasta", "ta_edge.dexta", "ta_small.dexta", 7), ("arrow", "ar_small.dexar", "ar_edge.dexar", 5),
                                               ("arrow", "ar_edge.dexar", "ar_small.dexar", 6)])
def test_an_image_against_another_images_k_mers(ctx, monkeypatch, kind, name, other, k):
    """k small enough that two unrelated images share some of their k-mers and not all"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, oth = O.golden(name), O.golden(other)
    canonical = kind == "fasta"
    codes = S.distinct(F.reads(kind, F.text_of(kind, oth)), k, canonical)
    want = S.file_screen(kind, F.text_of(kind, img), k, canonical, codes)
    with ctx.kmer_set(kind, oth, k, canonical=canonical) as s:
        assert np.array_equal(s.codes(), codes)
        got = ctx.screen(kind, img, s)
    same(got, want)
    assert 0 < want[0]["hits"] < want[0]["windows"] and 0 < want[0]["covered"] < want[0]["symbols"]
    for kw in ({}, {"min_hits": 3}, {"min_permille": 300}, {"min_permille": 300, "drop": True}):
        assert api.screen_select(got[1], got[2], **kw).tolist() == S.select(want[1], want[2], **kw)


# ---- slices ----------------------------------------------------------------------------------------------------------------------------
def test_the_answer_does_not_depend_on_the_slicing(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    text, lens = U2.synthetic()
    img = U2.image(ctx.dexta, text)
    k = 15
    rs = F.reads("fasta", F.text_of("fasta", img))
    assert [len(r) for r in rs] == lens and U2.slices(lens, 4096) >= 3
    own = S.distinct(rs, k, True)
    codes = own[np.random.default_rng(1).integers(0, 3, len(own)) == 0]
    want = S.file_screen("fasta", F.text_of("fasta", img), k, True, codes)
    with ctx.kmer_set_from_codes(codes, k, canonical=True) as s:
        whole = ctx.screen("fasta", img, s)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
        sliced = ctx.screen("fasta", img, s)
    same(whole, want)
    same(sliced, whole)
    assert 0 < want[0]["records_hit"] < want[0]["records"]              # (the empty records have no hit)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    with ctx.kmer_set("fasta", ta, 15) as fs, ctx.kmer_set("arrow", ar, 15) as as_:
        for kind, img, s in (("arrow", ar, fs), ("fasta", ta, as_)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.screen(kind, img, s)
            assert e.value.code == E_ARG and "dx_file_screen" in str(e.value)
        with pytest.raises(L.DexGPUError) as e:
            ctx.screen("quiva", O.golden("qv_tiny.dexqv"), fs)
        assert e.value.code == E_ARG and "dexqv" in str(e.value)
        with pytest.raises(L.DexGPUError) as e:
            ctx.screen("fasta", ta, None)
        assert e.value.code == E_ARG and "set" in str(e.value)
        rp = L.ScreenReport()
        rp.records = 77
        assert ctx.lib.dx_file_screen(ctx.h, 7, ta, len(ta), fs.h, api.C.byref(rp), None, None) == E_ARG
        assert ctx.lib.dx_file_screen(ctx.h, L.DX_KIND_FASTA, ta, len(ta), fs.h, None, None, None) == E_ARG and rp.records == 77
        for cut in (len(ta) - 1, len(ta) - 37):                        # a truncated image is unpack2's error
            with pytest.raises(L.DexGPUError) as want:
                ctx.undexta(ta[:cut])
            with pytest.raises(L.DexGPUError) as e:
                ctx.screen("fasta", ta[:cut], fs)
            assert e.value.code == want.value.code
        assert ctx.lib.dx_file_screen(ctx.h, L.DX_KIND_FASTA, ta, len(ta), fs.h, api.C.byref(rp), None, None) == 0      # the report alone
        assert rp.records == 12 and rp.hits == rp.windows > 0 and rp.k == 15


# ---- the planted case ------------------------------------------------------------------------------------------------------------------
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def planted(seed=11):
    """a random reference of 3000 symbols and 40 records of 200 to 900 symbols, 12 of them substrings of it, half of those
    reverse-complemented -> (the reference, the text, the planted records' indices)"""
    rng = np.random.default_rng(seed)
    ref = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
    from_ref = sorted(int(i) for i in rng.choice(40, 12, replace=False))
    out = []
    for i in range(40):
        ln = int(rng.integers(200, 901))
        if i in from_ref:
            at = int(rng.integers(0, 3000 - ln + 1))
            s = ref[at:at + ln]
            if from_ref.index(i) % 2:
                s = revcomp(s)
        else:
            s = "".join("ACGT"[c] for c in rng.integers(0, 4, ln))
        out.append(f">plant/{11 + 3 * i}/0_{ln} RQ=0.850" + "".join("\n" + s[j:j + 80] for j in range(0, ln, 80)))
    return ref, ("\n".join(out) + "\n").encode(), from_ref


def test_reads_of_a_reference_are_screened_out_and_the_rest_is_the_oracles_image(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    k = 15
    ref, text, from_ref = planted()
    img = O.dexta(text)
    decoded = F.text_of("fasta", img)
    ref_codes = S.distinct([np.array(["ACGT".index(c) for c in ref], np.uint8)], k, True)
    # the input first, WITH THE STATEMENT: 900 permille selects exactly the 12
    want = S.file_screen("fasta", decoded, k, True, ref_codes)
    assert S.select(want[1], want[2], min_permille=900) == from_ref and len(from_ref) == 12
    others = S.select(want[1], want[2], min_permille=900, drop=True)
    assert len(others) == 28 and sorted(others + from_ref) == list(range(40))
    # then the library: the set from letters of one strand, the screen, the selection, the subset
    fwd = np.array([api.kmer_code64(ref[p:p + k]) for p in range(len(ref) - k + 1)], np.uint64)
    with ctx.kmer_set_from_codes(fwd, k, canonical=True) as s:
        assert np.array_equal(s.codes(), ref_codes)
        got = ctx.screen("fasta", img, s)
    same(got, want)
    ids = api.screen_select(got[1], got[2], min_permille=900, drop=True)
    assert ids.tolist() == others
    assert api.screen_select(got[1], got[2], min_permille=900).tolist() == from_ref
    left = ctx.subset("fasta", img, ids=ids)
    assert left == O.dexta(SUB.cut("fasta", decoded, [(i, None, None) for i in others]))
    kept = ctx.subset("fasta", img, ids=api.screen_select(got[1], got[2], min_permille=900))
    assert kept == O.dexta(SUB.cut("fasta", decoded, [(i, None, None) for i in from_ref]))
