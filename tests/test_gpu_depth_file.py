"""Context.depth (dx_file_depth), the counted sets of images (Context.kmer_set_counted, kmer_set_files_counted), api.depth_select and
Context.subset on the GPU against tests/_depth.py, which works on the TEXT the oracle prints for an image: the goldens against their own
counted k-mers, the answer in slices record for record the unsliced one (the profile and its places too), the counted set of two
images in several passes, the refusals, and the selection by the median applied to the .dexta and its .dexar.  No expected value comes
from the library."""
import numpy as np
import pytest

import _depth as D
import _find as F
import _kmers_files as KF
import _oracle as O
import _subset as SUB
import _u2_slices as U2
from dextractor_amd import _lib as L
from dextractor_amd import api
from dextractor_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = -1
GOLDEN = [("fasta", "ta_small.dexta"), ("fasta", "ta_edge.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_small.dexar"),
          ("arrow", "ar_edge.dexar")]
_texts = {}


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def text_of(kind, name):
    """the oracle's text of a golden, made once"""
    if name not in _texts:
        _texts[name] = F.text_of(kind, O.golden(name))
    return _texts[name]


def same(got, want):
    (grep, grec, glen, gprof, goff), (wrep, wrec, wlen, wprof, woff) = got, want
    assert grep == wrep, (grep, wrep)
    assert np.array_equal(glen, wlen) and goff.dtype == np.uint64 and np.array_equal(goff, woff)
    D.same_entries(grec, wrec)
    assert gprof.dtype == np.uint16 and np.array_equal(gprof, wprof), np.flatnonzero(gprof != wprof)[:8]


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("k", [4, 15, 32])
@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_an_image_against_its_own_counted_k_mers(ctx, monkeypatch, kind, name, k, min_count):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, text = O.golden(name), text_of(kind, name)
    canonical = kind == "fasta"
    codes, counts = D.counted(F.reads(kind, text), k, canonical, min_count)
    want = D.file_depth(kind, text, k, canonical, codes, counts)
    with ctx.kmer_set_counted(kind, img, k, canonical=canonical, min_count=min_count) as s:
        assert s.counted and np.array_equal(s.codes(), codes) and np.array_equal(s.counts(), counts)
        with ctx.kmer_set(kind, img, k, canonical=canonical, min_count=min_count) as plain:
            assert not plain.counted and plain.codes().tobytes() == s.codes().tobytes()
        got = ctx.depth(kind, img, s, profile=True)
        same(got, want)
        brief = ctx.depth(kind, img, s)                                # without the profile: the same entries
        assert len(brief) == 3 and brief[0] == got[0] and brief[1].tobytes() == got[1].tobytes() and np.array_equal(brief[2], got[2])
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # in slices: the same answer, profile and places included
        same(ctx.depth(kind, img, s, profile=True), want)
    rep = got[0]
    if min_count == 1:
        assert rep["hits"] == rep["windows"] and int(counts.max(initial=0)) < 65535
        assert rep["sum"] == int((counts.astype(np.uint64) ** 2).sum())   # a code seen c times is c windows of depth c
    elif k == 4 and "small" in name:
        assert 0 < rep["hits"] <= rep["windows"]


def test_the_answer_does_not_depend_on_the_slicing(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    text, lens = U2.synthetic()
    img = U2.image(ctx.dexta, text)
    k = 15
    decoded = F.text_of("fasta", img)
    rs = F.reads("fasta", decoded)
    assert [len(r) for r in rs] == lens and U2.slices(lens, 4096) >= 3
    codes, counts = D.counted(rs, k, True)
    rng = np.random.default_rng(1)
    keep = rng.integers(0, 3, len(codes)) > 0
    pairs = [(int(c), int(x)) for c, x in zip(codes[keep], rng.choice([1, 2, 300, 65535, 70000], int(keep.sum())))]
    codes, counts = D.from_kmers(pairs, k, True)
    want = D.file_depth("fasta", decoded, k, True, codes, counts)
    with ctx.kmer_set_from_kmers(pairs, k, canonical=True) as s:
        whole = ctx.depth("fasta", img, s, profile=True)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
        sliced = ctx.depth("fasta", img, s, profile=True)
    same(whole, want)
    same(sliced, whole)
    assert 0 < want[0]["hits"] < want[0]["windows"] and 0 < want[0]["records_hit"] < want[0]["records"]


# ---- the counted set of several images, in passes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 15, 32])
def test_the_counted_set_of_two_images_in_several_passes(ctx, monkeypatch, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    names = ["ta_small.dexta", "ta_edge.dexta"]
    imgs, texts = [O.golden(n) for n in names], [text_of("fasta", n) for n in names]
    units = [r for t in texts for r in F.reads("fasta", t)]
    every = KF.text_codes("fasta", texts, k, True)
    bins = KF.bins(every, k, KF.bits_for(k))
    room = max(-(-len(every) // 3), int(bins.max()))                   # from the reference's bins: the plan exists
    ranges = len(KF.plan(bins, room)) - 1
    assert ranges >= 2
    for min_count in (1, 2):
        codes, counts = D.counted(units, k, True, min_count)
        with ctx.kmer_set_files_counted("fasta", imgs, k, canonical=True, min_count=min_count, room=room, report=True)[0] as s:
            assert s.counted and np.array_equal(s.codes(), codes) and np.array_equal(s.counts(), counts)
        s, rep = ctx.kmer_set_files_counted("fasta", imgs, k, canonical=True, min_count=min_count, report=True)      # ... and in one
        with s:
            assert rep["passes"] == 1 and np.array_equal(s.codes(), codes) and np.array_equal(s.counts(), counts)
        with ctx.kmer_set_files("fasta", imgs, k, canonical=True, min_count=min_count, room=room) as plain:
            assert not plain.counted and np.array_equal(plain.codes(), codes)
    s, rep = ctx.kmer_set_files_counted("fasta", imgs, k, canonical=True, room=room, report=True)
    with s:
        assert rep["passes"] == ranges and rep["windows"] == len(every)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    with ctx.kmer_set_counted("fasta", ta, 15) as fs, ctx.kmer_set_counted("arrow", ar, 15) as as_:
        for kind, img, s in (("arrow", ar, fs), ("fasta", ta, as_)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.depth(kind, img, s)
            assert e.value.code == E_ARG and "dx_file_depth" in str(e.value)
        with pytest.raises(L.DexGPUError) as e:
            ctx.depth("quiva", O.golden("qv_tiny.dexqv"), fs)
        assert e.value.code == E_ARG and "dexqv" in str(e.value)
        with pytest.raises(L.DexGPUError) as e:
            ctx.depth("fasta", ta, None)
        assert e.value.code == E_ARG and "set" in str(e.value)
        rp = L.DepthReport()
        rp.records = 77
        assert ctx.lib.dx_file_depth(ctx.h, 7, ta, len(ta), fs.h, api.C.byref(rp), None, None, None, None) == E_ARG
        assert ctx.lib.dx_file_depth(ctx.h, L.DX_KIND_FASTA, ta, len(ta), fs.h, None, None, None, None, None) == E_ARG and rp.records == 77
        with pytest.raises(L.DexGPUError) as want:
            ctx.undexta(ta[:len(ta) - 37])                              # a truncated image is unpack2's error
        with pytest.raises(L.DexGPUError) as e:
            ctx.depth("fasta", ta[:len(ta) - 37], fs)
        assert e.value.code == want.value.code and rp.records == 77
        assert ctx.lib.dx_file_depth(ctx.h, L.DX_KIND_FASTA, ta, len(ta), fs.h, api.C.byref(rp), None, None, None, None) == 0   # the report alone
        assert rp.records == 12 and rp.hits == rp.windows > 0 and rp.k == 15
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_set_counted("fasta", ta, 15, min_count=0)
    assert e.value.code == E_ARG


# ---- count the data set, depth of every read, subset by median -------------------------------------------------------------------------
def planted(seed=12):
    """30 records: 20 cut from one reference of 2000 symbols (every k-mer of it seen many times), 10 random ones (every k-mer once);
    and an .arrow text of records of the same lengths -> (the .fasta, the .arrow, the 20 records' indices)"""
    rng = np.random.default_rng(seed)
    ref = "".join("ACGT"[c] for c in rng.integers(0, 4, 2000))
    deep = sorted(int(i) for i in rng.choice(30, 20, replace=False))
    out, lens = [], []
    for i in range(30):
        ln = int(rng.integers(300, 901))
        at = int(rng.integers(0, 2000 - ln + 1))
        s = ref[at:at + ln] if i in deep else "".join("ACGT"[c] for c in rng.integers(0, 4, ln))
        out.append(f">plant/{11 + 3 * i}/0_{ln} RQ=0.850" + "".join("\n" + s[j:j + 80] for j in range(0, ln, 80)))
        lens.append(ln)
    return ("\n".join(out) + "\n").encode(), synth.make_seqfile("arrow", 30, seed=seed, lens=np.array(lens, np.uint32)).text, deep


def test_reads_are_selected_by_their_median_depth_and_the_rest_is_the_oracles_image(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    k = 15
    fasta, arrow, deep = planted()
    ta, ar = O.dexta(fasta), O.dexar(arrow)
    decoded, decoded_ar = F.text_of("fasta", ta), F.text_of("arrow", ar)
    # the input first, WITH THE STATEMENT: a median of 3 at least selects exactly the 20
    codes, counts = D.counted(F.reads("fasta", decoded), k, True)
    want = D.file_depth("fasta", decoded, k, True, codes, counts)
    assert D.select(want[1], "median", 3, 65535) == deep and len(deep) == 20
    shallow = D.select(want[1], "median", 3, 65535, drop=True)
    assert len(shallow) == 10 and (want[1]["median"][shallow] == 1).all()
    # then the library: count the data set, depth of every read, subset by median
    with ctx.kmer_set_counted("fasta", ta, k, canonical=True) as s:
        rep, rec, rec_len = ctx.depth("fasta", ta, s)
    D.same_entries(rec, want[1])
    assert rep == want[0]
    for kw in ({"lo": 3}, {"lo": 3, "drop": True}, {"stat": "max", "lo": 2, "hi": 9}, {"stat": "q1", "hi": 1, "min_windows": 500}):
        ids = api.depth_select(rec, **kw)
        assert ids.tolist() == D.select(want[1], **{"stat": "median", "lo": 0, "hi": 65535, **kw})
    ids = api.depth_select(rec, "median", lo=3)
    assert ids.tolist() == deep
    assert ctx.subset("fasta", ta, ids=ids) == O.dexta(SUB.cut("fasta", decoded, [(i, None, None) for i in deep]))
    assert ctx.subset("arrow", ar, ids=ids) == O.dexar(SUB.cut("arrow", decoded_ar, [(i, None, None) for i in deep]))
