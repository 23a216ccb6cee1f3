"""Context.kmers_wide_files (dx_files_kmers_wide) and Context.kmer_set_files (dx_files_kmer_set) on the GPU against
tests/_kmers_files.py, which counts the k-mers of the JOINED text the oracle's undexta -U / undexar prints for the images: one image
held against the existing route, three images in one pass and in slices, an image without a window among them, passes forced by a
`room` computed from the reference's bins, a list that ends inside a range, a tie of the largest count across two ranges, the set
and a screen against it, and the refusals.  Apart from the first test no expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _kmers_files as KF
import _oracle as O
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM = -1, -6
PLANT = "GGCCAATTGGCCATACGGTTAACCGTATGCAT"      # 32 letters; its halves are laid at the end of one record and the start of the next
GOLDEN = {"fasta": "ta_small.dexta", "arrow": "ar_small.dexar"}


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def synthetic(kind, n=260, seed=7, well0=100):
    """n records of 0 .. 700 symbols: every seventh empty, Ns and lower case among the letters (fasta), PLANT whole in some, and its
    two halves at the end of one record and the start of the next, where it must not be counted"""
    rng = np.random.default_rng(seed)
    letters = "ACGT" if kind == "fasta" else "1234"
    plant = PLANT if kind == "fasta" else PLANT.translate(str.maketrans("ACGT", "1234"))
    out, seqs = [], []
    for i in range(n):
        ln = 0 if i % 7 == 3 else int(rng.integers(1, 701))
        s = "".join(letters[c] for c in rng.integers(0, 4, ln))
        if i % 5 == 0 and ln >= 100:
            s = plant + s[32:ln - 32] + plant
        if i % 11 == 1 and ln >= 60:
            s = s[:-16] + plant[:16]                                # ... and the next record begins with the other half
        if i % 11 == 2 and ln >= 60 and seqs[-1].endswith(plant[:16]):
            s = plant[16:] + s[16:]
        if kind == "fasta" and i % 4 == 1:
            s = "".join(("N" if rng.integers(20) == 0 else c.lower() if rng.integers(2) else c) for c in s)
        seqs.append(s)
        head = f">syn/{well0 + 3 * i}/0_{len(s)} " + ("RQ=0.850" if kind == "fasta" else "SN=6.81,9.99,10.50,4.00")
        out.append(head + "".join("\n" + s[k:k + 70] for k in range(0, len(s), 70)))
    whole = sum(r.upper().replace("N", "A").count(plant) for r in seqs)              # (what undexta -U prints: an N is stored as a)
    assert whole >= 40
    return ("\n".join(out) + "\n").encode(), whole


def pack(ctx, kind, text):
    img = ctx.dexta(text) if kind == "fasta" else ctx.dexar(text)
    assert img == (O.dexta(text) if kind == "fasta" else O.dexar(text))
    return img


class Corpus:
    """three images of a kind -- two synthetic corpora with different seeds that share the planted 32-mer, and a golden -- with the
    oracle's text of each, and the reference's codes and bins of the joined text, made once a (k, canonical)"""
    def __init__(self, ctx, kind):
        self.kind = kind
        (ta, wa), (tb, wb) = synthetic(kind, seed=7), synthetic(kind, seed=8, well0=1000)
        self.whole = wa + wb                                       # the planted 32-mer's whole copies in the two corpora
        self.imgs = [pack(ctx, kind, ta), pack(ctx, kind, tb), O.golden(GOLDEN[kind])]
        self.texts = [F.text_of(kind, im) for im in self.imgs]
        self.have = {}

    def codes(self, k, canonical=False):
        if (k, canonical) not in self.have:
            c = KF.text_codes(self.kind, self.texts, k, canonical)
            self.have[k, canonical] = (c, KF.bins(c, k, KF.bits_for(k)))
        return self.have[k, canonical]


@pytest.fixture(scope="module", params=["fasta", "arrow"])
def corpus(request, ctx):
    return Corpus(ctx, request.param)


def check(ctx, kind, imgs, texts, k, canonical=False, nspec=256, min_count=0, max_list=0, room=0, passes=1):
    want = KF.files_kmers_wide(kind, texts, k, canonical, nspec, min_count, max_list)
    rep, spec, lst = ctx.kmers_wide_files(kind, imgs, k, canonical, nspec, min_count, max_list, room)
    assert rep.pop("passes") == passes and rep.pop("files") == KF.files_of(kind, texts, k)
    assert rep == want[0], (rep, want[0])
    assert np.array_equal(spec, want[1])
    assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in lst] == want[2]
    return want


# ---- the same answer as the existing route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 21, 32])
def test_one_image_is_kmers_wide_of_it(ctx, monkeypatch, corpus, k):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    for img in corpus.imgs[1:]:
        canonical = corpus.kind == "fasta"
        a = ctx.kmers_wide(corpus.kind, img, k, canonical, nspec=64, min_count=2, max_list=500)
        b = ctx.kmers_wide_files(corpus.kind, [img], k, canonical, nspec=64, min_count=2, max_list=500, room=0)
        assert b[0].pop("passes") == 1
        assert b[0].pop("files") == [{f: a[0][f] for f in ("records", "symbols", "windows")}]
        assert a[0] == b[0] and list(a[0]) == list(b[0])            # key for key
        assert np.array_equal(a[1], b[1])
        assert a[2].dtype == b[2].dtype == api.KMER64_LIST_DTYPE and a[2].tobytes() == b[2].tobytes()
        assert len(a[2]) > 3 or img is corpus.imgs[2]                 # (the corpus repeats its plant at any k)


# ---- several images --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [None, "4096"], ids=["whole", "slices"])
def test_three_images(ctx, monkeypatch, corpus, budget):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    if budget:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", budget)
        assert all(len(im) >= 3 * 4096 for im in corpus.imgs[:2])  # three slices at least
    kind = corpus.kind
    for k in (1, 8, 16, 21, 32):
        check(ctx, kind, corpus.imgs, corpus.texts, k, min_count=3, max_list=40)
        if kind == "fasta":
            check(ctx, kind, corpus.imgs, corpus.texts, k, canonical=True, min_count=3, max_list=40)
    plant = PLANT if kind == "fasta" else PLANT.translate(str.maketrans("ACGT", "1234"))
    want = check(ctx, kind, corpus.imgs, corpus.texts, 32, min_count=2, max_list=2000)
    code = api.kmer_code64(plant, arrow=kind == "arrow")
    assert (corpus.whole, code, plant.encode()) in want[2]         # the whole copies of both corpora in one count, none across two records
    assert want[0]["records"] == 2 * 260 + len(F.reads(kind, corpus.texts[2]))


def test_an_image_without_a_window_among_the_three(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind = corpus.kind
    head = b">syn/100/0_0 " + (b"RQ=0.850" if kind == "fasta" else b"SN=6.81,9.99,10.50,4.00") + b"\n"
    empty = pack(ctx, kind, head)
    imgs, texts = [corpus.imgs[0], empty, corpus.imgs[2]], [corpus.texts[0], F.text_of(kind, empty), corpus.texts[2]]
    want = check(ctx, kind, imgs, texts, 21, min_count=1, max_list=30)
    assert KF.files_of(kind, texts, 21)[1] == {"records": 1, "symbols": 0, "windows": 0} and want[0]["windows"] > 0
    room = -(-want[0]["windows"] // 2)
    bins = KF.bins(KF.text_codes(kind, texts, 21), 21, 12)
    check(ctx, kind, imgs, texts, 21, min_count=1, max_list=30, room=room, passes=len(KF.plan(bins, room)) - 1)
    check(ctx, kind, [empty], texts[1:2], 21, min_count=1, max_list=30, passes=0)     # no window at all: nothing is sorted
    check(ctx, kind, [], [], 21, nspec=4, min_count=1, max_list=30, passes=0)         # ... and no image


# ---- forced ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 16, 21, 32])
def test_a_third_of_the_windows_a_pass(ctx, monkeypatch, corpus, k):
    """room is computed FROM THE REFERENCE'S BINS, so the reference alone guarantees that the plan exists"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind = corpus.kind
    for canonical in ((False, True) if kind == "fasta" else (False,)):
        codes, bins = corpus.codes(k, canonical)
        room = -(-len(codes) // 3)
        if int(bins.max()) >= room:                                # (k = 1: four bins, one of them may hold more than a third)
            room = int(bins.max())
        plan = KF.plan(bins, room)
        assert len(plan) - 1 >= (3 if k >= 8 else 2)
        check(ctx, kind, corpus.imgs, corpus.texts, k, canonical, min_count=2, max_list=100, room=room, passes=len(plan) - 1)


@pytest.mark.parametrize("k,budget", [(1, None), (8, "4096"), (21, None)])
def test_the_most_passes(ctx, monkeypatch, corpus, k, budget):
    """room = the largest bin: no plan has more ranges (hundreds of them at k >= 8: every one uploads the three images again)"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    if budget:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", budget)
    kind, canonical = corpus.kind, corpus.kind == "fasta"
    codes, bins = corpus.codes(k, canonical)
    room = int(bins.max())
    plan = KF.plan(bins, room)
    assert k < 8 or len(plan) - 1 >= 3
    check(ctx, kind, corpus.imgs, corpus.texts, k, canonical, min_count=2, max_list=1 << 20, room=room, passes=len(plan) - 1)


# ---- the list and ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count,nspec", [(0, 2), (1, 3), (3, 256)])
def test_a_list_that_ends_inside_the_second_range(ctx, monkeypatch, corpus, min_count, nspec):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, k = corpus.kind, 16
    codes, bins = corpus.codes(k)
    room = -(-len(codes) // (3 if min_count == 3 else 40))         # (ranges of few windows where every code is listed: the list stays short)
    plan = KF.plan(bins, room)
    assert len(plan) - 1 >= 3
    seen, cnt = np.unique(codes, return_counts=True)
    passing = seen[cnt >= max(min_count, 1)]
    per_range = [int(KF.in_range(passing, k, 12, lo, hi).sum()) for lo, hi in zip(plan[:-1], plan[1:])]
    assert per_range[0] >= 1 and per_range[1] >= 2
    max_list = per_range[0] + per_range[1] // 2
    want = check(ctx, kind, corpus.imgs, corpus.texts, k, nspec=nspec, min_count=min_count, max_list=max_list, room=room, passes=len(plan) - 1)
    assert want[0]["listed"] == (max_list if min_count else 0)
    if min_count == 3:                                             # ... and one that no range ends
        check(ctx, kind, corpus.imgs, corpus.texts, k, nspec=nspec, min_count=min_count, max_list=1 << 40, room=room, passes=len(plan) - 1)


def test_a_tie_of_the_largest_count_in_two_ranges(ctx, monkeypatch):
    """two 21-mers planted equally often, far apart in code order, the larger code first in the file: max_code is the smaller"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    rng = np.random.default_rng(21)
    low, high = "ACGTTGCAAGGCTTAACCGGA", "TTGACCGGTAACGTCAGGCTA"
    recs = []
    for i in range(80):
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, 150))
        s = s[:70] + (high if i < 40 else low) + s[70:]
        recs.append(f">syn/{100 + i}/0_{len(s)} RQ=0.850" + "".join("\n" + s[j:j + 70] for j in range(0, len(s), 70)) + "\n")
    a, b = pack(ctx, "fasta", "".join(recs[:50]).encode()), pack(ctx, "fasta", "".join(recs[50:]).encode())
    texts = [F.text_of("fasta", a), F.text_of("fasta", b)]
    codes = KF.text_codes("fasta", texts, 21)
    bins = KF.bins(codes, 21, 12)
    room = -(-len(codes) // 4)
    plan = KF.plan(bins, room)
    c_low, c_high = api.kmer_code64(low), api.kmer_code64(high)
    range_of = lambda c: int(np.searchsorted(plan, c >> 30, side="right")) - 1
    assert range_of(c_low) != range_of(c_high) and len(plan) - 1 >= 4
    seen, cnt = np.unique(codes, return_counts=True)
    assert int(cnt.max()) == 40 and seen[cnt == 40].tolist() == [c_low, c_high]
    want = check(ctx, "fasta", [a, b], texts, 21, min_count=40, max_list=10, room=room, passes=len(plan) - 1)
    assert (want[0]["max_count"], want[0]["max_code"]) == (40, c_low) and [e[1] for e in want[2]] == [c_low, c_high]
    check(ctx, "fasta", [a, b], texts, 21, min_count=40, max_list=10)


# ---- the set over files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_count", [(8, 1), (21, 2), (32, 1)])
def test_the_set_over_files(ctx, monkeypatch, corpus, k, min_count):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, canonical = corpus.kind, corpus.kind == "fasta"
    codes, bins = corpus.codes(k, canonical)
    seen, cnt = np.unique(codes, return_counts=True)
    want = seen[cnt >= min_count]
    rep_want = KF.files_kmers_wide(kind, corpus.texts, k, canonical)[0]
    room = -(-len(codes) // 3)
    for rm, passes in ((0, 1), (room, len(KF.plan(bins, room)) - 1)):
        s, rep = ctx.kmer_set_files(kind, corpus.imgs, k, canonical, min_count, room=rm, report=True)
        with s:
            assert rep.pop("passes") == passes >= (3 if rm else 1)
            assert rep == {f: rep_want[f] for f in rep}
            assert np.array_equal(s.codes(), want)
            info = s.info
            assert (info["codes"], info["k"], info["canonical"], info["arrow"]) == (len(want), k, int(canonical), int(kind == "arrow"))
    with ctx.kmer_set_files(kind, [], k, canonical) as s:
        assert s.info["codes"] == 0


def test_a_screen_against_the_set_of_the_files_is_one_against_the_joined_image(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, canonical = corpus.kind, corpus.kind == "fasta"
    text = b"".join(corpus.texts[:2])
    joined = ctx.dexta(text) if kind == "fasta" else ctx.dexar(text)
    want = F.reads(kind, text)
    got = F.reads(kind, F.text_of(kind, joined))
    assert len(got) == len(want) == 520 and all(np.array_equal(g, w) for g, w in zip(got, want))
    room = -(-len(KF.text_codes(kind, corpus.texts[:2], 21, canonical)) // 3)
    with ctx.kmer_set_files(kind, corpus.imgs[:2], 21, canonical, 2, room=room) as a, ctx.kmer_set(kind, joined, 21, canonical, 2) as b:
        assert np.array_equal(a.codes(), b.codes()) and len(a.codes()) > 20
        ra, rb = ctx.screen(kind, corpus.imgs[2], a), ctx.screen(kind, corpus.imgs[2], b)
        assert ra[0] == rb[0] and ra[1].tobytes() == rb[1].tobytes() and np.array_equal(ra[2], rb[2])
        ra, rb = ctx.screen(kind, corpus.imgs[0], a), ctx.screen(kind, corpus.imgs[0], b)
        assert ra[0] == rb[0] and ra[0]["hits"] > 0 and ra[1].tobytes() == rb[1].tobytes()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmers_wide_files(*args, **kw)
    return e.value


def raw_args(imgs):
    keep = [api.C.c_char_p(b) for b in imgs]
    return (api.C.c_void_p * len(imgs))(*[api.C.cast(p, api.C.c_void_p) for p in keep]), (api.C.c_size_t * len(imgs))(*[len(b) for b in imgs]), keep


def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    e = refused(ctx, "quiva", [O.golden("qv_tiny.dexqv")], 21)
    assert e.code == E_ARG and "dexqv" in str(e) and "dx_files_kmers_wide" in str(e)
    e = refused(ctx, "arrow", [ar, ar], 21, canonical=True)
    assert e.code == E_ARG and "canonical" in str(e)
    for k in (0, 33):
        e = refused(ctx, "fasta", [ta], k)
        assert e.code == E_ARG and "k = %d" % k in str(e)
    e = refused(ctx, "fasta", [ta], 21, nspec=1)
    assert e.code == E_ARG and "spectrum" in str(e)
    with pytest.raises(L.DexGPUError) as e:
        ctx.kmer_set_files("fasta", [ta], 21, min_count=0)
    assert e.value.code == E_ARG and "min_count" in str(e.value) and "dx_files_kmer_set" in str(e.value)
    lib, km, lst, n, p = ctx.lib, L.Kmers64(), api.C.c_void_p(), api.C.c_uint64(), api.C.c_uint32(99)
    imgs, sizes, keep = raw_args([ta, ta])
    km.records = 77
    assert lib.dx_files_kmers_wide(ctx.h, L.DX_KIND_FASTA, imgs, sizes, 2, 21, 0, 1, 5, 0, api.C.byref(km), None, 0, api.C.byref(lst), None,
                                   None, api.C.byref(p)) == E_ARG
    assert b"list" in lib.dx_last_error(ctx.h) and km.records == 77 and p.value == 99
    assert lib.dx_files_kmers_wide(ctx.h, L.DX_KIND_FASTA, imgs, sizes, 2, 21, 0, 0, 0, 0, None, None, 0, None, None, None, None) == E_ARG
    assert lib.dx_files_kmers_wide(ctx.h, L.DX_KIND_FASTA, None, sizes, 2, 21, 0, 0, 0, 0, api.C.byref(km), None, 0, None, None, None, None) == E_ARG
    assert lib.dx_files_kmers_wide(ctx.h, L.DX_KIND_FASTA, imgs, sizes, 2, 21, 0, 0, 0, 0, api.C.byref(km), None, 0, None, None, None, None) == 0
    assert km.records == 2 * len(F.reads("fasta", F.text_of("fasta", ta))) and km.k == 21


def test_a_room_under_the_largest_bin_is_nomem_and_names_the_bin(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    rng = np.random.default_rng(3)
    recs = [f">syn/{100 + i}/0_3000 RQ=0.850\n" + "A" * 3000 + "\n" for i in range(3)]
    recs += [f">syn/{200 + i}/0_500 RQ=0.850\n" + "".join("ACGT"[c] for c in rng.integers(0, 4, 500)) + "\n" for i in range(20)]
    img = pack(ctx, "fasta", "".join(recs).encode())
    text = F.text_of("fasta", img)
    bins = KF.bins(KF.text_codes("fasta", [text], 21), 21, 12)
    assert int(np.argmax(bins)) == 0 and int(bins[0]) >= 3 * 2980
    with pytest.raises(KF.BinTooLarge) as want:
        KF.plan(bins, int(bins[0]) - 1)
    e = refused(ctx, "fasta", [img], 21, room=int(bins[0]) - 1)
    assert e.code == E_NOMEM and "bin %d " % want.value.bin in str(e) and "%d windows" % want.value.windows in str(e)
    with pytest.raises(L.DexGPUError) as e2:
        ctx.kmer_set_files("fasta", [img], 21, room=int(bins[0]) - 1)
    assert e2.value.code == E_NOMEM and "bin 0 " in str(e2.value)
    check(ctx, "fasta", [img], [text], 21, min_count=1, max_list=10, room=int(bins[0]), passes=len(KF.plan(bins, int(bins[0]))) - 1)


def test_a_truncated_second_image_is_unpack2s_error_and_names_the_image(ctx):
    for kind, name in (("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")):
        img = O.golden(name)
        for cut in (len(img) - 1, len(img) - 37):
            with pytest.raises(L.DexGPUError) as want:
                (ctx.undexta if kind == "fasta" else ctx.undexar)(img[:cut])
            e = refused(ctx, kind, [img, img[:cut], img], 21)
            assert e.code == want.value.code and "image 1" in str(e)
            km, spec, p = L.Kmers64(), np.full(8, 5, np.uint64), api.C.c_uint32(99)
            km.records = km.windows = 77
            imgs, sizes, keep = raw_args([img, img[:cut]])
            rc = ctx.lib.dx_files_kmers_wide(ctx.h, api._kind(kind), imgs, sizes, 2, 21, 0, 0, 0, 0, api.C.byref(km), spec.ctypes.data, 8, None, None,
                                             None, api.C.byref(p))
            assert rc == want.value.code and (km.records, km.windows, p.value) == (77, 77, 99) and (spec == 5).all()
            with pytest.raises(L.DexGPUError) as e2:
                ctx.kmer_set_files(kind, [img[:cut]], 21)
            assert e2.value.code == want.value.code and "image 0" in str(e2.value)


def test_codes_that_cannot_be_allocated_are_nomem_and_a_following_call_succeeds(monkeypatch):
    """DEXGPU_TEST=fail_malloc_over=<bytes>: the images go up, the array of the codes (8 bytes a window) does not"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden("ta_small.dexta")
    text = F.text_of("fasta", img)
    with api.Context(0) as c:
        windows = KF.files_of("fasta", [text, text], 21)
        windows = windows[0]["windows"] + windows[1]["windows"]
        assert 8 * windows > 4 * len(img)
        for room in (0, -(-windows // 2)):                          # one pass; and the passes' largest range, which is a fourth at least
            set_flag(monkeypatch, "fail_malloc_over", str(windows))
            with pytest.raises(L.DexGPUError) as e:
                c.kmers_wide_files("fasta", [img, img], 21, room=room)
            with pytest.raises(L.DexGPUError) as e2:
                c.kmer_set_files("fasta", [img, img], 21, room=room)
            set_flag(monkeypatch, "fail_malloc_over", None)
            assert e.value.code == E_NOMEM and e2.value.code == E_NOMEM
            check(c, "fasta", [img, img], [text, text], 21, min_count=2, max_list=20, room=room,
                  passes=len(KF.plan(KF.bins(KF.text_codes("fasta", [text, text], 21), 21, 12), room)) - 1)       # nothing of it is left behind
