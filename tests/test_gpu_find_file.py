"""Context.find (dx_file_find) on the GPU against tests/_find.py, which searches the TEXT the oracle's undexta -U / undexar prints for
the image: the goldens and their legacy and byte-swapped variants, images this library packs from small synthetic texts (empty
records, Ns, lower case, a pattern that lies across two records, both strands, a palindrome), every cap, the same in slices, and
the refusals.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
FASTA_PATTERNS = ["ACGT", "ttttcc", "GATC", "CAAAC", "A", "GGCCAATTGGCC"]         # (ACGT, GATC and the last are their own reverse complements)
ARROW_PATTERNS = ["1234", "11", "4", "32123"]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def check(ctx, kind, img, patterns, **kw):
    want = F.file_find(kind, F.text_of(kind, img), patterns, kw.get("max_mismatches", 0), kw.get("both_strands", False),
                       kw.get("max_hits", 1 << 20))
    got = ctx.find(kind, img, patterns, per_record=True, **kw)
    F.assert_same_find(got, want)
    plain = ctx.find(kind, img, patterns, **kw)                   # (no per-record array: the same report and list)
    assert "rec_hits" not in plain[0]
    F.assert_same_find(plain, want)
    return want


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
GOLDEN = [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("fasta", "ta_lower_w60.dexta"), ("fasta", "ta_small.legacy.dexta"),
          ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_edge.dexar"),
          ("arrow", "ar_small.dexar"), ("arrow", "ar_small.swapped.dexar")]


@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_goldens(ctx, monkeypatch, kind, name):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    pats = FASTA_PATTERNS if kind == "fasta" else ARROW_PATTERNS
    want = check(ctx, kind, img, pats)
    assert want[0]["hits"] > 0
    check(ctx, kind, img, [p for p in pats if len(p) > 1][:3], max_mismatches=1)
    if kind == "fasta":
        both = check(ctx, kind, img, pats, both_strands=True)
        assert both[0]["per_pattern"][0, 1] == 0                   # (a palindrome reports strand 0 only)
        assert both[0]["per_pattern"][3, 1] > 0 or "ta_small" not in name
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
    check(ctx, kind, img, pats)


def test_the_golden_figures_counted_by_hand(ctx):
    """tests/test_find_host.py counts these in ta_edge's text by hand"""
    rep, lst = ctx.find("fasta", O.golden("ta_edge.dexta"), ["TACG", "ACGT"], both_strands=True, per_record=True)
    assert rep["per_pattern"].tolist() == [[43, 44], [45, 0]] and rep["hits"] == 132 and rep["records_hit"] == 3
    assert rep["rec_hits"].tolist() == [2, 0, 3, 0, 0, 0, 0, 127, 0]
    assert [tuple(h) for h in lst[:5]] == [(0, 0, 1, 0, 0), (0, 1, 0, 1, 0), (2, 0, 1, 0, 0), (2, 1, 0, 1, 0), (2, 3, 0, 0, 0)]


# ---- synthetic texts, packed by this library -------------------------------------------------------------------------------------------
PLANT = "GGCCAATTGGCC"


def synthetic(kind, n=260, seed=7):
    """n records of 0 .. 700 symbols: every seventh empty, Ns and lower case among the letters (fasta), PLANT at the start, in the
    middle and at the end of some, and its two halves at the end of one record and the start of the next, where it must not be found"""
    rng = np.random.default_rng(seed)
    letters = "ACGT" if kind == "fasta" else "1234"
    plant = PLANT if kind == "fasta" else "123443211234"
    out, seqs = [], []
    for i in range(n):
        ln = 0 if i % 7 == 3 else int(rng.integers(1, 701))
        s = "".join(letters[c] for c in rng.integers(0, 4, ln))
        if i % 5 == 0 and ln >= 40:
            s = plant + s[12:ln // 2] + plant + s[ln // 2 + 12:ln - 12] + plant
        if i % 11 == 1 and ln >= 6:
            s = s[:-6] + plant[:6]                                  # ... and the next record begins with the other half
        if i % 11 == 2 and ln >= 6 and seqs[-1].endswith(plant[:6]):
            s = plant[6:] + s[6:]
        if kind == "fasta" and i % 4 == 1:
            s = "".join(("N" if rng.integers(20) == 0 else c.lower() if rng.integers(2) else c) for c in s)
        seqs.append(s)
        head = f">syn/{100 + 3 * i}/0_{len(s)} " + ("RQ=0.850" if kind == "fasta" else "SN=6.81,9.99,10.50,4.00")
        out.append(head + "".join("\n" + s[k:k + 70] for k in range(0, len(s), 70)))
    return ("\n".join(out) + "\n").encode(), plant


@pytest.fixture(scope="module", params=["fasta", "arrow"])
def corpus(request, ctx):
    text, plant = synthetic(request.param)
    img = ctx.dexta(text) if request.param == "fasta" else ctx.dexar(text)
    oracle = O.dexta(text) if request.param == "fasta" else O.dexar(text)
    assert img == oracle
    return request.param, img, plant


def test_synthetic_texts(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, img, plant = corpus
    pats = [plant, plant[:6], plant[6:], plant[3:5]] + (["acgt", "TTTTT"] if kind == "fasta" else ["4444"])
    want = check(ctx, kind, img, pats)
    assert want[0]["records"] == 260 and want[0]["per_pattern"][0, 0] >= 3 * 30 and want[0]["records_hit"] < 260
    lens = [len(r) for r in F.reads(kind, F.text_of(kind, img))]
    ends = {int(h["record"]) for h in want[1] if h["query"] == 1 and h["pos"] + 6 == lens[int(h["record"])]}
    begins = {int(h["record"]) for h in want[1] if h["query"] == 2 and h["pos"] == 0}
    across = {r for r in ends if r + 1 in begins}                  # PLANT lies across these records' ends: its halves are found,
    assert len(across) >= 5                                        # ... the whole is not: the reference reads record by record
    assert not any(h["query"] == 0 and h["pos"] + 12 > lens[int(h["record"])] for h in want[1])
    check(ctx, kind, img, pats[:2], max_mismatches=2)
    if kind == "fasta":
        both = check(ctx, kind, img, pats, both_strands=True)
        assert both[0]["per_pattern"][0, 1] == 0                   # (PLANT is its own reverse complement)
        assert both[0]["per_pattern"][1, 1] == both[0]["per_pattern"][2, 0]     # (GGCCAA's reverse complement is TTGGCC, pattern 2)


def test_max_hits_below_at_and_above_the_total(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    kind, img, plant = corpus
    pats = [plant[:3], plant]
    total = F.file_find(kind, F.text_of(kind, img), pats)[0]["hits"]
    assert total > 100
    for most in (0, 1, total // 2, total - 1, total, total + 1):
        want = check(ctx, kind, img, pats, max_hits=most)
        assert want[0]["listed"] == min(most, total) and want[0]["hits"] == total


def test_slices_give_the_one_slice_report(ctx, monkeypatch, corpus):
    kind, img, plant = corpus
    pats = [plant, plant[:4], plant[4:9]]
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    whole = ctx.find(kind, img, pats, max_mismatches=1, both_strands=kind == "fasta", per_record=True)
    total = whole[0]["hits"]
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    assert len(img) >= 3 * 4096                                    # three slices at least
    F.assert_same_find(ctx.find(kind, img, pats, max_mismatches=1, both_strands=kind == "fasta", per_record=True), whole)
    check(ctx, kind, img, pats, max_mismatches=1, both_strands=kind == "fasta")
    for most in (1, total // 3, total - 1):                        # (the cap runs across the slices as if there were none)
        check(ctx, kind, img, pats, max_mismatches=1, max_hits=most)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        ctx.find(*args, **kw)
    return e.value


def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    e = refused(ctx, "quiva", O.golden("qv_tiny.dexqv"), ["ACGT"])
    assert e.code == E_ARG and "dexqv" in str(e)
    e = refused(ctx, "fasta", ta, ["ACGT", "ACNT"])
    assert e.code == E_ARG and "pattern 1" in str(e) and "column 3" in str(e)
    e = refused(ctx, "arrow", ar, ["12345"])
    assert e.code == E_ARG and "pattern 0" in str(e) and "column 5" in str(e)
    assert refused(ctx, "fasta", ta, ["A" * 33]).code == E_ARG
    assert refused(ctx, "fasta", ta, [""]).code == E_ARG
    assert refused(ctx, "fasta", ta, []).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGT"] * 65).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGT"] * 33, both_strands=True).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGTACGT", "ACG"], max_mismatches=3).code == E_ARG
    assert refused(ctx, "arrow", ar, ["1234"], both_strands=True).code == E_ARG
    ctx.find("fasta", ta, ["ACGT"] * 32, both_strands=True)        # (32 palindromes: 32 queries)
    ctx.find("fasta", ta, ["ACGTACGT", "ACG"], max_mismatches=2)


def test_a_truncated_image_is_unpack2s_error(ctx):
    for kind, name in (("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")):
        img = O.golden(name)
        for cut in (len(img) - 1, len(img) - 37):
            with pytest.raises(L.DexGPUError) as want:
                (ctx.undexta if kind == "fasta" else ctx.undexar)(img[:cut])
            assert refused(ctx, kind, img[:cut], ["ACGT" if kind == "fasta" else "1234"]).code == want.value.code
