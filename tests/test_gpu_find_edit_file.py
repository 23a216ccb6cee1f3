"""Context.find_edit (dx_file_find_edit) on the GPU against tests/_find_edit.py, which applies the DP and the valley rule to the TEXT the
oracle's undexta -U / undexar prints for the image: the goldens and their legacy and byte-swapped variants, both strands with a
palindrome and a planted reverse complement that lacks a letter, max_hits across slices, the per-record counts, and the refusals.
No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_edit as E
import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG = -1
FASTA_PATTERNS = ["ACGTAC", "ttttcc", "GATC", "CAAACGGT", "GGCCAATTGGCC", "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT"]   # (GATC and GGCC.. are
ARROW_PATTERNS = ["1234", "112", "32123", "4444333322221111"]                                    # their own reverse complements; the last: 45 nt)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def check(ctx, kind, img, patterns, full=None, **kw):
    """full: the reference's answer without a cap, computed once by the caller: the answer for max_hits is its first max_hits hits"""
    most = kw.get("max_hits", 1 << 20)
    if full is None:
        full = E.file_find_edit(kind, F.text_of(kind, img), patterns, kw.get("max_errors", 0), kw.get("both_strands", False), 1 << 40)
    want = dict(full[0], listed=min(full[0]["hits"], most)), full[1][:most]
    got = ctx.find_edit(kind, img, patterns, per_record=True, **kw)
    F.assert_same_find(got, want)
    plain = ctx.find_edit(kind, img, patterns, **kw)              # (no per-record array: the same report and list)
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
    assert check(ctx, kind, img, pats + ["A" if kind == "fasta" else "4"])[0]["hits"] > 0
    one = check(ctx, kind, img, pats, max_errors=1)
    two = check(ctx, kind, img, pats[1:], max_errors=2)
    assert one[0]["hits"] > 0 and two[0]["records_hit"] > 0
    if kind == "fasta":
        both = check(ctx, kind, img, pats, both_strands=True, max_errors=1)
        assert both[0]["per_pattern"][2, 1] == 0 and both[0]["per_pattern"][4, 1] == 0       # (a palindrome reports strand 0 only)
        assert both[0]["per_pattern"][0, 1] > 0
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
    check(ctx, kind, img, pats, max_errors=1)


def test_the_golden_figures_counted_by_hand(ctx):
    """tests/test_find_edit_host.py counts these in ta_edge's text by hand"""
    rep, lst = ctx.find_edit("fasta", O.golden("ta_edge.dexta"), ["ACGTAC", "TTTT"], max_errors=1, per_record=True)
    assert rep["per_pattern"].tolist() == [[44, 0], [2, 0]] and rep["hits"] == 46 and rep["records_hit"] == 5
    assert rep["rec_hits"].tolist() == [1, 0, 1, 0, 1, 0, 0, 42, 1]
    assert [tuple(int(v) for v in h) for h in lst[:4]] == [(0, 5, 0, 0, 1), (2, 6, 0, 0, 0), (4, 4, 1, 0, 0), (7, 6, 0, 0, 0)]


# ---- a synthetic text, packed by this library ------------------------------------------------------------------------------------------
ADAPTER = "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT"            # 45 nt: beyond the 32 symbols of one dx_query word
PRIMER = "GGTTCACGATACCA"


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def synthetic(n=201, seed=9):
    """n records of 0 .. 900 letters: every seventh empty; the adapter whole, with a letter inserted, with one left out and with one
    changed; the primer's reverse complement whole and with one deletion; the two halves of the adapter at the end of one record and
    the start of the next, where it must not be found"""
    rng = np.random.default_rng(seed)
    out, seqs, planted = [], [], {"del_rc": []}
    for i in range(n):
        ln = 0 if i % 7 == 3 else int(rng.integers(1, 901))
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, ln))
        if ln >= 200:
            a = {0: ADAPTER, 1: ADAPTER[:20] + "G" + ADAPTER[20:], 2: ADAPTER[:30] + ADAPTER[31:], 3: ADAPTER[:9] + "G" + ADAPTER[10:]}.get(i % 5)
            if a:
                s = s[:60] + a + s[60 + len(a):]
            if i % 3 == 0:
                r = revcomp(PRIMER)
                s = s[:ln - 40] + r + s[ln - 40 + len(r):]
            if i % 3 == 1 and i % 11 != 1:
                r = revcomp(PRIMER[:6] + PRIMER[7:])             # the primer less one letter, on the other strand
                s = s[:ln - 13] + r
                planted["del_rc"].append((i, len(s)))
        if i % 11 == 1 and ln >= 30:
            s = s[:-22] + ADAPTER[:22]                          # ... and the next record begins with the other half
        if i % 11 == 2 and ln >= 30 and seqs[-1].endswith(ADAPTER[:22]):
            s = ADAPTER[22:] + s[23:]
        seqs.append(s)
        out.append(f">syn/{100 + 3 * i}/0_{len(s)} RQ=0.850" + "".join("\n" + s[k:k + 70] for k in range(0, len(s), 70)))
    return ("\n".join(out) + "\n").encode(), planted


@pytest.fixture(scope="module")
def corpus(ctx):
    text, planted = synthetic()
    img = ctx.dexta(text)
    assert img == O.dexta(text)
    return img, planted


def test_strands_and_a_planted_reverse_complement_with_a_deletion(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, planted = corpus
    pats = [ADAPTER, PRIMER, "GGCCAATTGGCC"]
    exact = check(ctx, "fasta", img, pats, both_strands=True)
    want = check(ctx, "fasta", img, pats, both_strands=True, max_errors=2)
    assert want[0]["per_pattern"][2, 1] == 0                      # (the palindrome: searched once)
    assert want[0]["per_pattern"][0, 0] >= 3 * exact[0]["per_pattern"][0, 0] > 0          # the adapter with an indel is found only with errors allowed
    assert want[0]["per_pattern"][1, 1] > exact[0]["per_pattern"][1, 1] > 0
    hit = {(int(h["record"]), int(h["pos"])): int(h["mis"]) for h in want[1] if h["query"] == 1 and h["strand"] == 1}
    assert planted["del_rc"] and all(hit.get(p) == 1 for p in planted["del_rc"])        # at the record's last symbol, one deletion away
    nine = check(ctx, "fasta", img, [ADAPTER], max_errors=9)
    assert nine[0]["per_pattern"][0, 0] >= want[0]["per_pattern"][0, 0]


def test_max_hits_and_slices(ctx, monkeypatch, corpus):
    """max_hits below, at and above the total; the same in slices (three at least), which give the unsliced report and list"""
    img, _ = corpus
    pats = [PRIMER[:7], ADAPTER, "GATC"]
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    full = E.file_find_edit("fasta", F.text_of("fasta", img), pats, 1, True, 1 << 40)
    whole = ctx.find_edit("fasta", img, pats, max_errors=1, both_strands=True, per_record=True)
    total = full[0]["hits"]
    assert total > 300 and len(img) >= 3 * 4096
    for most in (0, 1, total // 2, total - 1, total, total + 1):
        want = check(ctx, "fasta", img, pats, full=full, max_errors=1, both_strands=True, max_hits=most)
        assert want[0]["listed"] == min(most, total) and want[0]["hits"] == total
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    F.assert_same_find(ctx.find_edit("fasta", img, pats, max_errors=1, both_strands=True, per_record=True), whole)
    for most in (1, total // 3, total - 1, total + 5):            # (the cap runs across the slices as if there were none)
        check(ctx, "fasta", img, pats, full=full, max_errors=1, both_strands=True, max_hits=most)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        ctx.find_edit(*args, **kw)
    return e.value


def test_refusals(ctx):
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    e = refused(ctx, "quiva", O.golden("qv_tiny.dexqv"), ["ACGT"])
    assert e.code == E_ARG and "dexqv" in str(e) and "dx_file_find_edit" in str(e)
    e = refused(ctx, "fasta", ta, ["ACGT", "ACNT"])
    assert e.code == E_ARG and "pattern 1" in str(e) and "column 3" in str(e)
    e = refused(ctx, "fasta", ta, ["ACGT", "A" * 40 + "x"])
    assert e.code == E_ARG and "pattern 1" in str(e) and "column 41" in str(e)
    e = refused(ctx, "arrow", ar, ["12345"])
    assert e.code == E_ARG and "pattern 0" in str(e) and "column 5" in str(e)
    assert refused(ctx, "fasta", ta, ["A" * 65]).code == E_ARG
    assert refused(ctx, "fasta", ta, [""]).code == E_ARG
    assert refused(ctx, "fasta", ta, []).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGT"] * 65).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGT"] * 33, both_strands=True).code == E_ARG
    assert refused(ctx, "fasta", ta, ["ACGTACGT", "ACG"], max_errors=3).code == E_ARG
    assert refused(ctx, "arrow", ar, ["1234"], both_strands=True).code == E_ARG
    ctx.find_edit("fasta", ta, ["ACGT"] * 32, both_strands=True)   # (32 palindromes: 32 queries)
    ctx.find_edit("fasta", ta, ["ACGTACGT", "ACG"], max_errors=2)
    ctx.find_edit("fasta", ta, ["A" * 64])
    for img in (ta[:len(ta) - 1], ta[:len(ta) - 37]):              # a truncated image is unpack2's error
        with pytest.raises(L.DexGPUError) as want:
            ctx.undexta(img, upper=True)
        assert refused(ctx, "fasta", img, ["ACGT"]).code == want.value.code
