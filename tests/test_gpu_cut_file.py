"""Context.find_spans (dx_file_find_edit_spans) and Context.cut (dx_file_cut) on the GPU against tests/_find_span.py, which works on the
TEXT the oracle prints for an image: the starts by the plain DP, the plan in plain Python, the cut image the oracle's dexta / dexar /
dexqv of the cut text.  The goldens and oracle-made texts with planted, mutated adapters on both strands and for arrow; slices with
max_hits ending inside one; a slice with more than 2^20 hits; the three modes byte for byte; the selection applied to the .dexar and
the .dexqv of the same records; and the refusals.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_span as P
import _oracle as O
import _subset as S
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG, E_DEGENERATE, E_NOMEM = -1, -4, -6
ADAPTER = "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT"            # 45 nt: beyond the 32 symbols of one word
PRIMER = "GGTTCACGATACCA"
WIDTHS = "3321123441122334412"                                      # an arrow pattern: pulse widths have no complement


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def mutate(rng, word, edits, letters):
    w = list(word)
    for _ in range(edits):
        op, i = int(rng.integers(3)), int(rng.integers(len(w)))
        if op == 0:
            w[i] = letters[(letters.index(w[i]) + 1 + int(rng.integers(3))) % 4]
        elif op == 1:
            w.insert(i, letters[int(rng.integers(4))])
        elif len(w) > 1:
            del w[i]
    return "".join(w)


def replanted(kind, text, words, seed, edits=3):
    """the text with mutated copies of the words written over its records' letters (every length stays): one in the middle of two
    records of three, one at the very start of every fifth, one at the very end of every seventh"""
    rng = np.random.default_rng(seed)
    letters = "ACGT" if kind == "fasta" else "1234"
    out = []
    for i, (head, body) in enumerate(S.records(kind, text)):
        s = body[0].decode()
        places = ([len(s) // 2] if i % 3 else []) + ([0] if i % 5 == 0 else []) + ([-1] if i % 7 == 0 else [])
        for at in places:
            w = mutate(rng, words[int(rng.integers(len(words)))], int(rng.integers(0, edits + 1)), letters)
            if len(s) < 2 * len(w) + 20:
                continue
            at = len(s) - len(w) if at < 0 else at
            s = s[:at] + w + s[at + len(w):]
        out.append(head + b"".join(b"\n" + s[k:k + 80].encode() for k in range(0, len(s), 80)))
    return b"\n".join(out) + b"\n"


LENS = np.array([60 + (37 * i * i + 11 * i) % 700 for i in range(150)], np.uint32)


@pytest.fixture(scope="module")
def corpus():
    """the three files of one run, oracle-made: 150 records of 60 to 759 symbols; the .fasta has the adapter, the
    primer and their reverse complements planted under up to three edits, the .arrow a pattern of pulse widths"""
    fa = replanted("fasta", synth.make_seqfile("fasta", len(LENS), seed=31, lens=LENS).text, [ADAPTER, revcomp(ADAPTER), PRIMER, revcomp(PRIMER)], 32)
    ar = replanted("arrow", synth.make_seqfile("arrow", len(LENS), seed=31, lens=LENS).text, [WIDTHS], 33, edits=2)
    qv = synth.make_quiva(len(LENS), seed=31, lens=LENS).text
    out = {"fasta": O.dexta(fa), "arrow": O.dexar(ar), "quiva": O.dexqv(qv)}
    assert len(out["fasta"]) >= 3 * 4096
    return out


REPORT = ("records", "records_hit", "hits", "listed")


def check_spans(ctx, kind, img, patterns, full, max_errors=0, both_strands=False, max_hits=1 << 20):
    """full: the statement's answer without a cap, computed once by the caller"""
    n = min(full[0]["hits"], max_hits)
    want = dict(full[0], listed=n, start=full[0]["start"][:n]), full[1][:n]
    got = ctx.find_spans(kind, img, patterns, max_errors=max_errors, both_strands=both_strands, max_hits=max_hits, per_record=True)
    F.assert_same_find(got, want)
    assert np.array_equal(got[0]["start"], want[0]["start"]), [(tuple(int(v) for v in h), int(a), int(b)) for h, a, b in
                                                                zip(want[1], got[0]["start"], want[0]["start"]) if a != b][:6]
    assert np.array_equal(got[0]["rec_len"], want[0]["rec_len"])
    edit = ctx.find_edit(kind, img, patterns, max_errors=max_errors, both_strands=both_strands, max_hits=max_hits, per_record=True)
    assert all(edit[0][f] == got[0][f] for f in REPORT) and np.array_equal(edit[0]["per_pattern"], got[0]["per_pattern"])
    assert np.array_equal(edit[0]["rec_hits"], got[0]["rec_hits"]) and len(edit[1]) == len(got[1]) and (edit[1] == got[1]).all()
    return want


KNOWN = {}


def statement(kind, img, patterns, max_errors=0, both_strands=False):
    """the statement's answer without a cap, computed once for a question and shared"""
    key = (kind, img, tuple(patterns), max_errors, both_strands)
    if key not in KNOWN:
        KNOWN[key] = P.file_find_spans(kind, F.text_of(kind, img), patterns, max_errors, both_strands, 1 << 40)
    return KNOWN[key]


# ---- find_spans ------------------------------------------------------------------------------------------------------------------------
GOLDEN = [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_edge.dexar"),
          ("arrow", "ar_small.dexar")]


@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_spans_of_the_goldens(ctx, monkeypatch, kind, name):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = O.golden(name)
    pats = ["ACGTAC", "ttttcc", "GATC", "CAAACGGT"] if kind == "fasta" else ["1234", "112", "32123"]
    both = kind == "fasta"
    full = statement(kind, img, pats, 1, both)
    want = check_spans(ctx, kind, img, pats, full, max_errors=1, both_strands=both)
    assert want[0]["hits"] > 0 and (want[0]["start"] < want[1]["pos"]).all()
    check_spans(ctx, kind, img, pats, statement(kind, img, pats), max_errors=0)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
    check_spans(ctx, kind, img, pats, full, max_errors=1, both_strands=both)


def test_planted_adapters_on_both_strands(ctx, monkeypatch, corpus):
    """the adapter and the primer and their reverse complements under up to three edits, four allowed: whole, in slices (three at least),
    and with max_hits ending inside a slice"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, pats = corpus["fasta"], [ADAPTER, PRIMER]
    full = statement("fasta", img, pats, 4, True)
    total = full[0]["hits"]
    want = check_spans(ctx, "fasta", img, pats, full, max_errors=4, both_strands=True)
    per = want[0]["per_pattern"]
    assert total > 150 and (per > 10).all()
    n = (want[1]["pos"] - want[0]["start"]).astype(np.int64)
    m = np.where(want[1]["query"] == 0, len(ADAPTER), len(PRIMER))
    assert (np.abs(n - m) <= want[1]["mis"]).all() and (n != m).sum() > 20 and (want[0]["start"] == 0).sum() >= 5
    assert (want[1]["pos"] == want[0]["rec_len"][want[1]["record"].astype(np.int64)]).sum() >= 5
    for most in (0, 1, total // 2, total - 1, total + 1):
        check_spans(ctx, "fasta", img, pats, full, max_errors=4, both_strands=True, max_hits=most)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    for most in (1 << 20, 1, total // 3, 2 * total // 3 + 1, total - 1):
        check_spans(ctx, "fasta", img, pats, full, max_errors=4, both_strands=True, max_hits=most)


def test_planted_pulse_widths(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = corpus["arrow"]
    full = statement("arrow", img, [WIDTHS, "4444"], 3)
    want = check_spans(ctx, "arrow", img, [WIDTHS, "4444"], full, max_errors=3)
    assert want[0]["per_pattern"][0, 0] > 80
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    check_spans(ctx, "arrow", img, [WIDTHS, "4444"], full, max_errors=3, max_hits=full[0]["hits"] // 2)


def test_a_slice_with_more_than_2_to_the_20_hits(ctx, monkeypatch):
    """AC in a read of 2.2 M symbols ACAC..: an exact hit ends at every even position, 1.1 M of them in one slice -- the list is made a
    second time into enough room, and the starts behind that --, and a start is its end less two"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    n = 2200000
    body = "AC" * (n // 2)
    text = (">big/1/0_%d RQ=0.850\n" % n + "\n".join(body[k:k + 80] for k in range(0, n, 80)) + "\n>small/2/0_7 RQ=0.850\nGGACGTT\n").encode()
    img = ctx.dexta(text)
    rep, lst = ctx.find_spans("fasta", img, ["AC"], max_hits=1 << 21)
    assert rep["hits"] == rep["listed"] == n // 2 + 1 > 1 << 20 and rep["rec_len"].tolist() == [n, 7]
    assert (lst["pos"][:-1] == 2 * np.arange(1, n // 2 + 1)).all() and (lst["record"][:-1] == 0).all()
    assert tuple(int(v) for v in lst[-1]) == (1, 4, 0, 0, 0)
    assert (rep["start"] == lst["pos"] - 2).all()
    rep, lst = ctx.find_spans("fasta", img, ["AC"], max_hits=(1 << 20) + 5)
    assert rep["listed"] == len(lst) == len(rep["start"]) == (1 << 20) + 5 and (rep["start"] == lst["pos"] - 2).all()


# ---- cut -------------------------------------------------------------------------------------------------------------------------------
def units_of(sel):
    return list(zip(sel["ids"].tolist(), sel["beg"].tolist(), sel["end"].tolist()))


def check_cut(ctx, kind, img, full, patterns, max_errors, both_strands, min_len, mode):
    units, rep = P.plan(full[1]["record"], full[1]["pos"], full[0]["start"], full[0]["rec_len"], min_len, mode)
    got, cut, sel = ctx.cut(kind, img, patterns, max_errors=max_errors, both_strands=both_strands, min_len=min_len, mode=mode)
    assert units_of(sel) == units and cut == rep, (cut, rep)
    assert got == P.cut_image(kind, img, units), "the cut image is not the oracle's encoding of the cut text"
    return units, rep


@pytest.mark.parametrize("mode", ["split", "longest", "drop"])
def test_cut_is_the_oracles_encoding_of_the_cut_text(ctx, monkeypatch, corpus, mode):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, pats = corpus["fasta"], [ADAPTER, PRIMER]
    full = statement("fasta", img, pats, 4, True)
    for min_len in (0, 50):
        units, rep = check_cut(ctx, "fasta", img, full, pats, 4, True, min_len, mode)
        assert rep["records_cut" if mode != "drop" else "records_dropped"] > 60 and rep["spans"] > 100
    if mode == "split":
        assert len(units) > len(LENS) + 40 and rep["records_dropped"] > 0           # (ids that repeat; records with no piece of 50 symbols)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    check_cut(ctx, "fasta", img, full, pats, 4, True, 50, mode)
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET")
    ar = corpus["arrow"]
    check_cut(ctx, "arrow", ar, statement("arrow", ar, [WIDTHS], 3), [WIDTHS], 3, False, 25, mode)
    edge = O.golden("ta_edge.dexta")                                # (an empty record, a record that is one span, 42 spans that unite)
    units, rep = check_cut(ctx, "fasta", edge, statement("fasta", edge, ["ACGTAC", "TTTT"]), ["ACGTAC", "TTTT"], 0, False, 0, mode)
    if mode == "split":
        assert units == [(0, 0, 5), (1, 0, 0), (2, 6, 7), (3, 0, 2), (5, 0, 1), (6, 0, 6), (7, 170, 173), (8, 4, 80)]      # (counted by hand:
        assert rep == dict(records_in=9, records_cut=3, records_dropped=1, pieces=8, symbols_in=278, symbols_kept=94, spans=4)   # test_find_span_host.py)


def test_the_selection_cuts_the_arrow_and_the_quiva_of_the_same_records(ctx, monkeypatch, corpus):
    """what dx_file_cut hands back, applied by dx_file_subset to the .dexar and the .dexqv made for the same record lengths: the oracle's
    images of their cut texts, and record for record the lengths of the cut .dexta"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img, cut, sel = ctx.cut("fasta", corpus["fasta"], [ADAPTER, PRIMER], max_errors=4, both_strands=True, min_len=40, mode="split")
    units = units_of(sel)
    assert cut["pieces"] == len(units) > len(LENS)
    lens = ctx.census("fasta", img, per_record=True)["rec_len"]
    assert lens.tolist() == [e - b for _, b, e in units]
    for kind in ("arrow", "quiva"):
        got = ctx.subset(kind, corpus[kind], sel["ids"], sel["beg"], sel["end"])
        assert got == P.cut_image(kind, corpus[kind], units), kind
        assert np.array_equal(ctx.census(kind, got, per_record=True)["rec_len"], lens)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def refused(f, *args, **kw):
    with pytest.raises(L.DexGPUError) as e:
        f(*args, **kw)
    return e.value


def test_refusals(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    monkeypatch.delenv("DEXGPU_TEST", raising=False)
    ta = O.golden("ta_small.dexta")
    e = refused(ctx.cut, "quiva", O.golden("qv_tiny.dexqv"), ["ACGT"])
    assert e.code == E_ARG and "dexqv" in str(e) and "dx_file_cut" in str(e)
    assert refused(ctx.find_spans, "quiva", O.golden("qv_tiny.dexqv"), ["ACGT"]).code == E_ARG
    assert refused(ctx.cut, "fasta", ta, ["ACNT"]).code == E_ARG
    assert refused(ctx.cut, "fasta", ta, ["ACGT"], mode=7).code == E_ARG
    assert refused(ctx.cut, "fasta", ta, ["ACGT"], max_errors=4).code == E_ARG
    e = refused(ctx.cut, "fasta", ta, ["A"], mode="drop")          # every record has an A: nothing is kept
    assert e.code == E_DEGENERATE and "dx_file_cut" in str(e)
    assert refused(ctx.cut, "fasta", ta, ["A"], min_len=1 << 20).code == E_DEGENERATE
    ctx.cut("fasta", ta, ["GATC"])
    monkeypatch.setenv("DEXGPU_TEST", "cut_max_hits=3")            # a list that ends early: nothing is cut from part of the hits
    e = refused(ctx.cut, "fasta", ta, ["GATC"])
    assert e.code == E_NOMEM and "3 of 34 hits" in str(e)
    monkeypatch.delenv("DEXGPU_TEST")
    for img in (ta[:len(ta) - 1], ta[:len(ta) - 37]):              # a truncated image is unpack2's error
        with pytest.raises(L.DexGPUError) as want:
            ctx.undexta(img, upper=True)
        assert refused(ctx.cut, "fasta", img, ["ACGT"]).code == want.value.code
