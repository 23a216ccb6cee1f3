"""Context.screen_spans (dx_file_screen_spans) and Context.screen_cut (dx_file_screen_cut) on the GPU against tests/_spans.py, which works
on the TEXT the oracle prints for an image: the raw spans off the cover array, the join and the filter as a loop, the plan in plain
Python, the cut image the oracle's dexta / dexar / dexqv of the cut text.  The images are oracle-made: records of 0 to 759 symbols with
a vector planted under a few substitutions inside some reads and at both ends of others, on both strands for the .fasta.  Whole and in
slices, max_spans ending inside a later slice; the three modes byte for byte; the selection applied to the .dexar and the .dexqv of
the same records; and the refusals.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_span as P
import _oracle as O
import _screen as S
import _spans as SP
import _subset as SUB
import _u2_slices as U2
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG, E_DEGENERATE = -1, -4
ALL = 2 ** 32 - 1
K = {"fasta": 15, "arrow": 12}
LENS = np.array([0 if i % 23 == 4 else 7 if i % 29 == 6 else 60 + (37 * i * i + 11 * i) % 700 for i in range(118)], np.uint32)     # (the last is not empty)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def vector(kind, n=150, seed=71):
    letters = "ACGT" if kind == "fasta" else "1234"
    return "".join(letters[c] for c in np.random.default_rng(seed).integers(0, 4, n))


def planted(kind, text, seed):
    """the text with pieces of the vector (60 to 150 symbols, up to three substitutions, either strand for fasta) written over its records'
    letters, every length staying: in the middle of two records of three, at the very start of every fifth, at the very end of every
    seventh"""
    rng = np.random.default_rng(seed)
    letters = "ACGT" if kind == "fasta" else "1234"
    vec = vector(kind)
    out = []
    for i, (head, body) in enumerate(SUB.records(kind, text)):
        s = body[0].decode()
        places = ([len(s) // 2] if i % 3 else []) + ([0] if i % 5 == 0 else []) + ([-1] if i % 7 == 0 else [])
        for at in places:
            n = int(rng.integers(60, len(vec) + 1))
            a = int(rng.integers(0, len(vec) - n + 1))
            w = list(vec[a:a + n])
            for _ in range(int(rng.integers(0, 4))):
                j = int(rng.integers(len(w)))
                w[j] = letters[(letters.index(w[j]) + 1 + int(rng.integers(3))) % 4]
            w = "".join(w)
            if kind == "fasta" and rng.integers(2):
                w = revcomp(w)
            if len(s) < 2 * len(w) + 20:
                continue
            at = len(s) - len(w) if at < 0 else at
            s = s[:at] + w + s[at + len(w):]
        out.append(head + b"".join(b"\n" + s[k:k + 80].encode() for k in range(0, len(s), 80)))
    return b"\n".join(out) + b"\n"


def vector_codes(kind):
    v = np.array([("ACGT" if kind == "fasta" else "1234").index(c) for c in vector(kind)], np.uint8)
    return S.distinct([v], K[kind], kind == "fasta")


@pytest.fixture(scope="module")
def corpus():
    """the three files of one run, oracle-made, and per 2-bit kind the oracle's text of the image"""
    fa = planted("fasta", synth.make_seqfile("fasta", len(LENS), seed=41, lens=LENS).text, 42)
    ar = planted("arrow", synth.make_seqfile("arrow", len(LENS), seed=41, lens=LENS).text, 43)
    qv = synth.make_quiva(len(LENS), seed=41, lens=LENS).text
    out = {"fasta": O.dexta(fa), "arrow": O.dexar(ar), "quiva": O.dexqv(qv)}
    assert len(out["fasta"]) >= 3 * 4096 and U2.slices([int(n) for n in LENS], 4096) >= 3
    out["text"] = {kind: F.text_of(kind, out[kind]) for kind in ("fasta", "arrow")}
    return out


KNOWN = {}


def statement(corpus, kind, max_gap, min_span):
    """the statement's answer without a cap, computed once for a question and shared"""
    key = (kind, max_gap, min_span)
    if key not in KNOWN:
        KNOWN[key] = SP.file_spans(kind, corpus["text"][kind], K[kind], kind == "fasta", vector_codes(kind), max_gap, min_span, 1 << 40)
    return KNOWN[key]


def same(got, full, max_spans=1 << 20):
    n = min(full[0]["spans"], max_spans)
    assert got[0] == dict(full[0], listed=n), (got[0], full[0])
    assert got[1].dtype == api.SPAN_DTYPE and len(got[1]) == n
    diff = np.flatnonzero(got[1] != full[1][:n])
    assert len(diff) == 0, [(int(j), tuple(got[1][j]), tuple(full[1][j])) for j in diff[:5]]
    assert np.array_equal(got[2], full[2]) and np.array_equal(got[3], full[3])            # (rec_spans: every kept span, listed or not)


QUESTIONS = [(0, 0), (12, 40), (3, 60), (ALL, 0)]


@pytest.mark.parametrize("kind", ["fasta", "arrow"])
def test_screen_spans_whole_and_in_slices(ctx, monkeypatch, corpus, kind):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    img = corpus[kind]
    with ctx.kmer_set_from_codes(vector_codes(kind), K[kind], canonical=kind == "fasta", arrow=kind == "arrow") as s:
        scr = ctx.screen(kind, img, s)[0]
        for max_gap, min_span in QUESTIONS:
            full = statement(corpus, kind, max_gap, min_span)
            got = ctx.screen_spans(kind, img, s, max_gap, min_span)
            same(got, full)
            assert got[0]["covered"] == scr["covered"] and got[0]["records_hit"] == scr["records_hit"] and got[0]["records"] == len(LENS)
        raw, joined = statement(corpus, kind, 0, 0), statement(corpus, kind, 12, 40)
        assert raw[0]["raw_spans"] == raw[0]["spans"] > joined[0]["spans"] > 60 and raw[0]["span_symbols"] == raw[0]["covered"]
        lens = raw[3][raw[1]["record"].astype(np.int64)]
        assert (raw[1]["beg"] == 0).sum() >= 5 and (raw[1]["end"] == lens).sum() >= 5 and (raw[2][LENS < K[kind]] == 0).all()
        total = joined[0]["spans"]
        for most in (0, 1, total // 2, total, total + 1):
            same(ctx.screen_spans(kind, img, s, 12, 40, max_spans=most), joined, most)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")               # (the smallest figure the drivers take)
        for max_gap, min_span in QUESTIONS:
            same(ctx.screen_spans(kind, img, s, max_gap, min_span), statement(corpus, kind, max_gap, min_span))
        for most in (1, total // 3, 2 * total // 3 + 1, total - 1):       # max_spans ends inside a later slice
            same(ctx.screen_spans(kind, img, s, 12, 40, max_spans=most), joined, most)
        rp = L.SpansReport()
        assert ctx.lib.dx_file_screen_spans(ctx.h, api._kind(kind), img, len(img), s.h, 12, 40, 0, api.C.byref(rp), None, None, None) == 0
        assert rp.spans == total and rp.listed == 0 and rp.k == K[kind]                     # the report alone


# ---- the cut ---------------------------------------------------------------------------------------------------------------------------
def units_of(sel):
    return list(zip(sel["ids"].tolist(), sel["beg"].tolist(), sel["end"].tolist()))


def check_cut(ctx, corpus, kind, s, max_gap, min_span, min_len, mode):
    full = statement(corpus, kind, max_gap, min_span)
    img = corpus[kind]
    units, rep = SP.plan([tuple(int(v) for v in x) for x in full[1]], full[3], min_len, mode)
    got, cut, sel = ctx.screen_cut(kind, img, s, max_gap, min_span, min_len, mode)
    assert units_of(sel) == units and cut == rep, (cut, rep)
    assert got == ctx.subset(kind, img, *SUB.selection_arrays(units))
    assert got == P.cut_image(kind, img, units), "the cut image is not the oracle's encoding of the cut text"
    return units, rep


@pytest.mark.parametrize("mode", ["split", "longest", "drop"])
def test_screen_cut_is_the_oracles_encoding_of_the_cut_text(ctx, monkeypatch, corpus, mode):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    with ctx.kmer_set_from_codes(vector_codes("fasta"), K["fasta"], canonical=True) as s:
        for min_len in (0, 50):
            units, rep = check_cut(ctx, corpus, "fasta", s, 12, 40, min_len, mode)
            assert rep["records_cut" if mode != "drop" else "records_dropped"] > 50 and rep["spans"] > 60
        if mode == "split":
            assert len(units) > len(LENS) and rep["records_dropped"] > 0            # (ids that repeat; records with no piece of 50 symbols)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
        check_cut(ctx, corpus, "fasta", s, 12, 40, 50, mode)
        check_cut(ctx, corpus, "fasta", s, 0, 0, 0, mode)
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET")
    with ctx.kmer_set_from_codes(vector_codes("arrow"), K["arrow"], arrow=True) as s:
        check_cut(ctx, corpus, "arrow", s, 12, 40, 25, mode)


def test_the_selection_cuts_the_arrow_and_the_quiva_of_the_same_records(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    with ctx.kmer_set_from_codes(vector_codes("fasta"), K["fasta"], canonical=True) as s:
        img, cut, sel = ctx.screen_cut("fasta", corpus["fasta"], s, 12, 40, 40, "split")
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


def test_refusals(ctx, monkeypatch, corpus):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    ta, ar = O.golden("ta_small.dexta"), O.golden("ar_small.dexar")
    with ctx.kmer_set("fasta", ta, 15) as fs, ctx.kmer_set("arrow", ar, 15) as as_:
        for f, who in ((ctx.screen_spans, "dx_file_screen_spans"), (ctx.screen_cut, "dx_file_screen_cut")):
            for kind, img, s in (("arrow", ar, fs), ("fasta", ta, as_)):        # a set of the wrong kind
                e = refused(f, kind, img, s)
                assert e.code == E_ARG and "dx_file_screen" in str(e)
            e = refused(f, "quiva", O.golden("qv_tiny.dexqv"), fs)
            assert e.code == E_ARG and "dexqv" in str(e) and who in str(e)
            e = refused(f, "fasta", ta, None)
            assert e.code == E_ARG and "set" in str(e)
        assert refused(ctx.screen_cut, "fasta", ta, fs, mode=7).code == E_ARG
        rp = L.SpansReport()
        rp.records = 77
        assert ctx.lib.dx_file_screen_spans(ctx.h, 7, ta, len(ta), fs.h, 0, 0, 0, api.C.byref(rp), None, None, None) == E_ARG
        assert ctx.lib.dx_file_screen_spans(ctx.h, L.DX_KIND_FASTA, ta, len(ta), fs.h, 0, 0, 0, None, None, None, None) == E_ARG
        assert rp.records == 77
        for cut in (len(ta) - 1, len(ta) - 37):                        # a truncated image is unpack2's error
            with pytest.raises(L.DexGPUError) as want:
                ctx.undexta(ta[:cut])
            assert refused(ctx.screen_spans, "fasta", ta[:cut], fs).code == want.value.code
            assert refused(ctx.screen_cut, "fasta", ta[:cut], fs).code == want.value.code
    # a set that covers everything: nothing is kept in drop mode, and nothing of 100 symbols in the others
    text = b"".join(b">m/%d/0_60 RQ=0.850\n%s\n" % (i, "".join("ACGT"[c] for c in np.random.default_rng(i).integers(0, 4, 60)).encode())
                    for i in range(1, 5))
    img = O.dexta(text)
    with ctx.kmer_set("fasta", img, 15, canonical=True) as s:
        rep, spans, rec_spans, rec_len = ctx.screen_spans("fasta", img, s)
        assert [tuple(int(v) for v in x) for x in spans] == [(i, 0, 60) for i in range(4)] and rep["covered"] == rep["symbols"] == 240
        e = refused(ctx.screen_cut, "fasta", img, s, mode="drop")
        assert e.code == E_DEGENERATE and "dx_file_screen_cut" in str(e)
        assert refused(ctx.screen_cut, "fasta", img, s, mode="split").code == E_DEGENERATE
        assert ctx.screen_cut("fasta", img, s, min_span=61, mode="drop")[0] == img          # (no span is kept: every record whole)
