"""Context.place (dx_file_place), api.place_select and Context.subset on the GPU against tests/_place.py, which works on the TEXT the
oracle prints for an image: the records of tests/_u2_slices.py's synthetic text with reads planted from a three-target reference
(either strand, substitutions only), the whole image against DEXGPU_TEXT_BUDGET slices, a seed_room that forces many groups, a room
below one record's seeds, a .dexar against an index of pulse widths, a kind that does not match, and place, then place_select, then
subset against the oracle's image of the text's selected records.  No expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _oracle as O
import _place as P
import _subset as SUB
import _u2_slices as U2
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM = -1, -6
K, BAND = 15, 8
_made = {}


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def planted_text():
    """synthetic()'s text with every third record of 300 letters or more (the long one among them) replaced, letter for letter, by a
    piece of the reference: (the text, the three targets, {record: (target, position, strand)})"""
    text, lens = U2.synthetic()
    rng = np.random.default_rng(31)
    targets = [rng.integers(0, 4, n).astype(np.uint8) for n in (6000, 2500, 30000)]
    recs = text.decode().split(">")[1:]
    truth, out = {}, []
    for i, r in enumerate(recs):
        head = r.split("\n", 1)[0]
        ln = lens[i] if i < len(lens) else 4
        if i < len(lens) and i % 3 == 2 and ln >= 300:
            t = 2 if ln > 2500 else int(rng.integers(0, 3))
            at = int(rng.integers(0, len(targets[t]) - ln + 1))
            s = np.array(targets[t][at:at + ln], np.uint8)
            hit = rng.random(ln) < 0.03
            s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            strand = len(truth) % 2
            if strand:
                s = (3 - s)[::-1]
            body = "".join("ACGT"[c] for c in s)
            truth[i] = (t, at, strand)
            r = head + "".join("\n" + body[j:j + 70] for j in range(0, ln, 70)) + "\n"
        out.append(">" + r)
    return "".join(out).encode(), targets, truth


def made(ctx):
    """the image, its decoded text, the reference and the statement's answer, made once"""
    if not _made:
        text, targets, truth = planted_text()
        img = U2.image(ctx.dexta, text)
        decoded = F.text_of("fasta", img)
        x = P.Index(targets, K, True)
        _made.update(img=img, decoded=decoded, targets=targets, truth=truth, x=x, want=P.file_place("fasta", decoded, x, 2, BAND))
    return _made


def same(got, want, groups=None):
    (grep, grec, glen, gwhere), (wrep, wrec, wlen) = got, want
    g = dict(grep)
    assert g.pop("groups") >= 1 if groups is None else g.pop("groups") == groups
    assert g == wrep, (g, wrep)
    assert np.array_equal(glen, wlen)
    P.same_entries(grec, wrec)
    return gwhere


def test_planted_records_are_placed_whole_and_in_slices(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    m = made(ctx)
    assert len(m["truth"]) >= 8 and U2.BIG in m["truth"] and {s for _, _, s in m["truth"].values()} == {0, 1}
    with ctx.kmer_index_from_letters(["".join("ACGT"[c] for c in t) for t in m["targets"]], K, canonical=True) as x:
        whole = ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND)
        where = same(whole, m["want"], groups=1)
        assert [tuple(int(v) for v in e) for e in where] == P.where(m["want"][1], m["x"].toff)
        for i, (t, at, strand) in m["truth"].items():                       # the truth: target, strand, and the place within 2^band_bits
            assert int(where[i]["target"]) == t and int(whole[1][i]["strand"]) == strand and abs(int(where[i]["tbeg"]) - at) <= 2 ** BAND
        others = [i for i in range(len(whole[1])) if i not in m["truth"]]
        assert whole[1]["votes"][others].max() < 20 <= whole[1]["votes"][list(m["truth"])].min()
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")                    # in slices: the same answer
        sliced = ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND)
        same(sliced, m["want"])
        assert sliced[0]["groups"] >= 3 and sliced[1].tobytes() == whole[1].tobytes()
        for bits, occ in ((0, 1), (16, 1000)):
            same(ctx.place("fasta", m["img"], x, max_occ=occ, band_bits=bits), P.file_place("fasta", m["decoded"], m["x"], occ, bits))


def test_a_room_that_forces_many_groups_and_one_below_a_record(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    m = made(ctx)
    lst, off, _ = P.seeds(F.reads("fasta", m["decoded"]), m["x"], 2)
    per = np.diff(off.astype(np.int64))
    most = int(per.max())
    assert most > 10000 and (per > 0).sum() >= 8
    with ctx.kmer_index_from_letters(["".join("ACGT"[c] for c in t) for t in m["targets"]], K, canonical=True) as x:
        # the greedy groups of the statement: consecutive records while the sum stays within the room; a group without a seed is not listed
        groups, run, first = 0, 0, True
        for c in per:
            if not first and run + c > most:
                groups, run, first = groups + (1 if run else 0), 0, True
            run, first = run + c, False
        groups += 1 if run else 0
        got = ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND, seed_room=most)
        same(got, m["want"], groups=groups)
        assert groups >= 3
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
        same(ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND, seed_room=most), m["want"])
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET")
        with pytest.raises(L.DexGPUError) as e:
            ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND, seed_room=most - 1)
        assert e.value.code == E_NOMEM and f"record {int(np.argmax(per))} " in str(e.value)
        free = ctx.mem_info()[0] if hasattr(ctx, "mem_info") else None
        same(ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND), m["want"])                 # ... and nothing stays behind
        if free is not None:
            assert ctx.mem_info()[0] >= free


def test_a_dexar_against_an_index_of_pulse_widths_and_the_refusals(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    ar, ta = O.golden("ar_small.dexar"), O.golden("ta_small.dexta")
    text = F.text_of("arrow", ar)
    rs = F.reads("arrow", text)
    with ctx.kmer_index("arrow", ar, 14) as xa, ctx.kmer_index("fasta", ta, 14, canonical=True) as xf:
        got = ctx.place("arrow", ar, xa, max_occ=1000, band_bits=4)
        same(got, P.file_place("arrow", text, P.Index(rs, 14, False), 1000, 4))
        placed = got[1]["votes"] > 0
        assert placed.any() and (got[3]["target"][placed] <= len(rs)).all()
        for kind, img, x in (("arrow", ar, xf), ("fasta", ta, xa)):          # a kind that does not match the index's
            with pytest.raises(L.DexGPUError) as e:
                ctx.place(kind, img, x)
            assert e.value.code == E_ARG and "dx_file_place" in str(e.value)
        with pytest.raises(L.DexGPUError) as e:
            ctx.place("quiva", O.golden("qv_tiny.dexqv"), xf)
        assert e.value.code == E_ARG and "dexqv" in str(e.value)
        for kw in (dict(max_occ=0), dict(band_bits=32)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.place("fasta", ta, xf, **kw)
            assert e.value.code == E_ARG
        rp = L.PlaceReport()
        rp.records = 77
        f = ctx.lib.dx_file_place
        assert f(ctx.h, L.DX_KIND_FASTA, ta, len(ta), None, 1, 8, 0, api.C.byref(rp), None, None) == E_ARG and rp.records == 77
        assert f(ctx.h, 7, ta, len(ta), xf.h, 1, 8, 0, api.C.byref(rp), None, None) == E_ARG
        assert f(ctx.h, L.DX_KIND_FASTA, ta, len(ta), xf.h, 1, 8, 0, None, None, None) == E_ARG
        with pytest.raises(L.DexGPUError):
            ctx.place("fasta", ta[:len(ta) - 37], xf)                        # a truncated image is unpack2's error
        assert rp.records == 77
        assert f(ctx.h, L.DX_KIND_FASTA, ta, len(ta), xf.h, 1000, 8, 0, api.C.byref(rp), None, None) == 0      # the report alone
        assert rp.records == 12 and 0 < rp.records_placed <= 12 and rp.seeds >= rp.votes > 0 and rp.k == 14


def test_place_select_subset_is_the_oracles_image_of_the_selected_records(ctx, monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    m = made(ctx)
    toff = m["x"].toff
    # the input first, WITH THE STATEMENT: the reads that begin in the first 18500 symbols of target 2, of either strand, are planted ones
    want_ids = P.select(m["want"][1], toff, target=2, lo=0, hi=18500, min_votes=20)
    on_two = sorted(i for i, (t, at, _) in m["truth"].items() if t == 2 and at < 18500)
    assert want_ids == on_two and len(on_two) >= 2
    with ctx.kmer_index_from_letters(["".join("ACGT"[c] for c in t) for t in m["targets"]], K, canonical=True) as x:
        assert np.array_equal(x.targets(), toff)
        rep, rec, rec_len, where = ctx.place("fasta", m["img"], x, max_occ=2, band_bits=BAND)
        for kw in (dict(target=2, hi=18500, min_votes=20), dict(min_votes=20, strands=2), dict(target=0, drop=True), dict(lo=100, hi=101)):
            assert api.place_select(rec, x.targets(), **kw).tolist() == P.select(m["want"][1], toff, **kw)
        ids = api.place_select(rec, x.targets(), target=2, hi=18500, min_votes=20)
    assert ids.tolist() == on_two
    assert ctx.subset("fasta", m["img"], ids=ids) == O.dexta(SUB.cut("fasta", m["decoded"], [(i, None, None) for i in on_two]))
