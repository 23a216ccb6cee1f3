"""The numpy statement of the placement (tests/_place.py) against plain Python -- string slices, a dict of positions, a loop over
bins --, the planted truth it has to find, and the two host-only calls of the feature: api.place_select (dx_place_select) against a
plain loop and api.pack_letters (dx_pack_letters, the packer of Context.kmer_index_from_letters) against tests/_find.py's pack.
No GPU."""
import numpy as np
import pytest

import _find as F
import _place as P
from dextractor_amd import _lib as L
from dextractor_amd import api

LETTERS = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def text(s):
    return "".join(LETTERS[int(c)] for c in s)


def revcomp(w):
    return "".join(COMP[c] for c in reversed(w))


def plain_index(targets, k, canonical):
    """a dict: the k-mer kept (the smaller of a window and its reverse complement, as strings) -> [(g, flip)] ascending in g"""
    where, g0 = {}, 0
    for s in targets:
        t = text(s)
        for p in range(len(t) - k + 1):
            w = t[p:p + k]
            r = revcomp(w)
            kept, flip = (r, 1) if canonical and r < w else (w, 0)
            where.setdefault(kept, []).append((g0 + p, flip))
        g0 += len(t)
    return where


def plain_seeds(j, s, where, k, canonical, max_occ):
    t, out = text(s), []
    for p in range(len(t) - k + 1):
        w = t[p:p + k]
        r = revcomp(w)
        kept, f = (r, 1) if canonical and r < w else (w, 0)
        occ = where.get(kept, [])
        if 0 < len(occ) <= max_occ:
            out += [(j, p, g, flip ^ f) for g, flip in occ]
    return out


def plain_place(seeds, k, band_bits):
    if not seeds:
        return (0, 0, 0, P.NONE, P.NONE, P.NONE, P.NONE, P.NONE)
    c = {}
    for _, p, g, s in seeds:
        d = (g + p if s else g - p + 2 ** 31) % 2 ** 32
        c[(s, d >> band_bits)] = c.get((s, d >> band_bits), 0) + 1
    best = None
    for (s, b) in sorted(c):                                                 # ascending (s, b): the first of the largest wins the tie
        v = c[(s, b)] + c.get((s, b + 1), 0)
        if best is None or v > best[0]:
            best = (v, s, b)
    v, s, b = best
    voted = [(p, g) for _, p, g, st in seeds if st == s and ((g + p if s else g - p + 2 ** 31) % 2 ** 32) >> band_bits in (b, b + 1)]
    return (len(seeds), v, s, b << band_bits, min(p for p, _ in voted), max(p for p, _ in voted) + k, min(g for _, g in voted),
            max(g for _, g in voted) + k)


def some_targets(seed):
    rng = np.random.default_rng(seed)
    t = [rng.integers(0, 4, n).astype(np.uint8) for n in (0, 300, 70, 5, 140)]
    t.append(np.zeros(40, np.uint8))                                         # poly-A: one code, every position
    t.append(np.array([0, 1, 2, 3] * 8 + [0, 3, 0, 3, 1, 2, 1, 2], np.uint8))   # ACGT..., ATAT, CGCG: even-k words that are their own reverse complement
    t.append(t[1][100:220].copy())                                           # a repeat of a piece of target 1
    return t


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", [1, 4, 5, 14, 21, 32])
def test_the_statement_against_strings_and_a_dict(k, canonical):
    targets = some_targets(k)
    x = P.Index(targets, k, canonical)
    where = plain_index(targets, k, canonical)
    assert len(x.codes) == len(where) and x.windows == sum(len(v) for v in where.values()) == int(x.start[-1])
    for i, c in enumerate(x.codes):
        w = text([(int(c) >> (2 * (k - 1 - t))) & 3 for t in range(k)])
        got = [(int(v) >> 1, int(v) & 1) for v in x.pos[int(x.start[i]):int(x.start[i + 1])]]
        assert got == where[w] and int(x.counts[i]) == len(got), (w, got[:4], where[w][:4])
        if w == revcomp(w):
            assert all(f == 0 for _, f in got)                              # its own reverse complement: never flipped
    if canonical and k % 2 == 0:
        assert any(w == revcomp(w) for w in where)
    rng = np.random.default_rng(100 + k)
    reads, _ = P.planted([t for t in targets if len(t) >= 60], 6, 60, 0.03, k)
    reads += [rng.integers(0, 4, 90).astype(np.uint8), np.zeros(0, np.uint8), np.zeros(50, np.uint8)]
    for max_occ in (1, 2, 1000):
        lst, off, tot = P.seeds(reads, x, max_occ)
        want = [plain_seeds(j, s, where, k, canonical, max_occ) for j, s in enumerate(reads)]
        assert [tuple(int(v) for v in e) for e in lst] == [e for u in want for e in u]
        assert off.tolist() == np.cumsum([0] + [len(u) for u in want]).tolist() and tot[2] == len(lst)
        for bits in (0, 4, 8, 16, 31):
            rec, pt = P.place(lst, off, k, bits)
            assert [tuple(int(v) for v in r) for r in rec] == [plain_place(u, k, bits) for u in want]
            assert pt == [len(lst), int(rec["votes"].sum()), sum(1 for u in want if u)]


K, BAND, RATE, LENGTH = 15, 8, 0.03, 400


def test_planted_reads_are_found_by_the_statement():
    """Substitutions only keep a read on one diagonal, so with 3 % of them and k = 15 the clean windows (0.97^15 = 0.63 of all) carry
    the vote, and the first and the last of them lie well inside 2^8 symbols of the read's ends.  Every read must be placed on its
    target and strand with gbeg within 2^band_bits of where it was cut."""
    rng = np.random.default_rng(2024)
    targets = [rng.integers(0, 4, n).astype(np.uint8) for n in (3000, 1200, 5000)]
    x = P.Index(targets, K, True)
    reads, truth = P.planted(targets, 60, LENGTH, RATE, 7)
    lst, off, _ = P.seeds(reads, x, max_occ=2)
    rec, tot = P.place(lst, off, K, BAND)
    assert tot[2] == len(reads)
    for r, (t, p, s), (wt, tb, te) in zip(rec, truth, P.where(rec, x.toff)):
        assert int(r["strand"]) == s and wt == t and abs(tb - p) <= 2 ** BAND and abs(te - (p + LENGTH)) <= 2 ** BAND, (r, t, p, s)
        assert int(r["votes"]) >= 50 and int(r["rend"]) - int(r["rbeg"]) >= LENGTH - 2 * 2 ** BAND


def test_place_select_against_a_plain_loop():
    rng = np.random.default_rng(5)
    toff = np.array([0, 100, 100, 350, 1000], np.uint64)                    # (target 1 is empty)
    rec = np.zeros(300, P.PLACE)
    rec["votes"] = rng.integers(0, 6, 300)
    rec["strand"] = rng.integers(0, 2, 300)
    rec["gbeg"] = rng.integers(0, 1000, 300)
    rec["gend"] = rec["gbeg"] + rng.integers(1, 400, 300)                   # (some reach into the next target: cut at their own's end)
    rec[7] = (0, 0, 0, P.NONE, P.NONE, P.NONE, P.NONE, P.NONE)
    rec["gbeg"][11], rec["gend"][11] = 100, 140                             # on the seam behind the empty target
    rec["gbeg"][12], rec["gend"][12] = 999, 1030
    seen = set()
    for target in (None, 0, 2, 3):
        for lo, hi in ((0, P.M32), (0, 50), (120, 121), (649, 650), (30, 30)):
            for min_votes, strands, drop in ((0, 3, False), (3, 1, False), (1, 2, True), (5, 3, True)):
                got = api.place_select(rec, toff, target=target, lo=lo, hi=hi, min_votes=min_votes, strands=strands, drop=drop)
                assert got.dtype == np.uint64 and got.tolist() == P.select(rec, toff, target, lo, hi, min_votes, strands, drop)
                seen.add(len(got))
    assert len(seen) > 10
    assert api.place_select(rec, toff, target=1).tolist() == []             # nothing begins in an empty target
    w = api.place_where(rec, toff)
    assert [tuple(int(v) for v in e) for e in w] == P.where(rec, toff)
    assert api.place_select(rec[:0], toff).tolist() == [] and api.place_select(rec[:0], toff, drop=True).tolist() == []
    for bad in (dict(strands=0), dict(strands=4), dict(lo=5, hi=4), dict(target=4)):
        with pytest.raises(L.DexGPUError) as e:
            api.place_select(rec, toff, **bad)
        assert e.value.code == -1
    with pytest.raises(L.DexGPUError):
        api.place_select(rec, np.array([0, 10, 5], np.uint64))
    with pytest.raises(L.DexGPUError):
        api.place_select(rec, np.array([1, 10], np.uint64))


@pytest.mark.parametrize("arrow", [False, True], ids=["fasta", "arrow"])
def test_the_host_packer_against_pack(arrow):
    rng = np.random.default_rng(9)
    letters = "1234" if arrow else "ACGT"
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1001):
        s = rng.integers(0, 4, n)
        t = "".join(letters[int(c)] for c in s)
        assert api.pack_letters(t, arrow) == bytes(F.pack(s, pad=0))
        if not arrow:
            assert api.pack_letters(t.lower()) == bytes(F.pack(s, pad=0))
    with pytest.raises(L.DexGPUError) as e:
        api.pack_letters(letters * 3 + "N" + letters, arrow)
    assert e.value.code == -1 and e.value.bad_pos == 12
    with pytest.raises(L.DexGPUError) as e:
        api.pack_letters("1234" if not arrow else "ACGT", arrow)
    assert e.value.bad_pos == 0
