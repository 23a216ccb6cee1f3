"""The census on the GPU: dx_code_counts and dx_byte_hist_ranges against numpy, dx_file_census against a census Python takes of the
oracle's decoders' output (and of the reference's bytes in tests/golden), and DEXGPU_CENSUS in the tools.  No expected value comes
from the library."""
import ctypes
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import _oracle as O
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dextractor_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


# ---- dx_code_counts ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_units():
    """One random packed buffer and its units -> (bytes, boff, beg, len, running counts of the four codes over the buffer's symbols):
    every length 0..70 at every phase and at an odd and an even boff; 255..257, 1023..1025, and the wave-step boundaries 4095..4097 and
    8191..8193 (1 KiB a step), each at several phases; one unit of 300 000 symbols; two units that overlap and one that is there twice;
    the last unit ends on the buffer's last byte, two symbols short of its end."""
    rng = np.random.default_rng(41)
    boff, beg, ln, at = [], [], [], 3
    def put(b, n):
        nonlocal at
        boff.append(at); beg.append(b); ln.append(n)
        at += (b + n + 3) // 4 + 1
    for n in range(71):
        for phase in range(4):
            for parity in (0, 1):
                at += (parity - at) % 2
                put(phase + 4 * (n % 3), n)
    for k, n in enumerate((255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)):
        for phase in ((0, 1, 2, 3) if n >= 4095 else (k % 4,)):
            at += k % 2
            put(phase, n)
    put(2, 300000)
    big = len(ln) - 1
    boff += [boff[big] + 100, boff[big] + 150, boff[500], boff[big]]         # overlapping; repeated: a short unit and the long one
    beg += [1, 3, beg[500], beg[big]]
    ln += [3000, 3000, ln[500], ln[big]]
    at += at % 2
    boff.append(at + 1); beg.append(5); ln.append(4 * 501 - 5 - 2)          # bytes at + 1 .. at + 501, from an odd offset
    total = at + 1 + 501
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    boff, beg, ln = np.array(boff, np.uint64), np.array(beg, np.uint32), np.array(ln, np.uint32)
    assert int(boff[-1] + ((beg[-1] + ln[-1] - 1) >> 2)) == total - 1 and boff[-1] % 2 == 1
    sym = ((buf[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).ravel()
    run = np.zeros((4, len(sym) + 1), np.int64)
    for c in range(4):
        run[c, 1:] = np.cumsum(sym == c)
    return buf, boff, beg, ln, run


def counts_of(run, boff, beg, ln):
    s0 = 4 * boff.astype(np.int64) + beg.astype(np.int64)
    s1 = s0 + ln.astype(np.int64)
    return (run[:, s1] - run[:, s0]).T.astype(np.uint64)                      # [n, 4]


@pytest.mark.parametrize("with_beg", [True, False], ids=["beg", "beg_null"])
def test_code_counts_against_numpy(ctx, with_beg):
    buf, boff, beg, ln, run = packed_units()
    n = len(ln)
    want = counts_of(run, boff, beg if with_beg else np.zeros(n, np.uint32), ln)
    d_in, d_boff, d_beg, d_len, d_cnt = ctx.to_device(buf), ctx.to_device(boff), ctx.to_device(beg), ctx.to_device(ln), ctx.alloc(16 * n)
    try:
        tot = ctx.code_counts(d_in, len(buf), d_boff, d_beg if with_beg else None, d_len, n, d_cnt)
        got = d_cnt.download(np.uint32, 4 * n).reshape(n, 4)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, [(int(i), int(boff[i]), int(beg[i]), int(ln[i]), list(got[i]), list(want[i])) for i in bad[:8]]
        assert list(tot) == list(want.sum(axis=0))
        assert (got.sum(axis=1) == ln).all()
        # totals only
        assert list(ctx.code_counts(d_in, len(buf), d_boff, d_beg if with_beg else None, d_len, n, None)) == list(want.sum(axis=0))
    finally:
        free(d_in, d_boff, d_beg, d_len, d_cnt)


def test_code_counts_of_no_units_and_of_tiny_buffers(ctx):
    assert list(ctx.code_counts(None, 0, None, None, None, 0)) == [0, 0, 0, 0]
    for size in (1, 2, 5, 15, 16, 17):                                       # (under 16 bytes the kernel reads a padded copy)
        buf = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
        sym = ((buf[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).ravel()
        boff = np.array([0, size - 1, 0, size], np.uint64)
        beg = np.array([0, 1, 3, 0], np.uint32)
        ln = np.array([4 * size, 3, 4 * size - 3, 0], np.uint32)
        want = [np.bincount(sym[4 * int(o) + int(b):4 * int(o) + int(b) + int(k)], minlength=4) for o, b, k in zip(boff, beg, ln)]
        d_in, d_boff, d_beg, d_len, d_cnt = ctx.to_device(buf), ctx.to_device(boff), ctx.to_device(beg), ctx.to_device(ln), ctx.alloc(64)
        try:
            tot = ctx.code_counts(d_in, size, d_boff, d_beg, d_len, 4, d_cnt)
            assert d_cnt.download(np.uint32, 16).reshape(4, 4).tolist() == [list(w) for w in want], size
            assert list(tot) == list(np.sum(want, axis=0))
        finally:
            free(d_in, d_boff, d_beg, d_len, d_cnt)


def test_code_counts_leaves_the_pad_bits_out(ctx):
    """reads of t alone (code 3), as Compress_Read packs them: the pad bits behind the last symbol are zeros, and code 0 counts none"""
    lens = [1, 2, 3, 5, 6, 7]
    reads = [O.compress_read(b"t" * k) for k in lens]
    assert [len(r) for r in reads] == [(k + 3) // 4 for k in lens]
    buf = np.frombuffer(b"".join(reads), np.uint8)
    boff = np.cumsum([0] + [len(r) for r in reads[:-1]]).astype(np.uint64)
    ln = np.array(lens, np.uint32)
    d_in, d_boff, d_len, d_cnt = ctx.to_device(buf), ctx.to_device(boff), ctx.to_device(ln), ctx.alloc(16 * len(lens))
    try:
        tot = ctx.code_counts(d_in, len(buf), d_boff, None, d_len, len(lens), d_cnt)
        assert d_cnt.download(np.uint32, 4 * len(lens)).reshape(-1, 4).tolist() == [[0, 0, 0, k] for k in lens]
        assert list(tot) == [0, 0, 0, sum(lens)]
    finally:
        free(d_in, d_boff, d_len, d_cnt)


def test_code_counts_names_the_first_unit_out_of_bounds(ctx):
    buf = np.random.default_rng(9).integers(0, 256, 1000, dtype=np.uint8)
    sym = ((buf[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).ravel()
    boff = np.array([0, 10, 990, 990, 1000, 2000, 0], np.uint64)
    beg = np.array([0, 1, 0, 1, 0, 0, 0], np.uint32)
    ln = np.array([4000, 100, 40, 40, 0, 0, 4001], np.uint32)                 # unit 3's last byte is byte 1000; 5 and 6 are out too
    d_in, d_boff, d_beg, d_len, d_cnt = ctx.to_device(buf), ctx.to_device(boff), ctx.to_device(beg), ctx.to_device(ln), ctx.alloc(16 * 7)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.code_counts(d_in, len(buf), d_boff, d_beg, d_len, 7, d_cnt)
        assert e.value.code == -3 and e.value.bad_unit == 3
        tot = ctx.code_counts(d_in, len(buf), d_boff, d_beg, d_len, 3, d_cnt)  # (the valid ones in front of it, on their own)
        want = [np.bincount(sym[4 * int(o) + int(b):4 * int(o) + int(b) + int(k)], minlength=4) for o, b, k in zip(boff[:3], beg[:3], ln[:3])]
        assert d_cnt.download(np.uint32, 12).reshape(3, 4).tolist() == [list(w) for w in want]
        assert list(tot) == list(np.sum(want, axis=0))
    finally:
        free(d_in, d_boff, d_beg, d_len, d_cnt)


# ---- dx_byte_hist_ranges -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hist_ranges():
    """One buffer and its ranges -> (bytes, off, len): every length 0..80 at every start alignment 0..15; the lengths around the lane /
    wave threshold, 1 Ki and 64 Ki; one range of 3 MiB; 200 000 bytes of the value 7 and as many of 0xFF (every lane at one counter);
    two ranges that overlap and two that are there twice; the last range ends on the buffer's last byte, from an odd offset."""
    rng = np.random.default_rng(43)
    off, ln, at = [], [], 0
    for n in range(81):
        for a in range(16):
            at += (a - at) % 16
            off.append(at); ln.append(n)
            at += n
    for n in (511, 512, 513, 1023, 1024, 1025, 65535, 65536, 65537, 3 << 20):
        at += 1 + (at % 2)
        off.append(at); ln.append(n)
        at += n
    big = len(ln) - 1
    sevens, ffs = at + 3, at + 3 + 200000
    off += [sevens, ffs]; ln += [200000, 200000]
    at = ffs + 200000
    off += [off[big] + 1000, off[big] + 1500, off[700], off[big]]
    ln += [70000, 70000, ln[700], ln[big]]
    at += at % 2
    off.append(at + 1); ln.append(777)
    total = at + 1 + 777
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    buf[sevens:sevens + 200000] = 7
    buf[ffs:ffs + 200000] = 0xFF
    return buf, np.array(off, np.uint64), np.array(ln, np.uint64)


def hist_of(buf, off, ln, kind, nkinds):
    hist = np.zeros((nkinds, 256), np.uint64)
    sums = np.zeros(len(off), np.uint64)
    for j, (o, n) in enumerate(zip(off, ln)):
        part = buf[int(o):int(o) + int(n)]
        hist[kind[j]] += np.bincount(part, minlength=256).astype(np.uint64)
        sums[j] = int(part.sum(dtype=np.uint64))
    return hist, sums


@pytest.mark.parametrize("flush", [None, 8192], ids=["flush512M", "flush8K"])
@pytest.mark.parametrize("nkinds", [1, 5, 8])
def test_byte_hist_ranges_against_bincount(ctx, monkeypatch, nkinds, flush):
    if flush is not None:
        set_flag(monkeypatch, "hist_flush", flush)               # (the counters are swept into the global words every 8 KiB a wave)
    buf, off, ln = hist_ranges()
    n = len(off)
    kind = np.random.default_rng(nkinds).integers(0, nkinds, n).astype(np.uint8)
    want, sums = hist_of(buf, off, ln, kind, nkinds)
    d_buf, d_off, d_len, d_kind, d_sum = ctx.to_device(buf), ctx.to_device(off), ctx.to_device(ln), ctx.to_device(kind), ctx.alloc(8 * n)
    try:
        got = ctx.byte_hist_ranges(d_buf, len(buf), d_off, d_len, d_kind, nkinds, n, d_sum)
        assert (got == want).all(), np.argwhere(got != want)[:8].tolist()
        gs = d_sum.download(np.uint64, n)
        bad = np.flatnonzero(gs != sums)
        assert len(bad) == 0, [(int(i), int(off[i]), int(ln[i]), int(gs[i]), int(sums[i])) for i in bad[:8]]
        assert (ctx.byte_hist_ranges(d_buf, len(buf), d_off, d_len, d_kind, nkinds, n, None) == want).all()      # no sums
        if nkinds == 5:                                                                                           # no kinds: one table
            one = ctx.byte_hist_ranges(d_buf, len(buf), d_off, d_len, None, nkinds, n, None)
            assert (one[0] == want.sum(axis=0)).all() and one[1:].sum() == 0
    finally:
        free(d_buf, d_off, d_len, d_kind, d_sum)


def test_byte_hist_ranges_no_units_and_units_out_of_bounds(ctx):
    assert ctx.byte_hist_ranges(None, 0, None, None, None, 3, 0).sum() == 0       # n = 0: DX_OK, nothing is looked at
    data = np.arange(4096, dtype=np.uint8)
    off = np.array([0, 100, 4000, 4000, 4096, 0, 5000], np.uint64)
    ln = np.array([4096, 50, 96, 97, 0, 8000, 1], np.uint64)          # range 3 ends one byte past the buffer; 5 and 6 are further out
    kind = np.array([0, 1, 2, 0, 1, 2, 0], np.uint8)
    d_buf, d_off, d_len, d_kind = ctx.to_device(data), ctx.to_device(off), ctx.to_device(ln), ctx.to_device(kind)
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.byte_hist_ranges(d_buf, len(data), d_off, d_len, d_kind, 3, len(off))
        assert e.value.code == -3 and e.value.bad_unit == 3
        with pytest.raises(L.DexGPUError) as e:                       # range 2's kind is 2: not below 2
            ctx.byte_hist_ranges(d_buf, len(data), d_off, d_len, d_kind, 2, 3)
        assert e.value.code == -3 and e.value.bad_unit == 2
        got = ctx.byte_hist_ranges(d_buf, len(data), d_off, d_len, d_kind, 3, 3)
        want, _ = hist_of(data, off[:3], ln[:3], kind, 3)
        assert (got == want).all()
        for nk in (0, 9):
            with pytest.raises(L.DexGPUError) as e:
                ctx.byte_hist_ranges(d_buf, len(data), d_off, d_len, d_kind, nk, 3)
            assert e.value.code == -1
    finally:
        free(d_buf, d_off, d_len, d_kind)


# ---- dx_file_census ----------------------------------------------------------------------------------------------------------------
EXT = {"fasta": ".dexta", "arrow": ".dexar", "quiva": ".dexqv"}
LETTERS = {"fasta": b"acgt", "arrow": b"1234"}


def n50_of(lens):
    a = sorted((int(x) for x in lens), reverse=True)
    total, run = sum(a), 0
    for v in a:
        run += v
        if total and 2 * run >= total:
            return v
    return 0


def census_of_text(kind, text):
    """what Python counts in a decoder's output: undexta (lower case) / undexar / undexqv (no -U)"""
    lines = text.split(b"\n")[:-1] if text else []
    hist, code = np.zeros((5, 256), np.uint64), np.zeros(4, np.uint64)
    if kind == "quiva":
        assert len(lines) % 6 == 0
        ents = [lines[i + 1:i + 6] for i in range(0, len(lines), 6)]
        lens = [len(e[0]) for e in ents]
        rec = np.zeros((len(ents), 5), np.uint64)
        for i, e in enumerate(ents):
            for q in range(5):
                a = np.frombuffer(e[q], np.uint8)
                hist[q] += np.bincount(a, minlength=256).astype(np.uint64)
                rec[i, q] = int(a.sum(dtype=np.uint64))
        per = {"rec_sum": rec}
    else:
        starts = [i for i, l in enumerate(lines) if l.startswith(b">")] + [len(lines)]
        seqs = [b"".join(lines[a + 1:b]) for a, b in zip(starts, starts[1:])]
        lens = [len(s) for s in seqs]
        rec = np.array([[s.count(bytes([c])) for c in LETTERS[kind]] for s in seqs], np.uint32).reshape(len(seqs), 4)
        assert (rec.sum(axis=1) == np.array(lens)).all()
        code = rec.sum(axis=0).astype(np.uint64)
        per = {"rec_code": rec}
    out = {"records": len(lens), "symbols": sum(lens), "min_len": min(lens) if lens else 0, "max_len": max(lens) if lens else 0,
           "n50": n50_of(lens), "code": code, "hist": hist}
    per["rec_len"] = np.array(lens, np.uint32)
    return out, per


def decode(kind, img):
    return O.undexta(img, upper=False, width=80) if kind == "fasta" else (O.undexar(img, width=80) if kind == "arrow" else O.undexqv(img, upper=False))


def check_census(ctx, kind, img, text):
    want, per = census_of_text(kind, text)
    got = ctx.census(kind, img, per_record=True)
    for k in ("records", "symbols", "min_len", "max_len", "n50"):
        assert got[k] == want[k], (kind, k, got[k], want[k])
    assert (got["code"] == want["code"]).all(), (got["code"], want["code"])
    assert (got["hist"] == want["hist"]).all(), np.argwhere(got["hist"] != want["hist"])[:8].tolist()
    assert sorted(k for k in got if k.startswith("rec_")) == sorted(per)          # (what does not apply to the kind comes back NULL)
    for k, v in per.items():
        assert got[k].shape == v.shape and (got[k] == v).all(), (kind, k, np.argwhere(got[k] != v)[:8].tolist())
    plain = ctx.census(kind, img)
    assert sorted(plain) == ["code", "hist", "max_len", "min_len", "n50", "records", "symbols"]
    assert all(np.array_equal(plain[k], got[k]) for k in plain)
    return got


def golden_images():
    out = [(c["name"] + EXT[c["kind"]], c["kind"]) for c in O.cases()]
    out += [("ta_small.legacy.dexta", "fasta"), ("ta_small.swapped.dexta", "fasta"), ("ta_small.legacy_swapped.dexta", "fasta"),
            ("ar_small.swapped.dexar", "arrow"), ("qv_tiny.legacy.dexqv", "quiva")]
    return out


@pytest.mark.parametrize("name,kind", golden_images(), ids=[c[0] for c in golden_images()])
def test_file_census_of_the_goldens(ctx, name, kind):
    img = O.golden(name)
    check_census(ctx, kind, img, decode(kind, img))


@functools.lru_cache(maxsize=None)
def corpus(kind, variant="plain"):
    """300 records of 0 .. 3000 symbols (a .fasta / .arrow header with no sequence line behind it is not a record the reference reads: 1
    at least there), every tenth .quiva entry empty -> (the image by the oracle's encoder, what the oracle's decoder makes of it).
    quiva variants: run densities 0.3 and 0.95, and a lossy image."""
    n = 300
    lens = np.random.default_rng(2000 + len(variant)).integers(0, 3001, n).astype(np.uint32)
    if kind == "quiva":
        lens[::10] = 0
        dens = {"plain": (0.85, 0.80), "sparse": (0.3, 0.3), "dense": (0.95, 0.95), "lossy": (0.85, 0.80)}[variant]
        text = synth.make_quiva(n, seed=91, lens=lens, prof=synth.pacbio_profile(*dens)).text
        img = O.dexqv(text, lossy=variant == "lossy")
    else:
        lens[lens == 0] = 1
        text = synth.make_seqfile(kind, n, seed=91, lens=lens).text
        img = O.dexta(text) if kind == "fasta" else O.dexar(text)
    return img, decode(kind, img)


CORPORA = [("fasta", "plain"), ("arrow", "plain"), ("quiva", "plain"), ("quiva", "sparse"), ("quiva", "dense"), ("quiva", "lossy")]


@pytest.mark.parametrize("budget", [None, 65536], ids=["whole", "sliced"])
@pytest.mark.parametrize("kind,variant", CORPORA, ids=["-".join(c) for c in CORPORA])
def test_file_census_against_the_oracle(ctx, monkeypatch, kind, variant, budget):
    img, text = corpus(kind, variant)
    if budget is None:
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    else:                                                    # bytes of image for the 2-bit kinds, of text for quiva: three slices at least
        budget = budget if kind == "quiva" else budget // 4
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
        assert (len(img) if kind != "quiva" else len(text)) >= 3 * budget
    got = check_census(ctx, kind, img, text)
    assert got["records"] == 300 and got["symbols"] > 300000


def test_file_census_of_a_quiva_walked_on_the_device(ctx, monkeypatch):
    set_flag(monkeypatch, "device_walk_min", 1)
    img, text = corpus("quiva", "plain")
    for budget in (None, 1 << 20):
        if budget is None:
            monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
        else:
            monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
        check_census(ctx, "quiva", img, text)


def test_file_census_of_an_image_without_records(ctx):
    ta = O.golden("ta_small.dexta")
    plen = int.from_bytes(ta[2:6], "little")
    qv = O.golden("qv_mid.dexqv")
    first = int(api.qv_walk(qv)["rec_off"][0])                # (where the records begin: the head is the key and the coding)
    for kind, img in (("fasta", ta[:6 + plen]), ("quiva", qv[:first])):
        got = ctx.census(kind, img, per_record=True)
        assert [got[k] for k in ("records", "symbols", "min_len", "max_len", "n50")] == [0, 0, 0, 0, 0]
        assert got["code"].sum() == 0 and got["hist"].sum() == 0 and len(got["rec_len"]) == 0


def test_file_census_of_a_byte_swapped_image(ctx):
    img = O.golden("ta_small.dexta")
    swapped = O.rewrite_pack2(img, swap=True)
    assert swapped != img
    a = check_census(ctx, "fasta", swapped, decode("fasta", img))
    b = ctx.census("fasta", img, per_record=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_file_census_errors_are_the_decoders_and_leave_out_untouched(ctx):
    qv, ta = O.golden("qv_mid.dexqv"), O.golden("ta_small.dexta")
    cs = L.Census()
    cs.records, cs.n50, cs.code[1], cs.hist[2][3] = 11, 22, 33, 44
    for kind, bad in (("quiva", qv[:len(qv) - 7]), ("quiva", b"\x00" * 40), ("fasta", b"\x00\x01garbage"), ("fasta", ta[:-3]), ("arrow", ta)):
        with pytest.raises(L.DexGPUError) as e:              # the decoder's own verdict on the image
            ctx.digest(kind, bad)
        k = {"fasta": L.DX_KIND_FASTA, "arrow": L.DX_KIND_ARROW, "quiva": L.DX_KIND_QUIVA}[kind]
        rc = ctx.lib.dx_file_census(ctx.h, k, bad, len(bad), ctypes.byref(cs), None, None, None)
        assert rc == e.value.code and rc < 0, (kind, rc, e.value.code)
        assert (cs.records, cs.n50, cs.code[1], cs.hist[2][3]) == (11, 22, 33, 44)
        with pytest.raises(L.DexGPUError):
            ctx.census(kind, bad, per_record=True)
    assert ctx.lib.dx_file_census(ctx.h, 3, ta, len(ta), ctypes.byref(cs), None, None, None) == -1      # (no such kind)


# ---- the tools ---------------------------------------------------------------------------------------------------------------------
def tool(name, args, cwd, census, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("DEXGPU_TEXT_BUDGET", "DEXGPU_VERIFY", "DEXGPU_DIGEST", "DEXGPU_CENSUS")}
    if census is not None:
        e["DEXGPU_CENSUS"] = census
    e.update(env)
    return subprocess.run([os.path.join(BIN, name), *args], cwd=str(cwd), capture_output=True, env=e)


def line_of(kind, text, path):
    """the census line, from a census Python takes of the decoded text"""
    c, _ = census_of_text(kind, text)
    head = "records=%d symbols=%d min=%d max=%d n50=%d" % (c["records"], c["symbols"], c["min_len"], c["max_len"], c["n50"])
    if kind == "quiva":
        vals = np.arange(256, dtype=np.float64)
        mean = [float((c["hist"][q].astype(np.float64) * vals).sum()) / c["symbols"] if c["symbols"] else 0.0 for q in (0, 2, 3, 4)]
        tail = " ".join("%s=%.3f" % (n, m) for n, m in zip(("del", "ins", "mrg", "sub"), mean))
    else:
        tail = " ".join("%s=%d" % (chr(n), v) for n, v in zip(LETTERS[kind], c["code"]))
    return ("%s %s %s\n" % (head, tail, path)).encode()


def test_tools_print_the_census_line(tmp_path):
    text, img = O.golden("ta_small.fasta"), O.golden("ta_small.dexta")
    (tmp_path / "ta_small.fasta").write_bytes(text)
    r = tool("dexta", ["-k", "ta_small"], tmp_path, "1")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of("fasta", decode("fasta", img), "./ta_small.fasta")
    assert (tmp_path / "ta_small.dexta").read_bytes() == img and (tmp_path / "ta_small.fasta").read_bytes() == text
    text, img = O.golden("qv_mid.quiva"), O.golden("qv_mid.dexqv")
    (tmp_path / "qv_mid.quiva").write_bytes(text)
    r = tool("dexqv", ["-k", "qv_mid"], tmp_path, "1")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of("quiva", decode("quiva", img), "./qv_mid.quiva")
    assert (tmp_path / "qv_mid.dexqv").read_bytes() == img
    # with the digest's variable too: two lines, the digest's first (the .quiva goldens are undexqv -U's: the digest reads that off the text)
    r = tool("dexqv", ["-k", "qv_mid"], tmp_path, "1", DEXGPU_DIGEST="1")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == b"%08x %d ./qv_mid.quiva\n" % (zlib.crc32(text), len(text)) + line_of("quiva", decode("quiva", img), "./qv_mid.quiva")
    # with neither: the same file, nothing on stdout
    r = tool("dexqv", ["-k", "qv_mid"], tmp_path, None)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    assert (tmp_path / "qv_mid.dexqv").read_bytes() == img


def test_tools_census_only_writes_nothing(tmp_path):
    img = O.golden("qv_mid.dexqv")
    (tmp_path / "qv_mid.dexqv").write_bytes(img)
    r = tool("undexqv", ["qv_mid"], tmp_path, "only")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of("quiva", decode("quiva", img), "./qv_mid.quiva")
    assert not (tmp_path / "qv_mid.quiva").exists() and (tmp_path / "qv_mid.dexqv").read_bytes() == img
    (tmp_path / "ar_small.dexar").write_bytes(O.golden("ar_small.dexar"))
    r = tool("undexar", ["ar_small"], tmp_path, "only")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of("arrow", decode("arrow", O.golden("ar_small.dexar")), "./ar_small.arrow")
    assert not (tmp_path / "ar_small.arrow").exists()


def test_dex_tools_refuse_census_only(tmp_path):
    (tmp_path / "ar_small.arrow").write_bytes(O.golden("ar_small.arrow"))
    r = tool("dexar", ["ar_small"], tmp_path, "only")
    assert r.returncode == 1 and r.stdout == b"" and b"DEXGPU_CENSUS" in r.stderr
    assert (tmp_path / "ar_small.arrow").read_bytes() == O.golden("ar_small.arrow")
    assert not (tmp_path / "ar_small.dexar").exists()
