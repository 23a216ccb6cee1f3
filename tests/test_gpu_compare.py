"""dx_file_compare on the GPU: golden images against themselves, against their key / byte-order variants and against this library's
own image of their text; the reference's lossless and -l images of one .quiva against the figures counted from their texts; and
images made here from edited texts, each report held field by field to tests/_diff.py's, which works on the two TEXTS alone."""
import functools

import numpy as np
import pytest

import _diff as D
import _oracle as O
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

EXT = {"fasta": ".dexta", "arrow": ".dexar", "quiva": ".dexqv"}
IMAGES = [(c["kind"], c["name"] + EXT[c["kind"]]) for c in O.cases()] + [
    ("fasta", "ta_small.legacy.dexta"), ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"),
    ("arrow", "ar_small.swapped.dexar"), ("quiva", "qv_tiny.legacy.dexqv")]
VARIANTS = [("fasta", "ta_small.dexta", "ta_small.legacy.dexta"), ("fasta", "ta_small.dexta", "ta_small.swapped.dexta"),
            ("fasta", "ta_small.dexta", "ta_small.legacy_swapped.dexta"), ("fasta", "ta_small.legacy.dexta", "ta_small.swapped.dexta"),
            ("arrow", "ar_small.dexar", "ar_small.swapped.dexar"), ("quiva", "qv_tiny.dexqv", "qv_tiny.legacy.dexqv")]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@pytest.fixture(autouse=True)
def no_budget(monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)


def assert_equal_images(r, lines):
    assert r["same"] and r["lines"] == lines and r["records_a"] == r["records_b"] and not r["prefix_differs"]
    assert (r["headers_differ"], r["lengths_differ"], r["records_differ"]) == (0, 0, 0)
    assert (r["first_header"], r["first_length"], r["first_record"], r["first_line"], r["first_column"]) == (None,) * 5
    assert all(int(r[k].sum()) == 0 and len(r[k]) == lines for k in ("differ", "line_records", "sum_abs", "max_abs"))
    assert r["rec_differ"].shape == (r["records_a"], lines) and not r["rec_differ"].any()


@pytest.mark.parametrize("kind,name", IMAGES, ids=[n for _, n in IMAGES])
def test_a_golden_image_against_itself(ctx, kind, name):
    img = O.golden(name)
    r = ctx.compare(kind, img, img, per_record=True)
    assert r["records_a"] > 0
    assert_equal_images(r, 5 if kind == "quiva" else 1)
    plain = ctx.compare(kind, img, img)
    assert plain["same"] and "rec_differ" not in plain


@pytest.mark.parametrize("kind,a,b", VARIANTS, ids=[b for _, _, b in VARIANTS])
def test_key_and_byte_order_variants_are_the_same_records(ctx, kind, a, b):
    assert_equal_images(ctx.compare(kind, O.golden(a), O.golden(b), per_record=True), 5 if kind == "quiva" else 1)
    assert_equal_images(ctx.compare(kind, O.golden(b), O.golden(a), per_record=True), 5 if kind == "quiva" else 1)


@pytest.mark.parametrize("case", O.cases("quiva"), ids=[c["name"] for c in O.cases("quiva")])
def test_a_quiva_golden_against_this_librarys_image_of_its_text(ctx, case):
    mine = ctx.dexqv(O.golden(case["input"] + ".quiva"), lossy="-l" in case["flags"])
    assert_equal_images(ctx.compare("quiva", O.golden(case["name"] + ".dexqv"), mine, per_record=True), 5)


# ---- what dexqv -l does, on the reference's own two images ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lossy_report():
    return D.report("quiva", O.undexqv(O.golden("qv_full.dexqv")), O.undexqv(O.golden("qv_lossy.dexqv")))


def test_full_against_lossy_is_exactly_the_rounding(ctx):
    full, lossy = O.golden("qv_full.dexqv"), O.golden("qv_lossy.dexqv")
    r = ctx.compare("quiva", full, lossy, per_record=True)
    assert (r["records_a"], r["records_b"], r["headers_differ"], r["lengths_differ"], r["prefix_differs"]) == (24, 24, 0, 0, False)
    assert list(r["differ"]) == [0, 0, 134598, 183845, 0]
    assert list(r["sum_abs"]) == [0, 0, 134598, 356544, 0]
    assert list(r["max_abs"]) == [0, 0, 1, 3, 0]
    assert r["records_differ"] == 24 and list(r["line_records"]) == [0, 0, 24, 24, 0] and not r["same"]
    D.assert_same_report(r, lossy_report())                       # (rec_differ and the first difference with it)
    assert_equal_images(ctx.compare("quiva", full, lossy, lossy=True, per_record=True), 5)
    back = ctx.compare("quiva", lossy, full, lossy=True, per_record=True)
    assert not back["same"]
    D.assert_same_report(back, D.report("quiva", O.undexqv(lossy), O.undexqv(full), lossy=True))


@pytest.mark.parametrize("budget", [131072, 300000, 1000000])
def test_a_pair_in_slices_gives_the_identical_report(ctx, monkeypatch, budget):
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))         # (the two texts are 2.3 MB: 24, 10 and 3 slices)
    r = ctx.compare("quiva", O.golden("qv_full.dexqv"), O.golden("qv_lossy.dexqv"), per_record=True)
    D.assert_same_report(r, lossy_report())
    assert_equal_images(ctx.compare("quiva", O.golden("qv_full.dexqv"), O.golden("qv_lossy.dexqv"), lossy=True, per_record=True), 5)


@pytest.mark.parametrize("budget", [None, 300000], ids=["whole", "sliced"])
def test_images_walked_on_the_device_give_the_identical_report(ctx, monkeypatch, budget):
    """DEXGPU_TEST=device_walk_min=1: both plans are made on the device, as those of images from 256 MiB on are -- image and index
    stay there, and either decode installs its own group index"""
    set_flag(monkeypatch, "device_walk_min", 1)
    if budget is not None:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
    r = ctx.compare("quiva", O.golden("qv_full.dexqv"), O.golden("qv_lossy.dexqv"), per_record=True)
    D.assert_same_report(r, lossy_report())
    assert_equal_images(ctx.compare("quiva", O.golden("qv_full.dexqv"), O.golden("qv_lossy.dexqv"), lossy=True, per_record=True), 5)
    mine = ctx.dexqv(O.golden("qv_mid.quiva"))
    assert_equal_images(ctx.compare("quiva", O.golden("qv_mid.dexqv"), mine, per_record=True), 5)


# ---- images of edited texts ----------------------------------------------------------------------------------------------------------
def seq_records(text):
    """a .fasta / .arrow text -> [[header line, sequence]]"""
    out = []
    for line in text.split(b"\n")[:-1]:
        if line.startswith(b">"):
            out.append([line, b""])
        else:
            out[-1][1] += line
    return out


def seq_text(recs, width=80):
    return b"".join(h + b"\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)) for h, s in recs)


def quiva_records(text):
    lines = text.split(b"\n")[:-1]
    return [lines[i:i + 6] for i in range(0, len(lines), 6)]


def quiva_text(recs):
    return b"".join(l + b"\n" for r in recs for l in r)


def shorter_header(h, by):
    """.../beg_end ... -> .../beg_(end - by) ..."""
    name, _, rest = h.partition(b" ")
    front, end = name.rsplit(b"_", 1)
    return front + b"_" + str(int(end) - by).encode() + b" " + rest


def other_well(h, well):
    name, _, rest = h.partition(b" ")
    prefix, _, span = name.rsplit(b"/", 2)
    return prefix + b"/" + str(well).encode() + b"/" + span + b" " + rest


def swap_letter(s, k):
    """another base (pulse width) at place k, in the case of the one that was there"""
    was = s[k:k + 1]
    now = (b"2" if was == b"1" else b"1") if was.isdigit() else (b"c" if was.lower() == b"a" else b"a")
    return s[:k] + (now.upper() if was.isupper() else now) + s[k + 1:]


def seq_edits(kind):
    """name -> the edited text"""
    base = O.golden("ta_small.fasta" if kind == "fasta" else "ar_small.arrow")
    recs = seq_records(base)
    n = len(recs)
    out = {}
    r = [list(x) for x in recs]
    for i, k in ((0, 0), (n // 2, len(r[n // 2][1]) // 2), (n - 1, len(r[n - 1][1]) - 1)):
        r[i][1] = swap_letter(r[i][1], k)
    out["bases"] = seq_text(r)
    out["dropped"] = seq_text(recs[:-1])
    r = [list(x) for x in recs]
    r[3] = [shorter_header(r[3][0], 5), swap_letter(r[3][1][:-5], 7)]
    out["shorter"] = seq_text(r)
    r = [list(x) for x in recs]
    r[0][0] = other_well(r[0][0], 3)
    out["well"] = seq_text(r)
    prefix = recs[0][0][1:].split(b"/")[0]
    out["prefix"] = base.replace(b">" + prefix + b"/", b">" + prefix[:-1] + b"x/")
    return base, out


def quiva_edits():
    base = O.golden("qv_mid.quiva")
    recs = quiva_records(base)
    n = len(recs)
    out = {}
    r = [list(x) for x in recs]
    k = len(r[n // 2][3]) // 3
    c = r[n // 2][3][k]
    r[n // 2][3] = r[n // 2][3][:k] + bytes([c + 40 if c + 40 < 127 else c - 40]) + r[n // 2][3][k + 1:]
    out["qv40"] = quiva_text(r)
    r = [list(x) for x in recs]
    for i, k in ((0, 0), (n // 2, len(r[n // 2][5]) // 2), (n - 1, len(r[n - 1][5]) - 1)):
        r[i][5] = swap_letter(r[i][5], k)                         # (the substitution tags are bases)
    out["bases"] = quiva_text(r)
    out["dropped"] = quiva_text(recs[:-1])
    r = [list(x) for x in recs]
    r[2] = [shorter_header(r[2][0], 9)] + [l[:-9] for l in r[2][1:]]
    r[2][4] = r[2][4][:4] + bytes([r[2][4][4] ^ 1]) + r[2][4][5:]      # (a merge QV in what is left of it)
    out["shorter"] = quiva_text(r)
    r = [list(x) for x in recs]
    r[0][0] = b"@" + other_well(r[0][0], 1)[1:]
    out["well"] = quiva_text(r)
    prefix = recs[0][0][1:].split(b"/")[0]
    out["prefix"] = base.replace(b"@" + prefix + b"/", b"@" + prefix[:-1] + b"x/")
    return base, out


EDITS = [(k, e) for k in ("fasta", "arrow") for e in ("bases", "dropped", "shorter", "well", "prefix")] + \
        [("quiva", e) for e in ("qv40", "bases", "dropped", "shorter", "well", "prefix")]


@pytest.mark.parametrize("budget", [None, "small"], ids=["whole", "sliced"])
@pytest.mark.parametrize("kind,edit", EDITS, ids=[f"{k}-{e}" for k, e in EDITS])
def test_an_edited_text_is_reported_as_the_texts_differ(ctx, monkeypatch, kind, edit, budget):
    base, edits = quiva_edits() if kind == "quiva" else seq_edits(kind)
    enc = {"fasta": ctx.dexta, "arrow": ctx.dexar, "quiva": ctx.dexqv}[kind]
    a, b = enc(base), enc(edits[edit])
    if budget is not None:                                        # (the floors of the budget: 128 KiB of text, 4 KiB of image)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "131072" if kind == "quiva" else "4096")
    want = D.report(kind, base, edits[edit])
    assert not want["same"]
    D.assert_same_report(ctx.compare(kind, a, b, per_record=True), want)
    D.assert_same_report(ctx.compare(kind, b, a, per_record=True), D.report(kind, edits[edit], base))
    if edit == "qv40":
        assert list(want["max_abs"]) == [0, 0, 40, 0, 0] and list(want["differ"]) == [0, 0, 1, 0, 0]
    if edit == "shorter":
        assert (want["lengths_differ"], want["headers_differ"], want["records_differ"]) == (1, 1, 1)
    if edit == "well":
        assert (want["headers_differ"], want["first_header"], want["records_differ"]) == (1, 0, 0)
    if edit == "prefix":
        assert want["prefix_differs"] and want["headers_differ"] == 0 and want["records_differ"] == 0
    if edit == "dropped":
        assert want["records_a"] == want["records_b"] + 1 and want["records_differ"] == 0


# ---- errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar"), ("quiva", "qv_mid.dexqv")])
def test_a_truncated_image_is_its_drivers_error_and_names_the_side(ctx, kind, name):
    img = O.golden(name)
    hurt = img[:len(img) - 3] if kind != "quiva" else img[:len(img) // 2]
    with pytest.raises(L.DexGPUError) as own:
        ctx.undexqv(hurt) if kind == "quiva" else ctx.undexta(hurt) if kind == "fasta" else ctx.undexar(hurt)
    for a, b, side in ((hurt, img, b"a:"), (img, hurt, b"b:"), (hurt, hurt, b"a:")):
        with pytest.raises(L.DexGPUError) as e:
            ctx.compare(kind, a, b)
        assert e.value.code == own.value.code == -3
        assert ctx.lib.dx_last_error(ctx.h).startswith(side), ctx.lib.dx_last_error(ctx.h)
    for a, b, side in ((b"", img, b"a:"), (img, b"\x00\x01garbage", b"b:")):      # (no image of anything)
        with pytest.raises(L.DexGPUError):
            ctx.compare(kind, a, b)
        assert ctx.lib.dx_last_error(ctx.h).startswith(side), ctx.lib.dx_last_error(ctx.h)


def test_out_is_untouched_by_an_error_and_lossy_is_quivas_alone(ctx):
    import ctypes as C
    img = O.golden("ta_small.dexta")
    cm = L.Compare()
    C.memset(C.byref(cm), 0x5A, C.sizeof(cm))
    rec = C.c_void_p(0x1234)
    assert ctx.lib.dx_file_compare(ctx.h, L.DX_KIND_FASTA, img, len(img), img[:-3], len(img) - 3, 0, C.byref(cm), C.byref(rec)) == -3
    assert bytes(cm) == b"\x5a" * C.sizeof(cm) and not rec.value
    for kind, name in (("fasta", "ta_small.dexta"), ("arrow", "ar_small.dexar")):
        with pytest.raises(L.DexGPUError) as e:
            ctx.compare(kind, O.golden(name), O.golden(name), lossy=True)
        assert e.value.code == -1
