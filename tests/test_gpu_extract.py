"""dx_file_extract on the GPU (needs an MI355X): chosen records of a .dexta / .dexar / .dexqv image as the text undexta / undexar /
undexqv print for them alone.  Expected bytes are `cut` (tests/_subset.py, plain Python) of the oracle's decode of the image; for the
selections dx_file_subset accepts the text is also this library's decode of its subset image.  Bar: bit-exact."""
import functools

import numpy as np
import pytest

from _flags import set_flag

import _lines as LN
import _oracle as O
import _subset as S
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

pytestmark = pytest.mark.gpu

TWO_BIT = [("fasta", "ta_small.dexta"), ("fasta", "ta_edge.dexta"), ("fasta", "ta_lower_w60.dexta"), ("arrow", "ar_small.dexar"),
           ("fasta", "ta_small.legacy.dexta"), ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta")]
QUIVA = ["qv_tiny", "qv_runs", "qv_type2", "qv_nodel", "qv_lossy"]
WIDTHS = [1, 7, 60, 80, 10 ** 6]
WALKS = {"host": {"host_walk": "1"}, "device": {"device_walk_min": "0", "walk_piece": "8192"}}      # (as tests/test_gpu_walk.py selects them)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_budget(monkeypatch):
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)


def decode(kind, img, upper, width):
    return O.undexta(img, upper, width) if kind == "fasta" else O.undexar(img, width) if kind == "arrow" else O.undexqv(img, upper)


def own_decode(ctx, kind, img, upper, width):
    return ctx.undexta(img, upper, width) if kind == "fasta" else ctx.undexar(img, width) if kind == "arrow" else ctx.undexqv(img, upper)


def selections(lens):
    """name -> (units, does dx_file_subset accept them: ids that do not decrease, and a last unit with symbols)"""
    n = len(lens)
    mixed, empties = S.whole_and_intervals(lens, 20261019), S.one_empty_each(lens, 7)
    return {"whole_and_intervals": (mixed, True), "one_empty_each": (empties, True),
            "a_final_empty_unit": (LN.with_a_final_empty_unit(empties, lens), False), "reversed": (mixed[::-1], False),
            "shuffled_with_repeats": (LN.shuffled_with_repeats(lens, 11), False), "the_last_record": ([(n - 1, 0, lens[n - 1])], True)}


@functools.lru_cache(maxsize=None)
def case(kind, name, upper, width):
    """the oracle's text of an image under these options, its records' lengths, and every selection with its expected text: computed
    once, never changed"""
    img = O.golden(name)
    text = decode(kind, img, upper, width)
    lens = S.lengths(kind, text)
    return img, text, tuple(lens), {k: (tuple(u), ok, S.cut(kind, text, u, width)) for k, (u, ok) in selections(lens).items()}


def extract(ctx, kind, img, units, upper, width):
    """Context.extract with the offsets checked against the header lines of what came back -> the text"""
    got, toff = ctx.extract(kind, img, *S.selection_arrays(list(units)), upper=upper, width=width, offsets=True)
    assert toff.tolist() == LN.header_offsets(kind, got, len(units))
    return got


def check_case(ctx, kind, name, upper, width, agree):
    img, text, lens, sels = case(kind, name, upper, width)
    got, toff = ctx.extract(kind, img, upper=upper, width=width, offsets=True)                 # every record
    assert got == text and got == own_decode(ctx, kind, img, upper, width)
    assert toff.tolist() == LN.header_offsets(kind, text, len(lens))
    for key, (units, subset_takes_it, want) in sels.items():
        got = extract(ctx, kind, img, units, upper, width)
        assert got == want, (key, upper, width)
        if agree and subset_takes_it:
            sub = ctx.subset(kind, img, *S.selection_arrays(list(units)), lossy=False)           # (lossless: the subset image decodes to the cut text whatever the golden was made with)
            assert own_decode(ctx, kind, sub, upper, width) == got, (key, upper, width)


# ---- fasta, arrow ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", TWO_BIT, ids=[n for _, n in TWO_BIT])
def test_two_bit_selections_against_the_oracle(ctx, kind, name):
    for upper in (False, True) if kind == "fasta" else (False,):
        for width in WIDTHS:
            check_case(ctx, kind, name, upper, width, agree=width in (7, 80))


@pytest.mark.parametrize("key", ["reads_packed", "reads_whole"])
def test_a_two_bit_image_in_slices(ctx, monkeypatch, key):
    text = synth.make_seqfile("fasta", 60, seed=23, mean=3000).text
    img = O.dexta(text)
    lens = S.lengths("fasta", text)
    assert text == O.undexta(img, True, 80) and len(text) >= 2 * 65536       # (a slice of text is 64 KiB at least)
    set_flag(monkeypatch, key)
    for units, _ in selections(lens).values():
        want = S.cut("fasta", text, units)
        assert extract(ctx, "fasta", img, units, True, 80) == want   # (in one)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
        assert extract(ctx, "fasta", img, units, True, 80) == want
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET")


# ---- quiva -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", sorted(WALKS))
@pytest.mark.parametrize("name", QUIVA)
def test_quiva_selections_against_the_oracle(ctx, monkeypatch, name, walk):
    for k, v in WALKS[walk].items():
        set_flag(monkeypatch, k, v)
    for upper in (False, True):
        check_case(ctx, "quiva", name + ".dexqv", upper, 80, agree=walk == "host" and not upper)


@pytest.mark.parametrize("key", ["entries_packed", "entries_whole"])
def test_quiva_in_slices(ctx, monkeypatch, key):
    img = O.dexqv(synth.make_quiva(60, seed=23, mean=3000).text)
    text = O.undexqv(img, False)
    lens = S.lengths("quiva", text)
    assert len(text) >= 3 * 65536
    set_flag(monkeypatch, "host_walk")                               # (the image stays on the host: the loader decides what goes up)
    set_flag(monkeypatch, key)
    for units, _ in selections(lens).values():
        want = S.cut("quiva", text, units)
        assert extract(ctx, "quiva", img, units, False, 80) == want  # (in one)
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
        assert extract(ctx, "quiva", img, units, False, 80) == want
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET")


def test_quiva_in_slices_with_the_image_on_the_device(ctx, monkeypatch):
    img = O.dexqv(synth.make_quiva(60, seed=23, mean=3000).text)
    text = O.undexqv(img, True)
    units = LN.shuffled_with_repeats(S.lengths("quiva", text), 5)
    for k, v in WALKS["device"].items():
        set_flag(monkeypatch, k, v)
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    assert extract(ctx, "quiva", img, units, True, 80) == S.cut("quiva", text, units)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    img = O.golden("ta_small.dexta")
    for kind, image in (("fasta", img), ("quiva", O.golden("qv_tiny.dexqv"))):
        for ids, beg, end in (([0, 10 ** 6], None, None), ([0, 1], [0, 2], [0, 1]), ([0, 1], [0, 0], [0, 10 ** 6]), ([0, 1], [0, 0], None)):
            with pytest.raises(L.DexGPUError) as e:
                ctx.extract(kind, image, ids, beg, end)
            assert L.ERR_NAMES[e.value.code] == "DX_E_ARG" and ("unit 1:" in str(e.value) or end is None), str(e.value)
        one = [ctx.extract(kind, image, [i]) for i in (1, 0)]        # ids that decrease are an order like any other
        assert ctx.extract(kind, image, [1, 0]) == one[0] + one[1]
        text = decode(kind, image, False, 80)
        assert one[0] == S.cut(kind, text, [(1, None, None)]) and one[1] == S.cut(kind, text, [(0, None, None)])
        got, toff = ctx.extract(kind, image, np.zeros(0, np.uint64), offsets=True)
        assert got == b"" and toff.tolist() == [0]
        with pytest.raises(L.DexGPUError) as want:                   # a truncated image: the decoder's error
            own_decode(ctx, kind, image[:len(image) - 3], False, 80)
        for ids in (None, [0]):
            with pytest.raises(L.DexGPUError) as e:
                ctx.extract(kind, image[:len(image) - 3], ids)
            assert e.value.code == want.value.code
    with pytest.raises(L.DexGPUError) as e:
        ctx.extract("fasta", img, [0], width=0)
    assert L.ERR_NAMES[e.value.code] == "DX_E_ARG"
    assert ctx.extract("quiva", O.golden("qv_tiny.dexqv"), [0], width=0) == S.cut("quiva", O.undexqv(O.golden("qv_tiny.dexqv")), [(0, None, None)])
