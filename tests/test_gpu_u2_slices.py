"""The one slice loop under the packed-read drivers (csrc/dx_file_u2.c) on the GPU: census, find, find_edit spans, kmers and
kmers_wide over one small image this library packs from tests/_u2_slices.py's text -- empty records at the image's ends and side by
side, one record of 20000 symbols that alone exceeds the budget --, each whole and with DEXGPU_TEXT_BUDGET=4096.  The two runs agree
in every field, and each equals the reference its driver's own test holds it against (tests/_find.py, _find_span.py, _kmers.py,
_kmers_wide.py, test_gpu_census.py's census of the text): no expected value comes from the library."""
import numpy as np
import pytest

import _find as F
import _find_span as P
import _kmers as K
import _kmers_wide as W
import _oracle as O
import _u2_slices as U
from test_gpu_census import census_of_text, decode
from dextractor_amd import api

pytestmark = pytest.mark.gpu

PATTERNS = [U.PLANT, "ACGTAC", "ttttcc"]


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def image(ctx):
    """(the image, the text the oracle prints for it)"""
    text, lens = U.synthetic()
    img = U.image(ctx.dexta, text)
    assert img == U.image(O.dexta, text) and U.slices(lens, 4096) >= 3       # (tests/test_u2_slices_host.py holds the count against the loop's)
    return img, F.text_of("fasta", img)


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())
    return a == b


def whole_and_sliced(monkeypatch, run):
    """run() with the budget unset and with 4096 (the smallest figure the drivers take): the two answers agree in every field -> one"""
    monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    whole = run()
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", "4096")
    sliced = run()
    assert same(whole, sliced)
    return whole, sliced


def test_census(ctx, monkeypatch, image):
    img, _ = image
    want, per = census_of_text("fasta", decode("fasta", img))
    for got in whole_and_sliced(monkeypatch, lambda: ctx.census("fasta", img, per_record=True)):
        assert all(got[k] == want[k] for k in ("records", "symbols", "min_len", "max_len", "n50"))
        assert np.array_equal(got["code"], want["code"]) and not got["hist"].any()
        assert all(np.array_equal(got[k], v) for k, v in per.items())
    assert want["records"] == 40 and want["min_len"] == 0 and want["max_len"] == 20000


def test_find_with_per_record_counts(ctx, monkeypatch, image):
    img, text = image
    want = F.file_find("fasta", text, PATTERNS, 1, True)
    for got in whole_and_sliced(monkeypatch, lambda: ctx.find("fasta", img, PATTERNS, max_mismatches=1, both_strands=True, per_record=True)):
        F.assert_same_find(got, want)
    assert want[0]["rec_hits"][U.BIG] >= 2 and all(want[0]["rec_hits"][e] == 0 for e in U.EMPTY)


def test_find_edit_spans(ctx, monkeypatch, image):
    img, text = image
    want = P.file_find_spans("fasta", text, PATTERNS[:2], 1, True)
    for got in whole_and_sliced(monkeypatch, lambda: ctx.find_spans("fasta", img, PATTERNS[:2], max_errors=1, both_strands=True, per_record=True)):
        F.assert_same_find(got, want)
        assert np.array_equal(got[0]["start"], want[0]["start"]) and np.array_equal(got[0]["rec_len"], want[0]["rec_len"])
    assert want[0]["rec_hits"][U.BIG] >= 2 and list(want[0]["rec_len"][list(U.EMPTY)]) == [0, 0, 0, 0]


@pytest.mark.parametrize("k", [3, 9])
def test_kmers(ctx, monkeypatch, image, k):
    img, text = image
    want = K.file_kmers("fasta", text, k, True, 64, 2, 50)
    for rep, spec, lst in whole_and_sliced(monkeypatch, lambda: ctx.kmers("fasta", img, k, True, 64, 2, 50)):
        assert rep == want[0], (rep, want[0])
        assert np.array_equal(spec, want[1])
        assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in lst] == want[2]
    assert want[0]["records"] == 40 and want[0]["windows"] > 20000


def test_kmers_wide(ctx, monkeypatch, image):
    img, text = image
    want = W.file_kmers_wide("fasta", text, 17, True, 64, 1, 50)
    for rep, spec, lst in whole_and_sliced(monkeypatch, lambda: ctx.kmers_wide("fasta", img, 17, True, 64, 1, 50)):
        assert rep == want[0], (rep, want[0])
        assert np.array_equal(spec, want[1])
        assert [(int(e["count"]), int(e["code"]), bytes(e["letters"])) for e in lst] == want[2]
    assert want[0]["records"] == 40 and want[0]["windows"] > 20000
