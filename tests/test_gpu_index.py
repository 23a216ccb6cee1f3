"""The GPU text front end (dx_index_quiva_device / dx_index_seq_device, csrc/dx_index.hip) against the host indexer over the texts of
_index_cases.py: element by element and exact.  What those texts reach -- every phase of chunk, thread and tile, defects beyond the
first workgroup, more than 2^20 lines -- is asserted in tests/test_index_cases_host.py, without a GPU."""
import time

import numpy as np
import pytest

import _index_cases as G
import _oracle as O
from _flags import set_flag
from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

KINDS = ("fasta", "arrow")
ALL = ("quiva",) + KINDS


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


class At:
    """a device address"""
    def __init__(self, ptr):
        self.ptr = ptr


def device_index(ctx, kind, text, shift=0):
    """The device's index of `text`, which lies `shift` bytes into a buffer whose every other byte is a newline: a kernel that looks
    in front of the text or past its nbytes finds lines that the host does not."""
    a = np.full(shift + len(text) + 80, 10, np.uint8)
    a[shift: shift + len(text)] = np.frombuffer(text, np.uint8)
    d = ctx.to_device(a)
    try:
        if kind == "quiva":
            return ctx.index_quiva_device(At(d.ptr + shift), len(text))
        off, tl, ns, hdr, cnr, pl = ctx.index_seq_device(At(d.ptr + shift), len(text), arrow=kind == "arrow")
        return (off, tl, ns, hdr, pl, cnr) if kind == "arrow" else (off, tl, ns, hdr, pl)
    finally:
        d.free()


def host_index(kind, text):
    if kind == "quiva":
        return api.index_quiva(text)
    off, tl, ns, hdr, cnr, pl = api.index_seq(text, arrow=kind == "arrow")
    return (off, tl, ns, hdr, pl, cnr) if kind == "arrow" else (off, tl, ns, hdr, pl)


def device_refusal(ctx, kind, text):
    """-> (index, None) or (None, (line, code)); any refusal is DX_E_FORMAT"""
    try:
        return device_index(ctx, kind, text), None
    except L.DexGPUError as e:
        assert e.code == -3
        return None, (e.line, e.idx_code)


def same(got, want, name):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (name, k)


def good_texts(kind):
    return (G.quiva_phase_texts() + G.quiva_length_texts()) if kind == "quiva" else (G.seq_phase_texts(kind) + G.seq_length_texts(kind))


def dex(ctx, kind):
    return {"quiva": ctx.dexqv, "fasta": ctx.dexta, "arrow": ctx.dexar}[kind]


def oracle(kind):
    return {"quiva": O.dexqv, "fasta": O.dexta, "arrow": O.dexar}[kind]


# ---- good texts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ALL)
def test_index_of_every_phase_and_length_text_equals_the_hosts(ctx, kind):
    """a newline of every line role at every byte of a thread's 64, newlines and headers on and beside the tile edges; text lengths
    n mod 16 in {0, 1, 15}, n = 16384 k and one byte either side"""
    for c in good_texts(kind):
        same(device_index(ctx, kind, c.text), host_index(kind, c.text), c.name)


@pytest.mark.parametrize("kind", KINDS)
def test_a_line_of_99998_characters_is_taken_and_one_of_99999_refused(ctx, kind):
    for c, line in G.seq_limit_texts(kind):
        got, err = device_refusal(ctx, kind, c.text)
        if line is None:
            assert err is None, c.name
            same(got, host_index(kind, c.text), c.name)
        else:
            assert err == (line, G.TOO_LONG), c.name


@pytest.mark.parametrize("shift", [1, 3, 8, 15])
@pytest.mark.parametrize("kind", ALL)
def test_the_text_may_start_at_any_byte(ctx, kind, shift):
    c = good_texts(kind)[6]
    same(device_index(ctx, kind, c.text, shift), host_index(kind, c.text), c.name)


# ---- malformed texts -----------------------------------------------------------------------------------------------------------------

def test_quiva_defects_are_refused_at_the_hosts_line(ctx):
    """one defect in the third workgroup of k_qv_entries; two and three in different workgroups, where the lowest line wins whichever
    workgroup gets there first.  A header whose fields do not parse is met only once the structure has passed: with a ragged entry
    behind it the text is refused, at which of the two lines is not pinned; nor is it for a ragged entry in a text cut inside its
    last header, whose last byte is looked at first."""
    for d in G.quiva_defect_texts():
        got, err = device_refusal(ctx, "quiva", d.text)
        assert got is None, d.name
        if d.device is not None:
            assert err == d.device == (d.line, d.code), d.name


@pytest.mark.parametrize("kind", KINDS)
def test_seq_defects_are_refused_like_the_host(ctx, kind):
    """too long, no header, no final newline: the host's line and code; a header that does not parse: line 0 (include/dexgpu.h)"""
    for d in G.seq_defect_texts(kind):
        got, err = device_refusal(ctx, kind, d.text)
        assert d.device == ((0, G.BAD_HEADER) if d.code == G.BAD_HEADER else (d.line, d.code))
        assert got is None and err == d.device, d.name


@pytest.mark.parametrize("kind", ALL)
def test_single_byte_damage(ctx, kind):
    """200 one-byte edits of a good text: what the host refuses the device refuses; what the device takes it indexes as the host
    does; the device refuses nothing the host takes (no edit touches the last byte).  A sequence text that ends with a header
    never reaches the device (dx_file_pack2.c: ends_with_a_header) and is left out."""
    ms = G.mutants(good_texts(kind)[5].text, 200, 77)
    if kind != "quiva":
        left_out = [m for m in ms if G.ends_with_a_header(m.text)]
        assert len(left_out) <= 10
        ms = [m for m in ms if not G.ends_with_a_header(m.text)]
    for m in ms:
        want = G.host_refusal(kind, m.text)
        got, err = device_refusal(ctx, kind, m.text)
        if want is not None:
            assert got is None, (m.name, want)
        else:
            assert err is None, (m.name, err)
            same(got, host_index(kind, m.text), m.name)


# ---- through the whole-file drivers (1 MiB and more: indexed on the device) ----------------------------------------------------------------

def long_text(kind):
    text = G.quiva_text(7, 3, 2, min_bytes=(1 << 20) + 5000) if kind == "quiva" else G.seq_text(kind, 21, 3, 2, min_bytes=(1 << 20) + 5000)
    assert len(text) > 1 << 20
    return text


@pytest.mark.parametrize("kind", ALL)
def test_driver_on_a_long_phase_text_equals_the_oracle(ctx, kind):
    text = long_text(kind)
    same(device_index(ctx, kind, text), host_index(kind, text), kind)
    assert dex(ctx, kind)(text) == oracle(kind)(text)


@pytest.mark.parametrize("kind", ALL)
def test_driver_words_a_late_defect_as_with_the_host_index(ctx, kind, monkeypatch):
    d = G.big_defect_text(kind)
    assert device_refusal(ctx, kind, d.text) == (None, d.device)
    with pytest.raises(L.DexGPUError) as e1:
        dex(ctx, kind)(d.text)
    set_flag(monkeypatch, "host_index", "1")
    with pytest.raises(L.DexGPUError) as e2:
        dex(ctx, kind)(d.text)
    assert e1.value.code == e2.value.code == -3 and str(e1.value) == str(e2.value)
    assert f"line {d.line}:" in str(e2.value)


# ---- more than 2^20 items: the second round of k_scan_sums ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_more_than_2_20_lines(ctx, kind):
    """40 records of 30 000 symbols, one to a line: dx_scan_u32 over 1.2 M lines; records 35..39 lie beyond line 2^20"""
    text = G.big_seq_text(kind)
    want = host_index(kind, text)
    lines_before = np.cumsum(want[1][:-1].astype(np.int64) // 2 + 1)
    assert len(want[0]) == 40 and lines_before[33] < 1 << 20 < lines_before[34]
    same(device_index(ctx, kind, text), want, kind)
    assert dex(ctx, kind)(text) == oracle(kind)(text)


def test_more_than_2_20_entries(ctx):
    """2^20 + 4097 entries of 2..9 symbols: the front end's scans and the encoders' record-offset scans (dx_qv_sizes) past the first
    256 tile sums.  Timed: this is the suite's largest text (61 MB)."""
    t0 = time.perf_counter()
    text = G.big_quiva_text()
    want = host_index("quiva", text)
    assert len(want[0]) == (1 << 20) + 4097 and len(set(want[1].tolist())) == 8
    t1 = time.perf_counter()
    same(device_index(ctx, "quiva", text), want, "quiva")
    t2 = time.perf_counter()
    got = ctx.dexqv(text)
    t3 = time.perf_counter()
    ref = O.dexqv(text)
    t4 = time.perf_counter()
    print(f"61 MB quiva: text + host index {t1 - t0:.2f} s, device index {t2 - t1:.2f} s, dexqv {t3 - t2:.2f} s, oracle {t4 - t3:.2f} s")
    assert got == ref
