"""The texts of _index_cases.py under the host indexer (dx_index_quiva / dx_index_seq, the reference of tests/test_gpu_index.py): they
reach the edges they were built for, the good ones are taken, and every malformed one is refused at the line and with the code
written out in its generator.  No GPU."""
import numpy as np
import pytest

import _index_cases as G
from dextractor_amd import api

KINDS = ("fasta", "arrow")


def quiva_newlines(text):
    """[6, n] newline positions by line role (header, data lines 1..5), from the host index alone"""
    off, ln, _, _ = api.index_quiva(text)
    off, step = off.astype(np.int64), ln.astype(np.int64) + 1
    return np.stack([off - 1] + [off + (j + 1) * step - 1 for j in range(5)])


def seq_marks(kind, text):
    """-> newline positions of header lines, of all other lines, and the headers' first bytes: the record extents are the host
    index's, the newlines inside a record the text's"""
    off, tl, _, _, _, _ = api.index_seq(text, arrow=kind == "arrow")
    off, tl = off.astype(np.int64), tl.astype(np.int64)
    assert (off[1:] > off[:-1] + tl[:-1]).all() and off[-1] + tl[-1] == len(text)
    hdr_nl = off - 1
    starts = np.concatenate([[0], off[:-1] + tl[:-1]])
    return hdr_nl, np.setdiff1d(G.newlines(text), hdr_nl), starts


def residues(pos):
    return set((np.asarray(pos) % G.THREAD).tolist())


def test_quiva_phase_texts_put_every_line_role_at_every_phase_and_a_newline_on_every_tile_edge():
    texts = G.quiva_phase_texts()
    roles = [np.concatenate(r) for r in zip(*(quiva_newlines(c.text) for c in texts))]
    for j, pos in enumerate(roles):
        print(f"quiva line role {j}: {len(pos)} newlines, residues mod 64 covered: {len(residues(pos))}/64")
        assert residues(pos) == set(range(64)), j
    at = set(np.concatenate(roles).tolist())
    print("quiva newlines at tile edges:", [t for t in G.EDGES if t in at])
    assert all(t in at for t in G.EDGES)
    for c in texts:
        assert len(c.text) > 3 * G.TILE
        lens = api.index_quiva(c.text)[1]
        assert (lens == 0).any() and max(len(h) for h in c.text.split(b"\n")[::6]) > 64, c.name


@pytest.mark.parametrize("kind", KINDS)
def test_seq_phase_texts_put_headers_and_lines_at_every_phase_and_on_every_tile_edge(kind):
    texts = G.seq_phase_texts(kind)
    marks = [seq_marks(kind, c.text) for c in texts]
    hdr_nl, other_nl, starts = (np.concatenate(x) for x in zip(*marks))
    for name, pos in (("header", hdr_nl), ("other", other_nl)):
        print(f"{kind} {name} lines: {len(pos)} newlines, residues mod 64 covered: {len(residues(pos))}/64")
        assert residues(pos) == set(range(64)), name
    nl_at, hdr_at = set(hdr_nl.tolist()) | set(other_nl.tolist()), set(starts.tolist())
    print(f"{kind} newlines at tile edges:", [t for t in G.EDGES if t in nl_at], "header starts:", [t for t in G.EDGES if t in hdr_at])
    assert all(t in nl_at and t in hdr_at for t in G.EDGES)
    for c in texts:                                                # what each text holds besides
        lines = c.text.split(b"\n")[:-1]
        off, tl, ns, _, _, _ = api.index_seq(c.text, arrow=kind == "arrow")
        assert b"" in lines and (tl[1:-1] == 0).any(), c.name                     # blank lines; records of no line in the middle
        assert any(b">" in ln[1:] for ln in lines), c.name                      # a '>' that starts no line
        assert set(G.SEQ_WIDTHS) <= {len(ln) for ln in lines if ln[:1] != b">"}, c.name
        assert (tl - ns > (ns + 14) // 15).any(), c.name                         # more lines than symbols need: blank ones counted


def test_length_texts_have_the_lengths_they_name():
    for texts in (G.quiva_length_texts(), G.seq_length_texts("fasta"), G.seq_length_texts("arrow")):
        ns = [len(c.text) for c in texts]
        assert ns == list(G.QV_LENGTHS)
        assert {n % G.CHUNK for n in ns} == {0, 1, 15}
        assert all(k * G.TILE + d in ns for k in (1, 2) for d in (-1, 0, 1))
    print("text lengths:", G.QV_LENGTHS)


def test_host_takes_every_good_text():
    n = 0
    for c in G.quiva_phase_texts() + G.quiva_length_texts():
        assert G.host_refusal("quiva", c.text) is None, c.name
        n += 1
    for kind in KINDS:
        for c in G.seq_phase_texts(kind) + G.seq_length_texts(kind):
            assert G.host_refusal(kind, c.text) is None, c.name
            n += 1
    print("good texts:", n)


@pytest.mark.parametrize("kind", KINDS)
def test_host_takes_a_line_of_99998_characters_and_refuses_99999(kind):
    cases = G.seq_limit_texts(kind)
    assert [line is None for _, line in cases] == [True, True, False, False]
    for c, line in cases:
        longest = max(c.text.split(b"\n"), key=len)
        assert len(longest) == (G.LINE_LIMIT - 2 if line is None else G.LINE_LIMIT - 1)
        assert c.text.split(b"\n").index(longest) >= 300                         # beyond the first 256 lines
        assert G.host_refusal(kind, c.text) == (None if line is None else (line, G.TOO_LONG)), c.name


def test_host_refuses_every_quiva_defect_where_its_generator_says():
    cases = G.quiva_defect_texts()
    assert len(cases) == 18 and sum(d.device is None for d in cases) == 2
    for d in cases:
        assert G.host_refusal("quiva", d.text) == (d.line, d.code), d.name
    mixed, cut = cases[-2:]
    assert (mixed.line, mixed.code) == (1801, G.BAD_HEADER)
    assert (cut.line, cut.code) == (4204, G.RAGGED) and cut.text.rfind(b"@") > cut.text.rfind(b"\n")
    assert G.host_refusal("quiva", G._join(G._qv_entries(1000))) is None


@pytest.mark.parametrize("kind", KINDS)
def test_host_refuses_every_seq_defect_where_its_generator_says(kind):
    cases = G.seq_defect_texts(kind)
    assert len(cases) == (5 if kind == "arrow" else 4)
    for d in cases:
        assert G.host_refusal(kind, d.text) == (d.line, d.code), d.name
    assert [(d.line, d.code) for d in cases[:4]] == [(1, G.NO_HEADER), (5000, G.TOO_LONG), (6600, G.TOO_LONG), (4951, G.BAD_HEADER)]
    assert G.host_refusal(kind, G._join(G._seq_records(kind, 200))) is None


@pytest.mark.parametrize("kind", ("quiva",) + KINDS)
def test_mutants_are_of_both_kinds(kind):
    good = G.quiva_phase_texts()[5].text if kind == "quiva" else G.seq_phase_texts(kind)[5].text
    ms = G.mutants(good, 200, 77)
    assert len(ms) == 200 and all(m.text[-1:] == b"\n" for m in ms)
    refused = sum(G.host_refusal(kind, m.text) is not None for m in ms)
    exempt = sum(G.ends_with_a_header(m.text) for m in ms) if kind != "quiva" else 0
    print(f"{kind} mutants: {200 - refused} taken, {refused} refused by the host, {exempt} end with a header")
    if kind == "quiva":
        assert 200 - refused >= 10 and refused >= 100
    else:
        assert exempt <= 10 and 200 - refused >= 20 and refused >= 20
