"""Texts for the tests of the text front end (csrc/dx_index.hip), built around what its kernels can get wrong: a newline at every
phase of the 16-byte chunk, the 64 bytes of a thread and the 16 KiB tile of a workgroup; text lengths at and next to those edges;
lines at the length limit; defects far from the text's start and several at once; single-byte damage.  No GPU here: every generator
is a pure function of fixed seeds, and tests/test_index_cases_host.py checks with the host indexer that the texts reach what they
were built to reach.  Expected values are written out, never taken from the library."""
import functools
from collections import namedtuple

import numpy as np

from dextractor_amd import synth

CHUNK, THREAD, TILE = 16, 64, 16384                     # load_chunk, IDX_PER_THREAD, IDX_TILE
EDGES = tuple(k * TILE + d for k in (1, 2) for d in (-1, 0, 1))
LINE_LIMIT = 100000                                     # DX_LINE_LIMIT: a line of LINE_LIMIT - 2 characters is the longest taken
NO_NEWLINE, NO_HEADER, BAD_HEADER, INCOMPLETE, RAGGED, TOO_LONG = 1, 2, 3, 4, 5, 6       # DX_IDX_* (include/dexgpu.h)

Case = namedtuple("Case", "name text")
# line / code: what the host indexer says (1-based line).  device: the (line, code) the device call must give, None where only
# its refusal is pinned (a header whose fields do not parse, met behind a defect of structure).
Defect = namedtuple("Defect", "name text line code device")

MOVIE = "m54006_170209_" + "abcdefghijklmnopqrstuvwxyz" * 4             # movie names are prefixes of this
QV_LENS = (0, 1, 2, 3, 5, 7, 15, 16, 17, 31, 47, 48, 63, 64, 65, 100, 129, 200)
SEQ_WIDTHS = (1, 15, 16, 17, 63, 64, 65)
POOL = 4096


def movie(m):
    return MOVIE[:m]


@functools.lru_cache(maxsize=None)
def _pool():
    """[5, POOL] QV characters in line order (the tag line 'N' exactly where the deletion line holds its run character)"""
    return synth.qv_lines(4242, 0, POOL, synth.pacbio_profile())


@functools.lru_cache(maxsize=None)
def _body(L, s):
    p = _pool()
    return b"".join(p[r, s: s + L].tobytes() + b"\n" for r in range(5))


def newlines(text):
    return np.flatnonzero(np.frombuffer(text, np.uint8) == 10)


# ---- .quiva ------------------------------------------------------------------------------------------------------------------------

def quiva_text(seed, m, L0, min_bytes=3 * TILE + 1024):
    """Entries of mixed line lengths, five empty lines among them, every ninth header longer than 64 bytes (its well number written
    with leading zeros); the movie name has m characters and entry 0 has L0 symbols (written with three digits, so that the header's
    length does not depend on it): both only shift what follows."""
    rng = np.random.default_rng(seed)
    mv, parts, size, i = movie(m), [], 0, 0
    while size < min_bytes:
        L = L0 if i == 0 else int(rng.choice(QV_LENS))
        s = int(rng.integers(0, POOL - 256))
        well = f"{i + 1:060d}" if i % 9 == 4 else str(i + 1)
        end = f"{L:03d}" if i == 0 else str(L)
        parts.append(f"@{mv}/{well}/0_{end} RQ=0.{800 + i % 100}\n".encode())
        parts.append(_body(L, s))
        size += len(parts[-2]) + len(parts[-1])
        i += 1
    return b"".join(parts)


def _shifted(nl0, is_hdr, first, m, L0):
    """newline positions of the text whose m = 0, L0 = 0 form has its newlines at nl0"""
    lens = np.diff(np.concatenate([[-1], nl0]))
    lens = lens + m * is_hdr
    lens[first] += L0
    return np.cumsum(lens) - 1


def _aim(text_of, is_hdr_of, first, target, header_start=False):
    """The first (m, L0) for which text_of(m, L0) has a newline at `target` (header_start: a header's first byte there)."""
    t0 = text_of(0, 0)
    nl0 = newlines(t0)
    is_hdr = is_hdr_of(t0, nl0)
    for m in range(1, 33):
        for L0 in range(0, 64):
            nl = _shifted(nl0, is_hdr, first, m, L0)
            if header_start:
                k = np.searchsorted(nl, target - 1)
                hit = k + 1 < len(nl) and nl[k] == target - 1 and is_hdr[k + 1]
            else:
                k = np.searchsorted(nl, target)
                hit = k < len(nl) and nl[k] == target
            if hit:
                return m, L0
    raise AssertionError(f"no shift puts a line edge at {target}")


def _qv_is_hdr(text, nl):
    return (np.arange(len(nl)) % 6 == 0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def quiva_phase_texts():
    """One text shifted by the movie name's length (1..8) and entry 0's length (0..3), and for each tile edge a shift that puts a
    newline on it."""
    out = [Case(f"quiva m={m} L0={L0}", quiva_text(7, m, L0)) for m in range(1, 9) for L0 in range(4)]
    for t in EDGES:
        m, L0 = _aim(lambda m, L0: quiva_text(7, m, L0), _qv_is_hdr, slice(1, 6), t)
        c = Case(f"quiva m={m} L0={L0}: a newline at {t}", quiva_text(7, m, L0))
        assert c.text[t] == 10
        out.append(c)
    return out


def _quiva_of_length(n, seed=11):
    """a good text of exactly n bytes: the last entry's line length and the zeros in front of its well number take up the rest"""
    whole = quiva_text(seed, 5, 9, min_bytes=n)
    starts = np.concatenate([[0], newlines(whole) + 1])[::6]
    cut = int(starts[np.searchsorted(starts, n - 400, side="right") - 1])
    well, rest = int(np.searchsorted(starts, cut)) + 1, n - cut
    for L in range((rest - 5 - 12) // 5, 0, -1):
        least = len(f"@{movie(5)}/{well}/0_{L} RQ=0.85\n")
        pad = rest - 5 * (L + 1) - least
        if 0 <= pad <= 60:
            text = whole[:cut] + f"@{movie(5)}/{well:0{len(str(well)) + pad}d}/0_{L} RQ=0.85\n".encode() + _body(L, 17)
            assert len(text) == n
            return text
    raise AssertionError(n)


QV_LENGTHS = EDGES + (40000, 40001, 40015)              # n mod 16 = 15, 0, 1 at the tile edges; 0, 1, 15 inside a tile


@functools.lru_cache(maxsize=None)
def quiva_length_texts():
    return [Case(f"quiva of {n} bytes", _quiva_of_length(n)) for n in QV_LENGTHS]


# ---- .fasta / .arrow -----------------------------------------------------------------------------------------------------------------

def _seq_header(kind, mv, i, n, rng, end=None):
    beg = int(rng.integers(0, 5000))
    h = f">{mv}/{i * 3 + 1}/{beg}_{end if end is not None else beg + n}"
    if kind == "arrow":
        sn = rng.integers(100, 2000, 4)
        return (h + " SN=" + ",".join(f"{v / 100:.2f}" for v in sn) + "\n").encode()
    return (h + f" RQ=0.{int(rng.integers(750, 900))}\n").encode()


def seq_text(kind, seed, m, L0, min_bytes=3 * TILE + 1024):
    """Records of line widths 1, 15, 16, 17, 63, 64, 65; every fifth has no sequence line at all, others a blank line inside or behind
    them, others a '>' inside a line.  Record 0 is one line of L0 symbols (L0 = 0: a blank line)."""
    rng = np.random.default_rng(seed)
    abc = np.frombuffer(b"ACGT" if kind == "fasta" else b"1234", np.uint8)
    mv, parts, size, i = movie(m), [], 0, 0
    while size < min_bytes or (i - 1) % 5 == 0:         # (the last record has a sequence line: no header ends the text)
        width = SEQ_WIDTHS[i % 7]
        n = L0 if i == 0 else 0 if i % 5 == 0 else int(rng.integers(1, 40 if width == 1 else 400))
        seq = abc[(rng if i else np.random.default_rng(seed + 1000)).integers(0, 4, n)]
        lines = [seq[k: k + width].tobytes() for k in range(0, n, width)] if i else [seq.tobytes()]
        if i % 6 == 1 and lines and len(lines[-1]) > 1:
            lines[-1] = lines[-1][:-1] + b">"           # a '>' that starts no line
        if i % 7 == 3 and i % 5:
            lines.insert(len(lines) // 2, b"")          # a blank line inside the record
        if i % 11 == 2 and i % 5:
            lines.append(b"")                           # ... and behind it
        parts.append(_seq_header(kind, mv, i, n, rng, end=f"{L0:03d}" if i == 0 else None))
        parts.append(b"".join(ln + b"\n" for ln in lines))
        size += len(parts[-2]) + len(parts[-1])
        i += 1
    return b"".join(parts)


def _seq_is_hdr(text, nl):
    starts = np.concatenate([[0], nl[:-1] + 1])
    return ((np.frombuffer(text, np.uint8)[starts] == ord(">")) & (nl > starts)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def seq_phase_texts(kind):
    """As quiva_phase_texts; and for each tile edge a shift that puts a header's first byte on it."""
    seed = 21 if kind == "fasta" else 22
    out = [Case(f"{kind} m={m} L0={L0}", seq_text(kind, seed, m, L0)) for m in range(1, 9) for L0 in range(4)]
    for t in EDGES:
        for what in ("a newline", "a header's first byte"):
            m, L0 = _aim(lambda m, L0: seq_text(kind, seed, m, L0), _seq_is_hdr, slice(1, 2), t, header_start=what != "a newline")
            c = Case(f"{kind} m={m} L0={L0}: {what} at {t}", seq_text(kind, seed, m, L0))
            assert c.text[t] == (10 if what == "a newline" else ord(">")) and (what == "a newline" or c.text[t - 1] == 10)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def seq_length_texts(kind):
    """good texts of exactly n bytes: the last line takes up the rest"""
    out = []
    for n in QV_LENGTHS:
        whole = seq_text(kind, 31, 4, 6, min_bytes=n)
        nl = newlines(whole)
        hdr = np.flatnonzero(_seq_is_hdr(whole, nl))
        starts = np.concatenate([[0], nl[:-1] + 1])[hdr]
        cut = int(starts[np.searchsorted(starts, n - 300, side="right") - 1])           # the start of a record
        rng = np.random.default_rng(n)
        h = _seq_header(kind, movie(4), 99999, 7, rng)
        fill = (b"ACGT" if kind == "fasta" else b"1234") * 1000
        text = whole[:cut] + h + fill[: n - cut - len(h) - 1] + b"\n"
        assert len(text) == n and n - cut - len(h) - 1 > 0
        out.append(Case(f"{kind} of {n} bytes", text))
    return out


@functools.lru_cache(maxsize=None)
def seq_limit_texts(kind):
    """-> [(Case, refused line or None)]: a sequence line and a header line of LINE_LIMIT - 2 characters (taken) and of LINE_LIMIT - 1
    (refused), each behind more than 300 short lines"""
    front = seq_text(kind, 41, 3, 5, min_bytes=8000)
    at = len(newlines(front))
    assert at > 300
    rng = np.random.default_rng(5)
    abc = np.frombuffer(b"ACGT" if kind == "fasta" else b"1234", np.uint8)
    out = []
    for n in (LINE_LIMIT - 2, LINE_LIMIT - 1):
        h = _seq_header(kind, movie(3), 50000, n, rng)
        long_seq = front + h + abc[rng.integers(0, 4, n)].tobytes() + b"\n" + h + abc.tobytes() + b"\n"
        out.append((Case(f"{kind}: a sequence line of {n} characters", long_seq), None if n == LINE_LIMIT - 2 else at + 2))
        wide = h[:-1] + b" " + b"x" * (n - len(h))
        assert len(wide) == n
        out.append((Case(f"{kind}: a header line of {n} characters", front + wide + b"\n" + abc.tobytes() + b"\n" + h + abc.tobytes() + b"\n"),
                    None if n == LINE_LIMIT - 2 else at + 1))
    return out


# ---- malformed texts -----------------------------------------------------------------------------------------------------------------

def _qv_entries(n, L=7):
    """n good entries of L symbols -> a list of [header, line 1 .. line 5] (no newlines)"""
    p = _pool()
    return [[f"@{movie(6)}/{i + 1}/0_{L} RQ=0.{800 + i % 100}".encode()] + [p[r, i % 1000: i % 1000 + L].tobytes() for r in range(5)]
            for i in range(n)]


def _join(entries):
    return b"".join(ln + b"\n" for e in entries for ln in e)


def _damage(e, how):
    """entry e (a list of lines) with one defect -> (lines, line within the entry 1..6, code)"""
    e = list(e)
    if how == "no @":
        e[0] = b"X" + e[0][1:]
        return e, 1, NO_HEADER
    if how == "empty header":
        e[0] = b""
        return e, 1, NO_HEADER
    if how == "no /":
        e[0] = e[0].replace(b"/", b"_")
        return e, 1, BAD_HEADER
    if how == "no RQ":
        e[0] = e[0][: e[0].index(b" RQ=")]
        return e, 1, BAD_HEADER
    assert how.startswith("ragged ")
    j = int(how[7:])                                    # the entry's data line 2..5
    e[j] = e[j][:-1]
    return e, j + 1, RAGGED


def quiva_defect_texts(n=1000, at=(300, 600, 700, 900)):
    """n good entries of 7 symbols with defects planted at entries `at` = (a, b, c, d), c the place of every single defect."""
    good = _qv_entries(n)
    a, b, c, d = at

    def plant(*where):
        es, first = list(good), None
        for i, how in where:
            es[i], line, code = _damage(good[i], how)
            if first is None or 6 * i + line < first[0]:
                first = (6 * i + line, code)
        return _join(es), first

    out = []
    for how in ("no @", "empty header", "no /", "ragged 2", "ragged 3", "ragged 4", "ragged 5"):
        text, first = plant((c, how))
        out.append(Defect(f"quiva: {how} at entry {c}", text, *first, first))
    head = _join(good[:c])
    for k in range(1, 5):
        text = head + _join([good[c][: 1 + k]])
        out.append(Defect(f"quiva: entry {c}, the last, cut after {k} data lines", text, 6 * c + k + 2, INCOMPLETE, (6 * c + k + 2, INCOMPLETE)))
    text = head + good[c][0]
    out.append(Defect(f"quiva: no newline behind the header of entry {c}", text, 6 * c + 1, NO_NEWLINE, (6 * c + 1, NO_NEWLINE)))
    text = head + good[c][0] + b"\n" + good[c][1]
    out.append(Defect(f"quiva: no newline behind the first data line of entry {c}", text, 6 * c + 2, NO_NEWLINE, (6 * c + 2, NO_NEWLINE)))
    for name, where in ((f"ragged at entry {c}, no @ at entry {d}", ((c, "ragged 3"), (d, "no @"))),
                        (f"no @ at entry {c}, ragged at entry {d}", ((c, "no @"), (d, "ragged 3"))),
                        (f"no / at entry {d}, no @ at entry {b}, ragged at entry {a}", ((d, "no /"), (b, "no @"), (a, "ragged 5")))):
        text, first = plant(*where)
        out.append(Defect("quiva: " + name, text, *first, first))
    text, first = plant((a, "no RQ"), (c, "ragged 3"))
    assert first == (6 * a + 1, BAD_HEADER)
    out.append(Defect(f"quiva: no RQ field at entry {a}, ragged at entry {c}", text, *first, None))
    text, first = plant((c, "ragged 3"))                # the last byte is looked at before any line: only the refusal is pinned
    out.append(Defect(f"quiva: ragged at entry {c}, the text cut inside its last header", text[:-50], *first, None))
    return out


def _seq_records(kind, n, seed=51):
    """n good records of 33 lines of 20 symbols -> a list of lists of lines"""
    rng = np.random.default_rng(seed)
    abc = np.frombuffer(b"ACGT" if kind == "fasta" else b"1234", np.uint8)
    return [[_seq_header(kind, movie(6), i, 640, rng)[:-1]] + [abc[rng.integers(0, 4, 20)].tobytes() for _ in range(32)] for i in range(n)]


def seq_defect_texts(kind, n=200, rec=150, line=5000):
    """n good records of 33 lines each, one defect in each text."""
    good = _seq_records(kind, n)
    assert (line - 1) % 33 and line < 33 * n
    out = [Defect(f"{kind}: the first line is no header", b"ACGT\n" + _join(good), 1, NO_HEADER, (1, NO_HEADER))]
    es = [list(e) for e in good]
    es[(line - 1) // 33][(line - 1) % 33] = b"A" * LINE_LIMIT
    out.append(Defect(f"{kind}: line {line} is too long", _join(es), line, TOO_LONG, (line, TOO_LONG)))
    out.append(Defect(f"{kind}: no final newline", _join(good)[:-1], 33 * n, TOO_LONG, (33 * n, TOO_LONG)))
    es = [list(e) for e in good]
    es[rec][0] = es[rec][0].replace(b"/", b"_")
    out.append(Defect(f"{kind}: no / in the header of record {rec}", _join(es), 33 * rec + 1, BAD_HEADER, (0, BAD_HEADER)))
    if kind == "arrow":
        es = [list(e) for e in good]
        es[rec][0] = es[rec][0][: es[rec][0].rindex(b",")]
        out.append(Defect(f"arrow: three SN values in the header of record {rec}", _join(es), 33 * rec + 1, BAD_HEADER, (0, BAD_HEADER)))
    return out


def big_defect_text(kind):
    """One defect behind the first MiB of a text of more than 1 MiB (the whole-file drivers index such a text on the device)."""
    if kind == "quiva":
        es, at = _qv_entries(25000), 22000
        es[at], line, code = _damage(es[at], "ragged 3")
        d = Defect(f"quiva: ragged at entry {at} of 25000", _join(es), 6 * at + line, code, (6 * at + line, code))
    else:
        es, line = _seq_records(kind, 2000), 33 * 1800 + 17
        es[1800][16] = b"A" * LINE_LIMIT
        d = Defect(f"{kind}: line {line} of 66000 is too long", _join(es), line, TOO_LONG, (line, TOO_LONG))
    assert len(_join(es[: 22000 if kind == "quiva" else 1800])) > 1 << 20
    return d


def mutants(text, n, seed):
    """n single-byte edits of a good text, the four kinds in turn: a newline deleted, a newline inserted, a header's first byte
    overwritten, a '/' (of a header or of the data) overwritten.  None touches the last byte."""
    buf = np.frombuffer(text, np.uint8)
    lead = text[:1]
    nl = newlines(text)
    starts = np.concatenate([[0], nl[:-1] + 1])
    hdrs = starts[::6] if lead == b"@" else starts[(buf[starts] == ord(">")) & (nl > starts)]
    slashes = np.flatnonzero(buf == ord("/"))
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 4 == 0:
            p = int(rng.choice(nl[:-1]))
            out.append(Case(f"newline at {p} deleted", text[:p] + text[p + 1:]))
        elif i % 4 == 1:
            p = int(rng.integers(1, len(text) - 1))
            out.append(Case(f"newline inserted at {p}", text[:p] + b"\n" + text[p:]))
        elif i % 4 == 2:
            p = int(rng.choice(hdrs))
            out.append(Case(f"header start at {p} overwritten", text[:p] + b"x" + text[p + 1:]))
        else:
            p = int(rng.choice(slashes))
            out.append(Case(f"'/' at {p} overwritten", text[:p] + b"x" + text[p + 1:]))
        assert out[-1].text[-1:] == text[-1:] and out[-1].text != text
    return out


def ends_with_a_header(text):
    """dx_file_pack2.c: a sequence text whose last line is a header and not its only line never reaches the device index"""
    if len(text) < 2 or text[-1:] != b"\n":
        return False
    at = text.rfind(b"\n", 0, len(text) - 1) + 1
    return at > 0 and text[at: at + 1] == b">"


# ---- past 2^20 items -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def big_seq_text(kind, nrec=40, nsym=30000):
    """nrec records of nsym symbols, one to a line: more than 2^20 lines, the last records' lines beyond line 2^20"""
    rng = np.random.default_rng(61)
    abc = np.frombuffer(b"ACGT" if kind == "fasta" else b"1234", np.uint8)
    parts = []
    for i in range(nrec):
        body = np.full(2 * nsym, 10, np.uint8)
        body[::2] = abc[rng.integers(0, 4, nsym)]
        parts += [_seq_header(kind, movie(5), 7 ** (i // 5) + i, nsym, rng), body.tobytes()]       # (wells rise, 1 to 7 digits)
    return b"".join(parts)


@functools.lru_cache(maxsize=1)
def big_quiva_text(nent=(1 << 20) + 4097):
    """nent entries of 2..9 symbols cut from the pool at varying places, the well number the entry's number"""
    mv = movie(4).encode()
    return b"".join([b"@%b/%d/0_%d RQ=0.85%d\n%b" % (mv, i, 2 + i % 8, i % 10, _body(2 + i % 8, (i * 7) % 611)) for i in range(nent)])


# ---- the reference: the host indexer -------------------------------------------------------------------------------------------------

def host_refusal(kind, text):
    """None where dx_index_quiva / dx_index_seq takes the text, else its (line, code)"""
    import ctypes as C
    from dextractor_amd import _lib as L
    lib = L.load()
    cnt, pl, line, code = C.c_uint64(), C.c_size_t(), C.c_uint64(), C.c_int()
    if kind == "quiva":
        rc = lib.dx_index_quiva(text, len(text), 0, None, None, None, C.byref(cnt), C.byref(pl), C.byref(line), C.byref(code))
    else:
        rc = lib.dx_index_seq(int(kind == "arrow"), text, len(text), 0, None, None, None, None, None, C.byref(cnt), C.byref(pl),
                              C.byref(line), C.byref(code))
    assert rc in (0, -3)
    return None if rc == 0 else (line.value, code.value)
