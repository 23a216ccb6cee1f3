"""The round-trip check: dx_verify_ranges (device comparison of byte ranges), dx_file_verify (does an image give its text back?)
and DEXGPU_VERIFY=1 in dexta / dexar / dexqv.  Expected answers come from numpy, from the oracle's decoders (run with the options
the report names) and from a plain first-difference over bytes in Python -- never from the library."""
import os
import re
import subprocess

import numpy as np
import pytest

import _oracle as O
from _flags import test_env
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dextractor_amd", "bin")
BUDGETS = [None, 1 << 20, 5 << 20]


# ---- without a GPU ---------------------------------------------------------------------------------------------------------
def test_abi_has_the_round_trip_check():
    hdr = open(os.path.join(ROOT, "include", "dexgpu.h")).read()
    lib = L.load()
    for name in ("dx_verify_ranges", "dx_file_verify"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert hasattr(lib, name), f"{name} is not exported by libdexgpu.so"
        assert name in L.SIGNATURES
    assert "dx_verify_report" in hdr
    assert callable(getattr(api.Context, "verify", None)) and callable(getattr(api.Context, "verify_ranges", None))
    assert "DEXGPU_VERIFY" in open(os.path.join(ROOT, "dextractor_amd", "csrc", "dx_env.h")).read()


def test_report_layout_matches_the_header():
    """dx_verify_report as ctypes sees it: four 32-bit fields, then seven 64-bit ones, no padding"""
    assert [f for f, _ in L.VerifyReport._fields_] == ["ok", "upper", "width", "where", "records_src", "records_img", "record",
                                                      "line", "column", "src_byte", "img_byte"]
    import ctypes
    assert ctypes.sizeof(L.VerifyReport) == 16 + 7 * 8


# ---- Python's own answers ----------------------------------------------------------------------------------------------------
def first_difference(a: bytes, b: bytes):
    """first index at which a and b differ (min length when one is the other's beginning), None when equal"""
    n = min(len(a), len(b))
    x, y = np.frombuffer(a, np.uint8, n), np.frombuffer(b, np.uint8, n)
    d = np.flatnonzero(x != y)
    if len(d):
        return int(d[0])
    return None if len(a) == len(b) else n


def locate(kind: str, text: bytes, byte: int):
    """(record, line of the record, column) of a byte of a source text"""
    lines = text[:byte].count(b"\n")
    col = byte - (text.rfind(b"\n", 0, byte) + 1)
    if kind == "quiva":
        return lines // 6, lines % 6, col
    starts = [m.start() for m in re.finditer(rb"(?m)^>", text)]
    rec = int(np.searchsorted(np.array(starts), byte, side="right")) - 1
    return rec, lines - text[:starts[rec]].count(b"\n"), col


def oracle_decode(kind, img, rep):
    if kind == "fasta":
        return O.undexta(img, upper=rep["upper"], width=rep["width"])
    if kind == "arrow":
        return O.undexar(img, width=rep["width"])
    return O.undexqv(img, upper=rep["upper"])


def check_against_oracle(kind, text, img, rep, want_text=None):
    """the report says what decoding with its options and comparing byte by byte says"""
    back = oracle_decode(kind, img, rep)
    d = first_difference(text if want_text is None else want_text, back)
    assert rep["ok"] == (d is None), rep
    if d is None:
        assert rep["where"] == "NONE"
        return
    if d < len(text):
        assert (rep["record"], rep["line"], rep["column"]) == locate(kind, text, d), (rep, d)
        assert rep["src_byte"] == d
    assert rep["where"] in ("HEADER", "BODY", "LENGTH", "COUNT")
    assert (rep["where"] == "HEADER") == (rep["where"] != "COUNT" and rep["line"] == 0)


@pytest.fixture(params=BUDGETS, ids=lambda b: "whole" if b is None else f"budget{b >> 20}M")
def budget(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    else:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(request.param))
    return request.param


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


# ---- dx_verify_ranges against numpy --------------------------------------------------------------------------------------------
class Units:
    """units laid out in two buffers with chosen offset residues; b's units start as copies of a's, the gaps differ"""
    def __init__(self, lens, seed=1, res_a=None, res_b=None):
        rng = np.random.default_rng(seed)
        n = len(lens)
        self.lens = np.asarray(lens, np.int64)
        self.a_off, self.b_off = np.empty(n, np.uint64), np.empty(n, np.uint64)
        pa = pb = 0
        for i, ln in enumerate(self.lens):
            ra = (i % 16) if res_a is None else res_a
            rb = ((i // 16) % 16) if res_b is None else res_b
            pa += (ra - pa) % 16 + 16 * int(rng.integers(0, 3))
            pb += (rb - pb) % 16 + 16 * int(rng.integers(0, 3))
            self.a_off[i], self.b_off[i] = pa, pb
            pa += int(ln); pb += int(ln)
        self.a = rng.integers(0, 256, pa + 64, dtype=np.uint8)
        self.b = rng.integers(0, 256, pb + 64, dtype=np.uint8)
        for i, ln in enumerate(self.lens):
            self.b[int(self.b_off[i]):int(self.b_off[i]) + int(ln)] = self.a[int(self.a_off[i]):int(self.a_off[i]) + int(ln)]
        self.a_len = self.lens.astype(np.uint32)
        self.b_len = self.lens.astype(np.uint32)

    def flip(self, unit, pos):
        self.b[int(self.b_off[unit]) + pos] ^= 0x20

    def expected(self):
        first, pos, differ = None, 0, 0
        for i in range(len(self.lens)):
            x = self.a[int(self.a_off[i]):int(self.a_off[i]) + int(self.a_len[i])].tobytes()
            y = self.b[int(self.b_off[i]):int(self.b_off[i]) + int(self.b_len[i])].tobytes()
            d = first_difference(x, y)
            if d is not None:
                differ += 1
                if first is None:
                    first, pos = i, d
        return first, pos, differ

    def run(self, ctx, count=True):
        bufs = [ctx.to_device(v) for v in (self.a, self.a_off, self.a_len, self.b, self.b_off, self.b_len)]
        try:
            return ctx.verify_ranges(*bufs, len(self.lens), count=count)
        finally:
            for d in bufs:
                d.free()


@pytest.mark.gpu
def test_ranges_random_units_every_residue(ctx):
    rng = np.random.default_rng(7)
    u = Units(rng.integers(0, 5001, 600), seed=3)
    assert u.run(ctx) == (None, 0, 0)
    for unit in (599, 411, 400, 77):
        if u.lens[unit]:
            u.flip(unit, int(rng.integers(0, u.lens[unit])))
    want = u.expected()
    assert want[0] == 77 and want[2] == 4
    assert u.run(ctx) == want
    got = u.run(ctx, count=False)
    assert got[:2] == want[:2] and got[2] is None


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1500, 5000, 40, 9])
def test_ranges_one_flipped_byte_at_the_boundaries(ctx, length):
    places = sorted({p for p in (0, 15, 16, 255, 256, 511, 512, 1023, 1024, 4095, 4096, length - 17, length - 16, length - 1) if 0 <= p < length})
    for k, p in enumerate(places):
        u = Units([length] * 8, seed=100 + k, res_a=(3 * k) % 16, res_b=(5 * k + 1) % 16)
        u.flip(5, p)
        assert u.run(ctx) == (5, p, 1), (length, p)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [700, 6000])
def test_ranges_one_side_is_the_others_beginning(ctx, length):
    u = Units([length] * 6, seed=5)
    u.a_len[2] = length - 37
    assert u.run(ctx) == (2, length - 37, 1)
    u = Units([length] * 6, seed=6)
    u.b_len[4] = length - 1
    u.b_len[5] = 0
    assert u.run(ctx) == (4, length - 1, 2)
    u = Units([0, 0, 3], seed=8)
    assert u.run(ctx) == (None, 0, 0)


@pytest.mark.gpu
def test_ranges_many_short_units(ctx):
    rng = np.random.default_rng(11)
    u = Units(rng.integers(0, 301, 200_000), seed=12, res_a=None, res_b=None)
    assert u.run(ctx) == (None, 0, 0)
    picks = [199_999, 150_001, 90_000, 90_001, 123_456]
    picks = [p for p in picks if u.lens[p] > 0]
    for p in picks:
        u.flip(p, int(u.lens[p]) - 1)
    first = min(picks)
    assert u.run(ctx) == (first, int(u.lens[first]) - 1, len(picks))


@pytest.mark.gpu
def test_ranges_one_long_unit_differs_in_its_last_byte(ctx):
    n = 1_300_003
    u = Units([n], seed=13, res_a=7, res_b=2)
    assert u.run(ctx) == (None, 0, 0)
    u.flip(0, n - 1)
    assert u.run(ctx) == (0, n - 1, 1)


# ---- goldens -------------------------------------------------------------------------------------------------------------------
GOOD = [("ta_small", "fasta", True, 80), ("ta_lower_w60", "fasta", False, 60), ("ar_small", "arrow", False, None),
        ("qv_tiny", "quiva", None, 0), ("qv_mid", "quiva", None, 0), ("qv_full", "quiva", None, 0), ("qv_nodel", "quiva", None, 0),
        ("qv_type2", "quiva", None, 0), ("qv_runs", "quiva", None, 0)]
EXT = {"fasta": (".fasta", ".dexta"), "arrow": (".arrow", ".dexar"), "quiva": (".quiva", ".dexqv")}


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,upper,width", GOOD, ids=[g[0] for g in GOOD])
def test_goldens_that_come_back_verify(ctx, budget, name, kind, upper, width):
    text, img = O.golden(name + EXT[kind][0]), O.golden(name + EXT[kind][1])
    rep = ctx.verify(kind, text, img)
    assert oracle_decode(kind, img, rep) == text           # (what the report promises, by the oracle)
    assert rep["ok"] and rep["where"] == "NONE", rep
    if upper is not None:
        assert rep["upper"] == upper
    if width is not None:
        assert rep["width"] == width
    assert rep["records_src"] == rep["records_img"] > 0


@pytest.mark.gpu
def test_golden_ta_edge_does_not_come_back(ctx, budget):
    text, img = O.golden("ta_edge.fasta"), O.golden("ta_edge.dexta")
    assert text.split(b"\n")[1][4:5] == b"N"                # ('N' becomes 'A': SURVEY 8(c))
    rep = ctx.verify("fasta", text, img)
    assert not rep["ok"]
    assert (rep["record"], rep["where"], rep["line"], rep["column"]) == (0, "BODY", 1, 4), rep
    check_against_oracle("fasta", text, img, rep)


@pytest.mark.gpu
def test_golden_ar_edge_does_not_come_back(ctx, budget):
    text, img = O.golden("ar_edge.arrow"), O.golden("ar_edge.dexar")
    rep = ctx.verify("arrow", text, img)
    assert not rep["ok"]
    assert (rep["record"], rep["where"], rep["line"]) == (0, "HEADER", 0), rep
    assert rep["column"] == text.index(b"6.81") + 3       # (SN=6.81 comes back as 6.80)
    check_against_oracle("arrow", text, img, rep)


@pytest.mark.gpu
def test_golden_lossy(ctx, budget):
    text, img, kept = O.golden("qv_full.quiva"), O.golden("qv_lossy.dexqv"), O.golden("qv_lossy.rt.quiva")
    d = first_difference(text, kept)
    assert d == 16727
    rep = ctx.verify("quiva", text, img, lossy=True)
    assert rep["ok"], rep
    assert O.undexqv(img, upper=rep["upper"]) == kept
    rep = ctx.verify("quiva", text, img, lossy=False)
    assert not rep["ok"] and rep["where"] == "BODY"
    assert rep["src_byte"] == d
    assert (rep["record"], rep["line"], rep["column"]) == locate("quiva", text, d)


# ---- planted differences -------------------------------------------------------------------------------------------------------
def corpus(kind):
    if kind == "quiva":
        c = synth.make_quiva(260, seed=4242, mean=9000)
        return c.text, c, (lambda cx, t: cx.dexqv(t))
    c = synth.make_seqfile(kind, 300, seed=4243, mean=9000, width=70)
    return c.text, c, (lambda cx, t: cx.dexta(t)) if kind == "fasta" else (lambda cx, t: cx.dexar(t))


def other(ch: int, kind: str, line: int) -> int:
    if kind == "fasta":
        return ord("A") if ch != ord("A") else ord("C")
    if kind == "arrow":
        return ord("1") if ch != ord("1") else ord("2")
    if line == 2:                                           # the deletion tags
        return ord("A") if ch != ord("A") else ord("C")
    return ord("3") if ch != ord("3") else ord("4")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fasta", "arrow", "quiva"])
def test_planted_differences_are_found_where_they_are(ctx, budget, kind):
    text, c, pack = corpus(kind)
    img = pack(ctx, text)
    rep = ctx.verify(kind, text, img)
    assert rep["ok"], rep
    check_against_oracle(kind, text, img, rep)
    n = len(c.len)
    rng = np.random.default_rng(99)
    for rec in [0, n - 1] + [int(r) for r in rng.integers(1, n - 1, 4)]:
        L = int(c.len[rec])
        body = int(c.off[rec])
        # a body symbol
        if kind == "quiva":
            line, col = 1 + int(rng.integers(0, 5)), int(rng.integers(0, L))
            at = body + (line - 1) * (L + 1) + col
        else:
            sym = int(rng.integers(0, L))
            line, col = 1 + sym // 70, sym % 70
            at = body + sym + sym // 70
        t = bytearray(text)
        t[at] = other(t[at], kind, line)
        rep = ctx.verify(kind, bytes(t), img)
        assert (rep["ok"], rep["where"], rep["record"], rep["line"], rep["column"], rep["src_byte"]) == (False, "BODY", rec, line, col, at), rep
        # a header digit (the last one of the line)
        at = body - 2
        assert chr(text[at]).isdigit()
        t = bytearray(text)
        t[at] = ord("1") + (t[at] - ord("0")) % 9
        hstart = text.rfind(b"\n", 0, at) + 1
        rep = ctx.verify(kind, bytes(t), img)
        assert (rep["ok"], rep["where"], rep["record"], rep["line"], rep["column"]) == (False, "HEADER", rec, 0, at - hstart), rep
    # both at once in different records: the earlier record wins, whichever kind it is
    t = bytearray(text)
    a1, a2 = int(c.off[40]) - 2, int(c.off[20]) + 5
    t[a1] = ord("1") + (t[a1] - ord("0")) % 9
    t[a2] = other(t[a2], kind, 1)
    rep = ctx.verify(kind, bytes(t), img)
    assert (rep["where"], rep["record"], rep["line"], rep["column"]) == ("BODY", 20, 1, 5), rep


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fasta", "arrow", "quiva"])
def test_damaged_images_are_reported_not_decoded(ctx, budget, kind):
    text, c, pack = corpus(kind)
    img = pack(ctx, text)
    n = len(c.len)
    rep = ctx.verify(kind, text, img[: len(img) * 2 // 3])           # cut in the middle of things
    assert not rep["ok"] and rep["where"] in ("IMAGE", "COUNT"), rep
    # the image of the text without its last record: one record short, nothing else wrong
    hstart = text.rfind(b"\n", 0, int(c.off[n - 1]) - 1) + 1
    short = pack(ctx, text[:hstart])
    rep = ctx.verify(kind, text, short)
    assert (rep["ok"], rep["where"], rep["record"], rep["records_src"], rep["records_img"]) == (False, "COUNT", n - 1, n, n - 1), rep
    assert rep["src_byte"] == hstart
    rep = ctx.verify(kind, text, b"")
    assert not rep["ok"] and rep["where"] == "IMAGE"


# ---- the tools -----------------------------------------------------------------------------------------------------------------
def tool(name, args, cwd, **env):
    e = dict(os.environ, DEXGPU_VERIFY="1")
    e.pop("DEXGPU_TEXT_BUDGET", None)
    e.update(env)
    return subprocess.run([os.path.join(BIN, name), *args], cwd=str(cwd), capture_output=True, env=e)


ROUTES = [{}, {"DEXGPU_DEVICES": "0,0,0"}, {"DEXGPU_TEST": test_env(fd_min=1)}]


@pytest.mark.gpu
@pytest.mark.parametrize("env", ROUTES, ids=["plain", "three_contexts", "fd"])
def test_tools_keep_a_source_that_does_not_come_back(tmp_path, env):
    for name, cmd, ext in (("ta_edge", "dexta", EXT["fasta"]), ("ar_edge", "dexar", EXT["arrow"])):
        (tmp_path / (name + ext[0])).write_bytes(O.golden(name + ext[0]))
        (tmp_path / ("zz" + ext[0])).write_bytes(O.golden(name.replace("edge", "small") + ext[0]))
        r = tool(cmd, ["-v", name, "zz"], tmp_path, **env)
        assert r.returncode == 3, r.stderr
        assert (tmp_path / (name + ext[0])).read_bytes() == O.golden(name + ext[0])
        assert (tmp_path / (name + ext[1])).read_bytes() == O.golden(name + ext[1])
        assert b"record 0" in r.stderr and name.encode() in r.stderr
        assert b"Verified" not in r.stderr
        assert not (tmp_path / ("zz" + ext[1])).exists()          # (the files behind it are not touched)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ROUTES, ids=["plain", "three_contexts", "fd"])
def test_tools_verify_and_remove_a_source_that_comes_back(tmp_path, env):
    for name, cmd, ext, flags, line in (("ta_small", "dexta", EXT["fasta"], [], b"Verified (undexta -U -w80)"),
                                        ("ta_lower_w60", "dexta", EXT["fasta"], [], b"Verified (undexta -w60)"),
                                        ("ar_small", "dexar", EXT["arrow"], [], b"Verified (undexar -w80)"),
                                        ("qv_mid", "dexqv", EXT["quiva"], [], b"Verified (undexqv -U)"),
                                        ("qv_full", "dexqv", EXT["quiva"], ["-l"], b"Verified (undexqv -U)")):
        (tmp_path / (name + ext[0])).write_bytes(O.golden(name + ext[0]))
        r = tool(cmd, ["-v", *flags, name], tmp_path, **env)
        assert r.returncode == 0, r.stderr
        assert line in r.stderr, r.stderr
        assert not (tmp_path / (name + ext[0])).exists()
        want = O.golden(("qv_lossy" if flags else name) + ext[1])
        assert (tmp_path / (name + ext[1])).read_bytes() == want
        # without -v: silent; with -k: the source stays, verified or not
        (tmp_path / (name + ext[0])).write_bytes(O.golden(name + ext[0]))
        r = tool(cmd, ["-k", *flags, name], tmp_path, **env)
        assert r.returncode == 0 and r.stderr == b"" and (tmp_path / (name + ext[0])).exists()


@pytest.mark.gpu
def test_tools_unchanged_without_the_variable(tmp_path):
    (tmp_path / "ta_edge.fasta").write_bytes(O.golden("ta_edge.fasta"))
    e = {k: v for k, v in os.environ.items() if k != "DEXGPU_VERIFY"}
    r = subprocess.run([os.path.join(BIN, "dexta"), "-v", "ta_edge"], cwd=str(tmp_path), capture_output=True, env=e)
    assert r.returncode == 0 and b"Verified" not in r.stderr
    assert not (tmp_path / "ta_edge.fasta").exists()
    assert (tmp_path / "ta_edge.dexta").read_bytes() == O.golden("ta_edge.dexta")
