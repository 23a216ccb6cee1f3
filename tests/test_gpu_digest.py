"""The digest on the GPU: dx_crc32_ranges and dx_crc32_fold against zlib.crc32, dx_file_digest against the CRC of the reference's
bytes (tests/golden) and of the oracle's decoders, and DEXGPU_DIGEST in the tools.  No expected value comes from the library."""
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
SPLIT = 8192                       # DEXGPU_TEST=crc_split: units from here on go over several waves (1 MiB otherwise)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


# ---- dx_crc32_ranges ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_units():
    """One buffer and its units -> (bytes, off, len, the units' CRCs by zlib): every length 0..300 at every start alignment 0..15;
    the lengths around 1 Ki, 4 Ki (a lane's unit / a wave's) and 64 Ki, and two of megabytes (split over workgroups); zeros and 0xFF;
    two units that overlap and one that is there twice; the last unit ends on the buffer's last byte, at an odd offset."""
    rng = np.random.default_rng(31)
    off, ln, at = [], [], 0
    for n in range(301):
        for a in range(16):
            at += (a - at) % 16
            off.append(at); ln.append(n)
            at += n
    for n in (1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, (1 << 20) + 3, 5 * (1 << 20) - 1):
        at += 1 + (at % 2)                                        # (odd and even starts)
        off.append(at); ln.append(n)
        at += n
    zeros, ones = at, at + 1000
    off += [zeros, ones]; ln += [1000, 1000]
    at += 2000
    off += [off[4500], off[4500] + 100, off[4000], off[-8]]      # overlapping: two units over one stretch; repeated: units 4000 and a long one
    ln += [250, 250, ln[4000], ln[-8]]
    at += at % 2                                                  # the last unit: from an odd offset to the buffer's last byte
    off.append(at + 1); ln.append(777)
    total = at + 1 + 777
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    buf[zeros:zeros + 1000] = 0
    buf[ones:ones + 1000] = 0xFF
    data = buf.tobytes()
    assert off[-1] % 2 == 1 and off[-1] + ln[-1] == len(data)
    want = np.array([zlib.crc32(data[o:o + n]) for o, n in zip(off, ln)], np.uint32)
    return data, np.array(off, np.uint64), np.array(ln, np.uint64), want


@pytest.mark.parametrize("split", [None, SPLIT], ids=["split1M", "split8K"])
def test_crc32_ranges_against_zlib(ctx, monkeypatch, split):
    if split is not None:
        set_flag(monkeypatch, "crc_split", split)
    data, off, ln, want = range_units()
    d_buf, d_off, d_len = ctx.to_device(np.frombuffer(data, np.uint8)), ctx.to_device(off), ctx.to_device(ln)
    d_crc = ctx.alloc(4 * len(off))
    try:
        ctx.crc32_ranges(d_buf, len(data), d_off, d_len, len(off), d_crc)
        got = d_crc.download(np.uint32, len(off))
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [(int(i), int(off[i]), int(ln[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
        assert want[ln == 0].max() == 0                             # (an empty unit's CRC is 0)
    finally:
        for b in (d_buf, d_off, d_len, d_crc):
            b.free()


def test_crc32_ranges_more_split_units_than_the_list_holds(ctx, monkeypatch):
    """17 000 units at the split threshold (one 4 KiB range, again and again): the list of split units holds 16 384, the rest
    are a wave's each -- the same CRC whichever way"""
    set_flag(monkeypatch, "crc_split", 4096)
    data = np.random.default_rng(5).integers(0, 256, 5000, dtype=np.uint8)
    n = 17000
    d_buf, d_off, d_len = ctx.to_device(data), ctx.to_device(np.full(n, 3, np.uint64)), ctx.to_device(np.full(n, 4096, np.uint64))
    d_crc = ctx.alloc(4 * n)
    try:
        ctx.crc32_ranges(d_buf, len(data), d_off, d_len, n, d_crc)
        got = d_crc.download(np.uint32, n)
        assert (got == zlib.crc32(data.tobytes()[3:4099])).all(), np.flatnonzero(got != got[0])[:8]
    finally:
        for b in (d_buf, d_off, d_len, d_crc):
            b.free()


def test_crc32_ranges_no_units_and_units_out_of_bounds(ctx):
    ctx.crc32_ranges(None, 0, None, None, 0, None)                   # n = 0: DX_OK, nothing is looked at
    data = np.arange(4096, dtype=np.uint8)
    off = np.array([0, 100, 4000, 4000, 4096, 0, 5000], np.uint64)
    ln = np.array([4096, 50, 96, 97, 0, 8000, 1], np.uint64)          # unit 3 ends one byte past the buffer; 5 and 6 are further out
    d_buf, d_off, d_len, d_crc = ctx.to_device(data), ctx.to_device(off), ctx.to_device(ln), ctx.alloc(4 * len(off))
    try:
        with pytest.raises(L.DexGPUError) as e:
            ctx.crc32_ranges(d_buf, len(data), d_off, d_len, len(off), d_crc)
        assert e.value.code == -3 and e.value.bad_unit == 3
        ctx.crc32_ranges(d_buf, len(data), d_off, d_len, 3, d_crc)    # (the valid ones in front of it, on their own)
        raw = data.tobytes()
        assert list(d_crc.download(np.uint32, 3)) == [zlib.crc32(raw), zlib.crc32(raw[100:150]), zlib.crc32(raw[4000:4096])]
    finally:
        for b in (d_buf, d_off, d_len, d_crc):
            b.free()


# ---- dx_crc32_fold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 4097])
def test_crc32_fold_against_zlib(ctx, n):
    rng = np.random.default_rng(100 + n)
    ln = rng.integers(0, 5001, n).astype(np.uint64)
    ln[rng.random(n) < 1 / 3] = 0
    units = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in ln]
    crc = np.array([zlib.crc32(u) for u in units], np.uint32)
    d_crc, d_len = ctx.to_device(crc), ctx.to_device(ln)
    try:
        whole = b"".join(units)
        assert ctx.crc32_fold(d_crc, d_len, n) == (zlib.crc32(whole), len(whole))
    finally:
        d_crc.free(); d_len.free()


def test_crc32_fold_of_more_than_4_gib(ctx):
    """one 1 MiB range 5000 times: the units' CRCs from dx_crc32_ranges, the concatenation's from the host's dx_crc32_combine,
    5000 times over (test_digest_host.py holds that one to zlib)"""
    n, size = 5000, 1 << 20
    data = np.random.default_rng(8).integers(0, 256, size + 7, dtype=np.uint8)
    one = zlib.crc32(data.tobytes()[7:])
    d_buf, d_off, d_len = ctx.to_device(data), ctx.to_device(np.full(n, 7, np.uint64)), ctx.to_device(np.full(n, size, np.uint64))
    d_crc = ctx.alloc(4 * n)
    try:
        ctx.crc32_ranges(d_buf, len(data), d_off, d_len, n, d_crc)
        assert (d_crc.download(np.uint32, n) == one).all()
        want = 0
        for _ in range(n):
            want = api.crc32_combine(want, one, size)
        assert n * size > 1 << 32
        assert ctx.crc32_fold(d_crc, d_len, n) == (want, n * size)
    finally:
        for b in (d_buf, d_off, d_len, d_crc):
            b.free()


# ---- dx_file_digest on the reference's bytes ---------------------------------------------------------------------------------------
EXT = {"fasta": (".fasta", ".dexta"), "arrow": (".arrow", ".dexar"), "quiva": (".quiva", ".dexqv")}


def records_of(kind, text):
    """a text split at its header lines"""
    lines = text.splitlines(keepends=True)
    if kind == "quiva":                                           # (six lines an entry: a quality line may begin with '@')
        return [b"".join(lines[i:i + 6]) for i in range(0, len(lines), 6)]
    starts = [i for i, ln in enumerate(lines) if ln.startswith(b">")] + [len(lines)]
    return [b"".join(lines[a:b]) for a, b in zip(starts, starts[1:])]


def check_digest(ctx, kind, img, text, upper, width):
    d = ctx.digest(kind, img, upper=upper, width=width, per_record=True)
    recs = records_of(kind, text)
    assert (d["crc32"], d["bytes"], d["records"]) == (zlib.crc32(text), len(text), len(recs)), (kind, upper, width)
    assert list(d["rec_crc"]) == [zlib.crc32(r) for r in recs]
    plain = ctx.digest(kind, img, upper=upper, width=width)
    assert plain == {k: d[k] for k in ("crc32", "bytes", "records")}


def golden_cases():
    out = []
    for c in O.cases():
        kind = c["kind"]
        src, img = EXT[kind]
        flags = c.get("undex_flags", ["-U"] if kind == "quiva" else [])      # (the .quiva goldens are the reference's undexqv -U)
        width = next((int(f[2:]) for f in flags if f.startswith("-w")), 80)
        text = (c.get("input", c["name"]) + src) if c["rt_is_input"] else (c["name"] + ".rt" + src)
        out.append((c["name"] + img, kind, text, "-U" in flags, width))
    out += [("ta_small.legacy.dexta", "fasta", "ta_small.legacy.rt.fasta", True, 80),
            ("ta_small.swapped.dexta", "fasta", "ta_small.swapped.rt.fasta", True, 80),
            ("ta_small.legacy_swapped.dexta", "fasta", "ta_small.legacy_swapped.rt.fasta", True, 80),
            ("ar_small.swapped.dexar", "arrow", "ar_small.swapped.rt.arrow", False, 80),
            ("qv_tiny.legacy.dexqv", "quiva", "qv_tiny.legacy.rt.quiva", True, 80),
            ("qv_tiny.legacy.dexqv", "quiva", "qv_tiny.legacy.rt_lower.quiva", False, 80)]
    return out


@pytest.mark.parametrize("img,kind,text,upper,width", golden_cases(), ids=[c[2] for c in golden_cases()])
def test_file_digest_of_the_goldens(ctx, img, kind, text, upper, width):
    check_digest(ctx, kind, O.golden(img), O.golden(text), upper, width)


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(kind, n):
    """n entries of 0 .. 700 symbols and one of 70 000 behind them -> the image, by the oracle's encoder"""
    lens = np.random.default_rng(1000 + n).integers(0, 701, n).astype(np.uint32)
    if kind != "quiva":
        lens[lens == 0] = 1           # (a .fasta / .arrow header with no sequence line behind it is not a record the reference reads)
        lens[0] = 700
    else:
        lens[0] = 0
    lens = np.concatenate([lens, np.array([70000], np.uint32)])
    if kind == "quiva":
        return O.dexqv(synth.make_quiva(len(lens), seed=77 + n, lens=lens).text)
    text = synth.make_seqfile(kind, len(lens), seed=77 + n, lens=lens).text
    return O.dexta(text) if kind == "fasta" else O.dexar(text)


@functools.lru_cache(maxsize=None)
def decoded(kind, n, upper, width):
    img = corpus(kind, n)
    if kind == "fasta":
        return O.undexta(img, upper=upper, width=width)
    if kind == "arrow":
        return O.undexar(img, width=width)
    return O.undexqv(img, upper=upper)


@pytest.mark.parametrize("budget", [None, 1 << 20, 1 << 16], ids=["whole", "budget1M", "budget64K"])
@pytest.mark.parametrize("n", [1, 2, 65, 200])
@pytest.mark.parametrize("kind", ["fasta", "arrow", "quiva"])
def test_file_digest_against_the_oracle(ctx, monkeypatch, kind, n, budget):
    if budget is None:
        monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
    else:
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
    for upper in (False, True):
        for width in (1, 80, 4000):
            check_digest(ctx, kind, corpus(kind, n), decoded(kind, n, upper, width), upper, width)


@pytest.mark.parametrize("n", [1, 200])
def test_file_digest_of_a_quiva_walked_on_the_device(ctx, monkeypatch, n):
    set_flag(monkeypatch, "device_walk_min", 1)
    for budget in (None, 1 << 20):
        if budget is None:
            monkeypatch.delenv("DEXGPU_TEXT_BUDGET", raising=False)
        else:
            monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
        for upper in (False, True):
            check_digest(ctx, "quiva", corpus("quiva", n), decoded("quiva", n, upper, 80), upper, 80)


def test_file_digest_errors_are_the_decoders(ctx):
    img = O.golden("ta_small.dexta")
    for kind, bad in (("fasta", b""), ("fasta", b"\x00\x01garbage"), ("fasta", img[:len(img) - 3]), ("quiva", b"\x00" * 40)):
        with pytest.raises(L.DexGPUError):
            ctx.digest(kind, bad)
    with pytest.raises(L.DexGPUError) as e:
        ctx.digest("fasta", img, width=0)
    assert e.value.code == -1


# ---- damage ------------------------------------------------------------------------------------------------------------------------
def test_a_damaged_payload_byte_shows_in_its_record_alone(ctx):
    img = O.golden("ta_small.dexta")
    good = O.golden("ta_small.fasta")                              # (what undexta -U prints for it)
    hurt = bytearray(img)
    hurt[len(hurt) // 2] ^= 0x40                                   # inside some read's packed bases: one base becomes another
    was, now = records_of("fasta", good), records_of("fasta", O.undexta(bytes(hurt), upper=True, width=80))
    differ = [i for i, (a, b) in enumerate(zip(was, now)) if a != b]
    assert len(was) == len(now) and len(differ) == 1               # (the byte is a payload byte: one record's letters change)
    a = ctx.digest("fasta", img, upper=True, per_record=True)
    b = ctx.digest("fasta", bytes(hurt), upper=True, per_record=True)
    assert a["crc32"] == zlib.crc32(good) and b["crc32"] != a["crc32"] and b["bytes"] == a["bytes"]
    assert list(np.flatnonzero(a["rec_crc"] != b["rec_crc"])) == differ
    assert b["crc32"] == zlib.crc32(b"".join(now))


# ---- the tools ---------------------------------------------------------------------------------------------------------------------
def tool(name, args, cwd, digest, stdin=None, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("DEXGPU_TEXT_BUDGET", "DEXGPU_VERIFY", "DEXGPU_DIGEST")}
    if digest is not None:
        e["DEXGPU_DIGEST"] = digest
    e.update(env)
    return subprocess.run([os.path.join(BIN, name), *args], cwd=str(cwd), capture_output=True, env=e, input=stdin)


def line_of(text, path):
    return b"%08x %d %s\n" % (zlib.crc32(text), len(text), path.encode())


def test_tools_print_the_same_digest_both_ways(tmp_path):
    text, img = O.golden("qv_mid.quiva"), O.golden("qv_mid.dexqv")
    (tmp_path / "qv_mid.quiva").write_bytes(text)
    r = tool("dexqv", ["qv_mid"], tmp_path, "1")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of(text, "./qv_mid.quiva")
    assert (tmp_path / "qv_mid.dexqv").read_bytes() == img and not (tmp_path / "qv_mid.quiva").exists()
    r = tool("undexqv", ["-U", "qv_mid"], tmp_path, "1")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of(text, "./qv_mid.quiva")
    assert (tmp_path / "qv_mid.quiva").read_bytes() == text and not (tmp_path / "qv_mid.dexqv").exists()
    # ... and without the variable: the same files, nothing on stdout
    r = tool("dexqv", ["-k", "qv_mid"], tmp_path, None)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    assert (tmp_path / "qv_mid.dexqv").read_bytes() == img


def test_tools_digest_only_writes_nothing(tmp_path):
    (tmp_path / "ta_small.dexta").write_bytes(O.golden("ta_small.dexta"))
    r = tool("undexta", ["-U", "ta_small"], tmp_path, "only")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of(O.golden("ta_small.fasta"), "./ta_small.fasta")
    assert not (tmp_path / "ta_small.fasta").exists()
    assert (tmp_path / "ta_small.dexta").read_bytes() == O.golden("ta_small.dexta")
    r = tool("undexta", ["-w60", "ta_lower_w60"], tmp_path, "only")       # (a file that is not there: the tool's own words)
    assert r.returncode == 1 and r.stdout == b"" and b"Cannot open" in r.stderr


def test_dex_tools_refuse_digest_only(tmp_path):
    (tmp_path / "ta_small.fasta").write_bytes(O.golden("ta_small.fasta"))
    r = tool("dexta", ["ta_small"], tmp_path, "only")
    assert r.returncode == 1 and r.stdout == b"" and b"DEXGPU_DIGEST" in r.stderr
    assert (tmp_path / "ta_small.fasta").read_bytes() == O.golden("ta_small.fasta")
    assert not (tmp_path / "ta_small.dexta").exists()


def test_tools_print_a_line_a_file_in_argument_order(tmp_path):
    for name in ("ta_small", "ta_lower_w60"):
        (tmp_path / (name + ".fasta")).write_bytes(O.golden(name + ".fasta"))
    r = tool("dexta", ["-k", "ta_small", "ta_lower_w60"], tmp_path, "1", DEXGPU_DEVICES="0,0")
    assert (r.returncode, r.stderr) == (0, b""), r.stderr
    assert r.stdout == line_of(O.golden("ta_small.fasta"), "./ta_small.fasta") + line_of(O.golden("ta_lower_w60.fasta"), "./ta_lower_w60.fasta")
    for name in ("ta_small", "ta_lower_w60"):
        assert (tmp_path / (name + ".dexta")).read_bytes() == O.golden(name + ".dexta")
    r = tool("undexta", ["-k", "ta_lower_w60", "ta_small"], tmp_path, "only")     # (one -w for both: 80, not ta_lower_w60's 60)
    assert r.returncode == 0
    want = [line_of(O.undexta(O.golden(n + ".dexta"), upper=False, width=80), "./" + n + ".fasta") for n in ("ta_lower_w60", "ta_small")]
    assert r.stdout == b"".join(want)
    r = tool("undexta", ["-i", "-U"], tmp_path, "1", stdin=O.golden("ta_small.dexta"))   # -i: stdout carries the text, and nothing else
    assert (r.returncode, r.stdout) == (0, O.golden("ta_small.fasta"))
