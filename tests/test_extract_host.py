"""dx_file_extract's host side (no GPU): the two new entry points are declared, exported and bound; the oracle of the GPU tests --
`_subset.cut` of the reference's text -- is valid on its own over the whole option grid; and the numpy statement of
dx_reads_unpack_lines (tests/_lines.py) gives the reference's lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _lines as LN
import _oracle as O
import _subset as S
from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dx_reads_unpack_lines", "dx_file_extract"]
WIDTHS = [1, 7, 60, 80, 10 ** 6]
TWO_BIT = [("fasta", "ta_small.dexta"), ("fasta", "ta_edge.dexta"), ("fasta", "ta_lower_w60.dexta"), ("arrow", "ar_small.dexar"),
           ("fasta", "ta_small.legacy.dexta"), ("fasta", "ta_small.swapped.dexta"), ("fasta", "ta_small.legacy_swapped.dexta")]
QUIVA = ["qv_tiny", "qv_runs", "qv_type2", "qv_nodel", "qv_lossy"]


def test_new_symbols_are_exported_declared_and_bound():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert name in L.SIGNATURES
    for m in ("reads_unpack_lines", "extract"):
        assert callable(getattr(api.Context, m))


def test_no_context_is_an_argument_error():
    lib = L.load()
    out, n, toff, bad = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    img = O.golden("ta_small.dexta")
    assert lib.dx_file_extract(None, L.DX_KIND_FASTA, img, len(img), None, None, None, 2 ** 64 - 1, 0, 80,
                               C.byref(out), C.byref(n), C.byref(toff)) == -1
    assert lib.dx_reads_unpack_lines(None, L.DX_LETTERS_LOWER, None, 0, None, None, None, 0, 80, None, None, C.byref(bad)) == -1


def decode(kind, img, upper, width):
    return O.undexta(img, upper, width) if kind == "fasta" else O.undexar(img, width) if kind == "arrow" else O.undexqv(img, upper)


@pytest.mark.parametrize("kind,name", TWO_BIT + [("quiva", q + ".dexqv") for q in QUIVA])
def test_the_oracle_stays_valid_on_its_own(kind, name):
    """every record whole is the text itself, whatever the options: `cut` parses and prints what the reference printed"""
    img = O.golden(name)
    for upper in (False, True):
        for width in WIDTHS if kind != "quiva" else [80]:
            text = decode(kind, img, upper, width)
            n = len(S.lengths(kind, text))
            assert n > 0
            assert S.cut(kind, text, [(i, None, None) for i in range(n)], width) == text
            assert LN.header_offsets(kind, text, n)[-1] == len(text)


@pytest.mark.parametrize("kind,name,letters", [("fasta", "ta_small.dexta", L.DX_LETTERS_LOWER), ("fasta", "ta_edge.dexta", L.DX_LETTERS_UPPER),
                                               ("fasta", "ta_lower_w60.dexta", L.DX_LETTERS_UPPER), ("arrow", "ar_small.dexar", L.DX_LETTERS_ARROW)])
def test_the_numpy_reference_gives_the_references_lines(kind, name, letters):
    img = O.golden(name)
    boff, rlen = LN.two_bit_reads(img, kind == "arrow")
    for width in WIDTHS + [16, 17]:
        text = decode(kind, img, letters == L.DX_LETTERS_UPPER, width)
        got = LN.unpack_lines_ref(img, boff, np.zeros(len(rlen), np.uint32), rlen, width, letters)
        assert got == LN.bodies(text)
        assert [len(g) for g in got] == [LN.text_len(int(n), width) for n in rlen]


def test_the_numpy_reference_at_every_phase():
    """an interval is the whole read's letters cut: the lines of symbols [beg, beg + len) at any phase, against plain slices"""
    rng = np.random.Generator(np.random.PCG64(5))
    sym = rng.integers(0, 4, 203, dtype=np.uint8)
    q = np.concatenate([sym, np.zeros(1, np.uint8)]).reshape(-1, 4)
    buf = b"\xa5" + ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8).tobytes()
    for beg in (0, 1, 2, 3, 5, 101):
        for n in (0, 1, 4, 17, 100):
            for width in (1, 3, 16, 60):
                letters = np.frombuffer(b"acgt", np.uint8)[sym[beg: beg + n]].tobytes()
                want = b"".join(letters[k: k + width] + b"\n" for k in range(0, n, width))
                assert LN.unpack_lines_ref(buf, [1], [beg], [n], width, L.DX_LETTERS_LOWER) == [want]


# ---- the 2-bit driver with the host standing in for the device (tests/extract_standin.c) --------------------------------------------
@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    """the driver's C files and the stand-in, compiled with the host's sanitizers into a program of its own"""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build tests/extract_standin.c with")
    src = os.path.join(ROOT, "dextractor_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("standin") / "extract_standin")
    files = [os.path.join(ROOT, "tests", "extract_standin.c")] + [os.path.join(src, f) for f in
             ("dx_file_extract.c", "dx_select.c", "dx_file_subset.c", "dx_file_pack2.c", "dx_files.c", "dx_host.c", "dx_crew.c")]
    subprocess.check_call([cc, "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + src, "-o", exe, *files,
                           "-Wl,--unresolved-symbols=ignore-all", "-lpthread", "-lm"])
    return exe


@pytest.mark.parametrize("key", ["reads_packed", "reads_whole"])
def test_two_bit_driver_in_slices_on_the_host_stand_in(standin, tmp_path, key):
    """any order, repeats and empty units; in one slice and in slices of whole units under a budget of text: the same bytes and offsets,
    and `cut` of the oracle's text; packed, only the selected spans go up"""
    import re
    import struct
    import subprocess
    from dextractor_amd import synth
    text = synth.make_seqfile("fasta", 60, seed=23, mean=3000).text
    img = O.dexta(text)
    lens = S.lengths("fasta", text)
    (tmp_path / "in.dexta").write_bytes(img)
    few = [(7, 10, 1000), (3, 0, lens[3]), (7, 10, 1000), (40, 5, 5)]
    for width, units in ((80, S.whole_and_intervals(lens, 3)[::-1]), (7, LN.shuffled_with_repeats(lens, 4)),
                         (10 ** 6, LN.with_a_final_empty_unit(S.one_empty_each(lens, 4), lens)), (80, few)):
        (tmp_path / "units.bin").write_bytes(b"".join(struct.pack("<QII", *u) for u in units))
        r = subprocess.run([standin, str(tmp_path / "in.dexta"), str(tmp_path / "units.bin"), str(tmp_path / "out.txt"), "4096", str(width)],
                           capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, DEXGPU_TEST=key, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, r.stderr[-2000:]
        want = S.cut("fasta", O.undexta(img, True, width), units, width)
        assert (tmp_path / "out.txt").read_bytes() == want
        toff = np.frombuffer((tmp_path / "out.txt.toff").read_bytes(), np.uint64)
        assert toff.tolist() == LN.header_offsets("fasta", want, len(units))
        calls = [int(c) for c in re.findall(r"(\d+) unpack calls", r.stdout)]
        sent = [int(c) for c in re.findall(r"(\d+) packed bytes sent", r.stdout)]
        assert calls[0] == 1 and (calls[1] >= 3 or len(want) < 3 * 65536), r.stdout       # (a slice of text is 64 KiB at least)
        if key == "reads_whole":
            assert sent[0] == len(img)
        elif units is few:
            assert sent[0] <= 2 * (1000 // 4 + 2) + lens[3] // 4 + 2, r.stdout             # (the repeated unit's span goes up once)
