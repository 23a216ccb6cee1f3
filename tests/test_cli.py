"""The six drop-in tools: same command-line surface, files, messages and exit codes as the
reference's (compared live against oracle/_ref where present)."""
import os
import re
import shutil
import subprocess

import pytest

from _flags import set_flag, test_env

import _oracle as O
from dextractor_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dextractor_amd", "bin")
TOOLS = ["dexta", "undexta", "dexar", "undexar", "dexqv", "undexqv"]

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (compiled reference) not present")


def run(tool, args, cwd, ref=False, stdin=None, env=None):
    exe = os.path.join(O.REF_BIN if ref else BIN, tool)
    return subprocess.run([exe, *args], cwd=str(cwd), capture_output=True, input=stdin, env=env)


def test_tools_are_built():
    for t in TOOLS:
        assert os.access(os.path.join(BIN, t), os.X_OK), f"{t} missing: run `make cli`"


@needs_ref
@pytest.mark.parametrize("tool", TOOLS)
def test_usage_and_illegal_option_match_reference(tool, tmp_path):
    """Argument errors are reported before any GPU is touched, in the reference's words."""
    for args in ([], ["-Z"], ["-vZ", "x"]):
        a, b = run(tool, args, tmp_path), run(tool, args, tmp_path, ref=True)
        assert (a.returncode, a.stderr) == (b.returncode, b.stderr), (tool, args)
    if tool in ("undexta", "undexar"):
        for args in (["-wabc", "x"], ["-w-3", "x"], ["-w", "x"]):
            a, b = run(tool, args, tmp_path), run(tool, args, tmp_path, ref=True)
            assert (a.returncode, a.stderr) == (b.returncode, b.stderr), (tool, args)


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.gpu
@needs_ref
def test_cli_round_trips_equal_reference(tmp_path):
    fa = synth.make_seqfile("fasta", 30, seed=4, mean=1500).text
    ar = synth.make_seqfile("arrow", 30, seed=4, mean=1500).text
    qv = synth.make_quiva(40, seed=4, mean=7000).text
    mine, ref = tmp_path / "mine", tmp_path / "ref"
    for d, isref in ((mine, False), (ref, True)):
        d.mkdir()
        _write(d / "a.fasta", fa); _write(d / "b.arrow", ar); _write(d / "c.quiva", qv)
        _write(d / "c2.quiva", qv)
        assert run("dexta", ["-v", "a"], d, isref).returncode == 0
        assert not (d / "a.fasta").exists()                         # source removed without -k
        assert run("dexar", ["-k", "b.arrow"], d, isref).returncode == 0
        assert (d / "b.arrow").exists()
        assert run("dexqv", ["c"], d, isref).returncode == 0
        assert run("dexqv", ["-kl", "c2"], d, isref).returncode == 0
        shutil.copy(d / "a.dexta", d / "a2.dexta")
        assert run("undexta", ["-kU", "-w70", "a2"], d, isref).returncode == 0
        assert run("undexta", ["a"], d, isref).returncode == 0
        shutil.copy(d / "b.dexar", d / "b2.dexar")
        os.remove(d / "b.arrow")
        assert run("undexar", ["-k", "b"], d, isref).returncode == 0
        shutil.copy(d / "c.dexqv", d / "c3.dexqv")
        assert run("undexqv", ["-U", "c"], d, isref).returncode == 0
        assert run("undexqv", ["-k", "c3"], d, isref).returncode == 0
    names = sorted(os.listdir(ref))
    assert names == sorted(os.listdir(mine))
    for nme in names:
        assert _read(mine / nme) == _read(ref / nme), nme
    assert _read(mine / "c.quiva") == qv                            # dexqv | undexqv -U round trip


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("tool,kind", [("dexta", "fasta"), ("dexar", "arrow")])
def test_cli_pipe_and_large_file_go_through_in_pieces(tmp_path, tool, kind):
    """dexta -i / dexar -i and a "large" file (DEXGPU_TEST=fd_min=1) are packed a chunk of whole records at a time
    (stream_chunk=20000: many pieces): the reference's bytes, the source file removed as the reference removes it."""
    f = synth.make_seqfile(kind, 400, seed=21, mean=900, width=60)
    env = dict(os.environ, DEXGPU_TEST=test_env(stream_chunk=20000, fd_min=1))
    a, b = run(tool, ["-i"], tmp_path, stdin=f.text, env=env), run(tool, ["-i"], tmp_path, ref=True, stdin=f.text)
    assert a.returncode == 0 and a.stdout == b.stdout
    for sub in ("mine", "ref"):
        (tmp_path / sub).mkdir()
        _write(tmp_path / sub / ("x." + kind), f.text)
    un = "un" + tool
    a2 = run(un, ["-i"] + (["-U"] if tool == "dexta" else []), tmp_path, stdin=a.stdout, env=env)
    b2 = run(un, ["-i"] + (["-U"] if tool == "dexta" else []), tmp_path, ref=True, stdin=b.stdout)
    assert a2.returncode == 0 and a2.stdout == b2.stdout
    a3, b3 = run(un, ["-i"], tmp_path, stdin=b"xy" + a.stdout[2:], env=env), run(un, ["-i"], tmp_path, ref=True, stdin=b"xy" + b.stdout[2:])
    assert (a3.returncode, a3.stderr) == (b3.returncode, b3.stderr)                  # no endian key: the reference's words
    a = run(tool, ["x"], tmp_path / "mine", env=env)
    b = run(tool, ["x"], tmp_path / "ref", ref=True)
    assert a.returncode == b.returncode == 0
    assert sorted(os.listdir(tmp_path / "mine")) == sorted(os.listdir(tmp_path / "ref"))
    assert _read(tmp_path / "mine" / ("x.dex" + ("ta" if kind == "fasta" else "ar"))) == _read(tmp_path / "ref" / ("x.dex" + ("ta" if kind == "fasta" else "ar")))


@pytest.mark.gpu
@needs_ref
def test_cli_pipe_mode_and_verbose(tmp_path):
    fa = synth.make_seqfile("fasta", 5, seed=6, mean=400).text
    a, b = run("dexta", ["-i"], tmp_path, stdin=fa), run("dexta", ["-i"], tmp_path, ref=True, stdin=fa)
    assert a.returncode == 0 and a.stdout == b.stdout
    a2, b2 = run("undexta", ["-i", "-U"], tmp_path, stdin=a.stdout), run("undexta", ["-i", "-U"], tmp_path, ref=True, stdin=b.stdout)
    assert a2.stdout == b2.stdout == fa
    _write(tmp_path / "v.fasta", fa)
    a3 = run("dexta", ["-vk", "v.fasta"], tmp_path)
    assert a3.stderr == b"Processing 'v' ...\nDone\n"


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("tool,ext,data", [
    ("dexqv", ".quiva", b"@m/1/0_3 RQ=0.8\nabc\nabc\nab\nabc\nabc\n"),
    ("dexqv", ".quiva", b"m/1/0_3 RQ=0.8\nabc\nabc\nabc\nabc\nabc\n"),
    ("dexqv", ".quiva", b"@m/1/0_3\nabc\nabc\nabc\nabc\nabc\n"),
    ("dexqv", ".quiva", b"@m/1/0_3 RQ=0.8\nabc\nabc\n"),
    ("dexta", ".fasta", b"m/1/0_3 RQ=0.8\nACG\n"),
    ("dexta", ".fasta", b">m 1 0_3 RQ=0.8\nACG\n"),
    ("dexar", ".arrow", b">m/1/0_3 SN=1.0,2.0\n123\n"),
    ("dexqv", ".quiva", b"@m/1/0_3 RQ=0.8\nabc\nabc\nabc\nabc\nabc"),              # no newline behind an entry's LAST line: "not the same length"
    ("dexqv", ".quiva", b"@m/1/0_3 RQ=0.8\nabc"),                                  # ... behind its first line: "Last line does not end ..."
    ("dexar", ".arrow", b">m/1/0_3 SN=1.00,2.00,3.00,4.00\n123\n>m/2/0_3 SN=1.00,2.00,3.00,4.00\n12"),   # dexar's "Fasta line is too long"
    ("dexta", ".fasta", b">m/1/0_3 RQ=0.8\nACG\n>m/2/0_3 RQ=0.8\n"),               # a later header with the end of the file behind it
    ("dexar", ".arrow", b">m/1/0_3 SN=1.00,2.00,3.00,4.00\n123\n>m/2/0_3 SN=1.00,2.00,3.00,4.00\n"),
    ("undexta", ".dexta", b"\x01\x02\x03\x04\x05\x06"),
    ("undexar", ".dexar", b"\xcc\x33\x03\x04\x05\x06"),
])
def test_cli_error_messages_match_reference(tmp_path, tool, ext, data):
    mine, ref = tmp_path / "mine", tmp_path / "ref"
    for d in (mine, ref):
        d.mkdir()
        _write(d / ("x" + ext), data)
    a, b = run(tool, ["-k", "x"], mine), run(tool, ["-k", "x"], ref, ref=True)
    assert (a.returncode, a.stderr) == (b.returncode, b.stderr)


@pytest.mark.gpu
def test_cli_missing_file(tmp_path):
    a = run("dexta", ["nothere"], tmp_path)
    assert a.returncode == 1 and a.stderr == b"dexta: Cannot open ./nothere.fasta for 'r'\n"


@pytest.mark.gpu
def test_cli_dexqv_on_several_contexts(tmp_path):
    """DEXGPU_DEVICES shards one file over the listed GPUs (here: the same GPU three times)."""
    qv = synth.make_quiva(25, seed=8, mean=5000).text
    _write(tmp_path / "m.quiva", qv)
    env = dict(os.environ, DEXGPU_DEVICES="0,0,0")
    r = subprocess.run([os.path.join(BIN, "dexqv"), "-k", "m"], cwd=str(tmp_path), capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert _read(tmp_path / "m.dexqv") == O.dexqv(qv)


@pytest.mark.gpu
@pytest.mark.parametrize("tool,ext,kind", [("dexta", "fasta", "fasta"), ("dexar", "arrow", "arrow")])
def test_cli_pack2_on_several_contexts(tmp_path, tool, ext, kind):
    """DEXGPU_DEVICES also shards a .fasta/.arrow file's reads (dx_file_pack2_sharded)."""
    txt = synth.make_seqfile(kind, 40, seed=9, mean=3000).text
    _write(tmp_path / f"m.{ext}", txt)
    env = dict(os.environ, DEXGPU_DEVICES="0,0,0")
    r = subprocess.run([os.path.join(BIN, tool), "-k", "m"], cwd=str(tmp_path), capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    want = O.dexta(txt) if kind == "fasta" else O.dexar(txt)
    assert _read(tmp_path / f"m.{'dexta' if kind == 'fasta' else 'dexar'}") == want


@pytest.mark.gpu
def test_cli_pipe_mode_appends_to_an_existing_file(tmp_path):
    """`tool -i <in >>all` (stdout a regular file opened O_APPEND, or one that already holds bytes) must append: the
    direct-to-file output paths only lay out files that are empty, at offset 0 and not in append mode."""
    fa = synth.make_seqfile("fasta", 6, seed=11, mean=500).text
    dx = O.dexta(fa)
    _write(tmp_path / "a.dexta", dx)
    back = O.undexta(dx, True, 80)
    out = tmp_path / "all"
    _write(out, b"KEEP ME\n")
    for _ in range(2):
        r = subprocess.run(f"{os.path.join(BIN, 'undexta')} -i -U <a.dexta >>all", shell=True, cwd=str(tmp_path), capture_output=True)
        assert r.returncode == 0, r.stderr
    assert _read(out) == b"KEEP ME\n" + back + back
    # a file that already holds bytes, opened read-write at offset 0: its bytes beyond the new text survive as with fwrite
    out = tmp_path / "rw"
    _write(out, b"x" * (len(back) + 10))
    r = subprocess.run(f"{os.path.join(BIN, 'undexta')} -i -U <a.dexta 1<>rw", shell=True, cwd=str(tmp_path), capture_output=True)
    assert r.returncode == 0, r.stderr
    assert _read(out) == back + b"x" * 10


@pytest.mark.gpu
def test_cli_degenerate_file_is_refused_loudly_where_the_reference_reads_out_of_bounds(tmp_path):
    """A file whose deletion line holds nothing but the run character leaves the deletion scheme an EMPTY histogram: the
    reference builds a Huffman tree of no leaves and reads node[-1] (QV.c:201) -- undefined behaviour that happens to write a
    file.  Documented deviation: dexqv here says so and exits 1, its output file left empty and the source
    kept (as after any failure: the output is opened first, dexqv.c:70-72); what the compiled reference does with the same file
    is recorded beside it, not asserted (it is not defined)."""
    L_ = 40
    text = b"@m/1/0_%d RQ=0.850\n" % L_ + b"5" * L_ + b"\n" + b"N" * L_ + b"\n" + b"3" * L_ + b"\n" + b"7" * L_ + b"\n" + b"9" * L_ + b"\n"
    mine = tmp_path / "mine"; mine.mkdir()
    _write(mine / "d.quiva", text)
    r = run("dexqv", ["-k", "d.quiva"], mine)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert b"holds no symbols" in r.stderr and b"libdexgpu error -4" in r.stderr, r.stderr
    assert (mine / "d.dexqv").read_bytes() == b"" and (mine / "d.quiva").exists()
    if O.have_ref():
        ref = tmp_path / "ref"; ref.mkdir()
        _write(ref / "d.quiva", text)
        q = run("dexqv", ["-k", "d.quiva"], ref, ref=True)
        print("reference on the degenerate file: exit code", q.returncode, "stderr", q.stderr[:200], "wrote a file:", (ref / "d.dexqv").exists())


@pytest.mark.gpu
@needs_ref
def test_cli_large_file_paths_on_small_files(tmp_path):
    """What the tools do with LARGE files, brought down to test size by their thresholds: dexqv reads its input from the file
    descriptor into the upload's pinned buffers (dx_file_dexqv_fd_to, DEXGPU_TEST=fd_min) and writes into an output file whose pages an
    allocator thread lays out meanwhile (outfile_min: three tenths of the input, the rest given back) -- and hands a file
    that way refuses (a malformed one, one below 1 MiB) to the in-memory driver, which has the reference's words --; undexqv walks
    the records on the device (device_walk_min) and decodes with what the walk noted.  Same files as the reference's."""
    qv = synth.make_quiva(60, seed=9, mean=8000).text                 # ~2.4 MB
    env = dict(os.environ, DEXGPU_TEST=test_env(fd_min=1, outfile_min=1, device_walk_min=0, walk_piece=8192))
    mine, ref = tmp_path / "mine", tmp_path / "ref"
    for d, isref in ((mine, False), (ref, True)):
        d.mkdir()
        _write(d / "c.quiva", qv)
        exe = lambda t: os.path.join(O.REF_BIN if isref else BIN, t)
        assert subprocess.run([exe("dexqv"), "-k", "c"], cwd=str(d), env=env, capture_output=True).returncode == 0
        os.remove(d / "c.quiva")
        assert subprocess.run([exe("undexqv"), "-k", "-U", "c"], cwd=str(d), env=env, capture_output=True).returncode == 0
    for nme in ("c.dexqv", "c.quiva"):
        assert _read(mine / nme) == _read(ref / nme), nme
    assert _read(mine / "c.quiva") == qv
    small = synth.make_quiva(3, seed=10, mean=500).text               # below 1 MiB: DX_E_AGAIN, then through memory
    bad = qv[: len(qv) // 2 - 7] + qv[len(qv) // 2:]                  # a line seven symbols short
    for name, data in (("s", small), ("b", bad)):
        outs = []
        for d, isref in ((mine, False), (ref, True)):
            _write(d / (name + ".quiva"), data)
            r = subprocess.run([os.path.join(O.REF_BIN if isref else BIN, "dexqv"), "-k", name], cwd=str(d), env=env, capture_output=True)
            outs.append((r.returncode, r.stderr, _read(d / (name + ".dexqv")) if (d / (name + ".dexqv")).exists() and r.returncode == 0 else None))
        assert outs[0] == outs[1], name


# ---- the routes a file can take through a tool (cli_common.c's header lists them) ---------------------------------------------------
def tool_marks(stderr: bytes, tool: str):
    """names of the tool's own DEXGPU_TIMING marks (the library's carry dx_open / dx_file in the bracket), `leaving` left out:
    whether it is printed depends on LD_PRELOAD"""
    names = [m.group(1).strip() for m in re.finditer(r"(?m)^\[%s\s+[\d.]+ ms\] (.*)$" % tool, stderr.decode(errors="replace"))]
    return [n for n in names if n != "leaving"]


def timed(tool, args, cwd, stdin=None, **env):
    e = dict(os.environ, DEXGPU_TIMING="1")
    e.pop("DEXGPU_DEVICES", None)
    e.update(env)
    r = run(tool, args, cwd, stdin=stdin, env=e)
    assert r.returncode == 0, r.stderr
    return r


STREAMED = ["start", "GPU context open", "output written"]
PLANNED = ["start", "input read", "records walked", "output file allocated", "GPU context open", "output written"]
CHUNKED = ["start", "input read", "GPU context open", "output written"]
WHOLE = ["start", "input read", "GPU context open", "converted (index, copies, kernels)", "output written"]
# (tool, arguments, input: a file's kind or "-" for standard input, DEXGPU_TEST keys, other environment, the marks)
ROUTE_CASES = [
    ("1_descriptor_pwrite",    "dexqv",   ["-k", "x"], "quiva", dict(fd_min=1), {}, STREAMED),
    ("1_descriptor_outfile",   "dexqv",   ["-k", "x"], "quiva", dict(fd_min=1, outfile_min=1), {}, STREAMED),
    ("1_then_5_small_file",    "dexqv",   ["-k", "x"], "small_quiva", dict(fd_min=1), {},
     ["start", "GPU context open", "input read", "GPU context open", "output written"]),
    ("2_pack2_pipe",           "dexta",   ["-i"],      "-fasta", dict(stream_chunk=20000), {}, STREAMED),
    ("2_pack2_large_file",     "dexar",   ["-k", "x"], "arrow", dict(stream_chunk=20000, fd_min=1), {}, STREAMED),
    ("3_unpack2_pipe",         "undexta", ["-i"],      "-dexta", {}, {}, STREAMED),
    ("4_undexqv_plan",         "undexqv", ["-k", "x"], "dexqv", dict(device_walk_min=0), {}, PLANNED),
    ("5_dexqv_into_file",      "dexqv",   ["-k", "x"], "quiva", {}, {}, CHUNKED),
    ("5_undexta_into_file",    "undexta", ["-k", "x"], "dexta", {}, {}, CHUNKED),
    ("5_undexar_into_file",    "undexar", ["-k", "x"], "dexar", {}, {}, CHUNKED),
    ("6_dexta_whole",          "dexta",   ["-k", "x"], "fasta", {}, {}, WHOLE),
    ("6_dexqv_three_contexts", "dexqv",   ["-k", "x"], "quiva", {}, {"DEXGPU_DEVICES": "0,0,0"}, WHOLE),
]


def route_inputs():
    fa = synth.make_seqfile("fasta", 400, seed=21, mean=900, width=60).text
    ar = synth.make_seqfile("arrow", 400, seed=21, mean=900, width=60).text
    qv = synth.make_quiva(60, seed=9, mean=8000).text                 # ~2.4 MB (the descriptor route takes 1 MiB and more)
    return {"fasta": fa, "arrow": ar, "quiva": qv, "small_quiva": synth.make_quiva(3, seed=10, mean=500).text,
            "dexta": O.dexta(fa), "dexar": O.dexar(ar), "dexqv": O.dexqv(qv)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_cli_stage_marks_per_route(tmp_path, case):
    """Which route a file took shows in the tool's stage marks (DEXGPU_TIMING=1), brought down to small files by the thresholds of
    DEXGPU_TEST.  The lists are those of the commit before the routes became functions, read off its source (no GPU was to be
    had to run its binaries beside the new ones: profiles/cli_refactor_cli.txt); the one-shot ones are the names its tools
    printed in profiles/files_refactor_cli.txt, lines 17-20."""
    _, tool, args, source, keys, env, want = case
    data = route_inputs()[source.lstrip("-")]
    if keys:
        env = dict(env, DEXGPU_TEST=test_env(**keys))
    if source.startswith("-"):
        r = timed(tool, args, tmp_path, stdin=data, **env)
    else:
        _write(tmp_path / ("x." + source.replace("small_", "")), data)
        r = timed(tool, args, tmp_path, **env)
    assert tool_marks(r.stderr, tool) == want, r.stderr


@pytest.mark.gpu
def test_cli_device_count_is_honoured_for_large_files(tmp_path):
    """DEXGPU_DEVICES shards a "large" file (DEXGPU_TEST=fd_min=1) too: the device list is read before the route is chosen.
    The commit before this test fails it for dexqv: its main thread read the number of contexts while the thread that opens
    them was still at it, saw none, and sent the file down the single-context descriptor route (`dexqv: begin`)."""
    inputs = route_inputs()
    env = {"DEXGPU_DEVICES": "0,0,0", "DEXGPU_TEST": test_env(fd_min=1)}
    for tool, kind, ext, want in (("dexqv", "quiva", "dexqv", O.dexqv), ("dexta", "fasta", "dexta", O.dexta), ("dexar", "arrow", "dexar", O.dexar)):
        _write(tmp_path / ("x." + kind), inputs[kind])
        r = timed(tool, ["-k", "x"], tmp_path, **env)
        assert "converted (index, copies, kernels)" in tool_marks(r.stderr, tool), r.stderr
        assert b"dexqv: begin" not in r.stderr
        assert _read(tmp_path / ("x." + ext)) == want(inputs[kind]), tool
    os.remove(tmp_path / "x.quiva")
    timed("undexqv", ["-k", "x"], tmp_path, **env)
    assert _read(tmp_path / "x.quiva") == O.undexqv(inputs["dexqv"])
