"""dxf_u2_slices (csrc/dx_file_u2.c) without a GPU: the loop that hands the packed reads of a walked .dexta / .dexar image to the
drivers slice by slice, run by tests/u2_slices_standin.c -- a program of its own in which device memory is host memory -- under the
host's sanitizers.  The stand-in's hook holds every slice against the walk (the partition, the cap, the bytes, the offsets, the
lengths, the words of its own) and exits non-zero on the first breach; here its inputs are chosen and its slice counts read."""
import os
import re
import shutil
import subprocess

import pytest

import _oracle as O
import _u2_slices as U

GOLDEN = [("fasta", "ta_edge.dexta"), ("fasta", "ta_small.dexta"), ("fasta", "ta_small.legacy_swapped.dexta"), ("arrow", "ar_edge.dexar")]


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    """the loop's C file, the walk's and the stand-in, compiled with the host's sanitizers into a program of its own"""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build tests/u2_slices_standin.c with")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "dextractor_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("standin") / "u2_slices_standin")
    files = [os.path.join(root, "tests", "u2_slices_standin.c")] + [os.path.join(src, f) for f in
             ("dx_file_u2.c", "dx_file_pack2.c", "dx_files.c", "dx_host.c", "dx_crew.c")]
    subprocess.check_call([cc, "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(root, "include"), "-I" + src, "-o", exe, *files,
                           "-Wl,--unresolved-symbols=ignore-all", "-lpthread", "-lm"])
    return exe


def run(standin, tmp_path, kind, img):
    """the stand-in on an image -> (records, {cap: slices})"""
    (tmp_path / "image").write_bytes(img)
    env = {k: v for k, v in os.environ.items() if k != "DEXGPU_TEXT_BUDGET"}
    r = subprocess.run([standin, kind, str(tmp_path / "image")], capture_output=True, text=True, timeout=600,
                       env=dict(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    slices = {int(c): int(n) for c, n in re.findall(r"cap (\d+): (\d+) slices", r.stdout)}
    assert sorted(slices) == [0, 1, 5, 64, 4096]
    return int(re.match(r"(\d+) records", r.stdout).group(1)), slices


@pytest.mark.parametrize("kind,name", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_the_goldens_in_slices(standin, tmp_path, kind, name):
    records, slices = run(standin, tmp_path, kind, O.golden(name))
    assert records >= 3 and slices[0] == 1 and slices[1] == slices[5] == records        # (no record fits 5 bytes with a neighbour's header)
    # three slices at least at cap 64 -- but for ar_edge.dexar, an image of 125 bytes whose four records span fewer than 128: two is
    # all that 64 bytes a slice can cut it into, and its three or more slices are those of caps 1 and 5 above
    assert (2 if name == "ar_edge.dexar" else 3) <= slices[64] <= records and slices[4096] >= 1


def test_a_synthetic_image_with_empty_records_and_one_larger_than_the_cap(standin, tmp_path):
    text, lens = U.synthetic()
    assert len(lens) == 40 and lens[0] == lens[-1] == 0 and lens[12] == lens[13] == 0 and (lens[U.BIG] + 3) // 4 > 4096
    records, slices = run(standin, tmp_path, "fasta", U.image(O.dexta, text))
    assert records == 40 and slices[0] == 1 and slices[1] == 40
    assert 3 <= slices[4096] < slices[64] <= 40
    assert slices == {cap: U.slices(lens, cap) for cap in slices}                       # (what tests/test_gpu_u2_slices.py counts its slices by)


def test_an_image_without_records(standin, tmp_path):
    img = U.image(O.dexta, U.synthetic()[0])
    records, slices = run(standin, tmp_path, "fasta", img[:6 + int.from_bytes(img[2:6], "little")])
    assert records == 0 and set(slices.values()) == {0}                                 # nothing is launched, nothing is allocated
