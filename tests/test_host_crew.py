"""dx_crew.c (the thread crew under the sharded file drivers) compiled with ThreadSanitizer as a stand-alone program and run as a
child process: crews of 1, 2, 5 and 8 over a table of work + fold, work-only and fold-only phases; every work function once per member
and in table order, every fold once and on member 0, the published sums as expected, no race, no hang.  CPU only."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixed_layout():
    """In the child, before the program starts: no address-space randomisation (the personality flag `setarch -R` sets).  This
    ThreadSanitizer runtime knows where programs and libraries are mapped, and where a kernel randomises over more bits than it
    allows for it ends with 'unexpected memory mapping' before main() runs.  A kernel that does not let a process ask: as it was."""
    libc = ctypes.CDLL(None)
    now = libc.personality(0xffffffff)
    if now != -1:
        libc.personality(now | 0x0040000)          # ADDR_NO_RANDOMIZE


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_crew_under_tsan(tmp_path):
    exe = str(tmp_path / "host_crew")
    csrc = os.path.join(ROOT, "dextractor_amd", "csrc")
    cc = ["gcc", "-O1", "-g", "-fsanitize=thread", "-Wall", "-Wextra", "-I" + csrc,
          os.path.join(ROOT, "tests", "host_crew", "driver.c"), os.path.join(csrc, "dx_crew.c"), "-o", exe, "-lpthread"]
    r = subprocess.run(cc, capture_output=True)
    if r.returncode != 0 and (b"sanitize" in r.stderr or b"tsan" in r.stderr):
        pytest.skip("this gcc has no ThreadSanitizer runtime")
    assert r.returncode == 0, r.stderr.decode()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=60, preexec_fn=_fixed_layout)
    if r.stdout == b"" and b"FATAL: ThreadSanitizer: unexpected memory mapping" in r.stderr:
        pytest.skip("this ThreadSanitizer runtime cannot start under this kernel's address-space layout")
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-6000:]).decode(errors="replace")
    assert b"ThreadSanitizer" not in r.stderr, r.stderr[-6000:].decode(errors="replace")
    assert r.stdout == b"ok\n"
