"""dx_code_find_edit beside dx_code_find on the same buffer, and Context.find_edit beside what answers the question without it -- the
whole text by dx_file_unpack2 and a bit-vector scan of it on one core (tools/find_edit_scan.c, compiled here with -O2) -- on a .dexta
of READS reads of SYMS bases (100 000 x 10 000: 1 GB of bases, 0.25 GB of image).

    python tools/find_edit_rate.py [READS] [SYMS] [REPS]

Part 1, the kernel alone: the image stands on the device with its units (walked here), and the counting pass (cap 0, every unit's
count written) is timed with HIP events on the context's stream, one warm-up, then REPS (5) rounds in which the cases take turns:
dx_code_find_edit with 1 and with 64 queries at m = 20, k = 4 and at m = 45, k = 9, and dx_code_find with the same number of queries
beside each (20 symbols and 4 mismatches; 32 symbols, its longest, and 9 mismatches).  The ratio is the price of the distance.

Part 2, whole calls, host clocks around the Python calls with the device synchronised on both sides (host walk, upload and
read-backs included: what a caller waits for), one warm-up, then REPS rounds, taking turns:

    find_edit    Context.find_edit with one 45-letter pattern, k = 9
    unpack+scan  dx_file_unpack2 to upper-case text, one line a read, and find_edit_scan of that text on one core
    scan         that scan alone

The answers are asserted equal: hits and records with a hit.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dextractor_amd import api, synth     # noqa: E402
from find_rate import walk, turns, timed, query     # noqa: E402  (tools/find_rate.py: the image's walk, the clocks)


def host_scan():
    """tools/find_edit_scan.c as a shared object in a temporary directory"""
    out = os.path.join(tempfile.mkdtemp(prefix="find_edit_scan_"), "find_edit_scan.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-shared", "-fPIC", "-o", out, os.path.join(HERE, "find_edit_scan.c")])
    lib = C.CDLL(out)
    lib.find_edit_scan.restype = C.c_uint64
    lib.find_edit_scan.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    return lib.find_edit_scan


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(20261020)
    scan = host_scan()
    torch.cuda.init()
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
        img = ctx.dexta(text)
        n_text = len(text)
        del text
        off, ln = walk(img)
        positions = int(ln.sum())
        print(f"{reads} reads of {syms} bases: {n_text / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image, {positions / 1e9:.3f} G positions; "
              f"{reps} rounds after one warm-up, taking turns", flush=True)
        flat = ctx.undexta(img, upper=True, width=2**31 - 1)
        body = flat.split(b"\n")[1::2]
        words = []                                             # 64 words of 45 that do occur: one from each of 64 reads
        for k in range(64):
            at = int(rng.integers(0, syms - 45))
            words.append(body[k * (reads // 64)][at:at + 45].decode())
        del body

        # ---- part 1: the kernel alone ---------------------------------------------------------------------------------------------------
        bufs = [ctx.to_device(np.frombuffer(img, np.uint8)), ctx.to_device(off), ctx.to_device(ln), ctx.alloc(4 * reads + 4)]

        def edit(qs):
            return lambda: ctx.code_find_edit(bufs[0], len(img), bufs[1], None, bufs[2], reads, qs, d_count=bufs[3])

        def find(qs):
            return lambda: ctx.code_find(bufs[0], len(img), bufs[1], None, bufs[2], reads, qs, d_count=bufs[3])

        codes = lambda w: ["ACGT".index(c) for c in w]
        cases = {}
        for nq in (1, 64):
            cases[f"edit m=20 k=4 x{nq}"] = edit([(codes(w[:20]), 4) for w in words[:nq]])
            cases[f"find m=20 mis=4 x{nq}"] = find([query(w[:20], 4) for w in words[:nq]])
            cases[f"edit m=45 k=9 x{nq}"] = edit([(codes(w), 9) for w in words[:nq]])
            cases[f"find m=32 mis=9 x{nq}"] = find([query(w[:32], 9) for w in words[:nq]])
        for f in cases.values():
            f()
        ctx.sync()
        ev = {name: [] for name in cases}
        for _ in range(reps):
            for name, f in cases.items():
                ev[name].append(timed(f))
        print("the kernel alone (events; counting pass, every unit's count written):")
        med = {}
        for name, t in ev.items():
            med[name] = m = float(np.median(t))
            nq = int(name.rsplit("x", 1)[1])
            print(f"    {name:<22} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  spread {100 * (max(t) - min(t)) / m:5.1f} %   "
                  f"{m * 1e9 / (positions * nq):7.3f} ps a position and query   all: {' '.join(f'{x:.2f}' for x in t)}", flush=True)
        for nq in (1, 64):
            print(f"    x{nq}: edit m=20 k=4 / find m=20: {med[f'edit m=20 k=4 x{nq}'] / med[f'find m=20 mis=4 x{nq}']:.2f};  "
                  f"edit m=45 k=9 / find m=32: {med[f'edit m=45 k=9 x{nq}'] / med[f'find m=32 mis=9 x{nq}']:.2f}")
        for b in bufs:
            b.free()

        # ---- part 2: whole calls --------------------------------------------------------------------------------------------------------
        got = {}
        pat = words[0]

        def host(t):
            rec = C.c_uint64()
            return int(scan(t, len(t), pat.encode(), 9, C.byref(rec))), rec.value

        runs = {"find_edit": lambda: got.__setitem__("gpu", ctx.find_edit("fasta", img, [pat], max_errors=9)),
                "unpack+scan": lambda: got.__setitem__("host", host(ctx.undexta(img, upper=True, width=2**31 - 1))),
                "scan": lambda: host(flat)}
        ms = turns(ctx, runs, reps)
        print("whole calls (host clocks, the device synchronised on both sides):")
        for name, t in ms.items():
            m = float(np.median(t))
            print(f"    {name:<12} median {m:10.3f} ms  min {min(t):10.3f}  max {max(t):10.3f}  spread {100 * (max(t) - min(t)) / m:5.1f} %   "
                  f"all: {' '.join(f'{x:.1f}' for x in t)}", flush=True)
        rep = got["gpu"][0]
        print(f"    hits: find_edit {rep['hits']} in {rep['records_hit']} records; the host's scan: {got['host'][0]} in {got['host'][1]}")
        assert (rep["hits"], rep["records_hit"]) == got["host"] and rep["hits"] >= 1
        a, b = float(np.median(ms["find_edit"])), float(np.median(ms["unpack+scan"]))
        print(f"    find_edit / unpack+scan: {a / b:.4f}  ({'not slower' if a <= b else 'SLOWER'})", flush=True)
        assert a <= b, "Context.find_edit is slower than the unpack and the scan on one core"


if __name__ == "__main__":
    main()
