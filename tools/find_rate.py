"""Context.find beside the walk it shares with Context.census and beside what a user has today -- the whole text by dx_file_unpack2
and a search of it on one core -- on a .dexta of READS reads of SYMS bases (100 000 x 10 000: 1 GB of bases, 0.25 GB of image).

    python tools/find_rate.py [READS] [SYMS] [REPS]

Part 1, whole calls, host clocks around the Python calls with the device synchronised on both sides (host walk, upload and
read-backs included: what a caller waits for), one warm-up, then REPS (5) rounds in which the routes take turns:

    find-1      1 exact pattern of 20 symbols
    find-16x2   16 patterns of 20 symbols, one mismatch, both strands (32 queries)
    find-64     64 exact patterns of 20 symbols
    census      Context.census of the same image: the same walk and upload, the bytes read once
    unpack      dx_file_unpack2 to upper-case text, one line a read: what the search on the host needs first
    unpack+1    ... and bytes.count of one pattern in that text (memchr-fast, non-overlapping, exact only: the baseline at its best)
    count-1     that count alone

Part 2, the kernel alone: the image stands on the device with its units (walked here), and dx_code_find is timed with HIP events on
the context's stream, counting pass only (cap 0), for 1 to 64 queries of 20 symbols (two words) and of 12 (one word), exact and
with one mismatch, and for half the reads; dx_code_counts of the same units stands beside it.  If the time follows queries x
positions the kernel is bound by its instructions; if it follows the bytes alone, by memory.
"""
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402


def walk(img):
    """a current-layout .dexta: where every read's packed bases stand and how many there are (undexta.c:175-271)"""
    at, off, ln = 6 + int.from_bytes(img[2:6], "little"), [], []
    while at < len(img):
        while img[at] == 255:
            at += 1
        at += 1
        beg, end = int.from_bytes(img[at:at + 4], "little"), int.from_bytes(img[at + 4:at + 8], "little")
        at += 12
        off.append(at); ln.append(end - beg)
        at += (end - beg + 3) // 4
    return np.array(off, np.uint64), np.array(ln, np.uint32)


def turns(ctx, runs, reps):
    ms = {name: [] for name in runs}
    for r in range(reps + 1):
        for name, f in runs.items():
            ctx.sync()
            t0 = time.perf_counter()
            f()
            ctx.sync()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def query(word, max_mis=0):
    code = 0
    for c in word:
        code = (code << 2) | "ACGT".index(c)
    return code, len(word), max_mis


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(20261020)
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
        words = []                                             # 64 words of 20 that do occur: one from each of 64 reads
        for k in range(64):
            at = int(rng.integers(0, syms - 20))
            words.append(body[k * (reads // 64)][at:at + 20].decode())
        del body

        # ---- part 1: whole calls --------------------------------------------------------------------------------------------------------
        got = {}
        runs = {"find-1": lambda: got.__setitem__("1", ctx.find("fasta", img, words[:1])),
                "find-16x2": lambda: got.__setitem__("16x2", ctx.find("fasta", img, words[:16], max_mismatches=1, both_strands=True)),
                "find-64": lambda: got.__setitem__("64", ctx.find("fasta", img, words)),
                "census": lambda: ctx.census("fasta", img),
                "unpack": lambda: ctx.undexta(img, upper=True, width=2**31 - 1),
                "unpack+1": lambda: got.__setitem__("host", ctx.undexta(img, upper=True, width=2**31 - 1).count(words[0].encode())),
                "count-1": lambda: flat.count(words[0].encode())}
        ms = turns(ctx, runs, reps)
        for name, t in ms.items():
            med = float(np.median(t))
            print(f"    {name:<10} median {med:10.3f} ms  min {min(t):10.3f}  max {max(t):10.3f}  spread {100 * (max(t) - min(t)) / med:5.1f} %   "
                  f"all: {' '.join(f'{x:.1f}' for x in t)}", flush=True)
        h1 = got["1"][0]["hits"]
        print(f"    hits: find-1 {h1} (the host's non-overlapping count: {got['host']}), find-16x2 {got['16x2'][0]['hits']}, find-64 {got['64'][0]['hits']}")
        assert h1 >= got["host"] >= 1 and got["64"][0]["hits"] >= 64
        med = {name: float(np.median(t)) for name, t in ms.items()}
        print(f"    find-1 / unpack+1: {med['find-1'] / med['unpack+1']:.3f};  find-1 - census: {med['find-1'] - med['census']:.1f} ms", flush=True)
        del flat

        # ---- part 2: the kernel alone ---------------------------------------------------------------------------------------------------
        bufs = [ctx.to_device(np.frombuffer(img, np.uint8)), ctx.to_device(off), ctx.to_device(ln), ctx.alloc(4 * reads + 4)]
        half = reads // 2

        def kernel(qs, n=reads, count=True):
            return lambda: ctx.code_find(bufs[0], len(img), bufs[1], None, bufs[2], n, qs, d_count=bufs[3] if count else None)

        cases = {"counts": lambda: ctx.code_counts(bufs[0], len(img), bufs[1], None, bufs[2], reads)}
        for nq in (1, 2, 4, 8, 16, 32, 64):
            cases[f"20 exact x{nq}"] = kernel([query(w) for w in words[:nq]])
        for nq in (1, 16, 64):
            cases[f"12 exact x{nq}"] = kernel([query(w[:12]) for w in words[:nq]])
            cases[f"20 1-mis x{nq}"] = kernel([query(w, 1) for w in words[:nq]])
        cases["20 exact x16, half the reads"] = kernel([query(w) for w in words[:16]], n=half)
        cases["20 exact x64, half the reads"] = kernel([query(w) for w in words], n=half)
        for f in cases.values():
            f()
        ctx.sync()
        ev = {name: [] for name in cases}
        for _ in range(reps):
            for name, f in cases.items():
                ev[name].append(timed(f))
        print("the kernel alone (events; dx_code_find, counting pass, every unit's count written):")
        for name, t in ev.items():
            m = float(np.median(t))
            nq = int(re.search(r" x(\d+)", name).group(1)) if " x" in name else 0
            pq = (positions // 2 if "half" in name else positions) * max(nq, 1)
            print(f"    {name:<30} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   {len(img) / m / 1e6:8.1f} GB/s of image"
                  + (f"   {m * 1e9 / pq:6.3f} ps a position and query" if nq else ""), flush=True)
        k1, k64 = float(np.median(ev["20 exact x1"])), float(np.median(ev["20 exact x64"]))
        print(f"    64 queries / 1 query: {k64 / k1:.1f} x the time;  the kernel's share of find-1: {k1 / med['find-1']:.3f}, of find-64: {k64 / med['find-64']:.3f}")
        for b in bufs:
            b.free()


if __name__ == "__main__":
    main()
