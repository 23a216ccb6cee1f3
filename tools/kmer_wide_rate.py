"""The three steps of the wide k-mer route -- dx_code_kmer_codes, dx_sort_u64, dx_kmer_runs -- each alone, beside a plain copy of the
keys (the floor of a sort pass) and beside dx_code_kmers' global route at k = 14; and Context.kmers_wide as a caller sees it.

    python tools/kmer_wide_rate.py [READS] [SYMS] [REPS]

One process.  Every GPU step runs under a time limit of its own (STEP_LIMIT seconds, a watchdog that ends the process with status 124),
and the first error of any kind ends the run: nothing follows a fault.

Part 1, the kernels alone: READS reads of SYMS uniform random symbols (100 000 x 10 000: 10^9 positions, 0.25 GB packed) stand on the
device with their units; HIP events on the context's stream, one warm-up, then REPS (3) rounds, median, min and max reported.  At
k = 14, 16, 21, 32:

    codes       dx_code_kmer_codes: every window's code written out (its two small launches, prefix sum and read-back included)
    sort        dx_sort_u64 of those codes with bits = 2 k: ceil(k / 4) passes (the codes are made again before every round, untimed)
    runs        dx_kmer_runs of the sorted codes, counting only (cap 0), with a spectrum of 256 bins
    copy        a device-to-device copy of the 8 x windows bytes: what one pass costs at least (it reads and writes every key once)

and in the same run dx_code_kmers at k = 14 over the same units (the parent's 55 ms, profiles/kmer_rate.txt), and the k = 32 sort of
keys of which every fifth, every second and every one is one value (a homopolymer's share of a read set, and beyond): the
sort's cost must not grow with it.

Part 2, the whole call on a .dexta of the same shape (a 1 GB .fasta), host clocks with the device synchronised on both sides:
Context.kmers_wide at k = 21 -- host walk, allocations, upload, codes, sort, runs, read-backs, frees: what a caller waits for --,
and once more with DEXGPU_TIMING=1 for the driver's own stage marks.
"""
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402

STEP_LIMIT = 120


def _late():
    print("a step passed its time limit: the run ends here", flush=True)
    os._exit(124)


def step(f, limit=STEP_LIMIT):
    """f() under its own time limit (a watchdog thread: it runs while the main thread waits inside the library)"""
    w = threading.Timer(limit, _late)
    w.daemon = True
    w.start()
    try:
        return f()
    finally:
        w.cancel()


def timed(f):
    def g():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    return step(g)


def packed_reads(reads, syms, seed):
    """reads x syms uniform random symbols packed four a byte on the device (uint8 tensor)"""
    assert syms % 4 == 0
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(reads * syms // 4, dtype=torch.uint8, device="cuda")
    chunk = max(1, (1 << 24) // syms)
    for r0 in range(0, reads, chunk):
        n = (min(reads, r0 + chunk) - r0) * syms
        s = torch.randint(0, 4, (n,), generator=g, device="cuda", dtype=torch.int64).view(-1, 4)
        out[r0 * syms // 4:r0 * syms // 4 + n // 4] = ((s[:, 0] << 6) | (s[:, 1] << 4) | (s[:, 2] << 2) | s[:, 3]).to(torch.uint8)
    return out


def line(name, t, keys, floor=None, passes=None):
    m = float(np.median(t))
    out = f"    {name:<30} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   {keys / m / 1e6:8.2f} G keys/s"
    if floor:
        out += f"   {m / floor:6.2f} x copy"
    if floor and passes:
        out += f"   {passes} passes: {m / passes:7.3f} ms = {m / passes / floor:5.2f} x copy a pass"
    print(out, flush=True)
    return m


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch.cuda.init()
    print(f"device: {torch.cuda.get_device_name(0)}")
    positions = reads * syms
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        # ---- part 1: the kernels alone --------------------------------------------------------------------------------------------------
        boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
        ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
        data = step(lambda: packed_reads(reads, syms, 1))
        most = reads * (syms - 13)
        codes = torch.empty(most, dtype=torch.int64, device="cuda")
        tmp = torch.empty(most, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print(f"{reads} reads of {syms} symbols: {positions / 1e9:.3f} G positions, {positions / 4e9:.3f} GB packed; {reps} rounds after one "
              f"warm-up; events on the context's stream", flush=True)

        table = torch.zeros(4 ** 14, dtype=torch.int64, device="cuda")
        t14 = []
        for r in range(reps + 1):
            table.zero_(); torch.cuda.synchronize()
            t = timed(lambda: ctx.code_kmers(data, boff, None, ln, 14, False, table))
            if r:
                t14.append(t)
        m14 = line("dx_code_kmers k=14 (table)", t14, most)
        del table
        torch.cuda.empty_cache()

        for k in (14, 16, 21, 32):
            n, passes = reads * (syms - k + 1), (2 * k + 7) // 8
            c, s = codes[:n], tmp[:n]
            tc, ts, tr, tp = [], [], [], []
            fig = None
            for r in range(reps + 1):
                a = timed(lambda: ctx.code_kmer_codes(data, boff, None, ln, k, False, cap=n, codes=c))
                p = timed(lambda: s.copy_(c))
                b = timed(lambda: ctx.sort_u64(c, 2 * k, s))
                d = timed(lambda: ctx.kmer_runs(c, n, 1, 0, 256))
                if r:
                    tc.append(a); tp.append(p); ts.append(b); tr.append(d)
            fig = step(lambda: ctx.kmer_runs(c, n, 1, 0, 256))[2]
            print(f"  k = {k}: {n / 1e9:.3f} G windows, {8 * n / 1e9:.2f} GB of codes; distinct {fig['distinct']}, max_count {fig['max_count']}", flush=True)
            floor = line("copy of the codes", tp, n)
            line("codes  dx_code_kmer_codes", tc, n, floor)
            ms = line(f"sort   dx_sort_u64 bits={2 * k}", ts, n, floor, passes)
            mr = line("runs   dx_kmer_runs", tr, n, floor)
            print(f"    codes + sort + runs: {np.median(tc) + ms + mr:9.3f} ms   (dx_code_kmers at k = 14 in this run: {m14:.3f} ms)", flush=True)
            if k == 32:
                for every, name in ((5, "every fifth key one value"), (2, "every second key one value"), (1, "all keys one value")):
                    tq = []
                    for r in range(reps + 1):
                        step(lambda: ctx.code_kmer_codes(data, boff, None, ln, k, False, cap=n, codes=c))
                        c[::every] = 0x5555555555555555
                        torch.cuda.synchronize()
                        b = timed(lambda: ctx.sort_u64(c, 2 * k, s))
                        if r:
                            tq.append(b)
                    line("sort   " + name, tq, n, floor, passes)
                x = c ^ (-(1 << 63))                                # (unsigned order in signed words)
                assert step(lambda: bool((x[1:] >= x[:-1]).all())), "the keys are not in order"
                del x
        del data, codes, tmp
        torch.cuda.empty_cache()

        # ---- part 2: the whole call -----------------------------------------------------------------------------------------------------
        text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
        img = step(lambda: ctx.dexta(text), 600)
        print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
        del text
        got, tk = None, []
        for r in range(reps + 1):
            ctx.sync(); t0 = time.perf_counter()
            got = step(lambda: ctx.kmers_wide("fasta", img, 21), 600)
            ctx.sync(); t1 = time.perf_counter()
            if r:
                tk.append((t1 - t0) * 1e3)
        print(f"    kmers_wide k=21   median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f}  spread {100 * (max(tk) - min(tk)) / np.median(tk):5.1f} %")
        print(f"    the rounds: {' '.join(f'{t:.1f}' for t in tk)} ms;  windows {got[0]['windows']}, distinct {got[0]['distinct']}, max_count {got[0]['max_count']}", flush=True)
        os.environ["DEXGPU_TIMING"] = "1"                       # once more with the driver's stage marks (stderr)
        try:
            step(lambda: ctx.kmers_wide("fasta", img, 21), 600)
        finally:
            os.environ.pop("DEXGPU_TIMING", None)


if __name__ == "__main__":
    main()
