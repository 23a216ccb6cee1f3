"""What counting in passes costs: the two kernels the passes add -- dx_code_kmer_bins, dx_code_kmer_codes_range -- each alone beside the
kernels they were modelled on, Context.kmers_wide_files of one image beside Context.kmers_wide of it, and the same windows counted in
2, 4 and 8 passes.

    python tools/kmer_files_rate.py [READS] [SYMS] [REPS] [wide]

One process.  Every GPU step runs under a time limit of its own (STEP_LIMIT seconds, a watchdog that ends the process with status 124),
and the first error of any kind ends the run: nothing follows a fault.

Part 1, the kernels alone: READS reads of SYMS uniform random symbols (100 000 x 10 000: 10^9 positions, 0.25 GB packed) stand on the
device with their units; HIP events on the context's stream, one warm-up, then REPS (5) rounds, median, min and max reported.

    counts      dx_code_counts over the units: the walk's floor
    kmers k=6   dx_code_kmers at k = 6: the LDS route the bins' counting is
    bins        dx_code_kmer_bins at k = 21 canonical, 12 bits; and at k = 6, 12 bits, which counts what dx_code_kmers counts there
    codes       dx_code_kmer_codes at k = 21 canonical
    range       dx_code_kmer_codes_range over all bins, and over a quarter of them

Part 2, one pass, on a .dexta of the same shape, host clocks with the device synchronised on both sides, the two calls in turns:
Context.kmers_wide(img) and Context.kmers_wide_files([img]) at k = 21 canonical -- the same launches.  With `wide` as the fourth
argument only Context.kmers_wide is timed (part 1 and part 3 are left out): the run to make with the parent commit's library
(DEXGPU_LIB).

Part 3, several passes: the same windows with room = windows / 2, / 4, / 8 -- the total, and from the driver's DEXGPU_TIMING marks
the share of the bins pass, the walks (uploads and codes), the sorts and the runs.
"""
import os
import re
import sys
import tempfile
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402

STEP_LIMIT = 120
K = 21


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


def line(name, t, keys):
    m = float(np.median(t))
    print(f"    {name:<44} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   {keys / m / 1e6:8.2f} G windows/s", flush=True)
    return m


def rounds(reps, f, before=None):
    t = []
    for r in range(reps + 1):
        if before:
            before()
        x = timed(f)
        if r:
            t.append(x)
    return t


def marks(f):
    """f() with DEXGPU_TIMING=1 and the library's stderr kept: [(ms since the watch began, what)]"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["DEXGPU_TIMING"] = "1"
        try:
            f()
        finally:
            os.environ.pop("DEXGPU_TIMING", None)
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return [(float(m.group(1)), m.group(2)) for m in re.finditer(r"\[kmers_files\s+([0-9.]+) ms\] (.*)", text)]


def host_timed(ctx, reps, calls, limit=600):
    """the calls in turns, reps rounds after one warm-up: {name: [ms]}, and the last answer of each"""
    t, got = {n: [] for n, _ in calls}, {}
    for r in range(reps + 1):
        for name, f in calls:
            ctx.sync(); t0 = time.perf_counter()
            got[name] = step(f, limit)
            ctx.sync(); t1 = time.perf_counter()
            if r:
                t[name].append((t1 - t0) * 1e3)
    return t, got


def report(name, t):
    print(f"    {name:<34} median {np.median(t):10.3f} ms  min {min(t):10.3f}  max {max(t):10.3f}   the rounds: {' '.join(f'{x:.1f}' for x in t)}", flush=True)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    wide_only = len(sys.argv) > 4 and sys.argv[4] == "wide"
    torch.cuda.init()
    print(f"device: {torch.cuda.get_device_name(0)}; library: {os.environ.get('DEXGPU_LIB') or 'of this tree'}")
    positions = reads * syms
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        if not wide_only:
            # ---- part 1: the kernels alone ----------------------------------------------------------------------------------------------
            boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
            ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
            data = step(lambda: packed_reads(reads, syms, 1))
            n = reads * (syms - K + 1)
            codes = torch.empty(n, dtype=torch.int64, device="cuda")
            bins = torch.zeros(4096, dtype=torch.int64, device="cuda")
            table = torch.zeros(4096, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            print(f"{reads} reads of {syms} symbols: {positions / 1e9:.3f} G positions, {positions / 4e9:.3f} GB packed; {reps} rounds after one "
                  f"warm-up; events on the context's stream", flush=True)
            n6 = reads * (syms - 5)
            line("counts dx_code_counts", rounds(reps, lambda: ctx.code_counts(data, data.numel(), boff, None, ln, reads)), positions)
            line("kmers  dx_code_kmers k=6", rounds(reps, lambda: ctx.code_kmers(data, boff, None, ln, 6, False, table)), n6)
            line("kmers  dx_code_kmers k=6 canonical", rounds(reps, lambda: ctx.code_kmers(data, boff, None, ln, 6, True, table)), n6)
            line("bins   dx_code_kmer_bins k=6 bits=12", rounds(reps, lambda: ctx.code_kmer_bins(data, boff, None, ln, 6, 12, False, bins)), n6)
            line("bins   dx_code_kmer_bins k=6 bits=12 canonical", rounds(reps, lambda: ctx.code_kmer_bins(data, boff, None, ln, 6, 12, True, bins)), n6)
            line("bins   dx_code_kmer_bins k=21 bits=12", rounds(reps, lambda: ctx.code_kmer_bins(data, boff, None, ln, K, 12, False, bins)), n)
            bins.zero_(); torch.cuda.synchronize()
            rounds(1, lambda: ctx.code_kmer_bins(data, boff, None, ln, K, 12, True, bins))          # (two calls, for the counts themselves)
            half = bins.cpu().numpy().astype(np.uint64) // np.uint64(2)                  # (two calls have added to them)
            assert int(half.sum()) == n, "the bins do not hold every window"
            cum = np.cumsum(half)
            q = int(np.searchsorted(cum, n // 4)) + 1                                     # the bins that hold the first quarter of the windows
            print(f"  k = {K} canonical: {n / 1e9:.3f} G windows; the fullest of 4096 bins holds {int(half.max())}, "
                  f"bins [0, {q}) hold {int(cum[q - 1]) / n:.3f} of them", flush=True)
            line("bins   dx_code_kmer_bins k=21 canonical", rounds(reps, lambda: ctx.code_kmer_bins(data, boff, None, ln, K, 12, True, bins)), n)
            line("codes  dx_code_kmer_codes k=21 canonical", rounds(reps, lambda: ctx.code_kmer_codes(data, boff, None, ln, K, True, cap=n, codes=codes)), n)
            line("range  dx_code_kmer_codes_range, all bins", rounds(reps, lambda: ctx.code_kmer_codes_range(data, boff, None, ln, K, 12, 0, 4096, True, cap=n, codes=codes)), n)
            line(f"range  dx_code_kmer_codes_range, bins [0, {q})", rounds(reps, lambda: ctx.code_kmer_codes_range(data, boff, None, ln, K, 12, 0, q, True, cap=n, codes=codes)), n)
            del data, codes, bins, table
            torch.cuda.empty_cache()

        # ---- part 2: one pass -----------------------------------------------------------------------------------------------------------
        text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
        img = step(lambda: ctx.dexta(text), 600)
        print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image; host clocks, "
              f"{reps} rounds after one warm-up", flush=True)
        del text
        calls = [("kmers_wide(img)", lambda: ctx.kmers_wide("fasta", img, K, True))]
        if not wide_only:
            calls.append(("kmers_wide_files([img])", lambda: ctx.kmers_wide_files("fasta", [img], K, True)))
        t, got = host_timed(ctx, reps, calls)
        for name, _ in calls:
            report(name, t[name])
        one = got["kmers_wide(img)"][0]
        print(f"    windows {one['windows']}, distinct {one['distinct']}, max_count {one['max_count']}", flush=True)
        if wide_only:
            return
        rep = got["kmers_wide_files([img])"][0]
        assert rep["passes"] == 1 and all(rep[f] == one[f] for f in one), "the two routes differ"
        a, b = t["kmers_wide(img)"], t["kmers_wide_files([img])"]
        d = float(np.median(b) - np.median(a))
        print(f"    difference of the medians {d:+.3f} ms; the spreads (max - min) {max(a) - min(a):.3f} and {max(b) - min(b):.3f} ms: "
              + ("none" if abs(d) <= max(max(a) - min(a), max(b) - min(b)) else "MORE than the spread"), flush=True)

        # ---- part 3: several passes -----------------------------------------------------------------------------------------------------
        windows = one["windows"]
        for parts in (1, 2, 4, 8):
            room = 0 if parts == 1 else -(-windows // parts)
            call = lambda: ctx.kmers_wide_files("fasta", [img], K, True, room=room)      # noqa: E731
            t, got = host_timed(ctx, reps, [("x", call)])
            r = got["x"][0]
            assert all(r[f] == one[f] for f in one), "the passes' answer differs"
            report(f"room = windows / {parts}: {r['passes']} passes", t["x"])
            m = marks(lambda: step(call, 600))
            share, last = {}, 0.0
            for at, what in m:
                key = ("the bins pass" if "bins" in what else "walks (uploads, codes)" if "codes written" in what else "sorts" if "sorted" in what
                       else "runs" if "runs read" in what else "host walk, allocations, frees")
                share[key] = share.get(key, 0.0) + at - last
                last = at
            print("        of one call with DEXGPU_TIMING: " + ";  ".join(f"{k} {v:.1f} ms" for k, v in share.items()) + f";  in all {last:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
