"""dx_code_kmer_screen beside the walk it rides on, against sets of three sizes with none, about 1 % and all of the windows in the set;
the build of each set; and Context.screen as a caller sees it beside today's route on one core.

    python tools/screen_rate.py [READS] [SYMS] [REPS] [whole]

One process.  Every GPU step runs under a time limit of its own (STEP_LIMIT seconds, a watchdog that ends the process with status 124),
and the first error of any kind ends the run: nothing follows a fault.

Part 1, the kernels alone: READS reads of SYMS uniform random symbols (100 000 x 10 000: 10^9 positions, 0.25 GB packed) stand on the
device with their units; HIP events on the context's stream, one warm-up, then REPS (5) rounds, median, min and max reported; k = 21,
canonical.

    counts      dx_code_counts over the same units: the walk alone
    codes       dx_code_kmer_codes: the walk, the code of every window, 8 bytes written a window
    set         a "genome" of G random symbols (4.8 x 10^4: a phage; 5 x 10^6: a bacterium, 40 MB of codes; 10^8: 800 MB, beyond the
                Infinity Cache) -> its codes (one unit), sorted, dx_kmer_set_from_sorted: the three steps timed together, once
    screen      dx_code_kmer_screen of the reads against that set with none of the reads cut from the genome (a random window is in
                the set by chance only), with 1 % of them (whole reads copied from random places of it), and with all

Part 2 (with the fourth argument), the whole call on a .dexta of the same shape (a 1 GB .fasta), host clocks with the device synchronised
on both sides: Context.screen against the bacterium's set, and once more with DEXGPU_TIMING=1 for the driver's stage marks; beside it
today's route on an eighth of the text, on one core: undexta -U, the canonical codes of every record in numpy, np.isin against the
set's codes -- scaled by 8.
"""
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402

STEP_LIMIT = 180
K = 21
GENOMES = (48000, 5000000, 100000000)


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


class View:
    """a torch tensor as the methods that want a .ptr take it"""
    def __init__(self, t):
        self.ptr, self.nbytes = t.data_ptr(), t.numel() * t.element_size()


def packed_random(nbytes, seed):
    """nbytes of uniform random packed symbols on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for b0 in range(0, nbytes, 1 << 26):
        n = min(nbytes, b0 + (1 << 26)) - b0
        out[b0:b0 + n] = torch.randint(0, 256, (n,), generator=g, device="cuda", dtype=torch.int16).to(torch.uint8)
    return out


def plant(data, genome, reads, syms, count, seed):
    """the first `count` reads become copies of syms symbols from random byte offsets of the packed genome"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    per, room = syms // 4, genome.numel() - syms // 4
    for r0 in range(0, count, 4096):
        n = min(count, r0 + 4096) - r0
        at = torch.randint(0, room + 1, (n, 1), generator=g, device="cuda", dtype=torch.int64)
        idx = at + torch.arange(per, device="cuda", dtype=torch.int64).view(1, -1)
        data[r0 * per:(r0 + n) * per] = genome[idx.view(-1)]


def line(name, t, windows, extra=""):
    m = float(np.median(t))
    print(f"    {name:<44} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   {windows / m / 1e6:8.2f} G windows/s{extra}", flush=True)
    return m


def rounds(reps, f):
    out = []
    for r in range(reps + 1):
        t = timed(f)
        if r:
            out.append(t)
    return out


def host_route(ctx, text, codes, k):
    """today's route on one core: the image unpacked to text, every record's canonical codes in numpy, np.isin against the set ->
    (seconds, hits)"""
    img = ctx.dexta(text)
    ctx.sync(); t0 = time.perf_counter()
    up = ctx.undexta(img, upper=True)
    lut = np.full(256, 255, np.uint8)
    for c, l in enumerate(b"ACGT"):
        lut[l] = c
    every = []
    for rec in up.split(b">")[1:]:
        s = lut[np.frombuffer(rec[rec.index(b"\n") + 1:].replace(b"\n", b""), np.uint8)].astype(np.uint64)
        n = len(s) - k + 1
        if n <= 0:
            continue
        f, r = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for i in range(k):
            f = (f << np.uint64(2)) | s[i:i + n]
            r = (r << np.uint64(2)) | (np.uint64(3) - s[k - 1 - i:k - 1 - i + n])
        every.append(np.minimum(f, r))
    hits = int(np.isin(np.concatenate(every), codes).sum())              # (one look-up for all records: the set is sorted once)
    return time.perf_counter() - t0, hits


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    whole = len(sys.argv) > 4
    assert syms % 4 == 0
    torch.cuda.init()
    print(f"device: {torch.cuda.get_device_name(0)}")
    windows = reads * (syms - K + 1)
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
        ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
        data = step(lambda: packed_random(reads * syms // 4, 1))
        out = torch.empty(4 * reads, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        print(f"{reads} reads of {syms} symbols: {reads * syms / 1e9:.3f} G positions, {windows / 1e9:.3f} G windows at k = {K}, canonical; "
              f"{reps} rounds after one warm-up; events on the context's stream", flush=True)

        # ---- the floor ------------------------------------------------------------------------------------------------------------------
        line("counts dx_code_counts", rounds(reps, lambda: ctx.code_counts(View(data), data.numel(), View(boff), None, View(ln), reads)), windows)
        codes = torch.empty(windows, dtype=torch.int64, device="cuda")
        m_codes = line("codes  dx_code_kmer_codes", rounds(reps, lambda: ctx.code_kmer_codes(data, boff, None, ln, K, True, cap=windows, codes=codes)), windows)
        del codes
        torch.cuda.empty_cache()
        m_alt = m_codes + 49.077 * windows / 0.998e9          # (dx_sort_u64 at k = 21: 49.077 ms for 0.998 G keys, and linear in them)
        print(f"    the sort-merge alternative for these windows: codes + dx_sort_u64 of the reads' codes, {m_codes:.2f} + "
              f"{m_alt - m_codes:.2f} ms (profiles/kmer_wide_rate.txt, k = 21), before any merge", flush=True)

        # ---- the sets, and the screen against each ----------------------------------------------------------------------------------------
        kept = None
        for G in GENOMES:
            genome = step(lambda: packed_random(G // 4, 100 + G % 97))
            g_off, g_len = torch.zeros(1, device="cuda", dtype=torch.int64), torch.full((1,), G, device="cuda", dtype=torch.int32)
            gw = G - K + 1
            gc, gt = torch.empty(gw, dtype=torch.int64, device="cuda"), torch.empty(gw, dtype=torch.int64, device="cuda")
            made = []

            def build():
                ctx.code_kmer_codes(genome, g_off, None, g_len, K, True, cap=gw, codes=gc)
                ctx.sort_u64(gc, 2 * K, gt)
                made.append(ctx.kmer_set_from_sorted(gc, gw, K, canonical=True))
            t_build = timed(build)
            kset = made[0]
            info = kset.info
            del gc, gt
            torch.cuda.empty_cache()
            print(f"  a genome of {G} symbols: {info['codes']} codes, index of 2^{info['index_bits']} buckets, {info['device_bytes'] / 1e6:.1f} MB on "
                  f"the device; built (codes of one unit, sort, set) in {t_build:.2f} ms", flush=True)
            for share, name in ((0.0, "none of the reads from the genome"), (0.01, "1 % of the reads from the genome"), (1.0, "all reads from the genome")):
                if share:
                    step(lambda: plant(data, genome, reads, syms, int(reads * share), 7))
                    torch.cuda.synchronize()
                tot = step(lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out))
                t = rounds(reps, lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out))
                m = line("screen " + name, t, windows, f"   hits {int(tot[1])} ({100.0 * int(tot[1]) / windows:.3f} %), reads hit {int(tot[3])}")
                print(f"      {m / m_codes:5.2f} x codes;  {'under' if m < m_alt else 'OVER'} the sort-merge alternative's {m_alt:.2f} ms", flush=True)
            if G == GENOMES[1] and whole:
                kept = kset
            else:
                kset.free()
            del genome
            data = step(lambda: packed_random(reads * syms // 4, 1))        # (the reads as they were: random again)
        del data, out
        torch.cuda.empty_cache()

        # ---- the whole call ---------------------------------------------------------------------------------------------------------------
        if whole:
            text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
            img = step(lambda: ctx.dexta(text), 600)
            print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
            got, tk = None, []
            for r in range(reps + 1):
                ctx.sync(); t0 = time.perf_counter()
                got = step(lambda: ctx.screen("fasta", img, kept), 600)
                ctx.sync(); t1 = time.perf_counter()
                if r:
                    tk.append((t1 - t0) * 1e3)
            print(f"    Context.screen k={K}   median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f};  windows {got[0]['windows']}, "
                  f"hits {got[0]['hits']}, records hit {got[0]['records_hit']}", flush=True)
            os.environ["DEXGPU_TIMING"] = "1"                   # once more with the driver's stage marks (stderr)
            try:
                step(lambda: ctx.screen("fasta", img, kept), 600)
            finally:
                os.environ.pop("DEXGPU_TIMING", None)
            cut = text.index(b">", len(text) // 8)
            set_codes = kept.codes()
            sec, hits = host_route(ctx, text[:cut], set_codes, K)
            print(f"    today's route on one core, an eighth of the text ({cut / 1e9:.3f} GB): {sec:.1f} s, hits {hits}; scaled by "
                  f"{len(text) / cut:.2f}: {sec * len(text) / cut:.0f} s", flush=True)
            kept.free()


if __name__ == "__main__":
    main()
