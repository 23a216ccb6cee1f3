"""dx_code_kmers beside the walk it shares with dx_code_counts, its two counting routes on both sides of the cut between them, and
Context.kmers beside what a user has today -- the whole text by dx_file_unpack2 and a count of it on one core.

    python tools/kmer_rate.py [READS] [SYMS] [REPS]

Part 1, the kernel alone: READS reads of SYMS symbols (100 000 x 10 000: 10^9 positions, 0.25 GB packed) stand on the device with
their units, and dx_code_kmers is timed with HIP events on the context's stream -- one warm-up, then REPS (5) rounds in which the
cases take turns, median, min, max and spread reported:

    uniform     uniform random symbols, k = 4, 7 (the LDS route's last), 8 (the global route's first), 11, 14, plain and canonical
    runs        every symbol repeats its predecessor with probability 0.5, k = 14, with the consecutive-merge and without
                (DEXGPU_TEST=kmer_merge=0)
    counts      dx_code_counts over the same units: the floor of the walk

For the global route the atomic requests a second follow from the windows and the share of them that differs from its predecessor
(1 - 4^-k uniform, 1 - 0.625^k with the runs: a window equals the one before it when k + 1 symbols in a row are equal).
The table (2 GiB at k = 14) is zeroed outside the timed stretch; its spectrum and list are timed once each.

Part 2, whole calls on a .dexta of the same shape, host clocks with the device synchronised on both sides: Context.kmers at k = 14
(host walk, upload, table, count, spectrum, read-backs: what a caller waits for) beside dx_file_unpack2 to upper-case text and a
count of the text's 14-mers with numpy on one core (letters -> codes, 14 shifted adds, bincount into 4^14 cells) -- the count is
timed on the first READS / 8 reads and multiplied by 8, which is said in the output.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def packed_reads(reads, syms, runs, seed):
    """reads x syms symbols packed four a byte on the device (uint8 tensor); runs: a symbol repeats its predecessor with p = 0.5"""
    assert syms % 4 == 0
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(reads * syms // 4, dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 24) // syms)
    for r0 in range(0, reads, step):
        n = (min(reads, r0 + step) - r0) * syms
        s = torch.randint(0, 4, (n,), generator=g, device="cuda", dtype=torch.int64)
        if runs:
            fresh = torch.rand(n, generator=g, device="cuda") >= 0.5
            fresh[0] = True
            last = torch.cummax(torch.where(fresh, torch.arange(n, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")), 0).values
            s = s[last]
        s = s.view(-1, 4)
        out[r0 * syms // 4:r0 * syms // 4 + n // 4] = ((s[:, 0] << 6) | (s[:, 1] << 4) | (s[:, 2] << 2) | s[:, 3]).to(torch.uint8)
    return out


def report(name, t, positions, floor=None, share=None):
    m = float(np.median(t))
    line = (f"    {name:<28} median {m:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  spread {100 * (max(t) - min(t)) / m:5.1f} %   "
            f"{positions / m / 1e6:8.2f} G positions/s")
    if floor:
        line += f"   {m / floor:6.2f} x counts"
    if share is not None:
        line += f"   {share * positions / m / 1e6:7.2f} G atomic requests/s"
    print(line, flush=True)
    return m


def one_core_count(text_lines, k):
    """the k-mers of upper-case reads, one a line, counted with numpy: the table (one bincount for all reads: 4^14 cells are not
    walked once a read)"""
    lut = np.zeros(256, np.int64)
    for c, l in enumerate(b"ACGT"):
        lut[l] = c
    all_codes = []
    for line in text_lines:
        s = lut[np.frombuffer(line, np.uint8)]
        if len(s) < k:
            continue
        code = np.zeros(len(s) - k + 1, np.int64)
        for i in range(k):
            code = code * 4 + s[i:i + len(code)]
        all_codes.append(code)
    return np.bincount(np.concatenate(all_codes), minlength=4 ** k)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    torch.cuda.init()
    print(f"device: {torch.cuda.get_device_name(0)}")
    positions = reads * syms
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        # ---- part 1: the kernel alone ---------------------------------------------------------------------------------------------------
        boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
        ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
        data = {"uniform": packed_reads(reads, syms, False, 1), "runs": packed_reads(reads, syms, True, 2)}
        table = torch.zeros(4 ** 14, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print(f"{reads} reads of {syms} symbols: {positions / 1e9:.3f} G positions, {positions / 4e9:.3f} GB packed; {reps} rounds after one "
              f"warm-up, taking turns; events on the context's stream, the table zeroed outside them", flush=True)

        class V:
            def __init__(self, t): self.ptr, self.nbytes = t.data_ptr(), t.numel() * t.element_size()

        def counts(which):
            return lambda: ctx.code_counts(V(data[which]), data[which].numel(), V(boff), None, V(ln), reads)

        def kmers(which, k, canonical, merge=True):
            def f():
                if not merge:
                    os.environ["DEXGPU_TEST"] = "kmer_merge=0"
                try:
                    ctx.code_kmers(data[which], boff, None, ln, k, canonical, table[:4 ** k])
                finally:
                    os.environ.pop("DEXGPU_TEST", None)
            return f

        cases = {"counts uniform": (counts("uniform"), None), "counts runs": (counts("runs"), None)}
        for k in (4, 7, 8, 11, 14):
            for canonical in (False, True):
                cases[f"uniform k={k}{' canonical' if canonical else ''}"] = (kmers("uniform", k, canonical), (k, 1 - 4.0 ** -k))
        cases["runs k=14"] = (kmers("runs", 14, False), (14, 1 - 0.625 ** 14))
        cases["runs k=14 no merge"] = (kmers("runs", 14, False, merge=False), (14, 1.0))
        cases["runs k=7"] = (kmers("runs", 7, False), (7, None))
        cases["runs k=7 no merge"] = (kmers("runs", 7, False, merge=False), (7, None))
        ev = {name: [] for name in cases}
        for r in range(reps + 1):
            for name, (f, _) in cases.items():
                table.zero_()
                torch.cuda.synchronize()
                t = timed(f)
                if r:
                    ev[name].append(t)
        floor = {w: report(f"counts {w}", ev[f"counts {w}"], positions) for w in ("uniform", "runs")}
        med = {}
        for name, (_, info) in cases.items():
            if info is None:
                continue
            k, share = info
            med[name] = report(name, ev[name], positions - reads * (k - 1), floor[name.split()[0]], share if k > 7 else None)
        print(f"    the estimate of csrc/kmers/dx_kmers.hip for the global route: 20 G requests/s, 50 ms for 10^9 windows at k = 14; "
              f"measured: {med['uniform k=14']:.1f} ms for {(positions - reads * 13) / 1e9:.3f} G windows", flush=True)

        # the spectrum and the list of the k = 14 table of the uniform reads
        table.zero_(); torch.cuda.synchronize()
        kmers("uniform", 14, False)()
        ts = [timed(lambda: ctx.kmer_spectrum(table, 14, 256)) for _ in range(reps + 1)][1:]
        tl = [timed(lambda: ctx.kmer_list(table, 14, 1 << 40, 0)) for _ in range(reps + 1)][1:]
        sp = ctx.kmer_spectrum(table, 14, 256)
        print(f"    spectrum of 4^14 cells        median {np.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}   {2 ** 31 / np.median(ts) / 1e6:8.1f} GB/s"
              f"   (distinct {sp['distinct']}, max_count {sp['max_count']})")
        print(f"    list of 4^14 cells, counting  median {np.median(tl):9.3f} ms  min {min(tl):9.3f}  max {max(tl):9.3f}   {2 ** 31 / np.median(tl) / 1e6:8.1f} GB/s", flush=True)
        del data, table
        torch.cuda.empty_cache()

        # ---- part 2: whole calls --------------------------------------------------------------------------------------------------------
        text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
        img = ctx.dexta(text)
        print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
        del text
        got, tk, tu = None, [], []
        for r in range(reps + 1):
            ctx.sync(); t0 = time.perf_counter()
            got = ctx.kmers("fasta", img, 14)
            ctx.sync(); t1 = time.perf_counter()
            flat = ctx.undexta(img, upper=True, width=2**31 - 1)
            ctx.sync(); t2 = time.perf_counter()
            if r:
                tk.append((t1 - t0) * 1e3); tu.append((t2 - t1) * 1e3)
        part = max(1, reads // 8)
        body = flat.split(b"\n", 2 * part)[1:2 * part:2]
        t0 = time.perf_counter()
        host = one_core_count(body, 14)
        tc = (time.perf_counter() - t0) * 1e3
        print(f"    kmers k=14   median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f}  spread {100 * (max(tk) - min(tk)) / np.median(tk):5.1f} %")
        print(f"    unpack       median {np.median(tu):10.3f} ms  min {min(tu):10.3f}  max {max(tu):10.3f}  spread {100 * (max(tu) - min(tu)) / np.median(tu):5.1f} %")
        print(f"    one-core count (numpy) of the first {part} reads: {tc:.1f} ms once; x {reads / part:.0f} for the whole text: {tc * reads / part:.0f} ms (scaled, not run)")
        print(f"    kmers / (unpack + count): {np.median(tk) / (np.median(tu) + tc * reads / part):.4f};  windows {got[0]['windows']}, distinct {got[0]['distinct']}, "
              f"max_count {got[0]['max_count']}; the first {part} reads hold {int(host.sum())} windows, {int((host > 0).sum())} distinct", flush=True)


if __name__ == "__main__":
    main()
