"""Context.compare beside what the library offered for the same question before it -- two Context.digest(per_record=True) calls,
whose CRCs say WHICH records differ and no more -- on synthetic pairs of the sizes a store holds.

    python tools/compare_rate.py [ENTRIES] [READS] [MEAN] [REPS]

quiva: ENTRIES entries of about MEAN symbols (made on the device by dx_synth_quiva), encoded without and with -l; compared with
lossy=True, so the answer is "same".  fasta: READS reads of MEAN bases, encoded, against a copy with one payload byte changed.
The two routes take turns within one run, after one warm-up each.  Times are host clocks around the Python calls with the device
synchronised on both sides: host walks, transfers and read-backs included, what a caller waits for.  The spread over the
repetitions is printed with the median.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402


def quiva_text(ctx, n, mean, seed=20261019, movie="m000_000"):
    """n entries on the device (tools/digest_rate.py makes its corpus the same way), downloaded"""
    hlen = 1 + len(movie) + 1 + 8 + 1 + 7 + 1 + 7 + 6 + 3 + 1          # synth.header_text, fixed width
    lens = synth.lengths(n, seed, "lognormal", mean)
    hdr4 = synth.headers(n, seed, lens)
    start = np.concatenate([[0], np.cumsum(hlen + 5 * (lens.astype(np.uint64) + 1))]).astype(np.uint64)
    prof = synth.pacbio_profile()
    bufs = [ctx.alloc(int(start[n])), ctx.to_device(start[:n] + np.uint64(hlen)), ctx.to_device(lens), ctx.to_device(hdr4.reshape(-1)),
            ctx.to_device(prof.table().reshape(-1))]
    try:
        ctx.synth_quiva(seed, 0, n, bufs[1], bufs[2], bufs[3], bufs[4], prof.del_run, movie, bufs[0])
        return bufs[0].download(np.uint8, int(start[n])).tobytes()
    finally:
        for b in bufs:
            b.free()


def turns(ctx, runs, reps):
    """every route once for the warm-up, then `reps` rounds in which they take turns -> {name: [ms]}"""
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


def show(ms, text_bytes):
    for name, t in ms.items():
        med = float(np.median(t))
        print(f"    {name:<44} median {med:10.3f} ms  min {min(t):10.3f}  max {max(t):10.3f}  spread {100 * (max(t) - min(t)) / med:5.1f} %  "
              f"{text_bytes / med / 1e6:7.2f} GB/s of one text   all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)


def main():
    entries = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    reads = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
    mean = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    with api.Context(0) as ctx:
        if entries:
            text = quiva_text(ctx, entries, mean)
            a, b = ctx.dexqv(text), ctx.dexqv(text, lossy=True)
            print(f"quiva: {entries} entries of about {mean} symbols, {len(text) / 1e9:.3f} GB of text; images {len(a) / 1e9:.3f} and {len(b) / 1e9:.3f} GB; "
                  f"{reps} repetitions after one warm-up, taking turns")
            n_text = len(text)
            del text
            r = ctx.compare("quiva", a, b, lossy=True)
            assert r["same"] and r["records_a"] == entries, r
            assert not ctx.compare("quiva", a, b)["same"]
            show(turns(ctx, {"compare(lossy=True)": lambda: ctx.compare("quiva", a, b, lossy=True),
                             "compare(lossy=True, per_record=True)": lambda: ctx.compare("quiva", a, b, lossy=True, per_record=True),
                             "two digest(per_record=True)": lambda: (ctx.digest("quiva", a, per_record=True), ctx.digest("quiva", b, per_record=True))},
                       reps), n_text)
        if reads:
            text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=mean).text
            a = ctx.dexta(text)
            hurt = bytearray(a)
            hurt[len(hurt) // 2] ^= 0x40                           # (inside some read's packed bases)
            b = bytes(hurt)
            print(f"fasta: {reads} reads of {mean} bases, {len(text) / 1e9:.3f} GB of text; images of {len(a) / 1e9:.3f} GB; "
                  f"{reps} repetitions after one warm-up, taking turns")
            n_text = len(text)
            del text
            r = ctx.compare("fasta", a, b)
            assert not r["same"] and r["records_differ"] == 1 and int(r["differ"][0]) == 1, r
            da, db = ctx.digest("fasta", a, upper=True, per_record=True), ctx.digest("fasta", b, upper=True, per_record=True)
            assert list(np.flatnonzero(da["rec_crc"] != db["rec_crc"])) == [r["first_record"]]
            show(turns(ctx, {"compare": lambda: ctx.compare("fasta", a, b),
                             "compare(per_record=True)": lambda: ctx.compare("fasta", a, b, per_record=True),
                             "two digest(per_record=True)": lambda: (ctx.digest("fasta", a, upper=True, per_record=True),
                                                                     ctx.digest("fasta", b, upper=True, per_record=True))},
                       reps), n_text)


if __name__ == "__main__":
    main()
