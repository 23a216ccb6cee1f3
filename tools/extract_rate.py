"""Context.extract beside the route it replaces -- Context.subset, then undexta / undexqv of the image that made -- for 1 % of the
records of a synthetic .dexta and a synthetic .dexqv, whole records and an interval of each.

    python tools/extract_rate.py [READS] [ENTRIES] [MEAN] [REPS]

Both routes give the same text (asserted).  Times are wall-clock around the Python calls, host work, transfers and the read-back of
the text included: what a caller waits for.  The selection's ids rise, so that dx_file_subset takes it.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402


def timed(f, reps):
    out, ts = None, []
    for _ in range(reps + 1):                                  # (the first call is the warm-up)
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts[1:]


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    entries = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    mean = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    rng = np.random.Generator(np.random.PCG64(20261019))
    with api.Context(0) as ctx:
        for kind, n in (("fasta", reads), ("quiva", entries)):
            if kind == "fasta":
                text = synth.make_seqfile("fasta", n, seed=5, dist="fixed", mean=mean).text
                img = ctx.dexta(text)
                undex = lambda im: ctx.undexta(im, upper=True, width=80)      # noqa: E731
            else:
                text = synth.make_quiva(n, seed=5, dist="fixed", mean=mean).text
                img = ctx.dexqv(text)
                undex = lambda im: ctx.undexqv(im, upper=True)                       # noqa: E731
            ids = np.sort(rng.choice(n, max(n // 100, 1), replace=False)).astype(np.uint64)
            beg = rng.integers(0, mean // 2, len(ids)).astype(np.uint32)
            end = (beg + mean // 4).astype(np.uint32)
            print(f"{kind}: {n} records x {mean} symbols, image {len(img) / 1e6:.1f} MB, text {len(text) / 1e6:.1f} MB; {len(ids)} records selected; "
                  f"{reps} repetitions after one warm-up")
            for what, b, e in (("whole records", None, None), (f"intervals of {mean // 4}", beg, end)):
                got, t_new = timed(lambda: ctx.extract(kind, img, ids, b, e, upper=True, width=80), reps)
                want, t_old = timed(lambda: undex(ctx.subset(kind, img, ids, b, e)), reps)
                assert got == want, (kind, what)
                for name, t in (("extract", t_new), ("subset + undex", t_old)):
                    print(f"    {what:<20} {name:<16} median {np.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   text {len(got) / 1e6:.2f} MB   "
                          f"all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)


if __name__ == "__main__":
    main()
