"""What a file costs on the sharded file drivers, end to end: the thread scaffolding, the host's part and the transfers included.

One synthetic .quiva file (ENTRIES entries of about 2000 symbols: 300 MB at the default) and one .fasta file (READS reads of about
10 000 symbols: 300 MB) are made once, outside the timed region (kept in CACHE when one is named, and read from there the next time).
Over contexts that all stand on device 0:

    (a) api.dexqv_sharded, 2 contexts, by entries      the file's host index first (DEXGPU_TEST=shard_bytes_min above the file's size)
    (b) api.dexqv_sharded, 2 contexts, by bytes        every shard indexes its own byte range (the default threshold: 64 MiB a shard)
    (c) api.dexqv_sharded, 4 contexts, by entries
    (d) api.dexqv_sharded, 4 contexts, by bytes
    (e) api.pack2_sharded, 4 contexts                  dexta of the .fasta file

    python tools/shard_times.py [ENTRIES] [READS] [REPS] [CACHE]

Times are the host's clock around the call, which returns with the image in host memory (its last device call is a download that
waits); REPS repetitions of every line after one warm-up, the lines taking turns.  The warm-up's image is hashed, and (a) to (d)
must agree on it.  DEXGPU_LIB selects another build of the library.
"""
import hashlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth     # noqa: E402


def cached(path, make):
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    data = make()
    if path:
        with open(path, "wb") as f:
            f.write(data)
    return data


def main():
    entries = int(sys.argv[1]) if len(sys.argv) > 1 else 30000
    reads = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cache = sys.argv[4] if len(sys.argv) > 4 else None
    quiva = cached(cache and os.path.join(cache, f"shard_times_{entries}.quiva"), lambda: synth.make_quiva(entries, seed=20261019, mean=2000).text)
    fasta = cached(cache and os.path.join(cache, f"shard_times_{reads}.fasta"), lambda: synth.make_seqfile("fasta", reads, seed=20261019, mean=10000).text)
    cs = [api.Context(0) for _ in range(4)]
    plain = os.environ.get("DEXGPU_TEST")
    by_entries = (plain + "," if plain else "") + f"shard_bytes_min={1 << 40}"

    def dexqv(nctx, flags):
        def run():
            if flags is None:
                os.environ.pop("DEXGPU_TEST", None)
            else:
                os.environ["DEXGPU_TEST"] = flags
            try:
                return api.dexqv_sharded(cs[:nctx], quiva, 0)
            finally:
                if plain is None:
                    os.environ.pop("DEXGPU_TEST", None)
                else:
                    os.environ["DEXGPU_TEST"] = plain
        return run

    runs = {"a": ("api.dexqv_sharded, 2 contexts, by entries", dexqv(2, by_entries)),
            "b": ("api.dexqv_sharded, 2 contexts, by bytes", dexqv(2, plain)),
            "c": ("api.dexqv_sharded, 4 contexts, by entries", dexqv(4, by_entries)),
            "d": ("api.dexqv_sharded, 4 contexts, by bytes", dexqv(4, plain)),
            "e": ("api.pack2_sharded, 4 contexts", lambda: api.pack2_sharded(cs, fasta))}
    try:
        digest = {name: hashlib.sha1(run()).hexdigest() for name, (_, run) in runs.items()}      # the warm-up calls
        assert len({digest[k] for k in "abcd"}) == 1, digest
        ms = {name: [] for name in runs}
        for _ in range(reps):
            for name, (_, run) in runs.items():
                t0 = time.perf_counter()
                run()
                ms[name].append((time.perf_counter() - t0) * 1e3)
    finally:
        for c in cs:
            c.close()
    print(f".quiva {len(quiva) / 1e6:.1f} MB in {entries} entries, .fasta {len(fasta) / 1e6:.1f} MB in {reads} reads, "
          f"{reps} repetitions after one warm-up, taking turns; library: {os.path.basename(os.environ.get('DEXGPU_LIB', 'libdexgpu.so'))}")
    for name, (what, _) in runs.items():
        t = ms[name]
        size = len(fasta) if name == "e" else len(quiva)
        print(f"({name}) {what:<44} median {float(np.median(t)):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}  "
              f"{size / float(np.median(t)) / 1e6:6.2f} GB/s of text   sha1 {digest[name][:12]}   all: {' '.join(f'{x:.2f}' for x in t)}", flush=True)


if __name__ == "__main__":
    main()
