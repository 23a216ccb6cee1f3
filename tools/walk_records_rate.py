"""k_walk_records (records at known starts) beside k_walk_pieces (the walk of a framed stream) on the same records.

Makes the bench workload's corpus on the device (N entries, lognormal around 10 kb), encodes it twice with the tables of
one scan -- with framing bytes (a .dexqv's record stream) and without (a .qvs track: the bare stream, d_rec_off = every
entry's start) -- and runs each walk REPS times.  Meant to run under the profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/walk_records_rate.py [N] [REPS] [both|records|pieces]

whose kernel statistics have the two kernels' times; the script's own lines (host clock around a call that ends in a
synchronise: tables up, scratch, launch, answer back) are the calls' times, not the kernels'.  It also checks that the two
walks agree on every segment size.  `pieces` runs the walk of the framed stream alone and uses nothing newer than it, so the
same file also measures k_walk_pieces in a tree that has no k_walk_records yet.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import api, synth          # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    which = sys.argv[3] if len(sys.argv) > 3 else "both"
    assert which in ("both", "records", "pieces")
    seed, movie = 20261003, "m000_000"
    hlen = 1 + len(movie) + 1 + 8 + 1 + 7 + 1 + 7 + 6 + 3 + 1
    lens = synth.lengths(n, seed, "lognormal", 10000)
    hdr4 = synth.headers(n, seed, lens, 0)
    rec_bytes = hlen + 5 * (lens.astype(np.uint64) + 1)
    off = (np.concatenate([[0], np.cumsum(rec_bytes)[:-1]]) + hlen).astype(np.uint64)
    text_bytes = int(rec_bytes.sum())
    prof = synth.pacbio_profile()
    with api.Context(0) as ctx:
        d_text = ctx.alloc(text_bytes + 64)
        d_off, d_len = ctx.to_device(off), ctx.to_device(lens)
        ctx.synth_quiva(seed, 0, n, d_off, d_len, ctx.to_device(hdr4.reshape(-1)), ctx.to_device(prof.table().reshape(-1)),
                        prof.del_run, movie, d_text)
        batch = ctx.qv_batch(d_text, d_off, d_len, n, text_bytes=text_bytes + 64)
        p, hist, tot = ctx.qv_scan(batch, 0)
        coding = api.qv_build(hist, tot, p, False)
        ctx.qv_set_coding(coding, False)
        blob, hoff, _ = api.frame_headers(hdr4, None, 0)
        d_hdr, d_hoff = ctx.to_device(blob), ctx.to_device(hoff)
        cap = int(hoff[-1]) + api.qv_out_bound(hist, n, coding, False) + 4096
        d_seg, d_rec, d_framed = ctx.alloc(20 * n), ctx.alloc(8 * (n + 1)), ctx.alloc(cap)
        framed = ctx.qv_encode_onepass(batch, d_hdr, d_hoff, d_seg, d_rec, d_framed, cap)
        want = d_seg.download(np.uint32, 5 * n)
        print(f"{n} entries, {int(lens.sum())} symbols: framed stream {framed} bytes", flush=True)
        if which != "pieces":
            d_seg2, d_start, d_bare = ctx.alloc(20 * n), ctx.alloc(8 * (n + 1)), ctx.alloc(cap)
            p, hist, tot = ctx.qv_scan(batch, 0)               # (the encoder takes the tokens of the scan just before it)
            bare = ctx.qv_encode_onepass(batch, None, None, d_seg2, d_start, d_bare, cap)
            assert (d_seg2.download(np.uint32, 5 * n) == want).all() and bare == framed - int(hoff[-1])
            print(f"bare stream {bare} bytes", flush=True)
            d_got = ctx.alloc(20 * n)
        d_text.free()
        for r in range(reps if which != "pieces" else 0):
            d_got.zero(); ctx.sync()
            t = time.perf_counter()
            ctx.qv_walk_records_device(d_bare, bare, d_start, d_len, n, coding, d_got)
            ms = (time.perf_counter() - t) * 1e3
            ok = bool((d_got.download(np.uint32, 5 * n) == want).all())
            print(f"dx_qv_walk_records_device call {r}: {ms:.2f} ms, sizes {'agree' if ok else 'DIFFER'}", flush=True)
            assert ok
        if which == "records":
            return
        for r in range(reps):
            t = time.perf_counter()
            dix = ctx.qv_walk_device(d_framed, framed, 0, coding, 1, 0)
            ms = (time.perf_counter() - t) * 1e3
            ok = dix.n == n and bool((dix.download()["seg"].reshape(-1) == want).all()) if r == 0 else dix.n == n
            dix.free()
            print(f"dx_qv_walk_device call {r}: {ms:.2f} ms, {'agrees' if ok else 'DIFFERS'}", flush=True)
            assert ok


if __name__ == "__main__":
    main()
