"""The CRC kernels (csrc/digest/dx_crc.hip) and dx_file_digest beside the passes they follow, on the synthetic .quiva corpus.

N entries of about MEAN symbols (1 M x 10 000: 50 GB of text, made on the device by dx_synth_quiva) stand on the device, as a decoder
would have left them.  Timed in one process, on the same buffers, REPS repetitions each after one warm-up, taking turns:

    (a) dx_verify_ranges, the text against a copy of it, a unit a record       the yardstick: a read-only pass, 2 bytes read a byte
    (b) dx_crc32_ranges, the text as ONE unit                                  split over all workgroups
    (c) dx_crc32_ranges, a unit a record (N units of about 50 KB)              a wave a unit
    (d) dx_crc32_ranges, a unit a line (6 N units: 38 bytes or about 10 KB)    a wave a data line, a lane a header line
    (e) dx_crc32_fold of 2 N (crc, length) pairs

and, on the first E entries of the corpus (their text downloaded, their image made by dx_file_dexqv):

    (f) dx_file_undexqv_plan + _run into a sink that drops what it gets        the yardstick: decode, download, header lines
    (g) dx_file_digest of the same image                                       decode, hash; nothing comes back

    python tools/digest_rate.py [N] [MEAN] [REPS] [E]

(a) - (e) are HIP events on the stream the context issues on, one call each: the call's own memsets included, and its read-back.
(f) and (g) are wall-clock times of the calls.  (b), (c) and (d) are checked against each other through (e) -- the fold of the
records' and of the lines' CRCs is the one unit's CRC -- and against zlib.crc32 of the text of the first E entries.
"""
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import _lib as L      # noqa: E402
from dextractor_amd import api, synth     # noqa: E402


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    mean = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    few = min(n, int(sys.argv[4]) if len(sys.argv) > 4 else 20000)
    seed, movie = 20261003, "m000_000"
    hlen = 1 + len(movie) + 1 + 8 + 1 + 7 + 1 + 7 + 6 + 3 + 1          # synth.header_text, fixed width
    lens = synth.lengths(n, seed, "lognormal", mean)
    hdr4 = synth.headers(n, seed, lens)
    rec = hlen + 5 * (lens.astype(np.uint64) + 1)
    start = np.concatenate([[0], np.cumsum(rec)]).astype(np.uint64)   # where every record begins; [n]: the text's bytes
    total = int(start[n])
    prof = synth.pacbio_profile()
    torch.cuda.init()
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        d_text, d_copy = ctx.alloc(total), ctx.alloc(total)
        d_off, d_len = ctx.to_device(start[:n] + np.uint64(hlen)), ctx.to_device(lens)
        d_hdr4, d_lut = ctx.to_device(hdr4.reshape(-1)), ctx.to_device(prof.table().reshape(-1))
        ctx.synth_quiva(seed, 0, n, d_off, d_len, d_hdr4, d_lut, prof.del_run, movie, d_text)
        ctx.synth_quiva(seed, 0, n, d_off, d_len, d_hdr4, d_lut, prof.del_run, movie, d_copy)      # (the same text once more)
        ctx.sync()

        # the units: the whole text; the records; the lines (a header line and five data lines a record)
        line_off = np.empty((n, 6), np.uint64)
        line_len = np.empty((n, 6), np.uint64)
        line_off[:, 0], line_len[:, 0] = start[:n], hlen
        for k in range(5):
            line_off[:, 1 + k] = start[:n] + np.uint64(hlen) + np.uint64(k) * (lens.astype(np.uint64) + 1)
            line_len[:, 1 + k] = lens.astype(np.uint64) + 1
        units = {"b": (np.zeros(1, np.uint64), np.array([total], np.uint64)),
                 "c": (start[:n].copy(), rec.copy()),
                 "d": (line_off.reshape(-1), line_len.reshape(-1))}
        dev = {k: (ctx.to_device(o), ctx.to_device(ln), ctx.alloc(4 * len(o)), len(o)) for k, (o, ln) in units.items()}
        d_rlen32 = ctx.to_device(rec.astype(np.uint32))
        d_pcrc = ctx.to_device(np.random.default_rng(1).integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32))
        d_plen = ctx.to_device(np.repeat(rec // 2, 2))
        runs = {"a": lambda: ctx.verify_ranges(d_text, dev["c"][0], d_rlen32, d_copy, dev["c"][0], d_rlen32, n),
                "b": lambda: ctx.crc32_ranges(d_text, total, *dev["b"][:2], 1, dev["b"][2]),
                "c": lambda: ctx.crc32_ranges(d_text, total, *dev["c"][:2], n, dev["c"][2]),
                "d": lambda: ctx.crc32_ranges(d_text, total, *dev["d"][:2], 6 * n, dev["d"][2]),
                "e": lambda: ctx.crc32_fold(d_pcrc, d_plen, 2 * n)}
        # warm-up, and the three ways to the one CRC
        assert runs["a"]()[0] is None
        for k in "bcd":
            runs[k]()
        runs["e"]()
        one = int(dev["b"][2].download(np.uint32, 1)[0])
        assert ctx.crc32_fold(dev["c"][2], dev["c"][1], n) == (one, total)
        assert ctx.crc32_fold(dev["d"][2], dev["d"][1], 6 * n) == (one, total)
        some = int(start[few])
        text = d_text.download(np.uint8, some).tobytes()
        assert ctx.crc32_fold(dev["c"][2], dev["c"][1], few) == (zlib.crc32(text), some)
        ms = {name: [] for name in runs}
        for _ in range(reps):
            for name in runs:
                ms[name].append(timed(runs[name]))
        what = {"a": "dx_verify_ranges, text against its copy, a unit a record", "b": "dx_crc32_ranges, one unit",
                "c": f"dx_crc32_ranges, {n} units (records)", "d": f"dx_crc32_ranges, {6 * n} units (lines)",
                "e": f"dx_crc32_fold, {2 * n} pairs"}
        print(f"{n} entries, mean {mean} symbols, {total / 1e9:.2f} GB of text, {reps} repetitions after one warm-up, taking turns")
        for name in runs:
            t = ms[name]
            med = float(np.median(t))
            rate = f"{total / med / 1e9:6.2f} TB/s of text" if name != "e" else f"{2 * n / med / 1e3:6.1f} M pairs/s"
            print(f"({name}) {what[name]:<60} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  {rate}   "
                  f"all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)
        for b in (d_copy, d_pcrc, d_plen, d_rlen32, *[x for v in dev.values() for x in v[:3]]):
            b.free()

        # ---- the driver, end to end, on the first `few` entries ----
        img = ctx.dexqv(text)
        wall = {"f": [], "g": []}
        drop = L.SINK_FN(lambda user, data, nbytes, at: 0)      # (takes a chunk and lets it go: no copy on this side)
        got = None
        for r in range(reps + 1):
            plan, size = C.c_void_p(), C.c_size_t()
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.dx_file_undexqv_plan_on(ctx.h, img, len(img), C.byref(plan), C.byref(size)))
            ctx._chk(ctx.lib.dx_file_undexqv_run(ctx.h, plan, 1, drop, None))
            ctx.lib.dx_file_undexqv_plan_free(plan)
            t1 = time.perf_counter()
            got = ctx.digest("quiva", img, upper=True)
            t2 = time.perf_counter()
            assert size.value == some
            if r:
                wall["f"].append((t1 - t0) * 1e3); wall["g"].append((t2 - t1) * 1e3)
        assert (got["crc32"], got["bytes"], got["records"]) == (zlib.crc32(text), some, few), got
        print(f"the first {few} entries: {some / 1e9:.3f} GB of text, an image of {len(img) / 1e9:.3f} GB")
        for name, w in (("f", "dx_file_undexqv_plan + _run, the text dropped"), ("g", "dx_file_digest")):
            t = wall[name]
            med = float(np.median(t))
            print(f"({name}) {w:<60} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  {some / med / 1e6:6.2f} GB/s of text   "
                  f"all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)


if __name__ == "__main__":
    main()
