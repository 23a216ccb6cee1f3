"""The census kernels (csrc/census/dx_census.hip) beside the passes they replace or follow.

Part 1, the workload of tools/reads_rate.py: N reads of SYMS symbols (1 M x 10 000: 2.5 GB packed, random) stand on the device.

    (a) dx_reads_unpack, DX_LETTERS_NUMBERS, whole reads           the decode a count replaces: reads 2.5 GB, writes 10 GB
    (b) dx_code_counts, the same units, every unit's four counts   reads the same 2.5 GB, writes 16 MB
    (c) dx_code_counts, totals only

Part 2, the workload of tools/digest_rate.py: N entries of about MEAN symbols (1 M x 10 000: 50 GB of .quiva text, made on the device
by dx_synth_quiva) stand on the device, as a decoder would have left them; the units are every entry's five lines, newlines left out.

    (d) dx_verify_ranges, the lines against a copy of the text     a read-only pass, 2 bytes read a byte
    (e) dx_crc32_ranges, 5 N lines
    (f) dx_byte_hist_ranges, 5 N lines, kinds 0..4, every line's sum
    (g) dx_byte_hist_ranges, the same, no sums

    python tools/census_rate.py [N] [SYMS] [REPS] [E]

Every figure is HIP events on the stream the context issues on, one call each -- the call's own memsets, its ticket kernel and its
read-back included --, REPS (5) repetitions after one warm-up, the calls of a part taking turns; the median is what counts.  The
warm-up calls are checked: (b) against the counts of the first reads and the totals of the whole payload taken here, (f) against
np.bincount over the text of the first E entries, (g) against (f).  The one relation fixed in advance: (b)'s median is no longer
than (a)'s -- a count slower than the decode it replaces has no reason to exist.
"""
import os
import sys

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


def report(runs, what, ms, unit_bytes, unit):
    for name in runs:
        t = ms[name]
        med = float(np.median(t))
        print(f"({name}) {what[name]:<62} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  "
              f"{unit_bytes / med / 1e9:6.2f} TB/s {unit}   all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)


def reads_part(ctx, n, syms, reps):
    assert syms % 4 == 0
    clen = syms // 4
    rng = np.random.Generator(np.random.PCG64(20261018))
    block_reads = min(n, 10000)
    block = rng.integers(0, 256, block_reads * clen, dtype=np.uint8)          # the payload: this block, over and over
    d_in = ctx.alloc(n * clen)
    for r0 in range(0, n, block_reads):
        m = min(block_reads, n - r0)
        ctx._chk(ctx.lib.dx_h2d(ctx.h, d_in.ptr + r0 * clen, block.ctypes.data, m * clen))
    idx = np.arange(n, dtype=np.uint64)
    d_boff, d_len, d_ooff = ctx.to_device(idx * np.uint64(clen)), ctx.to_device(np.full(n, syms, np.uint32)), ctx.to_device(idx * np.uint64(syms + 1))
    d_out, d_cnt = ctx.alloc(n * (syms + 1)), ctx.alloc(16 * n)
    tot = {}
    runs = {"a": lambda: ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d_in, n * clen, d_boff, None, d_len, n, d_out, d_ooff),
            "b": lambda: tot.__setitem__("b", ctx.code_counts(d_in, n * clen, d_boff, None, d_len, n, d_cnt)),
            "c": lambda: tot.__setitem__("c", ctx.code_counts(d_in, n * clen, d_boff, None, d_len, n, None))}
    for name in runs:
        runs[name]()
    ctx.sync()
    # the warm-up calls' answers, against the counts taken here
    sym = ((block[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).reshape(block_reads, syms)
    per = np.stack([(sym == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint64)
    got = d_cnt.download(np.uint32, 4 * n).reshape(n, 4)
    assert (got[:block_reads] == per).all() and (got[n - block_reads:] == np.roll(per, -((n - block_reads) % block_reads), axis=0)).all()
    whole = per.sum(axis=0) * np.uint64(n // block_reads) + per[:n % block_reads].sum(axis=0)
    assert list(tot["b"]) == list(whole) and list(tot["c"]) == list(whole), (tot, whole)
    ms = {name: [] for name in runs}
    for _ in range(reps):
        for name in runs:
            ms[name].append(timed(runs[name]))
    what = {"a": "dx_reads_unpack, numbers, whole reads", "b": "dx_code_counts, every unit's counts", "c": "dx_code_counts, totals only"}
    print(f"{n} reads x {syms} symbols, {n * clen / 1e9:.2f} GB packed, {reps} repetitions after one warm-up, taking turns")
    report(runs, what, ms, n * clen, "of packed bytes read")
    a, b = float(np.median(ms["a"])), float(np.median(ms["b"]))
    print(f"(b) / (a) medians: {b / a:.3f}: dx_code_counts takes {'no longer than' if b <= a else 'LONGER than'} the decode it replaces")
    for buf in (d_in, d_boff, d_len, d_ooff, d_out, d_cnt):
        buf.free()


def lines_part(ctx, n, mean, reps, few):
    seed, movie = 20261003, "m000_000"
    hlen = 1 + len(movie) + 1 + 8 + 1 + 7 + 1 + 7 + 6 + 3 + 1          # synth.header_text, fixed width
    lens = synth.lengths(n, seed, "lognormal", mean)
    hdr4 = synth.headers(n, seed, lens)
    rec = hlen + 5 * (lens.astype(np.uint64) + 1)
    start = np.concatenate([[0], np.cumsum(rec)]).astype(np.uint64)   # where every record begins; [n]: the text's bytes
    total = int(start[n])
    prof = synth.pacbio_profile()
    d_text, d_copy = ctx.alloc(total), ctx.alloc(total)
    d_off, d_len = ctx.to_device(start[:n] + np.uint64(hlen)), ctx.to_device(lens)
    d_hdr4, d_lut = ctx.to_device(hdr4.reshape(-1)), ctx.to_device(prof.table().reshape(-1))
    ctx.synth_quiva(seed, 0, n, d_off, d_len, d_hdr4, d_lut, prof.del_run, movie, d_text)
    ctx.synth_quiva(seed, 0, n, d_off, d_len, d_hdr4, d_lut, prof.del_run, movie, d_copy)      # (the same text once more)
    ctx.sync()
    line_off = np.empty((n, 5), np.uint64)
    for k in range(5):
        line_off[:, k] = start[:n] + np.uint64(hlen) + np.uint64(k) * (lens.astype(np.uint64) + 1)
    line_len = np.repeat(lens.astype(np.uint64), 5)
    body = int(line_len.sum())
    d_loff, d_llen, d_llen32 = ctx.to_device(line_off.reshape(-1)), ctx.to_device(line_len), ctx.to_device(line_len.astype(np.uint32))
    d_kind = ctx.to_device(np.tile(np.arange(5, dtype=np.uint8), n))
    d_crc, d_sum = ctx.alloc(4 * 5 * n), ctx.alloc(8 * 5 * n)
    hist = {}
    runs = {"d": lambda: ctx.verify_ranges(d_text, d_loff, d_llen32, d_copy, d_loff, d_llen32, 5 * n),
            "e": lambda: ctx.crc32_ranges(d_text, total, d_loff, d_llen, 5 * n, d_crc),
            "f": lambda: hist.__setitem__("f", ctx.byte_hist_ranges(d_text, total, d_loff, d_llen, d_kind, 5, 5 * n, d_sum)),
            "g": lambda: hist.__setitem__("g", ctx.byte_hist_ranges(d_text, total, d_loff, d_llen, d_kind, 5, 5 * n, None))}
    assert runs["d"]()[0] is None
    for name in "efg":
        runs[name]()
    ctx.sync()
    assert (hist["f"] == hist["g"]).all() and int(hist["f"].sum()) == body
    # ... and the first `few` entries' lines against bincount, table by table, and their sums
    text = d_text.download(np.uint8, int(start[few]))
    some = ctx.byte_hist_ranges(d_text, total, d_loff, d_llen, d_kind, 5, 5 * few, d_sum)
    sums = d_sum.download(np.uint64, 5 * few)
    want = np.zeros((5, 256), np.uint64)
    for i in range(few):
        for k in range(5):
            part = text[int(line_off[i, k]): int(line_off[i, k]) + int(lens[i])]
            want[k] += np.bincount(part, minlength=256).astype(np.uint64)
            assert int(part.sum(dtype=np.uint64)) == int(sums[5 * i + k]), (i, k)
    assert (some == want).all()
    ms = {name: [] for name in runs}
    for _ in range(reps):
        for name in runs:
            ms[name].append(timed(runs[name]))
    what = {"d": f"dx_verify_ranges, {5 * n} lines against their copy", "e": f"dx_crc32_ranges, {5 * n} lines",
            "f": f"dx_byte_hist_ranges, {5 * n} lines, 5 tables, sums", "g": "dx_byte_hist_ranges, the same, no sums"}
    print(f"{n} entries, mean {mean} symbols, {total / 1e9:.2f} GB of text, {body / 1e9:.2f} GB in the lines, {reps} repetitions after one warm-up, taking turns")
    report(runs, what, ms, body, "of line bytes")
    top = [int(np.argmax(hist["f"][k])) for k in range(5)]
    print("the busiest value of each table and its share: " +
          ", ".join(f"{'del tag ins mrg sub'.split()[k]} {top[k]} {hist['f'][k][top[k]] / hist['f'][k].sum():.2f}" for k in range(5)))
    for buf in (d_text, d_copy, d_off, d_len, d_hdr4, d_lut, d_loff, d_llen, d_llen32, d_kind, d_crc, d_sum):
        buf.free()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    few = min(n, int(sys.argv[4]) if len(sys.argv) > 4 else 200)
    torch.cuda.init()
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        reads_part(ctx, n, syms, reps)
        lines_part(ctx, n, syms, reps, few)


if __name__ == "__main__":
    main()
