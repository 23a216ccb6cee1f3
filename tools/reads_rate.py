"""k_reads_unpack (reads and subreads out of a .bps payload) beside k_pack2_decode (undexta's text) on the same packed reads.

N reads of SYMS symbols (1 M x 10 000: 2.5 GB packed, random) stand on the device.  Three things are timed in one process, on the
same buffers, REPS repetitions each after one warm-up, taking turns:

    (a) dx_pack2_decode, DX_LETTERS_NUMBERS, width = SYMS        the symbols and one '\\n' a read
    (b) dx_reads_unpack, whole reads                             the symbols and one delimiter a read: the same bytes moved
    (c) dx_reads_unpack, subreads of SUB symbols at a uniformly random beg
    (d) dx_reads_unpack_lines, whole reads, lower case, width 80  k_reads_unpack with k_pack2_decode's line ends
    (e) dx_reads_unpack_lines, the subreads of (c), width 80      dx_file_extract's one launch
    (f) dx_reads_repack of those subreads into scratch, then dx_pack2_decode of the scratch, width 80: the two launches the same
        text took before there was (e)

    python tools/reads_rate.py [N] [SYMS] [REPS] [SUB]

Times are HIP events on the stream the context issues on, one call each: the call's own memsets and ticket kernel included, and
for dx_reads_unpack the read-back of its verdict.  The first reads of (a) and (b) and the first subreads of (c) are compared
with the symbols unpacked on the host, and so are the first texts of (d), (e) and (f).  The target for (b): its median no more
above (a)'s than (a)'s own max - min.  (d), (e) and (f) have no target: they are printed with the bytes they move by the roofline's
count -- 0.25 B read and 1 + 1 / 80 B written a symbol -- as a fraction of the 8 TB/s peak.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dextractor_amd import _lib as L      # noqa: E402
from dextractor_amd import api            # noqa: E402


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    sub = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    assert syms % 4 == 0 and sub <= syms
    clen = syms // 4
    rng = np.random.Generator(np.random.PCG64(20261018))
    block_reads = min(n, 100000)
    block = rng.integers(0, 256, block_reads * clen, dtype=np.uint8)          # the payload: this block, over and over
    torch.cuda.init()
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        d_in = ctx.alloc(n * clen)
        for r0 in range(0, n, block_reads):
            m = min(block_reads, n - r0)
            ctx._chk(ctx.lib.dx_h2d(ctx.h, d_in.ptr + r0 * clen, block.ctypes.data, m * clen))
        idx = np.arange(n, dtype=np.uint64)
        beg = rng.integers(0, syms - sub + 1, n).astype(np.uint32)
        d_boff, d_len, d_ooff = ctx.to_device(idx * np.uint64(clen)), ctx.to_device(np.full(n, syms, np.uint32)), ctx.to_device(idx * np.uint64(syms + 1))
        d_beg, d_slen, d_sooff = ctx.to_device(beg), ctx.to_device(np.full(n, sub, np.uint32)), ctx.to_device(idx * np.uint64(sub + 1))
        lw = 80                                                # (d), (e), (f): the lines' width
        t_whole, t_sub, csub = syms + (syms + lw - 1) // lw, sub + (sub + lw - 1) // lw, (sub + 3) // 4
        d_out = ctx.alloc(n * max(syms + 1, t_whole))
        d_looff, d_lsooff = ctx.to_device(idx * np.uint64(t_whole)), ctx.to_device(idx * np.uint64(t_sub))
        d_scr, d_roff = ctx.alloc(n * csub + 64), ctx.to_device(idx * np.uint64(csub))

        def two_launches():
            ctx.reads_repack(d_in, n * clen, d_boff, d_beg, d_slen, n, d_scr, d_roff)
            ctx.pack2_decode(L.DX_LETTERS_LOWER, d_scr, d_roff, d_slen, n, lw, d_out, d_lsooff)
        runs = {"a": lambda: ctx.pack2_decode(L.DX_LETTERS_NUMBERS, d_in, d_boff, d_len, n, syms, d_out, d_ooff),
                "b": lambda: ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d_in, n * clen, d_boff, None, d_len, n, d_out, d_ooff),
                "c": lambda: ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d_in, n * clen, d_boff, d_beg, d_slen, n, d_out, d_sooff)}
        # the warm-up calls, each checked against the symbols unpacked here
        k = min(n, 3)
        want = ((block[: k * clen, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).astype(np.uint8).reshape(k, syms)
        for name, tail, width in (("a", 10, syms), ("b", 4, syms), ("c", 4, sub)):
            runs[name](); ctx.sync()
            got = d_out.download(np.uint8, k * (width + 1)).reshape(k, width + 1)
            ref = want if name != "c" else np.stack([want[j, beg[j]: beg[j] + sub] for j in range(k)])
            assert (got[:, :width] == ref).all() and (got[:, width] == tail).all(), name
        ms = {name: [] for name in runs}
        for _ in range(reps):
            for name in runs:
                ms[name].append(timed(runs[name]))
        lines = {"d": lambda: ctx.reads_unpack_lines(L.DX_LETTERS_LOWER, d_in, n * clen, d_boff, None, d_len, n, lw, d_out, d_looff),
                 "e": lambda: ctx.reads_unpack_lines(L.DX_LETTERS_LOWER, d_in, n * clen, d_boff, d_beg, d_slen, n, lw, d_out, d_lsooff),
                 "f": two_launches}
        acgt = np.frombuffer(b"acgt", np.uint8)
        for name, t in (("d", t_whole), ("e", t_sub), ("f", t_sub)):
            lines[name](); ctx.sync()
            got = d_out.download(np.uint8, k * t).reshape(k, t)
            for j in range(k):
                s = acgt[want[j] if name == "d" else want[j, beg[j]: beg[j] + sub]].tobytes()
                assert got[j].tobytes() == b"".join(s[i: i + lw] + b"\n" for i in range(0, len(s), lw)), name
        lms = {name: [] for name in lines}
        for _ in range(reps):
            for name in lines:
                lms[name].append(timed(lines[name]))
        out_bytes = {"a": n * (syms + 1), "b": n * (syms + 1), "c": n * (sub + 1)}
        what = {"a": f"dx_pack2_decode, numbers, width {syms}", "b": "dx_reads_unpack, whole reads", "c": f"dx_reads_unpack, subreads of {sub} at a random beg"}
        print(f"{n} reads x {syms} symbols, {n * clen / 1e9:.2f} GB packed, {reps} repetitions after one warm-up, taking turns")
        for name in runs:
            t = ms[name]
            med = float(np.median(t))
            print(f"({name}) {what[name]:<50} median {med:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                  f"{out_bytes[name] / med / 1e9:6.2f} TB/s written   all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)
        spread = max(ms["a"]) - min(ms["a"])
        gap = float(np.median(ms["b"])) - float(np.median(ms["a"]))
        print(f"(b) - (a) medians: {gap:+.3f} ms; (a)'s max - min: {spread:.3f} ms: the target is {'met' if gap <= spread else 'MISSED'}")
        moved = {"d": n * (syms / 4 + t_whole), "e": n * (sub / 4 + t_sub), "f": n * (sub / 4 + t_sub)}      # (the roofline's count: what (f) moves through scratch is not in it)
        lwhat = {"d": f"dx_reads_unpack_lines, whole reads, width {lw}", "e": f"dx_reads_unpack_lines, subreads of {sub}, width {lw}",
                 "f": f"dx_reads_repack + dx_pack2_decode, subreads of {sub}, width {lw}"}
        for name in lines:
            t = lms[name]
            med = float(np.median(t))
            print(f"({name}) {lwhat[name]:<58} median {med:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                  f"{moved[name] / med / 1e9:6.2f} TB/s = {moved[name] / med / 1e9 / 8.0:5.1%} of 8 TB/s   all: {' '.join(f'{x:.3f}' for x in t)}", flush=True)


if __name__ == "__main__":
    main()
