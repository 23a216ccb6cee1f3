"""Rate of dx_verify_ranges on the bench's batch shapes, and of a whole dx_file_verify beside the decode it contains (GPU box):
    ./tools/microbench/copy_rate > copy.txt; python tools/microbench/verify_rate.py
The kernel reads two bytes per byte compared and writes nothing: its yardstick is the copy rate of the same run (copy_rate.hip).
Times are HIP events on the stream the context issues on, one call each (the call's own memsets, ticket kernel and the read of
its answer included), median of the repetitions after two warm-up calls."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dextractor_amd import api, synth   # noqa: E402


def timed(f, reps=7):
    for _ in range(2):
        f()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    torch.cuda.init()
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        for n, L in ((1_000_000, 50_000), (4_000_000, 1_500)):
            nbytes = n * L
            a, b = ctx.alloc(nbytes + 64), ctx.alloc(nbytes + 64)
            ctx._chk(ctx.lib.dx_memset(ctx.h, a.ptr, 0x41, nbytes + 64))
            ctx._chk(ctx.lib.dx_memset(ctx.h, b.ptr, 0x41, nbytes + 64))
            off = np.arange(n, dtype=np.uint64) * np.uint64(L)
            lens = np.full(n, L, np.uint32)
            d_len = ctx.to_device(lens)
            for shift in (0, 5):
                d_ao, d_bo = ctx.to_device(off), ctx.to_device(off + np.uint64(shift))
                for count in (True, False):
                    res = []
                    med, lo, hi = timed(lambda: res.append(ctx.verify_ranges(a, d_ao, d_len, b, d_bo, d_len, n, count=count)))
                    assert res[-1][0] is None
                    print(f"dx_verify_ranges {n:>8} units x {L:>6} B, b {shift} B off a, {'counting' if count else 'first only'}: "
                          f"{med:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {2 * nbytes / med / 1e9:6.2f} TB/s of traffic", flush=True)
                d_ao.free(); d_bo.free()
            a.free(); b.free(); d_len.free()

        c = synth.make_quiva(8000, seed=77, mean=10000)
        img = ctx.dexqv(c.text)
        for what, f in (("dx_file_undexqv (decode, text downloaded)", lambda: ctx.undexqv(img, upper=True)),
                        ("dx_file_verify  (decode, compared on the device)", lambda: ctx.verify("quiva", c.text, img))):
            ts = []
            for _ in range(4):
                t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
            if isinstance(r, dict):
                assert r["ok"], r
            print(f"{what}: .quiva of {len(c.text) / 1e6:.0f} MB, .dexqv of {len(img) / 1e6:.0f} MB: {min(ts[1:]) * 1e3:.1f} ms wall (best of 3 after one)", flush=True)


if __name__ == "__main__":
    main()
