"""dx_code_kmer_spans -- the count alone and with the list -- and dx_spans_join beside dx_code_kmer_screen over the same units, against
tools/screen_rate.py's three set sizes; and Context.screen_spans and Context.screen_cut as a caller sees them beside Context.screen.

    python tools/screen_spans_rate.py [READS] [SYMS] [REPS] [whole]

One process.  Every GPU step runs under a time limit of its own (screen_rate.py's step: a watchdog that ends the process with status
124), and the first error of any kind ends the run: nothing follows a fault.

Part 1, the kernels alone: READS reads of SYMS uniform random symbols (100 000 x 10 000: 10^9 positions) stand on the device with their
units, 1 % of them copied from the genome; HIP events on the context's stream, one warm-up, then REPS (5) rounds, median, min and max;
k = 21, canonical.  Per genome (4.8 x 10^4, 5 x 10^6, 10^8 symbols), in the same run:

    screen      dx_code_kmer_screen: the reference point
    count       dx_code_kmer_spans with cap 0: the counting launch alone
    list        dx_code_kmer_spans with room for every span: count, prefix sum, the listing launch (which repeats the look-ups of the
                units that have a span)
    join        dx_spans_join of that list (max_gap 50, min_span 100) into a second list

and once more with ALL reads from the genome -- every unit has a span, and the listing launch repeats every look-up.

Part 2 (with the fourth argument), the whole calls on a .dexta of the same shape (a 1 GB .fasta) against the bacterium's set, host
clocks with the device synchronised on both sides: Context.screen, Context.screen_spans, Context.screen_cut.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import screen_rate as R                   # noqa: E402
from dextractor_amd import api, synth     # noqa: E402

K = R.K
MAX_GAP, MIN_SPAN = 50, 100


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
        out = torch.empty(4 * reads, dtype=torch.int32, device="cuda")
        cnt = torch.empty(reads, dtype=torch.int32, device="cuda")
        print(f"{reads} reads of {syms} symbols: {reads * syms / 1e9:.3f} G positions, {windows / 1e9:.3f} G windows at k = {K}, canonical; "
              f"{reps} rounds after one warm-up; events on the context's stream", flush=True)
        kept = None
        for G in R.GENOMES:
            genome = R.step(lambda: R.packed_random(G // 4, 100 + G % 97))
            g_off, g_len = torch.zeros(1, device="cuda", dtype=torch.int64), torch.full((1,), G, device="cuda", dtype=torch.int32)
            gw = G - K + 1
            gc, gt = torch.empty(gw, dtype=torch.int64, device="cuda"), torch.empty(gw, dtype=torch.int64, device="cuda")
            made = []

            def build():
                ctx.code_kmer_codes(genome, g_off, None, g_len, K, True, cap=gw, codes=gc)
                ctx.sort_u64(gc, 2 * K, gt)
                made.append(ctx.kmer_set_from_sorted(gc, gw, K, canonical=True))
            R.step(build)
            kset = made[0]
            info = kset.info
            del gc, gt
            torch.cuda.empty_cache()
            print(f"  a genome of {G} symbols: {info['codes']} codes, {info['device_bytes'] / 1e6:.1f} MB on the device", flush=True)
            for share, name in ((0.01, "1 % of the reads from the genome"), (1.0, "all reads from the genome")):
                data = R.step(lambda: R.packed_random(reads * syms // 4, 1))
                R.step(lambda: R.plant(data, genome, reads, syms, int(reads * share), 7))
                torch.cuda.synchronize()
                print(f"   {name}", flush=True)
                m_screen = R.line("screen dx_code_kmer_screen", R.rounds(reps, lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out)), windows)
                tot = R.step(lambda: ctx.code_kmer_spans(data, boff, None, ln, kset, count=R.View(cnt), n=reads)[0])
                spans = int(tot[0])
                m = R.line("count  dx_code_kmer_spans, cap 0", R.rounds(reps, lambda: ctx.code_kmer_spans(data, boff, None, ln, kset, count=R.View(cnt), n=reads)),
                           windows, f"   spans {spans}, covered {int(tot[1])}, reads with a span {int(tot[2])}")
                print(f"      {m / m_screen:5.2f} x screen", flush=True)
                lst = torch.empty(2 * max(spans, 1) + 2, dtype=torch.int64, device="cuda")
                tot_b, cap_b = (api.C.c_uint64 * 3)(), spans

                def listing():
                    # (the C call: the Python wrapper would bring the list down inside the timed stretch)
                    rc = ctx.lib.dx_code_kmer_spans(ctx.h, data.data_ptr(), data.numel(), boff.data_ptr(), None, ln.data_ptr(), reads, kset.h,
                                                    cnt.data_ptr(), lst.data_ptr(), cap_b, api.C.byref(tot_b), None)
                    assert rc == 0 and tot_b[0] == spans
                m = R.line("list   dx_code_kmer_spans, every span", R.rounds(reps, listing), windows)
                print(f"      {m / m_screen:5.2f} x screen" + ("   MORE THAN TWICE the screen: the cover-word form is the next step" if m > 2 * m_screen else ""), flush=True)
                if spans:
                    joined = torch.empty(2 * spans + 2, dtype=torch.int64, device="cuda")
                    tot_j = (api.C.c_uint64 * 2)()

                    def join():
                        rc = ctx.lib.dx_spans_join(ctx.h, lst.data_ptr(), spans, MAX_GAP, MIN_SPAN, joined.data_ptr(), spans, api.C.byref(tot_j), None)
                        assert rc == 0
                    t = R.rounds(reps, join)
                    mj = float(np.median(t))
                    print(f"    join   dx_spans_join, max_gap {MAX_GAP}, min_span {MIN_SPAN}        median {mj:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   "
                          f"{spans / mj / 1e6:8.3f} G spans/s   kept {tot_j[0]}, their symbols {tot_j[1]}", flush=True)
                    del joined
                del lst, data
                torch.cuda.empty_cache()
            if G == R.GENOMES[1] and whole:
                kept = kset
            else:
                kset.free()
            del genome
        del out, cnt
        torch.cuda.empty_cache()

        # ---- the join at the size the raw spans of noisy reads have: a synthetic list ----------------------------------------------------
        # 40 spans of 21 symbols a record, 9 symbols apart, every eighth gap 60: five joined spans a record under max_gap 50
        for n in (10 ** 7, 10 ** 8):
            i = torch.arange(n, device="cuda", dtype=torch.int64)
            beg = (i % 40) * 30 + (i % 40 // 8) * 51
            lst = torch.stack([i // 40, beg | ((beg + 21) << 32)], dim=1).contiguous()
            joined = torch.empty(2 * n, dtype=torch.int64, device="cuda")
            tot_j = (api.C.c_uint64 * 2)()
            del i, beg

            def join():
                rc = ctx.lib.dx_spans_join(ctx.h, lst.data_ptr(), n, MAX_GAP, MIN_SPAN, joined.data_ptr(), n, api.C.byref(tot_j), None)
                assert rc == 0
            t = R.rounds(reps, join)
            mj = float(np.median(t))
            assert tot_j[0] == n // 8
            print(f"  join   dx_spans_join of {n} synthetic spans, 8 to a joined one   median {mj:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   "
                  f"{n / mj / 1e6:8.3f} G spans/s, {16 * n / mj / 1e6:8.1f} GB/s of input   kept {tot_j[0]}", flush=True)
            del lst, joined
            torch.cuda.empty_cache()

        # ---- the whole calls ------------------------------------------------------------------------------------------------------------
        if whole:
            text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
            img = R.step(lambda: ctx.dexta(text), 600)
            print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
            for name, call in (("Context.screen", lambda: ctx.screen("fasta", img, kept)[0]),
                               ("Context.screen_spans", lambda: ctx.screen_spans("fasta", img, kept, MAX_GAP, MIN_SPAN)[0]),
                               ("Context.screen_cut, split", lambda: ctx.screen_cut("fasta", img, kept, MAX_GAP, MIN_SPAN, 500, "split")[1])):
                got, tk = None, []
                for r in range(reps + 1):
                    ctx.sync(); t0 = time.perf_counter()
                    got = R.step(call, 600)
                    ctx.sync(); t1 = time.perf_counter()
                    if r:
                        tk.append((t1 - t0) * 1e3)
                print(f"    {name:<28} median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f};  {got}", flush=True)
            kept.free()


if __name__ == "__main__":
    main()
