"""dx_code_kmer_depths and dx_depth_stats beside the screen they ride on and the copy that is the floor of their stores, against counted
sets of three sizes with about 1 % and all of the windows in the set; and Context.depth as a caller sees it beside Context.screen.

    python tools/depth_rate.py [READS] [SYMS] [REPS] [whole | screen]

The workload, the sets and the timing are tools/screen_rate.py's (whose helpers are used): READS reads of SYMS uniform random symbols
(100 000 x 10 000: 10^9 windows) on the device with their units, k = 21 canonical, HIP events on the context's stream, one warm-up,
then REPS (5) rounds, median, min and max.  One process; every GPU step under a time limit of its own, and the first error ends the run.

Part 1, per set ("genomes" of 4.8 x 10^4, 5 x 10^6 and 10^8 symbols -> codes, sorted, dx_kmer_set_from_sorted_counted) and share of the
reads cut from the genome (1 %, all), in the same run:

    screen      dx_code_kmer_screen over the same units and set: the reference for the look-up
    copy        a device-to-device copy of the profile's bytes (2 a window): the floor of the stores
    depths      dx_code_kmer_depths (the two small launches, the prefix sum and its read-back included)
    stats       dx_depth_stats over the profile that has just been written

Part 2 (fourth argument `whole`), on a .dexta of the same shape (a 1 GB .fasta), host clocks with the device synchronised on both sides:
Context.screen and Context.depth against the middle set.  With `screen` Part 2 times Context.screen alone against the uncounted set and
Part 1 is left out: the run to make with DEXGPU_LIB naming the parent commit's library, which has no depth call, to show that the
existing call did not move.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import screen_rate as SR                  # noqa: E402
from dextractor_amd import api, synth     # noqa: E402

K = SR.K


def genome_set(ctx, G, counted):
    """the packed genome and the set of its codes -> (genome, set, milliseconds)"""
    genome = SR.step(lambda: SR.packed_random(G // 4, 100 + G % 97))
    g_off, g_len = torch.zeros(1, device="cuda", dtype=torch.int64), torch.full((1,), G, device="cuda", dtype=torch.int32)
    gw = G - K + 1
    gc, gt = torch.empty(gw, dtype=torch.int64, device="cuda"), torch.empty(gw, dtype=torch.int64, device="cuda")
    made = []

    def build():
        ctx.code_kmer_codes(genome, g_off, None, g_len, K, True, cap=gw, codes=gc)
        ctx.sort_u64(gc, 2 * K, gt)
        made.append((ctx.kmer_set_from_sorted_counted if counted else ctx.kmer_set_from_sorted)(gc, gw, K, canonical=True))
    t = SR.timed(build)
    del gc, gt
    torch.cuda.empty_cache()
    return genome, made[0], t


def whole_calls(ctx, reads, syms, reps, kset, with_depth):
    text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
    img = SR.step(lambda: ctx.dexta(text), 600)
    print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
    for name in ("screen", "depth")[:2 if with_depth else 1]:
        call, got, tk = getattr(ctx, name), None, []                # (a library of before this call has no Context.depth)
        for r in range(reps + 1):
            ctx.sync(); t0 = time.perf_counter()
            got = SR.step(lambda: call("fasta", img, kset), 600)
            ctx.sync(); t1 = time.perf_counter()
            if r:
                tk.append((t1 - t0) * 1e3)
        print(f"    Context.{name:<7} k={K}   median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f};  windows {got[0]['windows']}, "
              f"hits {got[0]['hits']}, records hit {got[0]['records_hit']}", flush=True)
    if with_depth:
        os.environ["DEXGPU_TIMING"] = "1"                       # once more with the driver's stage marks (stderr)
        try:
            SR.step(lambda: ctx.depth("fasta", img, kset), 600)
        finally:
            os.environ.pop("DEXGPU_TIMING", None)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    mode = sys.argv[4] if len(sys.argv) > 4 else ""
    assert syms % 4 == 0 and mode in ("", "whole", "screen")
    torch.cuda.init()
    which = os.environ.get("DEXGPU_LIB") or "the tree's"
    print(f"device: {torch.cuda.get_device_name(0)};  library: {which}")
    windows = reads * (syms - K + 1)
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        if mode == "screen":
            genome, kset, _ = genome_set(ctx, SR.GENOMES[1], False)
            del genome
            whole_calls(ctx, reads, syms, reps, kset, False)
            kset.free()
            return
        boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
        ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
        data = SR.step(lambda: SR.packed_random(reads * syms // 4, 1))
        out = torch.empty(8 * reads, dtype=torch.int32, device="cuda")
        prof = torch.empty(windows + 8, dtype=torch.int16, device="cuda")
        twin = torch.empty(windows + 8, dtype=torch.int16, device="cuda")
        off = torch.empty(reads + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print(f"{reads} reads of {syms} symbols: {windows / 1e9:.3f} G windows at k = {K}, canonical; {reps} rounds after one warm-up; "
              f"events on the context's stream", flush=True)
        SR.line("copy   device to device, 2 bytes a window", SR.rounds(reps, lambda: twin.copy_(prof)), windows)
        del twin
        torch.cuda.empty_cache()

        kept = None
        for G in SR.GENOMES:
            genome, kset, t_build = genome_set(ctx, G, True)
            info = kset.info
            print(f"  a genome of {G} symbols: {info['codes']} codes with counts, index of 2^{info['index_bits']} buckets, "
                  f"{info['device_bytes'] / 1e6:.1f} MB on the device; built (codes of one unit, sort, counted set) in {t_build:.2f} ms", flush=True)
            for share, name in ((0.01, "1 % of the reads from the genome"), (1.0, "all reads from the genome")):
                SR.step(lambda: SR.plant(data, genome, reads, syms, int(reads * share), 7))
                torch.cuda.synchronize()
                tot = SR.step(lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out))
                m_scr = SR.line("screen " + name, SR.rounds(reps, lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out)), windows,
                                f"   hits {int(tot[1])} ({100.0 * int(tot[1]) / windows:.3f} %)")
                m_dep = SR.line("depths " + name, SR.rounds(reps, lambda: ctx.code_kmer_depths(data, boff, None, ln, kset, cap=windows, depth=prof,
                                                                                              off=off)), windows)
                st = SR.step(lambda: ctx.depth_stats(prof, off, reads, out=out))
                SR.line("stats  " + name, SR.rounds(reps, lambda: ctx.depth_stats(prof, off, reads, out=out)), windows,
                        f"   hits {int(st[1])}, sum {int(st[2])}")
                assert int(st[1]) == int(tot[1]) and int(st[0]) == windows
                print(f"      depths = {m_dep / m_scr:5.2f} x the screen against the same set", flush=True)
            if G == SR.GENOMES[1] and mode == "whole":
                kept = kset
            else:
                kset.free()
            del genome
            data = SR.step(lambda: SR.packed_random(reads * syms // 4, 1))     # (the reads as they were: random again)
        del data, out, prof, off
        torch.cuda.empty_cache()
        if kept is not None:
            whole_calls(ctx, reads, syms, reps, kept, True)
            kept.free()


if __name__ == "__main__":
    main()
