"""The placement's steps -- the index build, the seed count, the seed list, the vote's sort and the rest of the vote -- beside the screen
against the same set in the same run, against references of three sizes with 1 % and all of the reads cut from the reference; and
Context.place as a caller sees it beside Context.screen.

    python tools/place_rate.py [READS] [SYMS] [REPS] [whole]  >  profiles/place_rate.txt

The workload, the references and the timing are tools/screen_rate.py's (whose helpers are used): READS reads of SYMS uniform random
symbols (100 000 x 10 000: 10^9 windows) on the device with their units, k = 21 canonical, HIP events on the context's stream, one
warm-up, then REPS (5) rounds, median, min and max.  One process; every GPU step under a time limit of its own, and the first error
ends the run.

Part 1, per reference ("genomes" of 4.8 x 10^4, 5 x 10^6 and 10^8 symbols, one target each) and share of the reads cut from it:

    index       dx_code_kmer_index of the packed genome (codes, sort, counted set, keys, sort, narrowing)
    screen      dx_code_kmer_screen over the same units and the set inside the index: the floor of the look-ups
    count       dx_code_kmer_seeds with no list
    list        dx_code_kmer_seeds with a list of exactly the seeds (the count, the prefix sum and the listing launch)
    sort        dx_sort_u64 of as many keys with the bits dx_seeds_place sorts: the place step's sort alone
    place       dx_seeds_place (the keys, the sort, the vote and the extents); the rest = place - sort

max_occ = 8, band_bits = 8.  Part 2 (fourth argument `whole`), on a .dexta of the same shape (a 1 GB .fasta), host clocks with the
device synchronised on both sides: Context.screen against the middle reference's set and Context.place against its index.
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

K, MAX_OCC, BAND = SR.K, 8, 8


def genome_index(ctx, G):
    """the packed genome as one target and its index -> (genome, index, the build's rounds)"""
    genome = SR.step(lambda: SR.packed_random(G // 4, 100 + G % 97))
    g_off, g_len = torch.zeros(1, device="cuda", dtype=torch.int64), torch.full((1,), G, device="cuda", dtype=torch.int32)
    made = []

    def build():
        made.append(ctx.code_kmer_index(genome, g_off, None, g_len, K, canonical=True))
    t = [SR.timed(build) for _ in range(3)]
    for x in made[:-1]:
        x.free()
    return genome, made[-1], t[1:]


def whole_calls(ctx, reads, syms, reps, index):
    text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
    img = SR.step(lambda: ctx.dexta(text), 600)
    print(f"a .dexta of {reads} reads of {syms} bases: {len(text) / 1e9:.3f} GB of text, {len(img) / 1e9:.3f} GB of image", flush=True)
    for name, call in (("screen", lambda: ctx.screen("fasta", img, index.kset())), ("place", lambda: ctx.place("fasta", img, index, MAX_OCC, BAND))):
        got, tk = None, []
        for r in range(reps + 1):
            ctx.sync(); t0 = time.perf_counter()
            got = SR.step(call, 600)
            ctx.sync(); t1 = time.perf_counter()
            if r:
                tk.append((t1 - t0) * 1e3)
        print(f"    Context.{name:<7} k={K}   median {np.median(tk):10.3f} ms  min {min(tk):10.3f}  max {max(tk):10.3f};  "
              + ", ".join(f"{f} {got[0][f]}" for f in got[0] if f not in ("records", "symbols", "k")), flush=True)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    syms = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    whole = len(sys.argv) > 4 and sys.argv[4] == "whole"
    assert syms % 4 == 0
    torch.cuda.init()
    print(f"device: {torch.cuda.get_device_name(0)}")
    windows = reads * (syms - K + 1)
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        boff = torch.arange(reads, device="cuda", dtype=torch.int64) * (syms // 4)
        ln = torch.full((reads,), syms, device="cuda", dtype=torch.int32)
        data = SR.step(lambda: SR.packed_random(reads * syms // 4, 1))
        out = torch.empty(8 * reads, dtype=torch.int32, device="cuda")
        cnt = torch.empty(reads, dtype=torch.int32, device="cuda")
        off = torch.empty(reads + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        print(f"{reads} reads of {syms} symbols: {windows / 1e9:.3f} G windows at k = {K}, canonical; max_occ {MAX_OCC}, band_bits {BAND}; "
              f"{reps} rounds after one warm-up; events on the context's stream", flush=True)
        ubits = max(int(reads - 1).bit_length(), 0)
        kept = None
        for G in SR.GENOMES:
            genome, index, t_build = genome_index(ctx, G)
            info = index.info
            print(f"  a reference of {G} symbols: {info['codes']} codes, {info['windows']} positions, {info['device_bytes'] / 1e6:.1f} MB on the "
                  f"device; index built in {min(t_build):.2f} ms ({G / min(t_build) / 1e6:.3f} G symbols/s)", flush=True)
            kset = index.kset()
            for share, name in ((0.01, "1 % of the reads from the reference"), (1.0, "all reads from the reference")):
                SR.step(lambda: SR.plant(data, genome, reads, syms, int(reads * share), 7))
                torch.cuda.synchronize()
                tot = SR.step(lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out))
                m_scr = SR.line("screen " + name, SR.rounds(reps, lambda: ctx.code_kmer_screen(data, boff, None, ln, kset, out=out)), windows,
                                f"   hits {int(tot[1])} ({100.0 * int(tot[1]) / windows:.3f} %)")
                st = SR.step(lambda: ctx.code_kmer_seeds(data, boff, None, ln, index, max_occ=MAX_OCC, count=cnt)[0])
                seeds = int(st[2])
                m_cnt = SR.line("count  " + name, SR.rounds(reps, lambda: ctx.code_kmer_seeds(data, boff, None, ln, index, max_occ=MAX_OCC, count=cnt)),
                                windows, f"   seeds {seeds}, windows with a seed {int(st[1])}")
                lst = torch.empty(4 * seeds + 4, dtype=torch.int32, device="cuda")
                m_lst = SR.line("list   " + name, SR.rounds(reps, lambda: ctx.lib.dx_code_kmer_seeds(
                    ctx.h, data.data_ptr(), data.numel(), boff.data_ptr(), None, ln.data_ptr(), reads, index.h, MAX_OCC, cnt.data_ptr(),
                    off.data_ptr(), lst.data_ptr(), seeds, api.C.byref((api.C.c_uint64 * 4)()), None)), windows)
                keys, tmp = torch.empty(seeds + 8, dtype=torch.int64, device="cuda"), torch.empty(seeds + 8, dtype=torch.int64, device="cuda")
                bits = ubits + 33 - BAND

                def sort_alone():
                    keys[:seeds] = lst.view(torch.int64)[1:2 * seeds:2] & ((1 << bits) - 1)       # (any keys of that many bits: the sort's cost does not depend on them)
                    ctx.sort_u64(keys, bits, tmp, n=seeds)
                m_fill = float(np.median(SR.rounds(reps, lambda: keys[:seeds].copy_(lst.view(torch.int64)[1:2 * seeds:2] & ((1 << bits) - 1)))))
                m_sort = float(np.median(SR.rounds(reps, sort_alone))) - m_fill
                del keys, tmp
                torch.cuda.empty_cache()
                print(f"    sort   {seeds} keys of {bits} bits{'':<14} median {m_sort:9.3f} ms", flush=True)
                pt = (api.C.c_uint64 * 3)()
                m_plc = SR.line("place  " + name, SR.rounds(reps, lambda: ctx.lib.dx_seeds_place(
                    ctx.h, lst.data_ptr(), off.data_ptr(), reads, K, BAND, out.data_ptr(), api.C.byref(pt))), windows,
                    f"   votes {pt[1]}, units placed {pt[2]}")
                print(f"      count = {m_cnt / m_scr:5.2f} x the screen, list = {m_lst / m_scr:5.2f} x, the vote's rest = {m_plc - m_sort:9.3f} ms, "
                      f"count + list + place = {(m_lst + m_plc) / m_scr:5.2f} x the screen against the same set", flush=True)
                del lst
                torch.cuda.empty_cache()
            if G == SR.GENOMES[1] and whole:
                kept = index
            else:
                index.free()
            del genome
            data = SR.step(lambda: SR.packed_random(reads * syms // 4, 1))     # (the reads as they were: random again)
        del data, out, cnt, off
        torch.cuda.empty_cache()
        if kept is not None:
            whole_calls(ctx, reads, syms, reps, kept)
            kept.free()


if __name__ == "__main__":
    main()
