"""dx_code_hit_starts alone, Context.find_spans beside Context.find_edit, and Context.cut beside today's route, on a .dexta of READS reads
of SYMS bases (100 000 x 10 000: 1 GB of bases, 0.25 GB of image) with the 45-letter SMRTbell adapter planted under up to four edits.

    python tools/find_span_rate.py [READS] [SYMS] [REPS] [--parent <libdexgpu.so of the parent commit>]

(a) The span launch alone: an image with ten copies of the adapter in every read stands on the device with its units (walked here) and
the list dx_code_find_edit made of it at m = 45, k = 9; dx_code_hit_starts over the list's first 10^3, 10^5 and 10^6 hits is timed with
HIP events on the context's stream (its memsets and its read-back of the bad-hit word included), one warm-up, then REPS (5) rounds in
which the sizes take turns.

(b) Whole calls on the image with the adapter in about 1 % of the reads, host clocks around the Python calls with the device
synchronised on both sides (host walk, upload and read-backs included: what a caller waits for), one warm-up, then REPS rounds, taking
turns: Context.find_edit and Context.find_spans with the adapter at k = 9.  With --parent the same find_edit is timed by a child
process of this tool that loads that library (DEXGPU_LIB) and reads the same image from a file, in the same session.

(c) Context.cut of that image (mode split) beside today's route AT ITS LEAST: dx_file_unpack2 to upper-case text, the one-core scan of
tools/find_edit_scan.c that finds the ENDS, and dx_file_pack2 of a text of that size -- the starts, the plan and the rewrite of the text,
which today's route needs too, are not in it.

The answers are asserted: find_spans' report and hits are find_edit's, every start lies within the hit's distance of pos - 45, and the
scan counts find_edit's hits.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ADAPTER = "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT"


def planted(img, off, ln, per_read, every, seed):
    """a copy of the image with copies of the adapter under 0 to 4 random edits, cut or filled with random bases to 48 symbols, written over
    the packed bases at byte-aligned places: per_read of them in every `every`-th read, evenly spread"""
    rng = np.random.default_rng(seed)
    out = np.frombuffer(img, np.uint8).copy()
    pool = np.zeros((4096, 12), np.uint8)                      # 4096 mutated copies, packed; a place draws one of them
    for p in range(len(pool)):
        w = ["ACGT".index(c) for c in ADAPTER]
        for _ in range(int(rng.integers(0, 5))):
            op, i = int(rng.integers(3)), int(rng.integers(len(w)))
            if op == 0:
                w[i] = (w[i] + 1 + int(rng.integers(3))) % 4
            elif op == 1:
                w.insert(i, int(rng.integers(4)))
            else:
                del w[i]
        w = (w + [int(c) for c in rng.integers(0, 4, 8)])[:48]
        pool[p] = [(w[k] << 6) | (w[k + 1] << 4) | (w[k + 2] << 2) | w[k + 3] for k in range(0, 48, 4)]
    r = np.arange(0, len(off), every)
    assert (ln[r] // per_read * (per_read - 1) + 248 <= ln[r]).all(), "the reads are too short for so many copies"
    at = (off[r].astype(np.int64)[:, None] + (ln[r].astype(np.int64)[:, None] // per_read * np.arange(per_read)[None, :] + 200) // 4).reshape(-1)
    out[at[:, None] + np.arange(12)[None, :]] = pool[rng.integers(0, len(pool), len(at))]
    return out.tobytes()


def child(path, reps):
    """--child: Context.find_edit of the image in `path` with whatever library DEXGPU_LIB names; prints the times of REPS rounds"""
    from dextractor_amd import api
    from dextractor_amd import _lib as L
    from find_rate import turns
    for name in ("dx_code_hit_starts", "dx_file_find_edit_spans", "dx_hits_cut_plan", "dx_file_cut"):
        L.SIGNATURES.pop(name, None)                           # (the parent's library has none of them, and load() binds every name)
    img = open(path, "rb").read()
    with api.Context(0) as ctx:
        got = {}
        ms = turns(ctx, {"find_edit": lambda: got.__setitem__("r", ctx.find_edit("fasta", img, [ADAPTER], max_errors=9, max_hits=1 << 24))}, reps)
        print("CHILD", got["r"][0]["hits"], " ".join(f"{x:.3f}" for x in ms["find_edit"]), flush=True)


def line(name, t):
    m = float(np.median(t))
    return (f"    {name:<28} median {m:10.3f} ms  min {min(t):10.3f}  max {max(t):10.3f}  spread {100 * (max(t) - min(t)) / m:5.1f} %   "
            f"all: {' '.join(f'{x:.2f}' for x in t)}")


def main():
    args = [a for a in sys.argv[1:]]
    parent = None
    if "--child" in args:
        return child(args[args.index("--child") + 1], int(args[args.index("--child") + 2]))
    if "--parent" in args:
        parent = os.path.abspath(args[args.index("--parent") + 1])
        del args[args.index("--parent"):args.index("--parent") + 2]
    reads = int(args[0]) if len(args) > 0 else 100000
    syms = int(args[1]) if len(args) > 1 else 10000
    reps = int(args[2]) if len(args) > 2 else 5
    import torch
    from dextractor_amd import api, synth
    from dextractor_amd import _lib as L
    from find_rate import walk, turns, timed
    from find_edit_rate import host_scan
    scan = host_scan()
    torch.cuda.init()
    codes = ["ACGT".index(c) for c in ADAPTER]
    with api.Context(0) as ctx:
        ctx.set_stream(None)                                   # the default stream: where torch's events are recorded
        text = synth.make_seqfile("fasta", reads, seed=5, dist="fixed", mean=syms).text
        plain = ctx.dexta(text)
        n_text = len(text)
        del text
        off, ln = walk(plain)
        print(f"{reads} reads of {syms} bases: {n_text / 1e9:.3f} GB of text, {len(plain) / 1e9:.3f} GB of image; {reps} rounds after one warm-up, "
              f"taking turns", flush=True)

        # ---- (a) the span launch alone ---------------------------------------------------------------------------------------------------
        dense = planted(plain, off, ln, 10, 1, 1)
        cap = 16 * reads + 1000
        bufs = [ctx.to_device(np.frombuffer(dense, np.uint8)), ctx.to_device(off), ctx.to_device(ln), ctx.alloc(16 * cap + 64), ctx.alloc(4 * cap + 64)]
        rep, lst = ctx.code_find_edit(bufs[0], len(dense), bufs[1], None, bufs[2], reads, [(codes, 9)], cap=cap, d_hits=bufs[3])
        found = rep["hits"]
        assert found <= cap
        q = (L.EQuery * 1)(api.equery(codes, 9))
        bad = C.c_uint64()

        def starts(n):
            def f():
                rc = ctx.lib.dx_code_hit_starts(ctx.h, bufs[0].ptr, len(dense), bufs[1].ptr, None, bufs[2].ptr, reads, q, 1, bufs[3].ptr, n,
                                                bufs[4].ptr, C.byref(bad))
                assert rc == 0, rc
            return f

        sizes = [n for n in (1000, 100000, 1000000) if n <= found] or [found]
        cases = {f"{n} hits": starts(n) for n in sizes}
        for f in cases.values():
            f()
        ctx.sync()
        ev = {name: [] for name in cases}
        for _ in range(reps):
            for name, f in cases.items():
                ev[name].append(timed(f))
        st = bufs[4].download(np.uint32, sizes[-1])
        n = (lst["pos"][:sizes[-1]].astype(np.int64) - st.astype(np.int64))
        assert (np.abs(n - 45) <= lst["mis"][:sizes[-1]]).all()
        print(f"(a) dx_code_hit_starts alone (events; m = 45, k = 9; the list has {found} hits, mean distance {lst['mis'].mean():.2f}, "
              f"mean length {n.mean():.2f}):")
        for name, t in ev.items():
            print(line(name, t) + f"   {float(np.median(t)) * 1e6 / int(name.split()[0]):8.2f} ns a hit", flush=True)
        for b in bufs:
            b.free()
        del dense

        # ---- (b) find_spans beside find_edit ---------------------------------------------------------------------------------------------
        img = planted(plain, off, ln, 1, 100, 2)
        del plain
        got = {}
        runs = {"find_edit": lambda: got.__setitem__("edit", ctx.find_edit("fasta", img, [ADAPTER], max_errors=9, max_hits=1 << 24)),
                "find_spans": lambda: got.__setitem__("spans", ctx.find_spans("fasta", img, [ADAPTER], max_errors=9, max_hits=1 << 24))}
        ms = turns(ctx, runs, reps)
        (er, el), (sr, sl) = got["edit"], got["spans"]
        assert all(er[f] == sr[f] for f in ("records", "records_hit", "hits", "listed")) and (el == sl).all() and er["hits"] == er["listed"]
        n = sl["pos"].astype(np.int64) - sr["start"].astype(np.int64)
        assert (np.abs(n - 45) <= sl["mis"]).all()
        print(f"(b) whole calls (host clocks, the device synchronised on both sides); {er['hits']} hits in {er['records_hit']} of {reads} reads:")
        for name, t in ms.items():
            print(line(name, t), flush=True)
        a, b = float(np.median(ms["find_edit"])), float(np.median(ms["find_spans"]))
        print(f"    find_spans - find_edit: {b - a:.3f} ms, {100 * (b - a) / a:.1f} % of find_edit")
        if parent:
            path = os.path.join(tempfile.mkdtemp(prefix="find_span_rate_"), "image.dexta")
            with open(path, "wb") as f:
                f.write(img)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, str(reps)], env=dict(os.environ, DEXGPU_LIB=parent),
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            os.remove(path)
            word = [l for l in out.splitlines() if l.startswith("CHILD")][0].split()
            assert int(word[1]) == er["hits"]
            pt = [float(x) for x in word[2:]]
            print(line("find_edit, parent's library", pt), flush=True)
            again = turns(ctx, {"find_edit": runs["find_edit"]}, reps)["find_edit"]
            print(line("find_edit, once more", again), flush=True)
            p = float(np.median(pt))
            print(f"    find_spans - the parent's find_edit: {b - p:.3f} ms, {100 * (b - p) / p:.1f} % of it "
                  f"({'within' if b - p <= p / 10 else 'MORE THAN'} a tenth)")

        # ---- (c) cut beside today's route ------------------------------------------------------------------------------------------------
        def today():
            t = ctx.undexta(img, upper=True, width=2**31 - 1)
            rec = C.c_uint64()
            got["scan"] = int(scan(t, len(t), ADAPTER.encode(), 9, C.byref(rec)))
            got["packed"] = len(ctx.dexta(t))

        runs = {"cut": lambda: got.__setitem__("cut", ctx.cut("fasta", img, [ADAPTER], max_errors=9, min_len=50, mode="split")),
                "unpack+scan+pack": today}
        ms = turns(ctx, runs, reps)
        out, cut, sel = got["cut"]
        assert got["scan"] == er["hits"] and got["packed"] == len(img) and cut["spans"] <= er["hits"]
        print(f"(c) Context.cut (split, min_len 50) beside today's route at its least: {cut['pieces']} pieces of {cut['records_in']} records, "
              f"{cut['spans']} spans, {len(out)} bytes of image:")
        for name, t in ms.items():
            print(line(name, t), flush=True)
        a, b = float(np.median(ms["cut"])), float(np.median(ms["unpack+scan+pack"]))
        print(f"    cut / unpack+scan+pack: {a / b:.4f}", flush=True)


if __name__ == "__main__":
    main()
