"""The range functions share one frame of device words (csrc/units/dx_units.hpp: ticket, bad unit, padded input, answer words).
What that sharing must not break: calls of different functions back to back on ONE context, in any order; a refused unit, a
padded tiny input and an answer must not be seen by the call behind them.  Every expected value is numpy's or zlib's."""
import functools
import zlib

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 130)            # one round of 64 units, its edges, three rounds
FUNCS = ("verify", "crc", "fold", "reads", "counts", "hist")
ORDERS = {"forth": FUNCS, "back": ("hist", "counts", "reads", "fold", "crc", "verify")}
SHIFTS = np.array([6, 4, 2, 0], np.uint8)


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def units(n, size=1 << 15, seed=0):
    """n units of a random buffer of `size` bytes, anywhere in it: most short (a lane's, or 16 lanes'), every eighth long (the wave's)"""
    rng = np.random.default_rng(1000 * seed + n)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    ln = np.where(np.arange(n) % 8 == 5, 5000, rng.integers(0, 300, n)).astype(np.uint64)
    ln = np.minimum(ln, np.uint64(size // 2))
    off = rng.integers(0, size - ln.astype(np.int64) + 1).astype(np.uint64)                   # the unit's bytes: [off, off + ln)
    return buf, off, ln


class Job:
    """one function's inputs on the device for n units, and its call checked against the host's answer"""

    def __init__(self, ctx, n, size=1 << 15, seed=0):
        self.ctx, self.n, self.size = ctx, n, size
        self.buf, self.off, self.ln = units(n, size, seed)
        self.sym = ((self.buf[:, None] >> SHIFTS) & 3).astype(np.uint8).ravel()
        self.parts = [self.buf[int(o):int(o) + int(k)] for o, k in zip(self.off, self.ln)]
        up = ctx.to_device
        other = self.buf.copy()                                   # verify: the middle unit's last byte differs (a unit of no bytes: the one in front)
        self.hit = next((j for j in range(n // 2, -1, -1) if self.ln[j]), None)
        if self.hit is not None:
            other[int(self.off[self.hit] + self.ln[self.hit]) - 1] ^= 0x40
        self.d = dict(buf=up(self.buf), other=up(other), off=up(self.off), ln=up(self.ln), ln32=up(self.ln.astype(np.uint32)),
                      crc=ctx.alloc(4 * n), kind=up((np.arange(n) % 5).astype(np.uint8)), sum=ctx.alloc(8 * n), cnt=ctx.alloc(16 * n),
                      crc_in=up(np.array([zlib.crc32(p.tobytes()) for p in self.parts], np.uint32)))
        # packed units for reads / counts: symbols [beg, beg + 4 ln - beg - 1) of the read at off (inside the unit's bytes)
        self.beg = (np.arange(n) % 4).astype(np.uint32)
        self.slen = np.maximum(4 * self.ln.astype(np.int64) - self.beg - 1, 0).astype(np.uint32)
        self.ooff = np.concatenate([[0], np.cumsum(self.slen.astype(np.uint64) + 1)]).astype(np.uint64)
        self.d.update(beg=up(self.beg), slen=up(self.slen), ooff=up(self.ooff[:n]), out=ctx.alloc(int(self.ooff[n])))

    def free(self):
        for b in self.d.values():
            b.free()

    def symbols(self, j):
        s0 = 4 * int(self.off[j]) + int(self.beg[j])
        return self.sym[s0:s0 + int(self.slen[j])]

    def verify(self):
        d, differing = self.d, [j for j, (o, k) in enumerate(zip(self.off, self.ln))
                                if self.hit is not None and o <= self.off[self.hit] + self.ln[self.hit] - 1 < o + k]
        got = self.ctx.verify_ranges(d["buf"], d["off"], d["ln32"], d["other"], d["off"], d["ln32"], self.n)
        if not differing:
            assert got == (None, 0, 0)
        else:
            first = differing[0]
            assert got == (first, int(self.off[self.hit] + self.ln[self.hit] - 1 - self.off[first]), len(differing))

    def crc(self):
        d = self.d
        self.ctx.crc32_ranges(d["buf"], self.size, d["off"], d["ln"], self.n, d["crc"])
        assert d["crc"].download(np.uint32, self.n).tolist() == [zlib.crc32(p.tobytes()) for p in self.parts]

    def fold(self):
        whole = b"".join(p.tobytes() for p in self.parts)
        assert self.ctx.crc32_fold(self.d["crc_in"], self.d["ln"], self.n) == (zlib.crc32(whole), len(whole))

    def reads(self):
        d = self.d
        d["out"].zero()
        self.ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d["buf"], self.size, d["off"], d["beg"], d["slen"], self.n, d["out"], d["ooff"])
        want = np.concatenate([np.append(self.symbols(j), np.uint8(4)) for j in range(self.n)])
        assert (d["out"].download(np.uint8, len(want)) == want).all()

    def counts(self):
        d = self.d
        want = np.array([np.bincount(self.symbols(j), minlength=4) for j in range(self.n)], np.uint64)
        tot = self.ctx.code_counts(d["buf"], self.size, d["off"], d["beg"], d["slen"], self.n, d["cnt"])
        assert (d["cnt"].download(np.uint32, 4 * self.n).reshape(self.n, 4) == want).all()
        assert tot.tolist() == want.sum(axis=0).tolist()

    def hist(self):
        d, want = self.d, np.zeros((5, 256), np.uint64)
        for j, p in enumerate(self.parts):
            want[j % 5] += np.bincount(p, minlength=256).astype(np.uint64)
        got = self.ctx.byte_hist_ranges(d["buf"], self.size, d["off"], d["ln"], d["kind"], 5, self.n, d["sum"])
        assert (got == want).all()
        assert d["sum"].download(np.uint64, self.n).tolist() == [int(p.sum(dtype=np.uint64)) for p in self.parts]


@pytest.fixture(scope="module")
def jobs(ctx):
    made = {n: Job(ctx, n) for n in COUNTS}
    yield made
    for j in made.values():
        j.free()


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("n", COUNTS)
def test_mixed_calls_back_to_back(jobs, n, order):
    for name in ORDERS[order]:
        getattr(jobs[n], name)()


BAD_AT = 64                                # (of 65 units: the second round's only unit)


def refused(ctx, job, name):
    """`name` called with unit BAD_AT out of bounds -> the error and the unit it names"""
    d, n = job.d, job.n
    off = job.off.copy()
    off[BAD_AT] = job.size + 100
    d_off = ctx.to_device(off)
    try:
        with pytest.raises(L.DexGPUError) as e:
            if name == "crc":
                ctx.crc32_ranges(d["buf"], job.size, d_off, d["ln"], n, d["crc"])
            elif name == "reads":
                ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d["buf"], job.size, d_off, d["beg"], d["slen"], n, d["out"], d["ooff"])
            elif name == "counts":
                ctx.code_counts(d["buf"], job.size, d_off, d["beg"], d["slen"], n, d["cnt"])
            else:
                ctx.byte_hist_ranges(d["buf"], job.size, d_off, d["ln"], d["kind"], 5, n, d["sum"])
    finally:
        d_off.free()
    return e.value


@pytest.mark.parametrize("name", ["crc", "reads", "counts", "hist"])
def test_a_bad_unit_does_not_stick(ctx, jobs, name):
    job = jobs[65]
    for other in FUNCS:
        if other == name:
            continue
        err = refused(ctx, job, name)
        assert err.code == -3 and err.bad_unit == BAD_AT and f" {BAD_AT} does not lie inside" in str(err)
        getattr(job, other)()


def test_the_pad_words_do_not_stick(ctx):
    """a buffer shorter than the kernels' loads is copied into the frame's pad: reads (8 bytes a load) on 3 bytes, counts (16) on 5, then both on 4 KiB"""
    def packed(size, seed):
        rng = np.random.default_rng(seed)
        buf = rng.integers(0, 256, size, dtype=np.uint8)
        sym = ((buf[:, None] >> SHIFTS) & 3).astype(np.uint8).ravel()
        boff = np.array([0, size - 1, 0, size // 2], np.uint64)
        beg = np.array([0, 1, 3, 2], np.uint32)
        ln = np.array([4 * size, 3, 4 * size - 3, 4 * (size - size // 2) - 2], np.uint32)
        return buf, [sym[4 * int(o) + int(b):4 * int(o) + int(b) + int(k)] for o, b, k in zip(boff, beg, ln)], boff, beg, ln

    def run(which, size, seed):
        buf, want, boff, beg, ln = packed(size, seed)
        ooff = np.concatenate([[0], np.cumsum(ln.astype(np.uint64) + 1)]).astype(np.uint64)
        d = [ctx.to_device(x) for x in (buf, boff, beg, ln, ooff[:4])] + [ctx.alloc(int(ooff[4])), ctx.alloc(64)]
        try:
            if which == "reads":
                ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d[0], size, d[1], d[2], d[3], 4, d[5], d[4])
                text = np.concatenate([np.append(w, np.uint8(4)) for w in want])
                assert (d[5].download(np.uint8, len(text)) == text).all(), (which, size)
            else:
                tot = ctx.code_counts(d[0], size, d[1], d[2], d[3], 4, d[6])
                per = np.array([np.bincount(w, minlength=4) for w in want], np.uint64)
                assert (d[6].download(np.uint32, 16).reshape(4, 4) == per).all(), (which, size)
                assert tot.tolist() == per.sum(axis=0).tolist()
        finally:
            for b in d:
                b.free()

    run("reads", 3, 1)
    run("counts", 5, 2)
    run("reads", 4096, 3)
    run("counts", 4096, 4)


def test_the_answer_words_do_not_stick(jobs):
    """dx_verify_ranges leaves unit << 32 | position and a count in the answer words, dx_crc32_fold a CRC and a length, dx_code_counts four totals"""
    job = jobs[130]
    assert job.hit is not None
    job.verify()
    job.fold()
    job.counts()
