"""How dextractor_amd.api passes its arguments on: every spelling of a device array -- a DevBuf, a DevView at offset 0, a torch tensor --
is one address to the library, so the same units give the same answer, which is the numpy statement the call's own tests use
(imported from them, not repeated); a failed call carries the attributes its docstring names; and None for an array that the entry
point does not check itself is refused in Python."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

pytestmark = pytest.mark.gpu

E_ARG, E_FORMAT = -1, -3          # DX_E_*
SPELLINGS = ("buf", "view", "tensor")


@pytest.fixture(scope="module")
def ctx():
    with api.Context(0) as c:
        yield c


class Spell:
    """numpy arrays onto the device and back, in one of the SPELLINGS"""
    def __init__(self, ctx, how, torch=None):
        self.ctx, self.how, self.torch, self.bufs = ctx, how, torch, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        if self.how == "tensor":
            t = self.torch.from_numpy(a.view(np.uint8).copy()).cuda()
            self.torch.cuda.synchronize()
            return t
        self.bufs.append(self.ctx.to_device(a))
        return self.bufs[-1] if self.how == "buf" else self.bufs[-1].offset(0)

    def down(self, d, dtype, count):
        if self.how == "tensor":
            return d.cpu().numpy().view(dtype)[:count].copy()
        return (d if self.how == "buf" else d.base).download(dtype, count)

    def free(self):
        for b in self.bufs:
            b.free()


# ---- the units: the small edge set of tests/test_gpu_census.py ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reads():
    """Three packed reads of 0, 5 and 130 symbols behind one odd byte -- one empty, one inside a byte group, one past a 16-byte chunk --
    and a unit in each: (symbols, payload, boff, beg, len)"""
    import test_gpu_repack as R
    rng = np.random.default_rng(2026)
    syms = [rng.integers(0, 4, n, dtype=np.uint8) for n in (0, 5, 130)]
    parts = [R.pack_bits(s) for s in syms]
    payload = np.frombuffer(b"\xa5" + b"".join(parts), np.uint8)
    boff = (1 + np.concatenate([[0], np.cumsum([len(p) for p in parts])[:-1]])).astype(np.uint64)
    return syms, payload, boff, np.array([0, 1, 2], np.uint32), np.array([0, 4, 128], np.uint32)


@functools.lru_cache(maxsize=None)
def ranges():
    """three byte ranges of 0, 1 and 17 bytes, the last one up to the buffer's last byte: (buffer, off, len)"""
    buf = np.random.default_rng(17).integers(0, 256, 40, dtype=np.uint8)
    return buf, np.array([3, 3, 23], np.uint64), np.array([0, 1, 17], np.uint64)


def pairs():
    """tests/test_verify.py's units of 0, 1 and 17 bytes in two buffers, one byte of the last flipped"""
    import test_verify as V
    u = V.Units([0, 1, 17], seed=5)
    u.flip(2, 9)
    return u


def wanted():
    """what the four calls are to answer, by the numpy statements of their own tests"""
    import test_gpu_census as CS
    import test_gpu_repack as R
    syms, payload, boff, beg, ln = reads()
    sym = ((payload[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).ravel()
    run = np.zeros((4, len(sym) + 1), np.int64)
    for c in range(4):
        run[c, 1:] = np.cumsum(sym == c)
    counts = CS.counts_of(run, boff, beg, ln)
    nb = (ln.astype(np.int64) + 3) >> 2
    out_off = (R.GUARD + 1 + np.concatenate([[0], np.cumsum(nb + 1)[:-1]])).astype(np.uint64)
    out = bytearray([R.FILL]) * (int(out_off[-1]) + int(nb[-1]) + R.GUARD)
    for s, b, n, o in zip(syms, beg, ln, out_off):
        out[int(o): int(o) + ((int(n) + 3) >> 2)] = R.pack_bits(s[int(b): int(b) + int(n)])
    buf, off, rl = ranges()
    raw = buf.tobytes()
    units = [raw[int(o): int(o + n)] for o, n in zip(off, rl)]
    return {"counts": counts, "totals": counts.sum(axis=0), "out_off": out_off, "repacked": bytes(out),
            "crc": np.array([zlib.crc32(u) for u in units], np.uint32), "fold": (zlib.crc32(b"".join(units)), sum(len(u) for u in units)),
            "verify": pairs().expected()}


def answers(ctx, sp):
    """the four calls on arrays spelled by sp"""
    import test_gpu_repack as R
    want = wanted()
    _, payload, boff, beg, ln = reads()
    got, n = {}, len(ln)
    try:
        d_in, d_boff, d_beg, d_len = sp.up(payload), sp.up(boff), sp.up(beg), sp.up(ln)
        d_cnt = sp.up(np.zeros(4 * n, np.uint32))
        got["totals"] = ctx.code_counts(d_in, len(payload), d_boff, d_beg, d_len, n, d_cnt)
        got["counts"] = sp.down(d_cnt, np.uint32, 4 * n).reshape(n, 4)
        d_out, d_out_off = sp.up(np.full(len(want["repacked"]), R.FILL, np.uint8)), sp.up(want["out_off"])
        ctx.reads_repack(d_in, len(payload), d_boff, d_beg, d_len, n, d_out, d_out_off)
        got["repacked"] = sp.down(d_out, np.uint8, len(want["repacked"])).tobytes()
        buf, off, rl = ranges()
        d_buf, d_off, d_rl, d_crc = sp.up(buf), sp.up(off), sp.up(rl), sp.up(np.zeros(n, np.uint32))
        ctx.crc32_ranges(d_buf, len(buf), d_off, d_rl, n, d_crc)
        got["crc"] = sp.down(d_crc, np.uint32, n)
        got["fold"] = ctx.crc32_fold(d_crc, d_rl, n)
        u = pairs()
        got["verify"] = ctx.verify_ranges(*[sp.up(v) for v in (u.a, u.a_off, u.a_len, u.b, u.b_off, u.b_len)], n)
    finally:
        sp.free()
    return got


def check(got, want, how):
    assert want["verify"] == (2, 9, 1) and want["fold"][1] == 18
    assert np.array_equal(got["counts"], want["counts"]), how
    assert list(got["totals"]) == list(want["totals"]) and got["totals"].dtype == np.uint64, how
    assert got["repacked"] == want["repacked"], how
    assert np.array_equal(got["crc"], want["crc"]) and got["fold"] == want["fold"], how
    assert got["verify"] == want["verify"], how


TORCH_SIDE = r"""
import sys
import torch
torch.cuda.init()                                  # (torch first, as in tools/: it does not find the device once the library has it open)
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import test_gpu_api_args as T
from dextractor_amd import api
want = T.wanted()
with api.Context(0) as ctx:
    for how in T.SPELLINGS:
        T.check(T.answers(ctx, T.Spell(ctx, how, torch)), want, how)
print("every spelling ok")
"""


def test_one_answer_for_every_spelling_of_a_device_array():
    """code_counts, reads_repack, crc32_ranges + crc32_fold and verify_ranges on a DevBuf, a DevView at offset 0 and a torch tensor: in
    a process of its own, which starts torch before the library"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", TORCH_SIDE, os.path.dirname(here), here], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "every spelling ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- what a failed call carries ----------------------------------------------------------------------------------------------------
def test_a_unit_past_the_input_is_named_by_every_range_call(ctx):
    """the last unit ends in the buffer's last byte: with one byte fewer it ends past in_bytes"""
    _, payload, boff, beg, ln = reads()
    buf, off, rl = ranges()
    sp = Spell(ctx, "buf")
    try:
        d_in, d_boff, d_beg, d_len = sp.up(payload), sp.up(boff), sp.up(beg), sp.up(ln)
        d_out, d_out_off = ctx.alloc(1024), sp.up(np.array([0, 64, 128], np.uint64))
        sp.bufs.append(d_out)
        d_buf, d_off, d_rl, d_crc = sp.up(buf), sp.up(off), sp.up(rl), sp.up(np.zeros(3, np.uint32))
        assert int(boff[2]) + ((int(beg[2]) + int(ln[2]) + 3) >> 2) == len(payload) and int(off[2] + rl[2]) == len(buf)
        for call in (lambda: ctx.code_counts(d_in, len(payload) - 1, d_boff, d_beg, d_len, 3),
                     lambda: ctx.reads_unpack(L.DX_LETTERS_NUMBERS, d_in, len(payload) - 1, d_boff, d_beg, d_len, 3, d_out, d_out_off),
                     lambda: ctx.crc32_ranges(d_buf, len(buf) - 1, d_off, d_rl, 3, d_crc)):
            with pytest.raises(L.DexGPUError) as e:
                call()
            assert e.value.code == E_FORMAT and e.value.bad_unit == 2
        assert list(ctx.code_counts(d_in, len(payload), d_boff, d_beg, d_len, 3)) == list(wanted()["totals"])
    finally:
        sp.free()


def test_a_record_past_the_stream_is_named_by_the_device_walk(ctx):
    """tests/test_gpu_entries.py's cut stream: the last record runs past nbytes, and stands first in the list"""
    import test_gpu_entries as E
    stream, coff, rlen, coding = E.bare("synth130")
    n = len(rlen)
    cut = stream[: int(coff[n - 1]) + int(coff[n] - coff[n - 1]) // 2]
    with pytest.raises(L.DexGPUError) as e:
        E.device_walk(ctx, cut, coff[:-1][::-1], rlen[::-1], coding)
    assert e.value.code == E_FORMAT and e.value.bad_entry == 0 and not hasattr(e.value, "bad_unit")


# ---- None ----------------------------------------------------------------------------------------------------------------------------
def test_none_is_the_librarys_to_refuse_or_refused_before_it(ctx):
    _, payload, boff, beg, ln = reads()
    sp = Spell(ctx, "buf")
    try:
        d_boff, d_beg, d_len, d_out, d_out_off = sp.up(boff), sp.up(beg), sp.up(ln), sp.up(np.zeros(256, np.uint8)), sp.up(np.zeros(3, np.uint64))
        with pytest.raises(L.DexGPUError) as e:                      # an optional array: None is NULL, and the library says DX_E_ARG
            ctx.reads_repack(None, len(payload), d_boff, d_beg, d_len, 3, d_out, d_out_off)
        assert e.value.code == E_ARG
        said = ctx.lib.dx_last_error(ctx.h)
        assert said
        with pytest.raises(TypeError, match="d_in"):                 # a required one: refused here, the library is not called
            ctx.pack2_decode(L.DX_LETTERS_LOWER, None, d_boff, d_len, 3, 80, d_out, d_out_off)
        assert ctx.lib.dx_last_error(ctx.h) == said
    finally:
        sp.free()
