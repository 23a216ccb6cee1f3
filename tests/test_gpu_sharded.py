"""The sharded file drivers -- dx_file_dexqv_sharded (csrc/dx_file_qv_shard.c) and dx_file_pack2_sharded (csrc/dx_file_pack2.c), a
thread crew (csrc/dx_crew.c) over several contexts -- against the oracle (needs an MI355X).  Bar: bit-exact."""
import numpy as np
import pytest

from _flags import set_flag

import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _dev(k):
    """Device of the k-th context of a sharded run: distinct GPUs when the box has several, else device 0."""
    return k % max(1, L.load().dx_device_count())


def test_file_dexqv_sharded_cut_beyond_shard0(ctx):
    """~250 k symbols over 4 contexts: the 100000-symbol threshold of QV.c:1006 lies beyond shard 0, whose
    prefix batch must then supply subChar (csrc/dx_file_qv_shard.c)."""
    c = synth.make_quiva(28, seed=17, mean=9000)
    cs = [api.Context(_dev(k)) for k in range(4)]
    try:
        assert api.dexqv_sharded(cs, c.text, 0) == O.dexqv(c.text, 0)
    finally:
        for x in cs:
            x.close()


@pytest.mark.parametrize("nctx", [2, 5])
@pytest.mark.parametrize("lossy", [0, 1])
def test_file_dexqv_sharded_over_contexts(ctx, nctx, lossy):
    """dx_file_dexqv_sharded: host threads + host-side merge; one context per GPU when several are
    visible, otherwise all on device 0."""
    c = synth.make_quiva(43, seed=71, mean=7000)
    cs = [api.Context(_dev(k)) for k in range(nctx)]
    try:
        got = api.dexqv_sharded(cs, c.text, lossy)
    finally:
        for x in cs:
            x.close()
    assert got == O.dexqv(c.text, lossy)
    tiny = synth.make_quiva(3, seed=72, mean=100)                 # fewer entries than contexts
    cs = [api.Context(_dev(k)) for k in range(nctx)]
    try:
        assert api.dexqv_sharded(cs, tiny.text, lossy) == O.dexqv(tiny.text, lossy)
    finally:
        for x in cs:
            x.close()


@pytest.mark.parametrize("nctx", [2, 5])
def test_file_dexqv_sharded_by_byte_ranges(ctx, monkeypatch, nctx):
    """A file too large to index on one thread first (BASELINE configs[4]): dx_file_dexqv_sharded deals BYTES, every shard counts the
    newlines of its range, finds the records that begin in it (six lines a record, data lines may begin with '@' too), uploads and
    indexes them on its own device (dx_index_quiva_device) -- no pass over the whole file anywhere.  DEXGPU_TEST=shard_bytes_min brings a
    small file that way: the reference's bytes; a malformed file comes back with what the one-context driver says about it; a file
    whose first 100000 symbols reach beyond shard 0 goes the serial way and comes out right."""
    set_flag(monkeypatch, "shard_bytes_min", "4096")
    c = synth.make_quiva(320, seed=73, mean=5000)
    cs = [api.Context(_dev(k)) for k in range(nctx)]
    try:
        for lossy in (0, 1):
            assert api.dexqv_sharded(cs, c.text, lossy) == O.dexqv(c.text, lossy)
        short = synth.make_quiva(9000, seed=74, lens=np.full(9000, 37, np.uint32))        # many entries in every range
        assert api.dexqv_sharded(cs, short.text, 0) == O.dexqv(short.text, 0)
        small = synth.make_quiva(24, seed=75, mean=9000)                                  # (100000 symbols reach beyond shard 0 of 5)
        assert api.dexqv_sharded(cs, small.text, 0) == O.dexqv(small.text, 0)
        bad = bytearray(c.text)
        at = c.text.index(b"\n", len(c.text) // 2)
        del bad[at - 3: at]                                                               # a data line three symbols short
        with pytest.raises(L.DexGPUError) as e1:
            ctx.dexqv(bytes(bad))
        with pytest.raises(L.DexGPUError) as e2:
            api.dexqv_sharded(cs, bytes(bad), 0)
        import re
        where = lambda e: (e.value.code, re.search(r"line (\d+)", str(e.value)).group(1), re.search(r"code (\d+)", str(e.value)).group(1))
        assert where(e1) == where(e2), (str(e1.value), str(e2.value))
        cut = c.text[: c.text.rindex(b"\n", 0, len(c.text) - 1) + 1]                      # the last entry a line short
        with pytest.raises(L.DexGPUError) as e3:
            api.dexqv_sharded(cs, cut, 0)
        assert e3.value.code == -3
    finally:
        for x in cs:
            x.close()


def test_file_dexqv_sharded_by_byte_ranges_in_which_no_record_begins(ctx, monkeypatch):
    """By bytes, two entries of about 200 KB over five ranges of about 80 KB: no record begins in three of the ranges, so three shards
    own nothing, the by-bytes run turns the file down and it goes the serial way -- members with no work still walk every phase of the
    crew's table (csrc/dx_file_qv_shard.c)."""
    set_flag(monkeypatch, "shard_bytes_min", "4096")
    c = synth.make_quiva(2, seed=76, lens=np.array([40000, 40000], np.uint32))
    cs = [api.Context(_dev(k)) for k in range(5)]
    try:
        assert api.dexqv_sharded(cs, c.text, 0) == O.dexqv(c.text, 0)
    finally:
        for x in cs:
            x.close()


def test_sharded_file_drivers_over_every_physical_device():
    """dx_file_dexqv_sharded / dx_file_pack2_sharded with ONE context on EVERY device hipGetDeviceCount reports: the
    hipSetDevice-per-thread path of csrc/dx_file_qv_shard.c and csrc/dx_file_pack2.c on real multi-GPU hardware (BASELINE configs[4]'s layout: contiguous
    entry ranges per GPU, host-side histogram sum, outputs concatenated), against the oracle.  Skips on a one-GPU box --
    there the same drivers run over several contexts of device 0 (the tests around this one)."""
    ndev = L.load().dx_device_count()
    if ndev < 2:
        pytest.skip("one GPU visible (%d): the multi-device path needs at least two" % ndev)
    cs = [api.Context(k) for k in range(ndev)]
    try:
        assert sorted(x.device for x in cs) == list(range(ndev))
        for lossy in (0, 1):
            c = synth.make_quiva(40 * ndev + 3, seed=91, mean=6000)        # ~250 k symbols per device: the 100000-symbol cut lies in shard 0
            assert api.dexqv_sharded(cs, c.text, lossy) == O.dexqv(c.text, lossy)
        small = synth.make_quiva(2 * ndev, seed=92, mean=4000)              # ... and beyond shard 0 here
        assert api.dexqv_sharded(cs, small.text, 0) == O.dexqv(small.text, 0)
        for kind in ("fasta", "arrow"):
            f = synth.make_seqfile(kind, 50 * ndev + 1, seed=93, mean=5000)
            assert api.pack2_sharded(cs, f.text, arrow=(kind == "arrow")) == (O.dexta(f.text) if kind == "fasta" else O.dexar(f.text))
    finally:
        for x in cs:
            x.close()


@pytest.mark.parametrize("nctx", [2, 5])
@pytest.mark.parametrize("kind", ["fasta", "arrow"])
def test_file_pack2_sharded_over_contexts(ctx, nctx, kind):
    """dx_file_pack2_sharded: read ranges on several contexts (here all on device 0), one host thread
    each; the image is byte-identical to the single-context one and to the reference's."""
    lens = np.array([0, 3, 900, 17, 20000] + [int(x) for x in np.random.default_rng(3).integers(1, 6000, 70)], np.uint32)
    c = synth.make_seqfile(kind, len(lens), seed=41, lens=lens)
    others = [api.Context(_dev(k + 1)) for k in range(nctx - 1)]
    try:
        got = api.pack2_sharded([ctx] + others, c.text, arrow=(kind == "arrow"))
    finally:
        for o in others:
            o.close()
    assert got == (O.dexta(c.text) if kind == "fasta" else O.dexar(c.text))
    with pytest.raises(L.DexGPUError):
        api.pack2_sharded([ctx, ctx], b"no header\nACGT\n")
