"""Records at known starts on the GPU (needs an MI355X): dx_qv_walk_records_device (k_walk_records, a lane a record) against
the host walk, and dx_entries_uncompress -- Load_QVentry (DB.c:2575-2621) for a selection of entries at once -- against
the reference's own bytes and text.  Bar: bit-exact."""
import functools

import numpy as np
import pytest

from _flags import set_flag

import _oracle as O
from dextractor_amd import _lib as L
from dextractor_amd import api, synth
from test_entries_host import GOLDENS, golden_walk, selections

pytestmark = pytest.mark.gpu

ROUND_TRIP_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 200000, 256, 257, 1000]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def synth_walk():
    """130 entries (two full waves and a partial one) as a .dexqv of the oracle's, walked on the host"""
    img = O.dexqv(synth.make_quiva(130, seed=4711, mean=3000).text)
    w = api.qv_walk(img)
    start = (w["rec_off"][:-1] + (w["hdr_off"][1:] - w["hdr_off"][:-1])).astype(np.uint64)
    return img, w, api.qv_read_coding(img[2:])[0], start


def walked(name):
    return synth_walk() if name == "synth130" else golden_walk(name)


@functools.lru_cache(maxsize=None)
def bare(name):
    """The image's records without their framing bytes, as a .qvs holds them: (stream, coff [n + 1], rlen, coding)"""
    img, w, coding, start = walked(name)
    size = w["seg"].sum(axis=1, dtype=np.uint64)
    coff = np.concatenate([[0], np.cumsum(size)]).astype(np.uint64)
    stream = b"".join(img[int(s): int(s + z)] for s, z in zip(start, size))
    assert len(stream) == int(coff[-1])
    return stream, coff, w["len"], coding


@functools.lru_cache(maxsize=None)
def reference_entries(name, upper):
    """per entry the five data lines, '\\n' after each, as the reference's undexqv prints them"""
    img = walked(name)[0]
    lines = O.undexqv(img, upper=upper).split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 6 == 0
    return [b"\n".join(lines[k + 1: k + 6]) + b"\n" for k in range(0, len(lines) - 1, 6)]


def entries_of(text, toff):
    return [text[int(toff[j]): int(toff[j + 1])] for j in range(len(toff) - 1)]


def device_walk(ctx, buf, start, rlen, coding, flip=False):
    d_buf = ctx.to_device(np.frombuffer(buf, np.uint8))
    d_start, d_len = ctx.to_device(np.asarray(start, np.uint64)), ctx.to_device(np.asarray(rlen, np.uint32))
    d_seg = ctx.alloc(20 * max(len(start), 1))
    try:
        ctx.qv_walk_records_device(d_buf, len(buf), d_start, d_len, len(start), coding, d_seg, flip=flip)
        return d_seg.download(np.uint32, 5 * len(start)).reshape(-1, 5)
    finally:
        for d in (d_buf, d_start, d_len, d_seg):
            d.free()


# ---- 1. the device walk is the host walk ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS + ["synth130"])
def test_device_walk_equals_host_walk(ctx, name):
    img, w, coding, start = walked(name)
    for what, sel in selections(w["n"]):
        want = api.qv_walk_records(img, start[sel], w["len"][sel], coding)
        assert (want == w["seg"][sel]).all()
        got = device_walk(ctx, img, start[sel], w["len"][sel], coding)
        assert (got == want).all(), (name, what, np.nonzero((got != want).any(axis=1))[0][:5])


def test_device_walk_leaves_long_entries_to_the_host(ctx, monkeypatch):
    """Entries beyond the bound of a lane's walk (4 M symbols; here lowered to 2500) are walked by the host function on a copy
    of their bytes: the same sizes, and a record among them that is cut off is named all the same."""
    img, w, coding, start = synth_walk()
    assert (w["len"] > 2500).sum() > 10 and (w["len"] <= 2500).sum() > 10
    set_flag(monkeypatch, "records_rlen_max", 2500)
    assert (device_walk(ctx, img, start, w["len"], coding) == w["seg"]).all()
    last = int(np.nonzero(w["len"] > 2500)[0][-1])
    cut = int(start[last]) + int(w["seg"][last].sum()) // 2
    with pytest.raises(L.DexGPUError) as e:
        device_walk(ctx, img[:cut], start[: last + 1], w["len"][: last + 1], coding)
    assert e.value.code == -3 and e.value.bad_entry == last


# ---- 2. reference bytes back to reference text ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_reference_bytes_back_to_reference_text(ctx, name):
    stream, coff, rlen, coding = bare(name)
    for ascii_, upper in ((2, True), (1, False)):
        text, toff = ctx.entries_uncompress(coding, stream, coff, rlen, ascii=ascii_)
        want = reference_entries(name, upper)
        assert len(toff) == len(want) + 1 and int(toff[-1]) == len(text)
        got = entries_of(text, toff)
        assert got == want, (name, ascii_, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5])
    if name == "qv_tiny":                                  # ... and the committed text the golden was made from
        lines = O.golden("qv_tiny.quiva").split(b"\n")
        src = [b"\n".join(lines[k + 1: k + 6]) + b"\n" for k in range(0, len(lines) - 1, 6)]
        upper = src[0].split(b"\n")[1][:1].isupper()
        text, toff = ctx.entries_uncompress(coding, stream, coff, rlen, ascii=2 if upper else 1)
        assert entries_of(text, toff) == src


# ---- 3. selection and order -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True], ids=["cut_by_size", "packed"])
def test_selection_and_order(ctx, packed, monkeypatch):
    stream, coff, rlen, coding = bare("synth130")
    n = len(rlen)
    text, toff = ctx.entries_uncompress(coding, stream, coff, rlen)
    every = entries_of(text, toff)
    assert every == reference_entries("synth130", False)
    if packed:                                             # the selected spans packed side by side, whatever share they have
        set_flag(monkeypatch, "entries_packed")
    for ids in (np.arange(n)[::-1], np.arange(0, n, 3), np.array([5, 5, 129, 0, 5, 64, 63, 64]), np.array([77]), np.arange(n)):
        t, o = ctx.entries_uncompress(coding, stream, coff, rlen, ids=ids)
        assert len(o) == len(ids) + 1 and int(o[-1]) == len(t)
        assert entries_of(t, o) == [every[int(i)] for i in ids], ids[:8]
    t, o = ctx.entries_uncompress(coding, stream, coff, rlen, ids=np.zeros(0, np.uint64))
    assert t == b"" and o.tolist() == [0]
    # offsets that do not tile the stream: the records moved apart, in another order
    gap, order = 37, np.arange(n)[::-1]
    moved, coff2 = bytearray(), np.zeros(n, np.uint64)
    for i in order:
        moved += b"\xa5" * gap
        coff2[i] = len(moved)
        moved += stream[int(coff[i]): int(coff[i + 1])]
    t, o = ctx.entries_uncompress(coding, bytes(moved), coff2, rlen)
    assert entries_of(t, o) == every


# ---- 4. round trip with the encoder ---------------------------------------------------------------------------------------

def round_trip_lines():
    prof = synth.pacbio_profile()
    return [synth.qv_lines(99, k, L, prof) for k, L in enumerate(ROUND_TRIP_LENGTHS)]


def pad_rule_counts(coding, lossy, lines):
    """How many plain insertion / merge segments of these entries end with the extra word of QV.c:436-442 and how many do
    not: the segment's words, from the oracle's encoder, against the words its code bits fill."""
    ref = O.Coding.from_buffer_copy(bytes(coding))
    extra = [0, 0]
    for e in lines:
        if e.shape[1] == 0:
            continue
        _, seg = O.qv_encode_entry(ref, lossy, e)
        for row, s, shift in ((2, L.DX_INS, 1), (3, L.DX_MRG, 2)):
            v = (e[row] >> shift) << shift if lossy else e[row]
            lens = np.array(ref.s[s].lens, np.int64)
            esc = lens[255] + 8 if ref.s[s].type == 2 else 0
            cost = np.where(lens[v] > 0, lens[v], esc)
            assert (cost > 0).all()
            words = (int(cost.sum()) + 31) // 32
            k = seg[row] // 4 - words
            assert k in (0, 1)
            extra[k] += 1
    return extra


@pytest.mark.parametrize("lossy", [False, True], ids=["lossless", "lossy"])
def test_round_trip_with_the_encoder(ctx, lossy):
    lines = round_trip_lines()
    coding, records, coff = ctx.entries_compress([[r.tobytes() for r in e] for e in lines], lossy=lossy)
    assert coding.delChar >= 0                             # the deletion line is run-coded: some entries end in the run character
    ends = [int(e[0][-1]) == coding.delChar for e in lines if e.shape[1] >= 15]
    assert any(ends) and not all(ends)
    without, with_ = pad_rule_counts(coding, lossy, lines)
    assert without > 0 and with_ > 0, (without, with_)     # both branches of the pad rule
    rlen = np.array(ROUND_TRIP_LENGTHS, np.uint32)
    want = []
    for e in lines:
        e = e.copy()
        if lossy:                                          # QV.c:1406-1415
            e[2] = (e[2] >> 1) << 1
            e[3] = (e[3] >> 2) << 2
        e[1] = np.frombuffer(e[1].tobytes().lower(), np.uint8)
        want.append(b"".join(r.tobytes() + b"\n" for r in e))
    # host and device agree on where every segment ends
    seg = api.qv_walk_records(records, coff[:-1], rlen, coding)
    assert (coff[:-1] + seg.sum(axis=1, dtype=np.uint64) == coff[1:]).all()
    assert (device_walk(ctx, records, coff[:-1], rlen, coding) == seg).all()
    text, toff = ctx.entries_uncompress(coding, records, coff, rlen)
    got = entries_of(text, toff)
    assert [len(g) for g in got] == [5 * (L_ + 1) for L_ in ROUND_TRIP_LENGTHS]
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    ids = np.arange(len(rlen))[::-1]
    text, toff = ctx.entries_uncompress(coding, records, coff, rlen, ids=ids)
    assert entries_of(text, toff) == want[::-1]


# ---- 5. ascii = 0 ------------------------------------------------------------------------------------------------------------

NUMBER_READ = bytes(1 if chr(c) in "cC" else 2 if chr(c) in "gG" else 3 if chr(c) in "tT" else 0 for c in range(256))   # DB.c:393-416


@pytest.mark.parametrize("name", ["qv_mid", "qv_nodel"])
def test_ascii_0_is_number_read_of_the_tag_line(ctx, name):
    stream, coff, rlen, coding = bare(name)
    lower = entries_of(*ctx.entries_uncompress(coding, stream, coff, rlen, ascii=1))
    nums = entries_of(*ctx.entries_uncompress(coding, stream, coff, rlen, ascii=0))
    assert len(lower) == len(nums) == len(rlen)
    for a, b, L_ in zip(lower, nums, rlen):
        L_ = int(L_)
        assert len(a) == len(b) == 5 * (L_ + 1)
        assert b[L_ + 1: 2 * L_ + 1] == a[L_ + 1: 2 * L_ + 1].translate(NUMBER_READ)
        assert b[: L_ + 1] == a[: L_ + 1] and b[2 * L_ + 1:] == a[2 * L_ + 1:]
    assert any(set(b[int(L_) + 1: 2 * int(L_) + 1]) - {0} for b, L_ in zip(nums, rlen))


# ---- 6. slices ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True], ids=["whole_stream", "packed"])
def test_slices_give_the_same_bytes(ctx, packed, monkeypatch):
    stream, coff, rlen, coding = bare("synth130")
    ids = np.concatenate([np.arange(130)[::-1], np.arange(0, 130, 7)])
    want = ctx.entries_uncompress(coding, stream, coff, rlen, ids=ids)
    budget = 400000
    assert len(want[0]) > 3 * budget                       # at least four slices
    monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
    set_flag(monkeypatch, "entries_packed" if packed else "entries_whole")
    got = ctx.entries_uncompress(coding, stream, coff, rlen, ids=ids)
    assert got[0] == want[0] and (got[1] == want[1]).all()


# ---- 7. byte-swapped stream --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["qv_mid", "qv_type2", "qv_runs"])
def test_byte_swapped_stream(ctx, name):
    img, w, coding, start = walked(name)
    stream, coff, rlen, _ = bare(name)
    fl = O.byteswap_dexqv(img, w)
    swapped = b"".join(fl[int(s): int(s + z)] for s, z in zip(start, w["seg"].sum(axis=1, dtype=np.uint64)))
    assert swapped != stream and len(swapped) == len(stream)
    assert (device_walk(ctx, fl, start, w["len"], coding, flip=True) == w["seg"]).all()
    text, toff = ctx.entries_uncompress(coding, swapped, coff, rlen, flip=True)
    assert entries_of(text, toff) == reference_entries(name, False)


# ---- 8. truncated stream -----------------------------------------------------------------------------------------------------

# budget: the selection in slices (test_slices_give_the_same_bytes' figure), every entry in order, so that the cut one lies in the last
# slice and its place there is not its place in the selection.  The sliced cases force their transport (entries_whole /
# entries_packed), as that test does; cut_by_size sets no flag and lets the cut stream's size decide.
@pytest.mark.parametrize("packed, budget", [(False, 0), (True, 0), (False, 400000), (True, 400000)],
                         ids=["cut_by_size", "packed", "sliced_whole_stream", "sliced_packed"])
def test_truncated_stream_is_an_error_of_the_library(ctx, packed, budget, monkeypatch):
    stream, coff, rlen, coding = bare("synth130")
    n = len(rlen)
    cut = stream[: int(coff[n - 1]) + int(coff[n] - coff[n - 1]) // 2]
    selections = (None, np.array([3, n - 1, 7]), np.arange(n)[::-1])
    if budget:
        assert 5 * (int(rlen[: n - 1].sum()) + n - 1) > budget      # the last entry begins behind the first slice
        monkeypatch.setenv("DEXGPU_TEXT_BUDGET", str(budget))
        set_flag(monkeypatch, "entries_packed" if packed else "entries_whole")
        selections = (np.arange(n),)
    elif packed:
        set_flag(monkeypatch, "entries_packed")
    for ids in selections:
        with pytest.raises(L.DexGPUError) as e:
            ctx.entries_uncompress(coding, cut, coff, rlen, ids=ids)
        assert e.value.code == -3 and f"entry {n - 1}," in str(e.value), str(e.value)
    with pytest.raises(L.DexGPUError) as e:                # the walk alone names the place in its list
        device_walk(ctx, cut, coff[:-1][::-1], rlen[::-1], coding)
    assert e.value.code == -3 and e.value.bad_entry == 0
    # the error came from the library, not from the device: the same context decodes another selection of the same stream
    ids = np.arange(n - 1)[::-1]
    text, toff = ctx.entries_uncompress(coding, cut, coff, rlen, ids=ids)
    assert entries_of(text, toff) == [reference_entries("synth130", False)[int(i)] for i in ids]
