"""Python mirror of the libdexgpu C-ABI (thin: device buffers, numpy in/out, errors -> exceptions).

Names follow the reference's tools and functions: `dexta/undexta/dexar/undexar/dexqv` are the
whole-file drivers (dexta.c ... dexqv.c); `Context.qv_*` are the batch forms of QVcoding_Scan,
Create_QVcoding and Compress_Next_QVentry (QV.h:48-97).  All compute happens in the HIP library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_NONE64 = 2**64 - 1                                           # the C-ABI's "no such unit / record / position"
_KINDS = {"fasta": L.DX_KIND_FASTA, "arrow": L.DX_KIND_ARROW, "quiva": L.DX_KIND_QUIVA}


# ---- one definition for each idiom of the calls below ------------------------------------------
def _kind(kind):
    """"fasta", "arrow" or "quiva" -> DX_KIND_* (anything else: KeyError)"""
    return _KINDS[kind]


def _addr(x):
    """a device array -> its address: a DevBuf, a DevView, a DeviceIndex._View or anything else with .ptr, or a torch tensor
    (data_ptr()); None -> None, the C-ABI's NULL, which the library answers with DX_E_ARG where the array is not optional"""
    if x is None:
        return None
    try:
        return x.ptr
    except AttributeError:
        return x.data_ptr()


def _need(x, name):
    """_addr for an array whose entry point launches without a NULL check of its own: None is refused here"""
    if x is None:
        raise TypeError(f"{name}: a device array, not None")
    return _addr(x)


def _dev(x):
    """a device array -> (its address, its bytes): a DevBuf, a DevView (bytes unknown: None), a torch tensor, or None"""
    if x is None:
        return None, 0
    return _addr(x), x.numel() * x.element_size() if hasattr(x, "data_ptr") else getattr(x, "nbytes", None)


def _words(lib, h):
    """the library's words for the last failure of context h (None: of a call without a context)"""
    return (lib.dx_last_error(h) or b"").decode()


def _error(rc, text, **attrs):
    """the DexGPUError of return code rc with `text` behind the code's name and attrs (bad_unit, line, ...) set on it"""
    e = L.DexGPUError(rc, text)
    e.__dict__.update(attrs)
    return e


def _index(word):
    """a c_uint64 the library left an index in -> that index, or None when the word is all ones"""
    return None if word.value == _NONE64 else word.value


def _unit_pos(word):
    """a c_uint64 of (unit << 32 | position) -> the pair, or None when the word is all ones"""
    return None if word.value == _NONE64 else (word.value >> 32, word.value & 0xffffffff)


class _Outs:
    """k pointers for a call to leave malloc'd results in (C.byref of each), given back to the library (dx_file_free) on the way out,
    whatever happened in between.  The library hands results over as its last step: after a call that failed they are all NULL."""

    def __init__(self, lib, k):
        self.lib, self.p = lib, [C.c_void_p() for _ in range(k)]

    def __enter__(self):
        return self.p

    def __exit__(self, *a):
        for p in self.p:
            self.lib.dx_file_free(p)


def _take(p, dtype, count, shape=None):
    """a copy of the `count` dtype values at the library's pointer p, as `shape` (None: flat).  Not a byte behind them is read, and
    with count 0 p is not read at all (it may be NULL): the result is empty, of that dtype and shape."""
    dt = np.dtype(dtype)
    if count:
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (count * dt.itemsize,)).view(dt).copy()
    else:
        a = np.zeros(0, dt)
    return a if shape is None else a.reshape(shape)


def _text(p, n):
    """a copy of the n.value bytes at the library's pointer p"""
    return C.string_at(p.value, n.value)


def _fields(s, skip=("reserved",)):
    """a C struct's fields as a dict, its padding word left out"""
    return {f: getattr(s, f) for f, _ in s._fields_ if f not in skip}


def _hist(hist=None):
    """an L.HIST (uint64 [6][256]) holding `hist`, or zeros"""
    h = L.HIST()
    if hist is not None:
        np.ctypeslib.as_array(h)[:] = np.asarray(hist, dtype=np.uint64).reshape(6, 256)
    return h


def _host_bytes(b):
    """bytes, or a numpy array (a big image: no copy into a bytes object) -> (what ctypes passes as its const uint8_t *, its size);
    the pointer made of an array keeps the array alive"""
    if isinstance(b, np.ndarray):
        b = np.ascontiguousarray(b, dtype=np.uint8)
        return b.ctypes.data_as(C.c_void_p), b.size
    return b, len(b)


def _patterns(patterns):
    """str or bytes patterns -> (the const char * array the file drivers take, how many)"""
    pats = [p.encode() if isinstance(p, str) else bytes(p) for p in patterns]
    return (C.c_char_p * max(len(pats), 1))(*pats), len(pats)


class DevView:
    """A pointer into a DevBuf (which stays the owner)."""

    def __init__(self, base: "DevBuf", byte_offset: int):
        self.base, self.ptr = base, base.ptr + int(byte_offset)


class DevBuf:
    """A device allocation owned by a Context."""

    def offset(self, nbytes: int) -> DevView:
        return DevView(self, nbytes)

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx._chk(ctx.lib.dx_malloc(ctx.h, self.nbytes + 64, C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.ctx.lib.dx_free(self.ctx.h, self.ptr)
            self.ptr = None

    def upload(self, arr) -> "DevBuf":
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        if a.nbytes:
            self.ctx._chk(self.ctx.lib.dx_h2d(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, dtype=np.uint8, count=None, offset=0) -> np.ndarray:
        dt = np.dtype(dtype)
        count = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(count, dtype=dt)
        if out.nbytes:
            self.ctx._chk(self.ctx.lib.dx_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def zero(self):
        self.ctx._chk(self.ctx.lib.dx_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self


class DeviceIndex:
    """The arrays dx_qv_walk_device left on the device (the library's memory: free())."""

    class _View:
        def __init__(self, ptr): self.ptr = ptr

    def __init__(self, ctx, x):
        self.ctx, self.x, self.n = ctx, x, int(x.n)
        self.pieces, self.piece_bytes = int(x.pieces), int(x.piece_bytes)
        self.rec_off, self.hdr_off = self._View(x.d_rec_off), self._View(x.d_hdr_off)
        self.seg, self.len, self.hdr4 = self._View(x.d_seg), self._View(x.d_len), self._View(x.d_hdr4)
        self.gidx_words, self.gidx_none, self.gidx_nosync = int(x.gidx_words), int(x.gidx_none), int(x.gidx_nosync)
        self.gidx = self._View(x.d_gidx) if x.d_gidx else None
        self.gidx_off = self._View(x.d_gidx_off) if x.d_gidx_off else None

    def use(self, d_in):
        """dx_qv_use_dindex: the run-coded lines' groups this walk has noted go to the decoder (d_in: the stream's device
        address, as dx_qv_decode will get it); use(None) takes them back."""
        self.ctx._chk(self.ctx.lib.dx_qv_use_dindex(self.ctx.h, _addr(d_in), C.byref(self.x) if d_in is not None else None))

    def download(self):
        """-> dict of numpy arrays, as qv_walk returns them"""
        n, out = self.n, {}
        for name, v, dt, shape in (("rec_off", self.rec_off, np.uint64, (n + 1,)), ("hdr_off", self.hdr_off, np.uint64, (n + 1,)),
                                   ("seg", self.seg, np.uint32, (n, 5)), ("len", self.len, np.uint32, (n,)), ("hdr4", self.hdr4, np.int32, (n, 4))):
            a = np.zeros(shape, dt)
            if a.nbytes:
                self.ctx._chk(self.ctx.lib.dx_d2h(self.ctx.h, a.ctypes.data, v.ptr, a.nbytes))
            out[name] = a
        out["n"] = n
        return out

    def free(self):
        if self.x is not None:
            self.ctx.lib.dx_qv_dindex_free(self.ctx.h, C.byref(self.x))
            self.x = None


class Context:
    def __init__(self, device: int = 0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.dx_open(device, C.byref(h))
        if rc != 0:
            raise _error(rc, _words(self.lib, None))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.dx_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _err(self, rc, text="{}", **attrs):
        """the DexGPUError of a call of this context that returned rc: `text` with the library's words for it in place of its {},
        and attrs set on it"""
        return _error(rc, text.format(_words(self.lib, self.h)), **attrs)

    def _chk(self, rc):
        if rc != 0:
            raise self._err(rc)

    def _bad_unit(self, rc, bad):
        return self._err(rc, bad_unit=_index(bad))

    # ---- memory ------------------------------------------------------------------------------
    def alloc(self, nbytes) -> DevBuf:
        return DevBuf(self, nbytes)

    def to_device(self, arr) -> DevBuf:
        a = np.ascontiguousarray(arr)
        return DevBuf(self, a.nbytes).upload(a)

    def _download(self, at, dtype, count):
        """`count` dtype values from the device address `at`, as a numpy array"""
        a = np.empty(count, dtype)
        if a.nbytes:
            self._chk(self.lib.dx_d2h(self.h, a.ctypes.data, at, a.nbytes))
        return a

    def sync(self):
        self._chk(self.lib.dx_sync(self.h))

    def set_stream(self, stream_ptr):
        self._chk(self.lib.dx_set_stream(self.h, stream_ptr))

    # ---- profiling ---------------------------------------------------------------------------
    def profile(self, enable=True):
        self._chk(self.lib.dx_profile(self.h, int(enable)))

    def kernel_times(self) -> dict:
        out = {}
        for k, name in enumerate(L.KERNELS):
            ms, cnt = C.c_double(), C.c_uint64()
            self._chk(self.lib.dx_profile_get(self.h, k, C.byref(ms), C.byref(cnt)))
            if cnt.value:
                out[name] = (ms.value, cnt.value)
        return out

    # ---- 2-bit packers -----------------------------------------------------------------------
    def pack2_encode(self, alphabet, d_text, d_off, d_tlen, d_nsym, n, d_hdr, d_hdr_off, d_out, d_out_off):
        self._chk(self.lib.dx_pack2_encode(self.h, alphabet, _need(d_text, "d_text"), _need(d_off, "d_off"), _need(d_tlen, "d_tlen"),
                                           _need(d_nsym, "d_nsym"), n, _addr(d_hdr), _addr(d_hdr_off), _need(d_out, "d_out"),
                                           _need(d_out_off, "d_out_off")))

    def pack2_decode(self, letters, d_in, d_in_off, d_nsym, n, width, d_out, d_out_off):
        self._chk(self.lib.dx_pack2_decode(self.h, letters, _need(d_in, "d_in"), _need(d_in_off, "d_in_off"), _need(d_nsym, "d_nsym"),
                                           n, width, _need(d_out, "d_out"), _need(d_out_off, "d_out_off")))

    # ---- QV coder ----------------------------------------------------------------------------
    @staticmethod
    def qv_batch(d_text, d_off, d_len, n, line_pad=1, text_bytes=0) -> L.QVBatch:
        return L.QVBatch(_need(d_text, "d_text"), _need(d_off, "d_off"), _need(d_len, "d_len"), n, text_bytes, line_pad)

    def qv_lossy_text(self, batch):
        """QV.c:1355-1372's rounding of the insertion / merge QVs, in place on the batch's device text."""
        self._chk(self.lib.dx_qv_lossy_text(self.h, C.byref(batch)))

    def qv_prescan(self, batch, entry0=0, params=None) -> L.QVParams:
        p = params or L.QVParams(-1, -1, -1, -1)
        self._chk(self.lib.dx_qv_prescan(self.h, C.byref(batch), entry0, C.byref(p)))
        return p

    def qv_hist(self, batch, params, entry0=0, hist=None, tot=0):
        """Returns (hist uint64 [6,256], totChar); adds into `hist`/`tot` when given (shards)."""
        h, t = _hist(hist), C.c_uint64(tot)
        self._chk(self.lib.dx_qv_hist(self.h, C.byref(batch), entry0, C.byref(params), C.byref(h), C.byref(t)))
        return np.ctypeslib.as_array(h).reshape(6, 256).copy(), t.value

    def qv_scan(self, batch, entry0=0, params=None, hist=None, tot=0):
        """dx_qv_scan: qv_prescan + qv_hist with one wait on the device.  Returns (params, hist uint64 [6,256], totChar)."""
        p = params or L.QVParams(-1, -1, -1, -1)
        h, t = _hist(hist), C.c_uint64(tot)
        self._chk(self.lib.dx_qv_scan(self.h, C.byref(batch), entry0, C.byref(p), C.byref(h), C.byref(t)))
        return p, np.ctypeslib.as_array(h).reshape(6, 256).copy(), t.value

    def qv_set_coding(self, coding, lossy=False):
        self._chk(self.lib.dx_qv_set_coding(self.h, C.byref(coding), int(lossy)))

    def qv_sizes(self, batch, d_hdr_off, d_seg, d_rec_off) -> int:
        tot = C.c_uint64()
        self._chk(self.lib.dx_qv_sizes(self.h, C.byref(batch), _addr(d_hdr_off), _need(d_seg, "d_seg"), _need(d_rec_off, "d_rec_off"),
                                       C.byref(tot)))
        return tot.value

    def qv_encode(self, batch, d_hdr, d_hdr_off, d_rec_off, d_seg, d_out):
        self._chk(self.lib.dx_qv_encode(self.h, C.byref(batch), _addr(d_hdr), _addr(d_hdr_off), _need(d_rec_off, "d_rec_off"),
                                        _need(d_seg, "d_seg"), _need(d_out, "d_out")))

    def qv_encode_onepass(self, batch, d_hdr, d_hdr_off, d_seg, d_rec_off, d_out, out_cap) -> int:
        """dx_qv_encode_onepass: sizes, offsets and the record stream without a size pass; returns the total."""
        tot = C.c_uint64()
        self._chk(self.lib.dx_qv_encode_onepass(self.h, C.byref(batch), _addr(d_hdr), _addr(d_hdr_off), _need(d_seg, "d_seg"),
                                                _need(d_rec_off, "d_rec_off"), _need(d_out, "d_out"), out_cap, C.byref(tot)))
        return tot.value

    def qv_encode_onepass_begin(self, batch, d_hdr, d_hdr_off, d_seg, d_rec_off, d_out, out_cap):
        """dx_qv_encode_onepass_begin: queue the encode; the next batch's prescan / hist / build / set_coding may follow."""
        self._chk(self.lib.dx_qv_encode_onepass_begin(self.h, C.byref(batch), _addr(d_hdr), _addr(d_hdr_off), _need(d_seg, "d_seg"),
                                                      _need(d_rec_off, "d_rec_off"), _need(d_out, "d_out"), out_cap))

    def qv_encode_onepass_end(self) -> int:
        """dx_qv_encode_onepass_end: wait for the encode that has begun; returns the stream's size."""
        tot = C.c_uint64()
        self._chk(self.lib.dx_qv_encode_onepass_end(self.h, C.byref(tot)))
        return tot.value

    def qv_decode(self, d_in, d_rec_off, d_hdr_off, d_seg, d_len, n, upper, d_out, d_out_off, flip=False):
        flags = (1 if upper else 0) | (2 if flip else 0)          # DX_DECODE_UPPER | DX_DECODE_FLIP
        self._chk(self.lib.dx_qv_decode(self.h, _need(d_in, "d_in"), _need(d_rec_off, "d_rec_off"), _addr(d_hdr_off),
                                        _need(d_seg, "d_seg"), _need(d_len, "d_len"), n, flags, _need(d_out, "d_out"),
                                        _need(d_out_off, "d_out_off")))

    def qv_walk_device(self, d_img, nbytes, first, coding, newv=1, flip=0):
        """dx_qv_walk_device: the record walk of the bare stream at d_img on the device -> DeviceIndex (device arrays
        rec_off, hdr_off, seg, len, hdr4 as views that dx_qv_decode takes; .free() when done).  Raises DexGPUError
        (DX_E_MISMATCH) when the stream has to be walked on the host."""
        x = L.QVDIndex()
        self._chk(self.lib.dx_qv_walk_device(self.h, _need(d_img, "d_img"), nbytes, first, C.byref(coding), newv, flip, C.byref(x)))
        return DeviceIndex(self, x)

    def qv_walk_records_device(self, d_buf, nbytes, d_start, d_len, n, coding, d_seg, flip=False):
        """dx_qv_walk_records_device: the five segment sizes of the n records that start at d_buf + d_start[i] (no framing
        bytes, d_len[i] symbols a line) into d_seg (n x 5 uint32) -- with d_start as d_rec_off what qv_decode takes.  Raises
        DexGPUError (DX_E_FORMAT, .bad_entry = the first such i) when a record does not end inside the nbytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_qv_walk_records_device(self.h, _need(d_buf, "d_buf"), int(nbytes), _need(d_start, "d_start"),
                                                _need(d_len, "d_len"), int(n), C.byref(coding), int(bool(flip)),
                                                _need(d_seg, "d_seg"), C.byref(bad))
        if rc != 0:
            raise self._err(rc, bad_entry=_index(bad))

    def entries_compress(self, lines_per_entry, lossy=False):
        """dx_entries_new / _add / _compress (QVcoding_Scan1 + Compress_Next_QVentry1 as a batch, what dex2DB writes into a
        .qvs track): lines_per_entry = per entry its five lines (bytes of one length) -> (coding, records: bytes -- the bare
        record stream --, coff: uint64 [n + 1], entry i's offset in it)."""
        e = self.lib.dx_entries_new()
        if not e:
            raise MemoryError("dx_entries_new")
        try:
            for lines in lines_per_entry:
                lines = [bytes(x) for x in lines]
                if len(lines) != 5 or any(len(x) != len(lines[0]) for x in lines):
                    raise ValueError("an entry is five lines of one length")
                rc = self.lib.dx_entries_add(e, len(lines[0]), *lines)
                if rc != 0:
                    raise L.DexGPUError(rc, "dx_entries_add")
            n = len(lines_per_entry)
            coding, nb = L.QVCoding(), C.c_size_t()
            with _Outs(self.lib, 2) as (rec, coff):
                self._chk(self.lib.dx_entries_compress(self.h, e, int(bool(lossy)), C.byref(coding), C.byref(rec), C.byref(nb), C.byref(coff)))
                return coding, _text(rec, nb), _take(coff, np.uint64, n + 1)
        finally:
            self.lib.dx_entries_free(e)

    def entries_uncompress(self, coding, records, coff, rlen, ids=None, ascii=1, flip=False):
        """dx_entries_uncompress (Load_QVentry, DB.c:2575-2621, for a selection at once): entry ids[j] (None: every entry of
        rlen, in order) starts at records[coff[ids[j]]] and has rlen[ids[j]] symbols a line -> (text: bytes, toff: uint64
        [len(ids) + 1]); its five lines, '\n' after each, are text[toff[j]: toff[j + 1]].  ascii as Load_QVentry's: 1 lower-case
        tag line, 2 upper-case, 0 numbers.  One coding per call."""
        coff = np.ascontiguousarray(coff, dtype=np.uint64)
        rlen = np.ascontiguousarray(rlen, dtype=np.uint32)
        if ids is None:
            n_ids, idp = len(rlen), None
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            if len(ids) and int(ids.max()) >= min(len(rlen), len(coff)):
                raise IndexError("an id beyond the entries of coff / rlen")
            n_ids, idp = len(ids), ids.ctypes.data
        rp, nb = _host_bytes(records)
        if ids is None and len(coff) < n_ids:
            raise IndexError("fewer offsets than lengths")
        n = C.c_size_t()
        with _Outs(self.lib, 2) as (out, toff):
            self._chk(self.lib.dx_entries_uncompress(self.h, C.byref(coding), int(bool(flip)), rp, nb, coff.ctypes.data, rlen.ctypes.data,
                                                     idp, n_ids, int(ascii), C.byref(out), C.byref(n), C.byref(toff)))
            return _text(out, n), _take(toff, np.uint64, n_ids + 1)

    def reads_unpack(self, letters, d_in, in_bytes, d_boff, d_beg, d_len, n, d_out, d_out_off):
        """dx_reads_unpack: unit j = symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j] (d_beg None:
        whole reads from symbol 0) as d_len[j] bytes of `letters` and one delimiter behind them at d_out + d_out_off[j].  Raises
        DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a unit does not lie inside the in_bytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_reads_unpack(self.h, int(letters), _need(d_in, "d_in"), int(in_bytes), _need(d_boff, "d_boff"), _addr(d_beg),
                                      _need(d_len, "d_len"), int(n), _need(d_out, "d_out"), _need(d_out_off, "d_out_off"),
                                      C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)

    @staticmethod
    def _reads_selection(boff, rlen, ids, beg, end):
        """the argument checks of reads_uncompress, before any device call -> (boff, rlen, ids or None, beg or None, end or None, n)"""
        boff = np.ascontiguousarray(boff, dtype=np.uint64)
        rlen = np.ascontiguousarray(rlen, dtype=np.uint32)
        if len(boff) < len(rlen):
            raise IndexError("fewer offsets than lengths")
        if ids is None:
            n, of = len(rlen), rlen
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            if len(ids) and int(ids.max()) >= len(rlen):
                raise IndexError("an id beyond the reads of boff / rlen")
            n, of = len(ids), rlen[ids.astype(np.int64)]
        if (beg is None) != (end is None):
            raise ValueError("beg and end are given together")
        if beg is not None:
            if np.any(np.asarray(beg) < 0) or np.any(np.asarray(end) < 0):
                raise ValueError("a negative beg or end")
            beg = np.ascontiguousarray(beg, dtype=np.uint32)
            end = np.ascontiguousarray(end, dtype=np.uint32)
            if len(beg) != n or len(end) != n:
                raise ValueError("beg / end: one value a selected read")
            if np.any(beg > end):
                raise ValueError("a subread with beg > end")
            if np.any(end > of):
                raise ValueError("a subread that ends behind its read (end > rlen)")
        return boff, rlen, ids, beg, end, n

    def reads_uncompress(self, payload, boff, rlen, ids=None, beg=None, end=None, letters=L.DX_LETTERS_NUMBERS):
        """dx_reads_uncompress (Load_Read / Load_Subread / Load_Arrow, DB.c:1232-1381, 1508-1548, for a selection at once): read
        ids[j] (None: every read of rlen, in order) starts at payload[boff[ids[j]]] and has rlen[ids[j]] symbols; all of it, or
        its symbols [beg[j], end[j]) -> (text: bytes, toff: uint64 [len(ids) + 1]) in Load_All_Reads' layout: unit j is
        text[toff[j]: toff[j + 1] - 1], a delimiter (4 for numbers, 0 for letters) in front of it and behind it."""
        boff, rlen, ids, beg, end, n_ids = self._reads_selection(boff, rlen, ids, beg, end)
        if not (L.DX_LETTERS_LOWER <= int(letters) <= L.DX_LETTERS_NUMBERS):
            raise ValueError("unknown letter set")
        pp, nb = _host_bytes(payload)
        n = C.c_size_t()
        with _Outs(self.lib, 2) as (out, toff):
            self._chk(self.lib.dx_reads_uncompress(self.h, int(letters), pp, nb, boff.ctypes.data, rlen.ctypes.data, _ptr(ids), _ptr(beg),
                                                   _ptr(end), n_ids, C.byref(out), C.byref(n), C.byref(toff)))
            return _text(out, n), _take(toff, np.uint64, n_ids + 1)

    def _index_device(self, fn, args, dev, host):
        """the two device indexers: fn(ctx, *args, the device arrays, &n, the header arrays, &prefix_len, &line, &code) ->
        [the n values of each device array (its dtype in `dev`), the n x 4 of each malloc'd header array (`host`), prefix_len].  The
        arrays are the caller's, so they are released here on every path once the call has succeeded."""
        d, hd = [C.c_void_p() for _ in dev], [C.c_void_p() for _ in host]
        cnt, pl, line, code = C.c_uint64(), C.c_size_t(), C.c_uint64(), C.c_int()
        rc = fn(self.h, *args, *[C.byref(p) for p in d], C.byref(cnt), *[C.byref(p) for p in hd], C.byref(pl), C.byref(line),
                C.byref(code))
        if rc != 0:
            raise _error(rc, f"line {line.value}: DX_IDX code {code.value}", line=line.value, idx_code=code.value)
        try:
            out = [self._download(p, dt, cnt.value) for p, dt in zip(d, dev)]
            return out + [_take(p, dt, 4 * cnt.value, (cnt.value, 4)) for p, dt in zip(hd, host)] + [pl.value]
        finally:
            for p in d:
                self.lib.dx_free(self.h, p)
            for p in hd:
                C.CDLL(None).free(p)

    def index_quiva_device(self, d_text, nbytes):
        """GPU text front end -> (off uint64, len uint32, hdr4 int32 [n,4], prefix_len); raises
        DexGPUError(DX_E_FORMAT) with .line / .idx_code on a malformed image."""
        return tuple(self._index_device(self.lib.dx_index_quiva_device, (_need(d_text, "d_text"), nbytes), (np.uint64, np.uint32),
                                        (np.int32,)))

    def index_seq_device(self, d_text, nbytes, arrow=False):
        """GPU text front end for .fasta/.arrow -> (off, tlen, nsym, hdr4, cnr4, prefix_len)."""
        return tuple(self._index_device(self.lib.dx_index_seq_device, (int(arrow), _need(d_text, "d_text"), nbytes),
                                        (np.uint64, np.uint32, np.uint32), (np.int32, np.uint16)))

    def synth_quiva(self, seed, entry0, n, d_off, d_len, d_hdr4, d_lut, del_run, movie, d_text):
        self._chk(self.lib.dx_synth_quiva(self.h, seed & 0xFFFFFFFF, entry0, n, _need(d_off, "d_off"), _need(d_len, "d_len"),
                                          _need(d_hdr4, "d_hdr4"), _need(d_lut, "d_lut"), del_run, movie.encode(),
                                          _need(d_text, "d_text")))

    # ---- whole-file drivers (what the CLI tools call) -------------------------------------------
    def _file_call(self, fn, *args, idx):
        """fn(ctx, *args, &out, &n) -> the bytes it made; idx: the entry point indexes text, and reports (&line, &code) behind them"""
        n, line, code = C.c_size_t(), C.c_uint64(), C.c_int()
        with _Outs(self.lib, 1) as (out,):
            rc = fn(self.h, *args, C.byref(out), C.byref(n), *((C.byref(line), C.byref(code)) if idx else ()))
            if rc != 0:
                raise self._err(rc, f"line {line.value}: input rejected (DX_IDX code {code.value}) {{}}" if rc == -3 and idx else "{}")
            return _text(out, n)

    def dexta(self, fasta: bytes) -> bytes:
        return self._file_call(self.lib.dx_file_pack2, 0, fasta, len(fasta), idx=True)

    def dexar(self, arrow: bytes) -> bytes:
        return self._file_call(self.lib.dx_file_pack2, 1, arrow, len(arrow), idx=True)

    def undexta(self, img: bytes, upper=False, width=80) -> bytes:
        return self._file_call(self.lib.dx_file_unpack2, L.DX_LETTERS_UPPER if upper else L.DX_LETTERS_LOWER,
                               img, len(img), width, idx=False)

    def undexar(self, img: bytes, width=80) -> bytes:
        return self._file_call(self.lib.dx_file_unpack2, L.DX_LETTERS_ARROW, img, len(img), width, idx=False)

    def dexqv(self, quiva: bytes, lossy=False) -> bytes:
        return self._file_call(self.lib.dx_file_dexqv, quiva, len(quiva), int(lossy), idx=True)

    def qv_use_index(self, d_in, d_seg, n, d_gidx, d_gidx_off, none=0):
        """dx_qv_use_index: a group index made elsewhere (qv_walk(index=True)) for the stream at d_in / d_seg; d_gidx None: take it back"""
        self._chk(self.lib.dx_qv_use_index(self.h, _addr(d_in), _addr(d_seg), n, _addr(d_gidx), _addr(d_gidx_off), none))

    def undexqv(self, img: bytes, upper=False) -> bytes:
        return self._file_call(self.lib.dx_file_undexqv, img, len(img), int(upper), idx=False)

    # ---- round-trip check --------------------------------------------------------------------------
    def verify_ranges(self, d_a, d_a_off, d_a_len, d_b, d_b_off, d_b_len, n, count=True):
        """dx_verify_ranges: (first differing unit or None, first differing byte in it, differing units -- None when count=False,
        which also lets the kernel skip what lies behind a difference already found)"""
        unit, pos, differ = C.c_uint64(), C.c_uint32(), C.c_uint64()
        self._chk(self.lib.dx_verify_ranges(self.h, _need(d_a, "d_a"), _need(d_a_off, "d_a_off"), _need(d_a_len, "d_a_len"),
                                            _need(d_b, "d_b"), _need(d_b_off, "d_b_off"), _need(d_b_len, "d_b_len"), n,
                                            C.byref(unit), C.byref(pos), C.byref(differ) if count else None))
        return _index(unit), pos.value, (differ.value if count else None)

    def verify(self, kind, text: bytes, img: bytes, lossy=False) -> dict:
        """dx_file_verify: does img (a .dexta / .dexar / .dexqv image) give text back?  kind: "fasta", "arrow" or "quiva".  The
        report as a dict; `where` is one of _lib.VERIFY_WHERE, `error` the library's words when it is "IMAGE"."""
        rep = L.VerifyReport()
        self._chk(self.lib.dx_file_verify(self.h, _kind(kind), text, len(text), img, len(img), int(lossy), C.byref(rep)))
        out = _fields(rep)
        out["ok"], out["upper"], out["where"] = bool(rep.ok), bool(rep.upper), L.VERIFY_WHERE[rep.where]
        if out["where"] == "IMAGE":
            out["error"] = _words(self.lib, self.h)
        return out

    # ---- digest ------------------------------------------------------------------------------------
    def crc32_ranges(self, d_buf, buf_bytes, d_off, d_len, n, d_crc):
        """dx_crc32_ranges: d_crc[j] = zlib's CRC-32 of d_buf[d_off[j] .. d_off[j] + d_len[j]) (offsets and lengths: uint64 on the
        device).  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a unit does not lie inside the buf_bytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_crc32_ranges(self.h, _addr(d_buf), int(buf_bytes), _addr(d_off), _addr(d_len), int(n), _addr(d_crc),
                                      C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)

    def crc32_fold(self, d_crc, d_len, n):
        """dx_crc32_fold: (CRC-32, length) of the units' concatenation in index order, from their CRCs (uint32) and lengths (uint64)"""
        crc, nbytes = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.dx_crc32_fold(self.h, _addr(d_crc), _addr(d_len), int(n), C.byref(crc), C.byref(nbytes)))
        return crc.value, nbytes.value

    def digest(self, kind, img: bytes, upper=False, width=80, per_record=False) -> dict:
        """dx_file_digest: the CRC-32 (zlib's) and size of the text undexta / undexar / undexqv writes for img with these options,
        decoded and hashed on the device.  kind: "fasta", "arrow" or "quiva".  {"crc32", "bytes", "records"}, and with per_record
        "rec_crc": every record's own CRC-32 (its header line included) as a uint32 array."""
        dg = L.Digest()
        with _Outs(self.lib, 1) as (rec,):
            self._chk(self.lib.dx_file_digest(self.h, _kind(kind), img, len(img), int(bool(upper)), int(width), C.byref(dg),
                                              C.byref(rec) if per_record else None))
            out = {"crc32": dg.crc32, "bytes": dg.bytes, "records": dg.records}
            if per_record:
                out["rec_crc"] = _take(rec, np.uint32, dg.records)
        return out

    # ---- census ------------------------------------------------------------------------------------
    def code_counts(self, d_in, in_bytes, d_boff, d_beg, d_len, n, d_counts=None):
        """dx_code_counts: unit j = symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j] (d_beg None: whole
        reads from symbol 0); d_counts (uint32, n x 4, or None) gets every unit's symbols code by code, the four totals over the
        call's units come back as a uint64 array.  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a unit does
        not lie inside the in_bytes."""
        tot, bad = (C.c_uint64 * 4)(), C.c_uint64()
        rc = self.lib.dx_code_counts(self.h, _addr(d_in), int(in_bytes), _addr(d_boff), _addr(d_beg), _addr(d_len), int(n),
                                     _addr(d_counts), C.byref(tot), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)
        return np.array(list(tot), dtype=np.uint64)

    def byte_hist_ranges(self, d_buf, buf_bytes, d_off, d_len, d_kind, nkinds, n, d_sum=None):
        """dx_byte_hist_ranges: range j = d_buf[d_off[j] .. d_off[j] + d_len[j]) (uint64 on the device) adds its bytes' values to table
        d_kind[j] (uint8; None: all 0) of nkinds (1 to 8); d_sum (uint64, n, or None) gets every range's byte sum.  The tables come
        back as a uint64 array (nkinds, 256).  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) for a range outside
        the buf_bytes or a kind that is not below nkinds."""
        nk = int(nkinds)
        hist, bad = np.zeros((max(nk, 1), 256), dtype=np.uint64), C.c_uint64()
        rc = self.lib.dx_byte_hist_ranges(self.h, _addr(d_buf), int(buf_bytes), _addr(d_off), _addr(d_len), _addr(d_kind), nk, int(n),
                                          _addr(d_sum), hist.ctypes.data, C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)
        return hist

    def census(self, kind, img: bytes, per_record=False) -> dict:
        """dx_file_census: what the image holds, counted on the device (no text is made or downloaded).  kind: "fasta", "arrow" or
        "quiva".  {"records", "symbols", "min_len", "max_len", "n50", "code" (uint64[4]), "hist" (uint64[5, 256])}, and with
        per_record "rec_len" (uint32) and "rec_code" (uint32 [n, 4]; fasta, arrow) or "rec_sum" (uint64 [n, 5]; quiva)."""
        cs = L.Census()
        with _Outs(self.lib, 3) as (rl, rc_, rs):
            self._chk(self.lib.dx_file_census(self.h, _kind(kind), img, len(img), C.byref(cs), C.byref(rl) if per_record else None,
                                              C.byref(rc_) if per_record else None, C.byref(rs) if per_record else None))
            out, n = census_dict(cs), cs.records
            if per_record:
                out["rec_len"] = _take(rl, np.uint32, n)
                if rc_.value:
                    out["rec_code"] = _take(rc_, np.uint32, 4 * n, (n, 4))
                if rs.value:
                    out["rec_sum"] = _take(rs, np.uint64, 5 * n, (n, 5))
        return out

    # ---- compare -----------------------------------------------------------------------------------
    def diff_ranges(self, d_a, a_bytes, d_a_off, d_b, b_bytes, d_b_off, d_len, n, d_kind=None, nkinds=1, a_and=None,
                    d_differ=None, d_first=None) -> dict:
        """dx_diff_ranges: unit j = d_a[d_a_off[j] .. + d_len[j]) against d_b[d_b_off[j] .. + d_len[j]) (offsets uint64, lengths
        uint32, on the device); d_kind (uint8; None: all 0) names one of nkinds (1 to 8) tallies, a_and (nkinds byte values; None:
        all 0xff) is ANDed onto side a's bytes first.  d_differ / d_first (uint32, n, or None) get every unit's differing bytes and
        the first of them (2**32 - 1: none).  {"differ", "units", "sum_abs", "max_abs"} (uint64 arrays, a kind each) and "first":
        (unit, position) of the first difference, or None.  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) for a
        range outside either buffer or a kind that is not below nkinds."""
        nk = int(nkinds)
        tally, first, bad = (L.DiffTally * max(nk, 1))(), C.c_uint64(), C.c_uint64()
        masks = None if a_and is None else (C.c_uint8 * max(nk, 1))(*[int(v) for v in a_and])
        rc = self.lib.dx_diff_ranges(self.h, _addr(d_a), int(a_bytes), _addr(d_a_off), _addr(d_b), int(b_bytes), _addr(d_b_off),
                                     _addr(d_len), _addr(d_kind), nk, masks, int(n), _addr(d_differ), _addr(d_first), tally,
                                     C.byref(first), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)
        out = {f: np.array([getattr(t, f) for t in tally][:nk], dtype=np.uint64) for f, _ in L.DiffTally._fields_}
        out["first"] = _unit_pos(first)
        return out

    def code_diff(self, d_a, a_bytes, d_a_boff, d_b, b_bytes, d_b_boff, d_len, n, d_differ=None, d_first=None) -> dict:
        """dx_code_diff: unit j = the first d_len[j] symbols of the packed read at d_a + d_a_boff[j] against those of the one at
        d_b + d_b_boff[j]; the pad bits of a read's last byte are not compared.  d_differ / d_first as for diff_ranges, in
        symbols.  {"symbols", "units", "first": (unit, symbol) or None}.  Raises DexGPUError (DX_E_FORMAT, .bad_unit) when a unit
        does not lie inside its side's bytes."""
        tot, first, bad = (C.c_uint64 * 2)(), C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_diff(self.h, _addr(d_a), int(a_bytes), _addr(d_a_boff), _addr(d_b), int(b_bytes), _addr(d_b_boff),
                                   _addr(d_len), int(n), _addr(d_differ), _addr(d_first), C.byref(tot), C.byref(first), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)
        return {"symbols": tot[0], "units": tot[1], "first": _unit_pos(first)}

    def compare(self, kind, a: bytes, b: bytes, lossy=False, per_record=False) -> dict:
        """dx_file_compare: how two images of one kind ("fasta", "arrow" or "quiva") differ, records paired by index, compared on the
        device without either text.  The fields of dx_compare as a dict -- `same` a bool, the first_* None when there is none, the
        per-line fields uint64 arrays of `lines` values -- and with per_record "rec_differ": uint32 [records compared, lines].
        lossy (quiva): side a's insertion and merge lines are masked as dexqv -l rounds them."""
        cm = L.Compare()
        with _Outs(self.lib, 1) as (rec,):
            self._chk(self.lib.dx_file_compare(self.h, _kind(kind), a, len(a), b, len(b), int(bool(lossy)), C.byref(cm),
                                               C.byref(rec) if per_record else None))
            out = compare_dict(cm)
            if per_record:
                n, ln = min(cm.records_a, cm.records_b), cm.lines
                out["rec_differ"] = _take(rec, np.uint32, n * ln, (n, ln))
        return out

    # ---- find --------------------------------------------------------------------------------------
    def _listed(self, call, cap, dtype, d_list=None):
        """the scheme of the listing calls: call(address of a device list of `cap` 16-byte entries) -> how many there were to list;
        the list is d_list, or with None made and freed here (cap 0: none, NULL).  Returns the first min(cap, found) entries."""
        own = self.alloc(16 * cap + 16) if d_list is None and cap > 0 else None
        try:
            at = _addr(own if own is not None else d_list)
            return self._download(at, dtype, min(cap, call(at)))
        finally:
            if own is not None:
                own.free()

    def _code_find(self, fn, q, nq, d_in, in_bytes, d_boff, d_beg, d_len, n, d_count, cap, d_hits):
        """dx_code_find / dx_code_find_edit: one argument list, one answer; q: the nq queries as the entry point's array"""
        cap, tot, hits, bad = int(cap), (C.c_uint64 * max(nq, 1))(), C.c_uint64(), C.c_uint64()

        def call(p_hits):
            rc = fn(self.h, _addr(d_in), int(in_bytes), _addr(d_boff), _addr(d_beg), _addr(d_len), int(n), q, nq, _addr(d_count),
                    p_hits, cap, tot, C.byref(hits), C.byref(bad))
            if rc != 0:
                raise self._bad_unit(rc, bad)
            return hits.value
        lst = self._listed(call, cap, HIT_DTYPE, d_hits)
        return {"hits": hits.value, "total": np.array(list(tot)[:nq], dtype=np.uint64)}, lst

    def code_find(self, d_in, in_bytes, d_boff, d_beg, d_len, n, queries, d_count=None, cap=0, d_hits=None):
        """dx_code_find: unit j = symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j] (d_beg None: whole
        reads from symbol 0); queries: (code, len, max_mis) triples, symbol i of a query in bits 2 (len - 1 - i) + 1, 2 (len - 1 - i)
        of its code.  d_count (uint32, n, or None) gets every unit's hits; d_hits (16 cap bytes, or None: made here) the list.
        ({"hits": all of them, "total": uint64 a query}, the first min(cap, hits) hits in the order (unit, pos, query) as a
        HIT_DTYPE array).  Raises DexGPUError (DX_E_FORMAT,
        .bad_unit = the first such j) when a unit does not lie inside the in_bytes."""
        nq = len(queries)
        q = (L.Query * max(nq, 1))(*[L.Query(int(c), int(m), int(x)) for c, m, x in queries])
        return self._code_find(self.lib.dx_code_find, q, nq, d_in, in_bytes, d_boff, d_beg, d_len, n, d_count, cap, d_hits)

    def find(self, kind, img: bytes, patterns, max_mismatches=0, both_strands=False, max_hits=1 << 20, per_record=False):
        """dx_file_find: where the patterns (str, 1 to 32 letters: acgtACGT for "fasta", 1234 for "arrow") occur in the reads of the
        image, within max_mismatches substitutions, searched on the device in the packed reads (no text is made).  both_strands
        ("fasta"): the reverse complements too, strand 1.  ({"records", "records_hit", "hits", "listed", "per_pattern": uint64
        [patterns, 2]} and with per_record "rec_hits": uint32 a record, the first max_hits hits in the order (record, pos, pattern,
        strand) as a HIT_DTYPE array, `query` being the pattern's index)."""
        return self._file_find(self.lib.dx_file_find, kind, img, patterns, max_mismatches, both_strands, max_hits, per_record)

    def _file_find(self, fn, kind, img, patterns, bound, both_strands, max_hits, per_record, spans=False):
        """dx_file_find / dx_file_find_edit / (spans) dx_file_find_edit_spans: one argument list, one report"""
        k, (arr, npat), fd = _kind(kind), _patterns(patterns), L.Find()
        with _Outs(self.lib, 4) as (lst, rec, st, rl):
            self._chk(fn(self.h, k, img, len(img), arr, npat, int(bound), int(bool(both_strands)), int(max_hits), C.byref(fd),
                         C.byref(lst), C.byref(rec) if per_record else None, *((C.byref(st), C.byref(rl)) if spans else ())))
            out = {"records": fd.records, "records_hit": fd.records_hit, "hits": fd.hits, "listed": fd.listed,
                   "per_pattern": np.array([[fd.per_pattern[p][0], fd.per_pattern[p][1]] for p in range(npat)],
                                           dtype=np.uint64).reshape(npat, 2)}
            hits = _take(lst, HIT_DTYPE, fd.listed)
            if spans:
                out["start"], out["rec_len"] = _take(st, np.uint32, fd.listed), _take(rl, np.uint32, fd.records)
            if per_record:
                out["rec_hits"] = _take(rec, np.uint32, fd.records)
        return out, hits

    # ---- find with indels ----------------------------------------------------------------------------
    def code_find_edit(self, d_in, in_bytes, d_boff, d_beg, d_len, n, queries, d_count=None, cap=0, d_hits=None):
        """dx_code_find_edit: units as for code_find; queries: (codes, max_err) pairs, codes being 1 to 64 symbols 0..3, or ready
        (code0, code1, len, max_err) tuples (symbol i in bits 2 (31 - (i & 31)) + 1, 2 (31 - (i & 31)) of code[i >> 5]).  A hit is an
        end e with c(e) <= k, c(e) < c(e - 1) and c(e) <= c(e + 1), c being the semi-global edit distance capped at k + 1: one hit for
        each valley of the distance, at the leftmost end of its floor; pos = e, the exclusive end of the occurrence, mis = the
        distance.  Returns what code_find returns, in the same order (unit, pos, query)."""
        nq = len(queries)
        q = (L.EQuery * max(nq, 1))(*[equery(*x) for x in queries])
        return self._code_find(self.lib.dx_code_find_edit, q, nq, d_in, in_bytes, d_boff, d_beg, d_len, n, d_count, cap, d_hits)

    def find_edit(self, kind, img: bytes, patterns, max_errors=0, both_strands=False, max_hits=1 << 20, per_record=False):
        """dx_file_find_edit: where the patterns (str, 1 to 64 letters) END in the reads of the image within max_errors edits
        (substitution, insertion and deletion cost one each; the start in the read is free): one hit for each valley of the distance,
        at the leftmost end of its floor, pos = the exclusive end of the occurrence on the read as stored, mis = the distance.
        Everything else, and what is returned, as for find."""
        return self._file_find(self.lib.dx_file_find_edit, kind, img, patterns, max_errors, both_strands, max_hits, per_record)

    # ---- cut: where the occurrences start, and an image cut at them ----------------------------------
    def code_hit_starts(self, d_in, in_bytes, d_boff, d_beg, d_len, n, queries, d_hits, n_hits, d_start=None):
        """dx_code_hit_starts: units and queries as for code_find_edit; d_hits: n_hits hits on the device exactly as code_find_edit
        left them.  For every hit the LARGEST s with Levenshtein(query, unit[s, pos)) == mis -- the start of the shortest stretch that
        ends at pos and lies mis edits from the query.  d_start (uint32, n_hits, or None: made here): the starts, which come back as a
        uint32 array.  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the smallest index of a bad hit, whose start is 2**32 - 1; the
        others' are written, and .starts has them all) for a hit that is none of these units and queries."""
        nq, n_hits = len(queries), int(n_hits)
        q = (L.EQuery * max(nq, 1))(*[equery(*x) for x in queries])
        bad = C.c_uint64()
        own = self.alloc(4 * n_hits + 16) if d_start is None and n_hits > 0 else None
        try:
            at = _addr(own if own is not None else d_start)
            rc = self.lib.dx_code_hit_starts(self.h, _addr(d_in), int(in_bytes), _addr(d_boff), _addr(d_beg), _addr(d_len), int(n), q, nq,
                                             _addr(d_hits), n_hits, at, C.byref(bad))
            starts = None
            if rc in (0, -3) and n_hits and at is not None and n_hits < 2**32:
                starts = self._download(at, np.uint32, n_hits)
            if rc != 0:
                raise self._err(rc, bad_unit=_index(bad), starts=starts)
        finally:
            if own is not None:
                own.free()
        return starts if starts is not None else np.zeros(0, np.uint32)

    def find_spans(self, kind, img: bytes, patterns, max_errors=0, both_strands=False, max_hits=1 << 20, per_record=False):
        """dx_file_find_edit_spans: find_edit's return -- the same report, the same hits -- and in the report "start": uint32, one a
        listed hit, the first symbol of its occurrence on the read as stored (the occurrence is the record's symbols [start, pos)),
        and "rec_len": uint32 a record, its symbols."""
        return self._file_find(self.lib.dx_file_find_edit_spans, kind, img, patterns, max_errors, both_strands, max_hits, per_record,
                               spans=True)

    def cut(self, kind, img: bytes, patterns, max_errors=0, both_strands=False, min_len=0, mode="split"):
        """dx_file_cut: the image ("fasta" or "arrow") with the occurrences of the patterns within max_errors edits cut out of its
        records -- find_spans with every hit listed, cut_plan, subset -- byte for byte what dexta / dexar writes for the cut text.
        mode: "split" (every piece of at least min_len symbols between the occurrences, the id repeating), "longest" (the longest
        such piece of a record, on a tie the first) or "drop" (only the records without an occurrence, whole).  Returns (image,
        report, selection): the report is cut_plan's, and the selection {"ids", "beg", "end"} is what Context.subset takes to cut the
        .dexar and the .dexqv of the same records in the same places."""
        k, (arr, npat) = _kind(kind), _patterns(patterns)
        ln, cut, n = C.c_size_t(), L.Cut(), C.c_uint64()
        with _Outs(self.lib, 4) as (out, *sel):
            self._chk(self.lib.dx_file_cut(self.h, k, img, len(img), arr, npat, int(max_errors), int(bool(both_strands)),
                                           int(min_len), _cut_mode(mode), C.byref(out), C.byref(ln), C.byref(cut),
                                           *[C.byref(a) for a in sel], C.byref(n)))
            return _text(out, ln), cut_dict(cut), _cut_selection(sel, n.value)

    # ---- k-mers ------------------------------------------------------------------------------------
    def code_kmers(self, d_in, boff, beg, length, k, canonical=False, table=None, in_bytes=None, n=None):
        """dx_code_kmers: unit j = symbols [beg[j], beg[j] + length[j]) of the packed read at d_in + boff[j] (beg None: whole reads
        from symbol 0); every window of k symbols (1 to 14) adds one to cell `code` of the table, the first symbol on top of the
        code, with canonical to cell min(code, rc).  The arguments are device arrays: torch tensors (uint8; int64 / uint64; int32 /
        uint32) or DevBufs; in_bytes and n default to what d_in and length hold.  table: 4^k 64-bit counters that are ADDED to; None
        makes a zeroed torch int64 tensor on the context's device (a process that uses torch starts it before it opens a Context,
        torch.cuda.init(), as tools/ do).  Returns (table, windows of this call).  Raises DexGPUError
        (DX_E_FORMAT, .bad_unit = the first such j) when a unit does not lie inside the in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        k = int(k)
        if table is None and 1 <= k <= 14:
            import torch                                          # (only here: who brings a table of their own needs none)
            table = torch.zeros(4 ** k, dtype=torch.int64, device=f"cuda:{self.device}")
            torch.cuda.synchronize(self.device)                   # (zeroed on torch's stream, counted into on the context's)
        win, bad = C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_kmers(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                    int(b_len // 4 if n is None else n), k, int(bool(canonical)), _addr(table), C.byref(win),
                                    C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)
        return table, win.value

    def kmer_spectrum(self, table, k, nspec=256) -> dict:
        """dx_kmer_spectrum of a device table of 4^k counters: {"spectrum": uint64[nspec] -- [c] the codes counted c times, the last
        bin everything from nspec - 1 on, [0] always 0 --, "distinct", "max_count", "max_code": the smallest code with the largest
        count}; nspec None or 0: no spectrum."""
        spec = np.zeros(int(nspec), np.uint64) if nspec else None
        d, m, mc = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._chk(self.lib.dx_kmer_spectrum(self.h, _addr(table), int(k), spec.ctypes.data if spec is not None else None,
                                            int(nspec or 0), C.byref(d), C.byref(m), C.byref(mc)))
        return {"spectrum": spec, "distinct": d.value, "max_count": m.value, "max_code": mc.value}

    def kmer_list(self, table, k, min_count, cap):
        """dx_kmer_list of a device table: (found: the codes counted min_count times at least, the first min(cap, found) of them in
        ascending code order as a KMER_DTYPE array)."""
        cap, found = int(cap), C.c_uint64()

        def call(p_out):
            self._chk(self.lib.dx_kmer_list(self.h, _addr(table), int(k), int(min_count), p_out, cap, C.byref(found)))
            return found.value
        lst = self._listed(call, cap, KMER_DTYPE)
        return found.value, lst

    def kmers_add(self, kind, img: bytes, k, canonical, table) -> dict:
        """dx_file_kmers_add: the k-mers of the reads of the image ("fasta" or "arrow") added to the device table of 4^k counters,
        so that several files are counted into one.  {"records", "symbols", "windows"} of this image."""
        r, s, w = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.dx_file_kmers_add(self.h, _kind(kind), img, len(img), int(k), int(bool(canonical)), _addr(table), C.byref(r),
                                             C.byref(s), C.byref(w)))
        return {"records": r.value, "symbols": s.value, "windows": w.value}

    def _file_kmers(self, fn, km, raw, listed, letters, kind, img, k, canonical, nspec, min_count, max_list, table=None):
        """dx_file_kmers / dx_file_kmers_wide: one argument list, one answer.  km: the entry point's report struct, raw: the dtype of
        its list, listed: of the list returned, whose `letters` letters(code, k, arrow=) makes; table: whether the counters are wanted
        too, None for the entry point that has none to give."""
        kd, spec, n = _kind(kind), np.zeros(int(nspec), np.uint64), C.c_uint64()
        with _Outs(self.lib, 2) as (lst, tab):
            self._chk(fn(self.h, kd, img, len(img), int(k), int(bool(canonical)), int(min_count), int(max_list), C.byref(km),
                         spec.ctypes.data, int(nspec), C.byref(lst), C.byref(n),
                         *(() if table is None else (C.byref(tab) if table else None,))))
            rep = _fields(km)
            rep["listed"] = n.value
            got, out = _take(lst, raw, n.value), np.zeros(n.value, listed)
            if n.value:
                out["count"], out["code"] = got["count"], got["code"]
                out["letters"] = [letters(int(c), int(k), arrow=kind == "arrow") for c in got["code"]]
            return (rep, spec, out, _take(tab, np.uint64, 4 ** int(k))) if table else (rep, spec, out)

    def kmers(self, kind, img: bytes, k, canonical=False, nspec=256, min_count=0, max_list=0, table=False):
        """dx_file_kmers: the exact counts of all k-mers (1 <= k <= 14) of the reads of the image ("fasta" or "arrow"), counted on
        the device in the packed reads (no text is made); canonical ("fasta"): a window counts under min(code, reverse complement).
        Returns (report, spectrum, list) and with table=True the 4^k counters behind them (uint64).  report: {"records", "symbols",
        "windows", "distinct", "max_count", "max_code", "k", "listed"}; spectrum: uint64[nspec] as kmer_spectrum's; list: the first
        max_list codes counted min_count times at least (min_count 0: none), ascending, as a KMER_LIST_DTYPE array whose `letters`
        are what Context.find takes as a pattern."""
        return self._file_kmers(self.lib.dx_file_kmers, L.Kmers(), KMER_DTYPE, KMER_LIST_DTYPE, kmer_letters, kind, img, k, canonical,
                                nspec, min_count, max_list, bool(table))

    # ---- k-mers up to k = 32: codes written out, sorted, counted off the runs ---------------------------
    def sort_u64(self, keys, bits, tmp=None, n=None):
        """dx_sort_u64: the n 64-bit keys of the device array `keys` (a torch tensor or a DevBuf; n defaults to what it holds) sorted
        ascending in place, every key < 2^bits; tmp: n keys of room (None: made and freed here).  Returns keys."""
        p, b = _dev(keys)
        n = int(b // 8 if n is None else n)
        own = self.alloc(8 * n + 8) if tmp is None and n else None
        try:
            self._chk(self.lib.dx_sort_u64(self.h, p, _addr(own if own is not None else tmp), n, int(bits)))
        finally:
            if own:
                own.free()
        return keys

    def code_kmer_codes(self, d_in, boff, beg, length, k, canonical=False, cap=None, codes=None, in_bytes=None, n=None):
        """dx_code_kmer_codes: unit j = symbols [beg[j], beg[j] + length[j]) of the packed read at d_in + boff[j] (beg None: whole
        reads from symbol 0); window p of unit j -> codes[off[j] + p], off the exclusive sums of max(0, length[j] - k + 1); the code
        is the window's symbols as a base-4 number (k 1 to 32), with canonical min(code, rc).  The arguments are device arrays as
        code_kmers takes them.  codes: a device array of cap 64-bit words; None: a DevBuf of cap words made here (cap None: every
        unit's windows, from a host copy of `length`), the caller's to free.  Returns (codes, windows).  Raises
        DexGPUError: DX_E_NOMEM (.windows = what is needed) when cap is short, DX_E_FORMAT (.bad_unit) for a unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        k, n = int(k), int(b_len // 4 if n is None else n)
        own = None
        if codes is None:
            if cap is None:
                ln = (length.cpu().numpy()[:n] if hasattr(length, "cpu") else length.download(np.uint32, n)).astype(np.int64)
                cap = int(np.maximum(ln - k + 1, 0).sum())
            codes = own = self.alloc(8 * int(cap) + 8)
        elif cap is None:
            cap = _dev(codes)[1] // 8
        win, bad = C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_kmer_codes(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                         n, k, int(bool(canonical)), _addr(codes), int(cap), C.byref(win), C.byref(bad))
        if rc != 0:
            if own:
                own.free()
            raise self._err(rc, bad_unit=_index(bad), windows=win.value)
        return codes, win.value

    def kmer_runs(self, sorted_codes, n, min_count, cap, nspec=256):
        """dx_kmer_runs of a sorted device array of n codes: (found: the runs of min_count keys at least, the first min(cap, found)
        of them in ascending code order as a KMER64_DTYPE array, {"spectrum": uint64[nspec] -- [c] the runs of length c, the last bin
        everything from nspec - 1 on --, "distinct", "max_count", "max_code"}); nspec None or 0: no spectrum."""
        cap, found = int(cap), C.c_uint64()
        spec = np.zeros(int(nspec), np.uint64) if nspec else None
        d, m, mc = C.c_uint64(), C.c_uint64(), C.c_uint64()

        def call(p_out):
            self._chk(self.lib.dx_kmer_runs(self.h, _addr(sorted_codes), int(n), int(min_count), p_out, cap, C.byref(found),
                                            spec.ctypes.data if spec is not None else None, int(nspec or 0), C.byref(d), C.byref(m),
                                            C.byref(mc)))
            return found.value
        lst = self._listed(call, cap, KMER64_DTYPE)
        return found.value, lst, {"spectrum": spec, "distinct": d.value, "max_count": m.value, "max_code": mc.value}

    def kmers_wide(self, kind, img: bytes, k, canonical=False, nspec=256, min_count=0, max_list=0):
        """dx_file_kmers_wide: Context.kmers for 1 <= k <= 32, by sorting -- every window's code written out on the device, sorted,
        the counts read off the runs; 16 bytes of device memory a window.  Returns (report, spectrum, list) as kmers does, the
        report with the same keys; the list is a KMER64_LIST_DTYPE array (64-bit codes, `letters` 32 bytes wide)."""
        return self._file_kmers(self.lib.dx_file_kmers_wide, L.Kmers64(), KMER64_DTYPE, KMER64_LIST_DTYPE, kmer_letters64, kind, img, k,
                                canonical, nspec, min_count, max_list)

    # ---- ... of several files, in passes over ranges of the codes ------------------------------------------
    def code_kmer_bins(self, d_in, boff, beg, length, k, bits, canonical=False, bins=None, in_bytes=None, n=None):
        """dx_code_kmer_bins: the windows of code_kmer_codes' units counted by the top `bits` bits (1 to min(2 k, 12)) of their codes,
        ADDED to bins[code >> (2 k - bits)].  bins: a device array of 2^bits 64-bit words; None: a zeroed DevBuf made here, the
        caller's to free.  Returns (bins, windows of this call).  Raises DexGPUError: DX_E_FORMAT (.bad_unit, .windows) for a unit
        outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        own = None
        if bins is None:
            bins = own = self.alloc(8 << max(0, min(int(bits), 12))).zero()
        win, bad = C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_kmer_bins(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                        int(b_len // 4 if n is None else n), int(k), int(bool(canonical)), int(bits), _addr(bins),
                                        C.byref(win), C.byref(bad))
        if rc != 0:
            if own:
                own.free()
            raise self._err(rc, bad_unit=_index(bad), windows=win.value)
        return bins, win.value

    def code_kmer_codes_range(self, d_in, boff, beg, length, k, bits, bin_lo, bin_hi, canonical=False, cap=None, codes=None,
                              in_bytes=None, n=None):
        """dx_code_kmer_codes_range: code_kmer_codes for the windows with bin_lo <= code >> (2 k - bits) < bin_hi alone, written
        densely in the order (unit, position).  codes, cap as for code_kmer_codes (cap None without codes: room for every window).
        Returns (codes, the windows kept).  Raises DexGPUError: DX_E_NOMEM (.windows = the windows kept) when cap is short,
        DX_E_FORMAT (.bad_unit) for a unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        k, n = int(k), int(b_len // 4 if n is None else n)
        own = None
        if codes is None:
            if cap is None:
                ln = (length.cpu().numpy()[:n] if hasattr(length, "cpu") else length.download(np.uint32, n)).astype(np.int64)
                cap = int(np.maximum(ln - k + 1, 0).sum())
            codes = own = self.alloc(8 * int(cap) + 8)
        elif cap is None:
            cap = _dev(codes)[1] // 8
        win, bad = C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_kmer_codes_range(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                               n, k, int(bool(canonical)), int(bits), int(bin_lo), int(bin_hi), _addr(codes), int(cap),
                                               C.byref(win), C.byref(bad))
        if rc != 0:
            if own:
                own.free()
            raise self._err(rc, bad_unit=_index(bad), windows=win.value)
        return codes, win.value

    def sorted_take(self, sorted_codes, n, min_count=1, cap=0):
        """dx_sorted_take of a sorted device array of n keys: (found: the runs of min_count keys at least, the first keys of the first
        min(cap, found) of them as a uint64 array); cap 0 counts only."""
        cap, found = int(cap), C.c_uint64()
        own = self.alloc(8 * cap + 8) if cap > 0 else None
        try:
            self._chk(self.lib.dx_sorted_take(self.h, _addr(sorted_codes), int(n), int(min_count), _addr(own), cap, C.byref(found)))
            return found.value, self._download(_addr(own), np.uint64, min(cap, found.value))
        finally:
            if own is not None:
                own.free()

    @staticmethod
    def _images(imgs):
        """a sequence of images (bytes) -> (what ctypes passes as const uint8_t *const *, as const size_t *, how many, what keeps them alive)"""
        keep = [C.c_char_p(bytes(b)) for b in imgs]
        n = len(keep)
        ptrs = (C.c_void_p * max(n, 1))(*[C.cast(p, C.c_void_p) for p in keep])
        sizes = (C.c_size_t * max(n, 1))(*[len(b) for b in imgs])
        return ptrs, sizes, n, keep

    def kmers_wide_files(self, kind, imgs, k, canonical=False, nspec=256, min_count=0, max_list=0, room=0):
        """dx_files_kmers_wide: kmers_wide over several images of one kind, counted into one answer -- in passes over ranges of the
        codes when the windows do not fit the device at once.  room: the windows a pass may hold (16 bytes of device memory each), 0:
        chosen from the free memory.  Returns (report, spectrum, list) as kmers_wide does; the report also has "passes" (the ranges
        that were sorted) and "files": a {"records", "symbols", "windows"} an image."""
        ptrs, sizes, n, keep = self._images(imgs)
        kd, spec, km, cnt, passes = _kind(kind), np.zeros(int(nspec), np.uint64), L.Kmers64(), C.c_uint64(), C.c_uint32()
        per = (L.Kmers64 * max(n, 1))()
        with _Outs(self.lib, 1) as (lst,):
            self._chk(self.lib.dx_files_kmers_wide(self.h, kd, ptrs, sizes, n, int(k), int(bool(canonical)), int(min_count), int(max_list),
                                                   int(room), C.byref(km), spec.ctypes.data, int(nspec), C.byref(lst), C.byref(cnt), per,
                                                   C.byref(passes)))
            rep = _fields(km)
            rep["listed"], rep["passes"] = cnt.value, passes.value
            rep["files"] = [{f: getattr(per[i], f) for f in ("records", "symbols", "windows")} for i in range(n)]
            got, out = _take(lst, KMER64_DTYPE, cnt.value), np.zeros(cnt.value, KMER64_LIST_DTYPE)
            if cnt.value:
                out["count"], out["code"] = got["count"], got["code"]
                out["letters"] = [kmer_letters64(int(c), int(k), arrow=kind == "arrow") for c in got["code"]]
            return rep, spec, out

    def _kmer_set_files(self, fn, kind, imgs, k, canonical, min_count, room, report):
        """dx_files_kmer_set or its counted sibling"""
        ptrs, sizes, n, keep = self._images(imgs)
        h, km, passes = C.c_void_p(), L.Kmers64(), C.c_uint32()
        self._chk(fn(self.h, _kind(kind), ptrs, sizes, n, int(k), int(bool(canonical)), int(min_count), int(room), C.byref(h), C.byref(km),
                     C.byref(passes)))
        s = KmerSet(self, h)
        return (s, dict(_fields(km), passes=passes.value)) if report else s

    def kmer_set_files(self, kind, imgs, k, canonical=False, min_count=1, room=0, report=False):
        """dx_files_kmer_set: kmer_set over several images of one kind, by kmers_wide_files' passes.  report: (set, what
        kmers_wide_files reports without its list and its files)."""
        return self._kmer_set_files(self.lib.dx_files_kmer_set, kind, imgs, k, canonical, min_count, room, report)

    def kmer_set_files_counted(self, kind, imgs, k, canonical=False, min_count=1, room=0, report=False):
        """dx_files_kmer_set_counted: kmer_set_files with every code's count over all the images kept beside it (KmerSet.counts)"""
        return self._kmer_set_files(self.lib.dx_files_kmer_set_counted, kind, imgs, k, canonical, min_count, room, report)

    # ---- screen: the reads that share k-mers with a set ---------------------------------------------------
    def _kmer_set_file(self, fn, kind, img, k, canonical, min_count, report):
        """dx_file_kmer_set or its counted sibling"""
        h, km = C.c_void_p(), L.Kmers64()
        self._chk(fn(self.h, _kind(kind), img, len(img), int(k), int(bool(canonical)), int(min_count), C.byref(h), C.byref(km)))
        s = KmerSet(self, h)
        return (s, _fields(km)) if report else s

    def kmer_set(self, kind, img: bytes, k, canonical=False, min_count=1, report=False):
        """dx_file_kmer_set: the distinct k-mers (1 <= k <= 32) of a .dexta / .dexar image that are counted min_count times at least,
        as a KmerSet on the device -- kmers_wide's route up to the sorted codes.  report: (set, what kmers_wide reports for the image)."""
        return self._kmer_set_file(self.lib.dx_file_kmer_set, kind, img, k, canonical, min_count, report)

    def kmer_set_counted(self, kind, img: bytes, k, canonical=False, min_count=1, report=False):
        """dx_file_kmer_set_counted: kmer_set with every code's count in the image kept beside it, saturated at 2^32 - 1
        (KmerSet.counts): the set that Context.depth and code_kmer_depths read depths from."""
        return self._kmer_set_file(self.lib.dx_file_kmer_set_counted, kind, img, k, canonical, min_count, report)

    def kmer_set_from_codes(self, codes, k, canonical=False, arrow=False):
        """dx_kmer_set_from_codes: the KmerSet of the given 64-bit codes (any order, repeats allowed, none at all: the empty set); with
        canonical each is folded to min(code, rc(code)) first.  api.kmer_code64 makes a code of letters."""
        a = np.ascontiguousarray(np.asarray(codes, np.uint64))
        h = C.c_void_p()
        self._chk(self.lib.dx_kmer_set_from_codes(self.h, a.ctypes.data if len(a) else None, len(a), int(k), int(bool(canonical)),
                                                  int(bool(arrow)), C.byref(h)))
        return KmerSet(self, h)

    def kmer_set_from_kmers(self, kmers, k, canonical=False, arrow=False):
        """dx_kmer_set_from_kmers: the counted KmerSet of (code, count) pairs in any order -- a KMER64_DTYPE array, the `code` and
        `count` fields of kmers_wide's list, or a sequence of pairs.  With canonical each code is folded first; equal codes add; sums
        saturate at 2^32 - 1; a pair with count 0 is dropped."""
        a = np.asarray(kmers)
        if a.dtype.names is None:
            a = np.asarray(kmers, np.uint64).reshape(-1, 2)
            a = np.rec.fromarrays([a[:, 0], a[:, 1]], dtype=KMER64_DTYPE)
        lst = np.zeros(len(a), KMER64_DTYPE)
        lst["code"], lst["count"] = a["code"], a["count"]
        h = C.c_void_p()
        self._chk(self.lib.dx_kmer_set_from_kmers(self.h, lst.ctypes.data if len(lst) else None, len(lst), int(k), int(bool(canonical)),
                                                  int(bool(arrow)), C.byref(h)))
        return KmerSet(self, h)

    def _kmer_set_sorted(self, fn, sorted_codes, n, k, min_count, canonical, arrow):
        """dx_kmer_set_from_sorted or its counted sibling"""
        h = C.c_void_p()
        self._chk(fn(self.h, _addr(sorted_codes), int(n), int(min_count), int(k), int(bool(canonical)), int(bool(arrow)), C.byref(h)))
        return KmerSet(self, h)

    def kmer_set_from_sorted(self, sorted_codes, n, k, min_count=1, canonical=False, arrow=False):
        """dx_kmer_set_from_sorted: the KmerSet of the codes whose run in the sorted device array of n keys has min_count keys at least"""
        return self._kmer_set_sorted(self.lib.dx_kmer_set_from_sorted, sorted_codes, n, k, min_count, canonical, arrow)

    def kmer_set_from_sorted_counted(self, sorted_codes, n, k, min_count=1, canonical=False, arrow=False):
        """dx_kmer_set_from_sorted_counted: kmer_set_from_sorted's codes, each with the length of its run as its count"""
        return self._kmer_set_sorted(self.lib.dx_kmer_set_from_sorted_counted, sorted_codes, n, k, min_count, canonical, arrow)

    def code_kmer_screen(self, d_in, boff, beg, length, kset, out=None, in_bytes=None, n=None):
        """dx_code_kmer_screen: unit j = symbols [beg[j], beg[j] + length[j]) of the packed read at d_in + boff[j] (beg None: whole
        reads from symbol 0), against the KmerSet kset: per unit the windows that are in the set (hits), the symbols they cover, the
        first and the last such window (2^32 - 1: none).  The arguments are device arrays as code_kmer_codes takes them; out: a
        device array of n 16-byte entries (SCREEN_DTYPE), or None for the totals alone.  Returns the totals as a uint64 array:
        windows, hits, covered, units with a hit.  Raises DexGPUError: DX_E_FORMAT (.bad_unit, .totals) for a unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        n = int(b_len // 4 if n is None else n)
        tot, bad = (C.c_uint64 * 4)(), C.c_uint64()
        rc = self.lib.dx_code_kmer_screen(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                          n, kset.h if kset is not None else None, _addr(out), C.byref(tot), C.byref(bad))
        totals = np.array(list(tot), np.uint64)
        if rc != 0:
            raise self._err(rc, bad_unit=_index(bad), totals=totals)
        return totals

    def screen(self, kind, img: bytes, kset):
        """dx_file_screen: the records of a .dexta / .dexar image screened against the KmerSet kset -> (report: records, symbols,
        windows, hits, covered, records_hit, k; rec: a SCREEN_DTYPE array, one entry a record; rec_len: every record's symbols).
        api.screen_select turns (rec, rec_len) into the ids that Context.subset takes."""
        rp = L.ScreenReport()
        with _Outs(self.lib, 2) as (rec, rl):
            self._chk(self.lib.dx_file_screen(self.h, _kind(kind), img, len(img), kset.h if kset is not None else None, C.byref(rp),
                                              C.byref(rec), C.byref(rl)))
            return _fields(rp), _take(rec, SCREEN_DTYPE, rp.records), _take(rl, np.uint32, rp.records)

    # ---- depth: how often a read's k-mers were seen ---------------------------------------------------------
    def code_kmer_depths(self, d_in, boff, beg, length, kset, cap=None, depth=None, off=None, in_bytes=None, n=None):
        """dx_code_kmer_depths: units as for code_kmer_codes, against the KmerSet kset; window p of unit j -> depth[off[j] + p] =
        min(the count of its code in the set, 65535), 0 for a code the set does not hold, 1 for every code of an uncounted set.
        depth: a device array of cap 16-bit words; None: a DevBuf of cap words made here (cap None: every unit's windows, from a
        host copy of `length`), the caller's to free.  off: a device array of n + 1 uint64 for the units' places, or None.  Returns
        (depth, windows).  Raises DexGPUError: DX_E_NOMEM (.windows = what is needed) when cap is short, DX_E_FORMAT (.bad_unit)
        for a unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        n = int(b_len // 4 if n is None else n)
        own = None
        if depth is None:
            if cap is None:
                ln = (length.cpu().numpy()[:n] if hasattr(length, "cpu") else length.download(np.uint32, n)).astype(np.int64)
                cap = int(np.maximum(ln - kset.info["k"] + 1, 0).sum())
            depth = own = self.alloc(2 * int(cap) + 16)
        elif cap is None:
            cap = _dev(depth)[1] // 2
        win, bad = C.c_uint64(), C.c_uint64()
        rc = self.lib.dx_code_kmer_depths(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                          n, kset.h if kset is not None else None, _addr(depth), int(cap), _addr(off), C.byref(win),
                                          C.byref(bad))
        if rc != 0:
            if own:
                own.free()
            raise self._err(rc, bad_unit=_index(bad), windows=win.value)
        return depth, win.value

    def depth_stats(self, depth, off, n, out=None):
        """dx_depth_stats: per stretch depth[off[j] .. off[j + 1]) of a profile (device arrays: 16-bit words, n + 1 uint64) its
        windows, hits, sum, min, q1, median, q3 and max -- the quantiles exact, s[(t (w - 1)) // 4] of the sorted values.  out: a
        device array of n 32-byte entries (DEPTH_DTYPE), or None for the totals alone.  Returns the totals as a uint64 array:
        windows, hits, sum, units with a hit.  Raises DexGPUError: DX_E_FORMAT (.totals) when off decreases."""
        tot = (C.c_uint64 * 4)()
        rc = self.lib.dx_depth_stats(self.h, _addr(depth), _addr(off), int(n), _addr(out), C.byref(tot))
        totals = np.array(list(tot), np.uint64)
        if rc != 0:
            raise self._err(rc, totals=totals)
        return totals

    def depth(self, kind, img: bytes, kset, profile=False):
        """dx_file_depth: the records of a .dexta / .dexar image against the (counted) KmerSet kset -> (report: records, symbols,
        windows, hits, sum, records_hit, k; rec: a DEPTH_DTYPE array, one entry a record; rec_len: every record's symbols); with
        profile also (the whole profile as a uint16 array, rec_off: every record's place in it, records + 1 uint64).
        api.depth_select turns rec into the ids that Context.subset takes."""
        rp = L.DepthReport()
        with _Outs(self.lib, 4) as (rec, rl, pf, ro):
            self._chk(self.lib.dx_file_depth(self.h, _kind(kind), img, len(img), kset.h if kset is not None else None, C.byref(rp),
                                             C.byref(rec), C.byref(rl), C.byref(pf) if profile else None, C.byref(ro) if profile else None))
            out = (_fields(rp), _take(rec, DEPTH_DTYPE, rp.records), _take(rl, np.uint32, rp.records))
            return out + (_take(pf, np.uint16, rp.windows), _take(ro, np.uint64, rp.records + 1)) if profile else out

    # ---- place: where on a reference a read lies ------------------------------------------------------------
    def kmer_index(self, kind, img: bytes, k, canonical=False):
        """dx_file_kmer_index: the records of a .dexta / .dexar image as the targets of a KmerIndex -- a counted KmerSet of their
        windows that also keeps where on the reference (the targets one behind the other) every k-mer stands, and on which strand"""
        h = C.c_void_p()
        self._chk(self.lib.dx_file_kmer_index(self.h, _kind(kind), img, len(img), int(k), int(bool(canonical)), C.byref(h)))
        return KmerIndex(self, h)

    def kmer_index_from_letters(self, seqs, k, canonical=False, arrow=False):
        """dx_kmer_index_from_letters: the KmerIndex of plain sequences (str or bytes: acgtACGT, or 1234 with arrow), packed on the
        host.  Raises DexGPUError (DX_E_ARG, the target and the position named) for a letter that is not the kind's."""
        pats, n = _patterns(seqs)
        lens = np.array([len(p) for p in pats[:n]], np.uint32)
        h = C.c_void_p()
        self._chk(self.lib.dx_kmer_index_from_letters(self.h, int(bool(arrow)), pats, lens.ctypes.data if n else None, n, int(k),
                                                      int(bool(canonical)), C.byref(h)))
        return KmerIndex(self, h)

    def code_kmer_index(self, d_in, boff, beg, length, k, canonical=False, arrow=False, in_bytes=None, n=None):
        """dx_code_kmer_index: the units of a packed device buffer (as for code_kmer_codes) are the targets of the KmerIndex"""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        h = C.c_void_p()
        self._chk(self.lib.dx_code_kmer_index(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                              int(b_len // 4 if n is None else n), int(k), int(bool(canonical)), int(bool(arrow)),
                                              C.byref(h)))
        return KmerIndex(self, h)

    def code_kmer_seeds(self, d_in, boff, beg, length, index, max_occ=1, count=None, off=None, cap=0, seeds=None, in_bytes=None, n=None):
        """dx_code_kmer_seeds: units as for code_kmer_codes, against the KmerIndex index; every occurrence on the reference of a
        window whose code the index holds at most max_occ times is a seed {unit, pos, gpos, strand}.  count: a device array of n
        uint32 for every unit's seeds, or None; off: a device array of n + 1 uint64 for the units' places in the list, or None;
        seeds: a device array of 16 cap bytes, or None: made and freed here (cap 0: counted only).  Returns (totals: uint64
        [windows, windows with a seed, seeds, units with a seed], the seeds in the order (unit, pos, gpos) as a SEED_DTYPE array).
        Raises DexGPUError: DX_E_NOMEM (.totals) when cap is short -- nothing is written --, DX_E_FORMAT (.bad_unit, .totals) for a
        unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        n, cap = int(b_len // 4 if n is None else n), int(cap)
        tot, bad = (C.c_uint64 * 4)(), C.c_uint64()

        def call(p_seeds):
            rc = self.lib.dx_code_kmer_seeds(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                             n, index.h if index is not None else None, int(max_occ), _addr(count), _addr(off),
                                             p_seeds, cap, C.byref(tot), C.byref(bad))
            if rc != 0:
                raise self._err(rc, bad_unit=_index(bad), totals=np.array(list(tot), np.uint64))
            return tot[2]
        lst = self._listed(call, cap, SEED_DTYPE, seeds)
        return np.array(list(tot), np.uint64), lst

    def seeds_place(self, seeds, off, k, band_bits=8, n=None, out=None):
        """dx_seeds_place: per unit j the vote over the diagonals of its seeds seeds[off[j] .. off[j + 1]) -- seeds: a SEED_DTYPE
        array on the host (uploaded here) or a device array; off: n + 1 uint64, on the host or the device.  out: a device array of n
        32-byte entries, or None: made and freed here.  Returns (totals: uint64 [seeds, votes, units placed], a PLACE_DTYPE array,
        one entry a unit).  Raises DexGPUError: DX_E_FORMAT (.totals) when off decreases or a seed names another unit."""
        own = []
        try:
            if isinstance(seeds, np.ndarray):
                a = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
                seeds = self.to_device(a) if len(a) else None
                own.append(seeds)
            if isinstance(off, np.ndarray):
                o = np.ascontiguousarray(off, dtype=np.uint64)
                n = len(o) - 1 if n is None else int(n)
                off = self.to_device(o)
                own.append(off)
            else:
                n = int(_dev(off)[1] // 8 - 1 if n is None else n)
            if out is None:
                out = self.alloc(32 * n + 32)
                own.append(out)
            tot = (C.c_uint64 * 3)()
            rc = self.lib.dx_seeds_place(self.h, _addr(seeds), _addr(off), n, int(k), int(band_bits), _addr(out), C.byref(tot))
            totals = np.array(list(tot), np.uint64)
            if rc != 0:
                raise self._err(rc, totals=totals)
            return totals, self._download(_addr(out), PLACE_DTYPE, n)
        finally:
            for b in own:
                if b is not None:
                    b.free()

    def place(self, kind, img: bytes, index, max_occ=1, band_bits=8, seed_room=0):
        """dx_file_place: the records of a .dexta / .dexar image placed on the KmerIndex's reference -> (report: records, symbols,
        windows, hits, seeds, votes, records_placed, groups, k, band_bits; rec: a PLACE_DTYPE array, one entry a record; rec_len: every
        record's symbols; where: a PLACE_WHERE_DTYPE array -- target: the one that holds gbeg, tbeg and tend: gbeg and min(gend, the
        target's end) relative to it, all UINT32_MAX for a record that is not placed).  api.place_select turns rec into the ids that
        Context.subset takes."""
        rp = L.PlaceReport()
        with _Outs(self.lib, 2) as (rec, rl):
            self._chk(self.lib.dx_file_place(self.h, _kind(kind), img, len(img), index.h if index is not None else None, int(max_occ),
                                             int(band_bits), int(seed_room), C.byref(rp), C.byref(rec), C.byref(rl)))
            r = _take(rec, PLACE_DTYPE, rp.records)
            return _fields(rp), r, _take(rl, np.uint32, rp.records), place_where(r, index.targets())

    # ---- screen spans: where a read matches the set, and the image cut there ------------------------------
    def code_kmer_spans(self, d_in, boff, beg, length, kset, count=None, cap=0, spans=None, in_bytes=None, n=None):
        """dx_code_kmer_spans: units and set as for code_kmer_screen; the spans of a unit are the maximal runs of symbols that lie in
        a window whose code is in the set.  count: a device array of n uint32 for every unit's spans, or None; spans: a device array
        of 16 cap bytes, or None: made and freed here (cap 0: counted only).  Returns (totals: uint64 [spans, covered symbols, units
        with a span], the first min(cap, spans) spans in the order (unit, beg) as a SPAN_DTYPE array).  Raises DexGPUError:
        DX_E_FORMAT (.bad_unit, .totals) for a unit outside in_bytes."""
        p_in, b_in = _dev(d_in)
        p_len, b_len = _dev(length)
        n, cap = int(b_len // 4 if n is None else n), int(cap)
        tot, bad = (C.c_uint64 * 3)(), C.c_uint64()

        def call(p_spans):
            rc = self.lib.dx_code_kmer_spans(self.h, p_in, int(b_in if in_bytes is None else in_bytes), _addr(boff), _addr(beg), p_len,
                                             n, kset.h if kset is not None else None, _addr(count), p_spans, cap, C.byref(tot),
                                             C.byref(bad))
            if rc != 0:
                raise self._err(rc, bad_unit=_index(bad), totals=np.array(list(tot), np.uint64))
            return tot[0]
        lst = self._listed(call, cap, SPAN_DTYPE, spans)
        return np.array(list(tot), np.uint64), lst

    def spans_join(self, spans, max_gap=0, min_span=0, cap=None, n=None, out=None):
        """dx_spans_join: a list as code_kmer_spans leaves it -- a SPAN_DTYPE array on the host (uploaded here) or a device array of n
        16-byte entries -- joined across gaps of at most max_gap within a record, then the joined spans of fewer than min_span
        symbols dropped.  out: a device array of 16 cap bytes, or None: made and freed here (cap None: n, which always suffices; 0:
        counted only).  Returns (totals: uint64 [spans kept, their symbols], the first min(cap, kept) as a SPAN_DTYPE array).  Raises
        DexGPUError: DX_E_FORMAT (.bad_unit = the smallest index that breaks the list's order)."""
        own = None
        if isinstance(spans, np.ndarray):
            a = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
            n = len(a) if n is None else int(n)
            spans = own = self.to_device(a) if len(a) else None
        else:
            n = int(_dev(spans)[1] // 16 if n is None else n)
        cap = n if cap is None else int(cap)
        tot, bad = (C.c_uint64 * 2)(), C.c_uint64()

        def call(p_out):
            rc = self.lib.dx_spans_join(self.h, _addr(spans), n, int(max_gap), int(min_span), p_out, cap, C.byref(tot), C.byref(bad))
            if rc != 0:
                raise self._bad_unit(rc, bad)
            return tot[0]
        try:
            lst = self._listed(call, cap, SPAN_DTYPE, out)
        finally:
            if own is not None:
                own.free()
        return np.array(list(tot), np.uint64), lst

    def screen_spans(self, kind, img: bytes, kset, max_gap=0, min_span=0, max_spans=1 << 20):
        """dx_file_screen_spans: where the records of a .dexta / .dexar image match the KmerSet kset -- per slice the raw spans
        listed on the device, joined across gaps of at most max_gap and those of fewer than min_span symbols dropped -> (report:
        records, symbols, covered, records_hit, raw_spans, spans, span_symbols, listed, k; spans: the first max_spans kept spans in
        the order (record, beg) as a SPAN_DTYPE array; rec_spans: uint32 a record, its kept spans; rec_len: every record's symbols).
        api.spans_cut_plan turns (spans, rec_len) into the selection Context.subset takes."""
        rp = L.SpansReport()
        with _Outs(self.lib, 3) as (sp, rs, rl):
            self._chk(self.lib.dx_file_screen_spans(self.h, _kind(kind), img, len(img), kset.h if kset is not None else None,
                                                    int(max_gap), int(min_span), int(max_spans), C.byref(rp), C.byref(sp), C.byref(rs),
                                                    C.byref(rl)))
            return (_fields(rp), _take(sp, SPAN_DTYPE, rp.listed), _take(rs, np.uint32, rp.records), _take(rl, np.uint32, rp.records))

    def screen_cut(self, kind, img: bytes, kset, max_gap=0, min_span=0, min_len=0, mode="split"):
        """dx_file_screen_cut: the image ("fasta" or "arrow") with what matches the KmerSet kset cut out of its records -- screen_spans
        with every span listed, spans_cut_plan, subset -- byte for byte what dexta / dexar writes for the cut text.  mode and min_len
        as for Context.cut.  Returns (image, report, selection) as Context.cut does: the selection {"ids", "beg", "end"} is what
        Context.subset takes to cut the .dexar and the .dexqv of the same records in the same places."""
        ln, cut, n = C.c_size_t(), L.Cut(), C.c_uint64()
        with _Outs(self.lib, 4) as (out, *sel):
            self._chk(self.lib.dx_file_screen_cut(self.h, _kind(kind), img, len(img), kset.h if kset is not None else None,
                                                  int(max_gap), int(min_span), int(min_len), _cut_mode(mode), C.byref(out),
                                                  C.byref(ln), C.byref(cut), *[C.byref(a) for a in sel], C.byref(n)))
            return _text(out, ln), cut_dict(cut), _cut_selection(sel, n.value)

    # ---- subset ------------------------------------------------------------------------------------
    def reads_repack(self, d_in, in_bytes, d_boff, d_beg, d_len, n, d_out, d_out_off):
        """dx_reads_repack: unit j = symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j] (d_beg None:
        whole reads from symbol 0) as (d_len[j] + 3) >> 2 packed bytes at d_out + d_out_off[j], not a byte outside them.  Raises
        DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a unit does not lie inside the in_bytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_reads_repack(self.h, _addr(d_in), int(in_bytes), _addr(d_boff), _addr(d_beg), _addr(d_len), int(n),
                                      _addr(d_out), _addr(d_out_off), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)

    def copy_ranges(self, d_src, src_bytes, d_src_off, d_len, n, d_dst, d_dst_off):
        """dx_copy_ranges: d_dst[d_dst_off[j] .. + d_len[j]) = d_src[d_src_off[j] .. + d_len[j]) (offsets and lengths: uint64 on the
        device), nothing written outside them.  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a source range
        does not lie inside the src_bytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_copy_ranges(self.h, _addr(d_src), int(src_bytes), _addr(d_src_off), _addr(d_len), int(n), _addr(d_dst),
                                     _addr(d_dst_off), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)

    def subset(self, kind, img: bytes, ids=None, beg=None, end=None, lossy=False) -> bytes:
        """dx_file_subset: the image dexta / dexar / dexqv [-l] writes for the text of img's records ids (None: all of them; they
        must not decrease, and may repeat; with beg and end too: records 0 .. len(beg) - 1), whole or cut to [beg[j], end[j]) -- made on the device, no text on the way.  kind:
        "fasta", "arrow" or "quiva"."""
        k = _kind(kind)
        ids, beg, end, n = _subset_selection(ids, beg, end)
        if n is None:
            n = _NONE64                                      # (ids == beg == end == NULL with UINT64_MAX: every record whole)
        ln = C.c_size_t()
        with _Outs(self.lib, 1) as (out,):
            self._chk(self.lib.dx_file_subset(self.h, k, img, len(img), _ptr(ids), _ptr(beg), _ptr(end), n, int(bool(lossy)),
                                              C.byref(out), C.byref(ln)))
            return _text(out, ln)

    # ---- extract -----------------------------------------------------------------------------------
    def reads_unpack_lines(self, letters, d_in, in_bytes, d_boff, d_beg, d_len, n, width, d_out, d_out_off):
        """dx_reads_unpack_lines: unit j = symbols [d_beg[j], d_beg[j] + d_len[j]) of the packed read at d_in + d_boff[j] (d_beg None:
        whole reads from symbol 0) as the lines undexta -w<width> prints for them -- d_len[j] + ceil(d_len[j] / width) bytes at d_out +
        d_out_off[j], not a byte outside them.  Raises DexGPUError (DX_E_FORMAT, .bad_unit = the first such j) when a unit does not lie
        inside the in_bytes."""
        bad = C.c_uint64()
        rc = self.lib.dx_reads_unpack_lines(self.h, int(letters), _addr(d_in), int(in_bytes), _addr(d_boff), _addr(d_beg), _addr(d_len),
                                            int(n), int(width), _addr(d_out), _addr(d_out_off), C.byref(bad))
        if rc != 0:
            raise self._bad_unit(rc, bad)

    def extract(self, kind, img: bytes, ids=None, beg=None, end=None, upper=False, width=80, offsets=False):
        """dx_file_extract: the text undexta [-U] [-w<width>] / undexar [-w<width>] / undexqv [-U] prints for img's records ids alone
        (None: all of them; with beg and end too: records 0 .. len(beg) - 1), in that order -- any order, and an id may repeat --, whole
        or cut to [beg[j], end[j]).  kind: "fasta", "arrow" or "quiva" (which ignores width).  offsets: (text, toff) with toff[j] where
        unit j's header line begins and toff[n] = len(text)."""
        k = _kind(kind)
        ids, beg, end, n = _subset_selection(ids, beg, end)
        every, ln = n is None, C.c_size_t()
        with _Outs(self.lib, 2) as (out, toff):
            self._chk(self.lib.dx_file_extract(self.h, k, img, len(img), _ptr(ids), _ptr(beg), _ptr(end), _NONE64 if every else n,
                                               int(bool(upper)), int(width), C.byref(out), C.byref(ln), C.byref(toff) if offsets else None))
            text = _text(out, ln)
            if not offsets:
                return text
            if every:                                        # (the count is the library's; every unit has a header line, so the
                n, at = 0, C.cast(toff, C.POINTER(C.c_uint64))   #  offsets rise, and the first that is the text's length is the last)
                while at[n] != ln.value:
                    n += 1
            return text, _take(toff, np.uint64, n + 1)

    def qv_subindex(self, on=True):
        self._chk(self.lib.dx_qv_subindex(self.h, int(bool(on))))

    def qv_onepass_info(self) -> dict:
        """dx_qv_onepass_info: the route the last one-pass encode took (groups / direct, scratch, budget)."""
        o = L.OnepassInfo()
        self._chk(self.lib.dx_qv_onepass_info(self.h, C.byref(o)))
        d = _fields(o, skip=("reserved", "chain_waits"))
        d["chain_waits"] = [int(x) for x in o.chain_waits]
        return d

    def trim(self, what=7):
        """dx_trim: give the context's scratch (1), token slots (2), group index (4) back to the device."""
        self._chk(self.lib.dx_trim(self.h, int(what)))

    def set_scratch_budget(self, nbytes: int):
        self._chk(self.lib.dx_set_scratch_budget(self.h, int(nbytes)))

    @staticmethod
    def _sink(sink):
        """ctypes callback around a Python sink.  An exception raised inside a ctypes callback is printed and
        swallowed (the callback then returns 0 = go on), so it is caught here, the library is told to stop
        (it returns DX_E_IO) and the caller re-raises it through `box`."""
        box = []

        def cb(user, data, n, at):
            try:
                return 1 if sink(C.string_at(data, n), at) else 0
            except BaseException as e:                       # noqa: BLE001 -- re-raised by the caller
                box.append(e)
                return 1
        return L.SINK_FN(cb), box

    @staticmethod
    def _source(read, box):
        """ctypes callback around a Python read(want) -> bytes; what it raises goes into the sink's `box`, and the library is told
        that reading failed"""
        def rd(user, buf, want):
            try:
                data = read(want)
                C.memmove(buf, data, len(data))
                return len(data)
            except BaseException as e:                       # noqa: BLE001 -- re-raised by the caller
                box.append(e)
                return -1
        return L.READ_FN(rd)

    def _streamed(self, box, rc, total, where=None):
        """the end of a streaming call: what a callback raised goes on from here; else rc is checked -- where: the (line, code) of
        an entry point that indexes text, which go in front of the library's words -- and the stream's size returned"""
        if box:
            raise box[0]
        if rc != 0:
            raise self._err(rc, f"line {where[0].value} (DX_IDX code {where[1].value}): {{}}" if where else "{}")
        return total.value

    def unpack2_stream(self, img: bytes, sink, mode=L.DX_LETTERS_LOWER, width=80) -> int:
        """dx_file_unpack2_to: sink(data: bytes, at: int) -> falsy to go on; returns the text's size."""
        total = C.c_size_t()
        cb, box = self._sink(sink)
        rc = self.lib.dx_file_unpack2_to(self.h, int(mode), img, len(img), int(width), cb, None, C.byref(total))
        return self._streamed(box, rc, total)

    def pack2_stream(self, read, sink, arrow=False, chunk=0) -> int:
        """dx_file_pack2_stream: read(want: int) -> bytes (fewer than want only at the end); sink(data: bytes, at: int) -> falsy
        to go on; returns the image's size."""
        total, line, code = C.c_size_t(), C.c_uint64(), C.c_int()
        cb, box = self._sink(sink)
        rcb = self._source(read, box)
        rc = self.lib.dx_file_pack2_stream(self.h, int(arrow), rcb, None, int(chunk), cb, None, C.byref(total), C.byref(line), C.byref(code))
        return self._streamed(box, rc, total, (line, code))

    def unpack2_pieces(self, read, sink, mode=L.DX_LETTERS_LOWER, width=80, chunk=0) -> int:
        """dx_file_unpack2_stream: read(want: int) -> bytes of the image; sink(data: bytes, at: int); returns the text's size."""
        total = C.c_size_t()
        cb, box = self._sink(sink)
        rcb = self._source(read, box)
        rc = self.lib.dx_file_unpack2_stream(self.h, int(mode), rcb, None, int(chunk), int(width), cb, None, C.byref(total))
        return self._streamed(box, rc, total)

    def dexqv_stream(self, quiva: bytes, sink, lossy=False) -> int:
        """dx_file_dexqv_to: sink(data: bytes, at: int) -> falsy to go on; returns the image's size."""
        total, line, code = C.c_size_t(), C.c_uint64(), C.c_int()
        cb, box = self._sink(sink)
        rc = self.lib.dx_file_dexqv_to(self.h, quiva, len(quiva), int(lossy), cb, None, C.byref(total),
                                       C.byref(line), C.byref(code))
        return self._streamed(box, rc, total, (line, code))

    def undexqv_stream(self, img: bytes, sink, upper=False) -> int:
        """dx_file_undexqv_plan + dx_file_undexqv_run: sink(data: bytes, at: int) -> falsy to go on; returns the
        text's size.  (The plan alone -- the host walk -- is `undexqv_plan_size`, which needs no GPU.)"""
        plan, total = C.c_void_p(), C.c_size_t()
        keep = C.create_string_buffer(img, len(img))              # must outlive the run
        rc = self.lib.dx_file_undexqv_plan(keep, len(img), C.byref(plan), C.byref(total))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_file_undexqv_plan")
        try:
            cb, box = self._sink(sink)
            rc = self.lib.dx_file_undexqv_run(self.h, plan, int(upper), cb, None)
            return self._streamed(box, rc, total)
        finally:
            self.lib.dx_file_undexqv_plan_free(plan)


def _sharded(contexts, name, *args):
    """the sharded file drivers: lib.<name>(the contexts' handles, how many, *args, &out, &n, &line, &code) -> the bytes it made"""
    lib = contexts[0].lib
    arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    n, line, code = C.c_size_t(), C.c_uint64(), C.c_int()
    with _Outs(lib, 1) as (out,):
        rc = getattr(lib, name)(arr, len(contexts), *args, C.byref(out), C.byref(n), C.byref(line), C.byref(code))
        if rc != 0:
            raise _error(rc, f"line {line.value} (DX_IDX code {code.value})")
        return _text(out, n)


def dexqv_sharded(contexts, quiva: bytes, lossy=False) -> bytes:
    """One .quiva file over several contexts/GPUs (dx_file_dexqv_sharded)."""
    return _sharded(contexts, "dx_file_dexqv_sharded", quiva, len(quiva), int(lossy))


def pack2_sharded(contexts, text: bytes, arrow=False) -> bytes:
    """One .fasta/.arrow file over several contexts/GPUs (dx_file_pack2_sharded)."""
    return _sharded(contexts, "dx_file_pack2_sharded", int(arrow), text, len(text))


# ---- host-only helpers (no GPU needed) ---------------------------------------------------------
HIT_DTYPE = np.dtype([("record", "<u8"), ("pos", "<u4"), ("query", "<u2"), ("strand", "u1"), ("mis", "u1")])      # dx_hit


KMER_DTYPE = np.dtype([("count", "<u8"), ("code", "<u4"), ("reserved", "<u4")])                                   # dx_kmer
KMER_LIST_DTYPE = np.dtype([("count", "<u8"), ("code", "<u4"), ("letters", "S14")])                              # Context.kmers' list


KMER64_DTYPE = np.dtype([("code", "<u8"), ("count", "<u8")])                                                      # dx_kmer64
KMER64_LIST_DTYPE = np.dtype([("count", "<u8"), ("code", "<u8"), ("letters", "S32")])                            # Context.kmers_wide's list


SCREEN_DTYPE = np.dtype([("hits", "<u4"), ("covered", "<u4"), ("first", "<u4"), ("last", "<u4")])                 # dx_screen
SPAN_DTYPE = np.dtype([("record", "<u8"), ("beg", "<u4"), ("end", "<u4")])                                         # dx_span
DEPTH_DTYPE = np.dtype([("windows", "<u4"), ("hits", "<u4"), ("sum", "<u8"), ("min", "<u2"), ("q1", "<u2"), ("median", "<u2"),
                        ("q3", "<u2"), ("max", "<u2"), ("reserved", "<u2", (3,))])                                    # dx_depth
SEED_DTYPE = np.dtype([("unit", "<u4"), ("pos", "<u4"), ("gpos", "<u4"), ("strand", "<u4")])                       # dx_seed
PLACE_DTYPE = np.dtype([("seeds", "<u4"), ("votes", "<u4"), ("strand", "<u4"), ("diag", "<u4"), ("rbeg", "<u4"), ("rend", "<u4"),
                        ("gbeg", "<u4"), ("gend", "<u4")])                                                           # dx_place
PLACE_WHERE_DTYPE = np.dtype([("target", "<u4"), ("tbeg", "<u4"), ("tend", "<u4")])                               # Context.place's
_DEPTH_STATS = {"min": L.DX_DEPTH_MIN, "q1": L.DX_DEPTH_Q1, "median": L.DX_DEPTH_MEDIAN, "q3": L.DX_DEPTH_Q3, "max": L.DX_DEPTH_MAX}


class KmerSet:
    """A dx_kmer_set: a set of k-mers on a Context's device (Context.kmer_set, .kmer_set_from_codes).  free() it, or use it as a
    context manager, before the Context is closed."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    @property
    def info(self) -> dict:
        """{"codes", "device_bytes", "k", "canonical", "arrow", "index_bits"}"""
        i = L.KmerSetInfo()
        self.ctx._chk(self.ctx.lib.dx_kmer_set_info(self.h, C.byref(i)))
        return _fields(i)

    def codes(self) -> np.ndarray:
        """the set's codes, ascending, as a uint64 array"""
        out = np.zeros(self.info["codes"], np.uint64)
        self.ctx._chk(self.ctx.lib.dx_kmer_set_codes(self.ctx.h, self.h, out.ctypes.data if len(out) else None, len(out)))
        return out

    @property
    def counted(self) -> bool:
        """whether the set keeps a count beside every code (Context.kmer_set_counted, .kmer_set_from_kmers)"""
        return self.ctx.lib.dx_kmer_set_counted(self.h) == 1

    def counts(self) -> np.ndarray:
        """a counted set's counts, in the order of codes(), as a uint32 array; DexGPUError (DX_E_ARG) for an uncounted set"""
        out = np.zeros(self.info["codes"], np.uint32)
        self.ctx._chk(self.ctx.lib.dx_kmer_set_counts(self.ctx.h, self.h, out.ctypes.data if len(out) else None, len(out)))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.dx_kmer_set_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class _IndexSet(KmerSet):
    """the KmerSet inside a KmerIndex: the index's own, so free() only forgets it"""

    def free(self):
        self.h = None


class KmerIndex:
    """A dx_kmer_index: a counted set of a reference's k-mers that keeps their positions, on a Context's device (Context.kmer_index,
    .kmer_index_from_letters, .code_kmer_index).  free() it, or use it as a context manager, before the Context is closed."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    @property
    def info(self) -> dict:
        """{"codes", "windows", "targets", "symbols", "device_bytes", "k", "canonical", "arrow"}"""
        i = L.IndexInfo()
        self.ctx._chk(self.ctx.lib.dx_kmer_index_info(self.h, C.byref(i)))
        return _fields(i)

    def kset(self) -> KmerSet:
        """the counted KmerSet inside (the index's own: it goes when the index does); screen, screen_spans and depth take it"""
        return _IndexSet(self.ctx, C.c_void_p(self.ctx.lib.dx_kmer_index_set(self.h)))

    def targets(self) -> np.ndarray:
        """toff: the exclusive sums of the targets' lengths, targets + 1 uint64"""
        n = C.c_uint64()
        p = self.ctx.lib.dx_kmer_index_targets(self.h, C.byref(n))
        return _take(C.c_void_p(p), np.uint64, n.value + 1) if p else np.zeros(1, np.uint64)

    def positions(self):
        """(start: codes + 1 uint32, the exclusive sums of the counts; pos: windows uint32, the occurrences of code i as
        gpos << 1 | flip in pos[start[i] : start[i + 1]], ascending)"""
        i = self.info
        start, pos = np.zeros(i["codes"] + 1, np.uint32), np.zeros(i["windows"], np.uint32)
        self.ctx._chk(self.ctx.lib.dx_kmer_index_positions(self.ctx.h, self.h, start.ctypes.data, len(start),
                                                           pos.ctypes.data if len(pos) else None, len(pos)))
        return start, pos

    def free(self):
        if self.h:
            self.ctx.lib.dx_kmer_index_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def pack_letters(seq, arrow=False) -> bytes:
    """dx_pack_letters: letters (acgtACGT, or 1234 with arrow) -> four symbols a byte, the first on top, as
    Context.kmer_index_from_letters packs a target.  Host only.  Raises DexGPUError (.bad_pos) for a letter that is not the kind's."""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    out, bad = C.create_string_buffer((len(b) + 3) // 4 + 1), C.c_uint32()
    rc = L.load().dx_pack_letters(int(bool(arrow)), b, len(b), out, C.byref(bad))
    if rc != 0:
        raise _error(rc, f"dx_pack_letters: position {bad.value} is not a letter of the kind", bad_pos=bad.value)
    return out.raw[:(len(b) + 3) // 4]


def place_where(rec, toff) -> np.ndarray:
    """per record of Context.place's answer the target that holds gbeg (np.searchsorted over toff) and [tbeg, tend) = [gbeg,
    min(gend, the target's end)) relative to it, as a PLACE_WHERE_DTYPE array; all UINT32_MAX where votes == 0.  Host only."""
    r, toff = np.asarray(rec, PLACE_DTYPE), np.asarray(toff, np.uint64).astype(np.int64)
    out = np.full(len(r), 0xffffffff, PLACE_WHERE_DTYPE)
    ok = (r["votes"] > 0) & (r["gbeg"] < toff[-1])
    t = np.searchsorted(toff, r["gbeg"][ok].astype(np.int64), side="right") - 1
    out["target"][ok] = t
    out["tbeg"][ok] = r["gbeg"][ok] - toff[t]
    out["tend"][ok] = np.minimum(r["gend"][ok].astype(np.int64), toff[t + 1]) - toff[t]
    return out


def place_select(rec, toff, target=None, lo=0, hi=0xffffffff, min_votes=1, strands=3, drop=False) -> np.ndarray:
    """dx_place_select: the records of Context.place's answer that lie on a locus -- votes >= max(min_votes, 1), the strand allowed
    (strands: 1 = forward, 2 = reverse, 3 = both), the target that holds gbeg being `target` (None: any), and [gbeg, min(gend, the
    target's end)) relative to the target meeting [lo, hi) --, or with drop the others, ascending, as the uint64 ids Context.subset
    takes.  toff: KmerIndex.targets().  Host only."""
    r = np.ascontiguousarray(np.asarray(rec, PLACE_DTYPE))
    t = np.ascontiguousarray(np.asarray(toff, np.uint64))
    n = C.c_uint64()
    with _Outs(L.load(), 1) as (ids,):
        rc = L.load().dx_place_select(r.ctypes.data if len(r) else None, len(r), t.ctypes.data if len(t) else None, max(len(t), 1) - 1,
                                      0xffffffff if target is None else int(target), int(lo), int(hi), int(min_votes), int(strands),
                                      L.DX_SCREEN_DROP if drop else L.DX_SCREEN_KEEP, C.byref(ids), C.byref(n))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_place_select: strands is 1, 2 or 3, lo <= hi, target below the targets, toff ascending from 0")
        return _take(ids, np.uint64, n.value)


def screen_select(rec, rec_len, min_hits=1, min_permille=0, drop=False) -> np.ndarray:
    """dx_screen_select: the records of Context.screen's answer that match -- hits >= max(min_hits, 1) and covered * 1000 >=
    min_permille * length --, or with drop the others, ascending, as the uint64 ids Context.subset takes.  Host only."""
    r = np.ascontiguousarray(np.asarray(rec, SCREEN_DTYPE))
    ln = np.ascontiguousarray(np.asarray(rec_len, np.uint32))
    if len(r) != len(ln):
        raise L.DexGPUError(-1, "dx_screen_select: an entry and a length a record")
    n = C.c_uint64()
    with _Outs(L.load(), 1) as (ids,):
        rc = L.load().dx_screen_select(r.ctypes.data if len(r) else None, ln.ctypes.data if len(ln) else None, len(r), int(min_hits),
                                       int(min_permille), L.DX_SCREEN_DROP if drop else L.DX_SCREEN_KEEP, C.byref(ids), C.byref(n))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_screen_select: min_permille is 0 to 1000")
        return _take(ids, np.uint64, n.value)


def depth_select(rec, stat="median", lo=0, hi=65535, min_windows=1, drop=False) -> np.ndarray:
    """dx_depth_select: the records of Context.depth's answer that match -- windows >= max(min_windows, 1) and lo <= stat <= hi, stat
    one of "min", "q1", "median", "q3", "max" (or a DX_DEPTH_* number) --, or with drop the others, ascending, as the uint64 ids
    Context.subset takes.  Host only."""
    r = np.ascontiguousarray(np.asarray(rec, DEPTH_DTYPE))
    n = C.c_uint64()
    with _Outs(L.load(), 1) as (ids,):
        rc = L.load().dx_depth_select(r.ctypes.data if len(r) else None, len(r), int(_DEPTH_STATS.get(stat, stat)), int(lo), int(hi),
                                      int(min_windows), L.DX_SCREEN_DROP if drop else L.DX_SCREEN_KEEP, C.byref(ids), C.byref(n))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_depth_select: stat is min, q1, median, q3 or max, and lo <= hi")
        return _take(ids, np.uint64, n.value)


def kmer_code(letters, arrow=False, canonical=False) -> int:
    """dx_kmer_code: 1 to 14 letters (acgtACGT, or 1234 with arrow) -> the k-mer's code, the first letter on top; canonical:
    min(code, reverse complement's).  Host only."""
    s = letters.encode() if isinstance(letters, str) else bytes(letters)
    code = C.c_uint32()
    rc = L.load().dx_kmer_code(int(bool(arrow)), s, len(s), int(bool(canonical)), C.byref(code))
    if rc != 0:
        raise L.DexGPUError(rc, f"dx_kmer_code: {letters!r} is not 1 to 14 letters of the kind's")
    return code.value


def kmer_letters(code, k, arrow=False) -> bytes:
    """dx_kmer_letters: a code of k symbols -> its letters, upper case or 1234.  Host only."""
    out = C.create_string_buffer(16)
    code, k = int(code), int(k)
    rc = L.load().dx_kmer_letters(int(bool(arrow)), code, k, out) if 0 <= code < 2**32 and 0 <= k < 2**32 else -1
    if rc != 0:
        raise L.DexGPUError(rc, f"dx_kmer_letters: code {code} is not one of {k} symbols, or k is not 1 to 14")
    return out.value


def kmer_code64(letters, arrow=False, canonical=False) -> int:
    """dx_kmer_code64: 1 to 32 letters (acgtACGT, or 1234 with arrow) -> the k-mer's 64-bit code, the first letter on top; canonical:
    min(code, reverse complement's).  Host only."""
    s = letters.encode() if isinstance(letters, str) else bytes(letters)
    code = C.c_uint64()
    rc = L.load().dx_kmer_code64(int(bool(arrow)), s, len(s), int(bool(canonical)), C.byref(code))
    if rc != 0:
        raise L.DexGPUError(rc, f"dx_kmer_code64: {letters!r} is not 1 to 32 letters of the kind's")
    return code.value


def kmer_letters64(code, k, arrow=False) -> bytes:
    """dx_kmer_letters64: a code of k symbols (1 to 32) -> its letters, upper case or 1234.  Host only."""
    out = C.create_string_buffer(40)
    code, k = int(code), int(k)
    rc = L.load().dx_kmer_letters64(int(bool(arrow)), code, k, out) if 0 <= code < 2**64 and 0 <= k < 2**32 else -1
    if rc != 0:
        raise L.DexGPUError(rc, f"dx_kmer_letters64: code {code} is not one of {k} symbols, or k is not 1 to 32")
    return out.value


def kmer_range_plan(bins, room) -> np.ndarray:
    """dx_kmer_range_plan: the bins (what code_kmer_bins counted) cut into ranges of consecutive bins of at most `room` windows each,
    greedily; room 0: one range.  Returns the cuts as a uint32 array: range r is bins [cut[r], cut[r + 1]), cut[0] = 0, cut[-1] =
    len(bins).  Host only.  Raises DexGPUError (DX_E_NOMEM, the bin and its windows named) for a single bin above room."""
    b = np.ascontiguousarray(np.asarray(bins, np.uint64))
    cut, ranges, lib = np.zeros(len(b) + 1, np.uint32), C.c_uint32(), L.load()
    rc = lib.dx_kmer_range_plan(None, b.ctypes.data if len(b) else None, len(b), int(room), cut.ctypes.data, C.byref(ranges))
    if rc != 0:
        raise _error(rc, _words(lib, None))
    return cut[:ranges.value + 1].copy()


def equery(*x):
    """a dx_equery from (codes, max_err) -- 1 to 64 symbols 0..3, the first on top of code[0] -- or from (code0, code1, len, max_err)"""
    if len(x) == 4:
        return L.EQuery((C.c_uint64 * 2)(int(x[0]), int(x[1])), int(x[2]), int(x[3]))
    codes, max_err = x
    code = [0, 0]
    for i, c in enumerate(codes):
        code[i >> 5] |= int(c) << (2 * (31 - (i & 31)))
    return L.EQuery((C.c_uint64 * 2)(*code), len(codes), int(max_err))


def _cut_mode(mode):
    return mode if isinstance(mode, int) else {"split": L.DX_CUT_SPLIT, "longest": L.DX_CUT_LONGEST, "drop": L.DX_CUT_DROP}[mode]


def cut_dict(cut) -> dict:
    """a dx_cut as a dict"""
    return _fields(cut)


def _cut_selection(sel, n):
    return {name: _take(a, t, n) for name, a, t in zip(("ids", "beg", "end"), sel, (np.uint64, np.uint32, np.uint32))}


def cut_plan(hits, start, rec_len, min_len=0, mode="split"):
    """dx_hits_cut_plan (host, no GPU): what is kept of every record once the occurrences [start[i], hits[i].pos) are cut out.  hits: a
    HIT_DTYPE array (record and pos are read), start: uint32 beside it, rec_len: every record's symbols; mode as for Context.cut.
    Returns (selection {"ids", "beg", "end"} as Context.subset takes it, report {"records_in", "records_cut", "records_dropped",
    "pieces", "symbols_in", "symbols_kept", "spans"})."""
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    st = np.ascontiguousarray(start, dtype=np.uint32)
    rl = np.ascontiguousarray(rec_len, dtype=np.uint32)
    if len(h) != len(st):
        raise ValueError("hits / start: one start a hit")
    lib = L.load()
    n, cut = C.c_uint64(), L.Cut()
    with _Outs(lib, 3) as sel:
        rc = lib.dx_hits_cut_plan(h.ctypes.data if len(h) else None, st.ctypes.data if len(st) else None, len(h),
                                  rl.ctypes.data if len(rl) else None, len(rl), int(min_len), _cut_mode(mode),
                                  *[C.byref(a) for a in sel], C.byref(n), C.byref(cut))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_hits_cut_plan")
        return _cut_selection(sel, n.value), cut_dict(cut)


def spans_cut_plan(spans, rec_len, min_len=0, mode="split"):
    """dx_spans_cut_plan (host, no GPU): cut_plan over spans given directly -- a SPAN_DTYPE array, symbols [beg, end) of record
    `record`, as Context.screen_spans lists them.  Returns (selection, report) as cut_plan does."""
    sp = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    rl = np.ascontiguousarray(rec_len, dtype=np.uint32)
    lib = L.load()
    n, cut = C.c_uint64(), L.Cut()
    with _Outs(lib, 3) as sel:
        rc = lib.dx_spans_cut_plan(sp.ctypes.data if len(sp) else None, len(sp), rl.ctypes.data if len(rl) else None, len(rl),
                                   int(min_len), _cut_mode(mode), *[C.byref(a) for a in sel], C.byref(n), C.byref(cut))
        if rc != 0:
            raise L.DexGPUError(rc, "dx_spans_cut_plan")
        return _cut_selection(sel, n.value), cut_dict(cut)


def census_dict(cs) -> dict:
    """a dx_census as a dict: the scalars, "code" (uint64[4]) and "hist" (uint64[5, 256])"""
    out = {f: int(getattr(cs, f)) for f in ("records", "symbols", "min_len", "max_len", "n50")}
    out["code"] = np.array(list(cs.code), dtype=np.uint64)
    out["hist"] = np.array([list(row) for row in cs.hist], dtype=np.uint64)
    return out


def compare_dict(cm) -> dict:
    """a dx_compare as Context.compare returns it"""
    out = {f: int(getattr(cm, f)) for f in ("lines", "records_a", "records_b", "headers_differ", "lengths_differ", "records_differ")}
    out["same"], out["prefix_differs"] = bool(cm.same), bool(cm.prefix_differs)
    for f in ("first_header", "first_length", "first_record"):
        out[f] = None if getattr(cm, f) == _NONE64 else int(getattr(cm, f))
    out["first_line"] = None if out["first_record"] is None else int(cm.first_line)
    out["first_column"] = None if out["first_record"] is None else int(cm.first_column)
    for f in ("differ", "line_records", "sum_abs", "max_abs"):
        out[f] = np.array(list(getattr(cm, f))[:cm.lines], dtype=np.uint64)
    return out


def census_lengths(lengths) -> dict:
    """dx_census_lengths (host): {"records", "symbols", "min_len", "max_len", "n50"} of read lengths (uint32).  N50: over the lengths
    sorted downward, the length at which the running sum first reaches half of the total; 0 without symbols."""
    a = np.ascontiguousarray(lengths, dtype=np.uint32)
    cs = L.Census()
    rc = L.load().dx_census_lengths(a.ctypes.data if a.size else None, int(a.size), C.byref(cs))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_census_lengths")
    return {f: int(getattr(cs, f)) for f in ("records", "symbols", "min_len", "max_len", "n50")}


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _subset_selection(ids, beg, end):
    """the arrays of a dx_file_subset selection as the C-ABI takes them -> (ids or None, beg or None, end or None, n).  What the
    library checks (the order of the ids, the intervals) is left to it; ids None with no intervals has no count here: None."""
    for a in (ids, beg, end):
        if a is not None and len(a) and np.any(np.asarray(a) < 0):
            raise ValueError("a negative id, beg or end")
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64)
    beg = None if beg is None else np.ascontiguousarray(beg, dtype=np.uint32)
    end = None if end is None else np.ascontiguousarray(end, dtype=np.uint32)
    n = [len(a) for a in (ids, beg, end) if a is not None]
    if len(set(n)) > 1:
        raise ValueError("ids / beg / end: one value a unit")
    return ids, beg, end, (n[0] if n else None)


def subset_layout(kind, img: bytes, ids=None, beg=None, end=None) -> dict:
    """dx_file_subset_layout (host, no GPU): the framing of the image Context.subset makes of a .dexta / .dexar image, and the units
    dx_reads_repack fills it with.  {"frame": bytes (every payload byte 0), "src_off", "dst_off" (uint64), "src_beg", "len" (uint32)}:
    unit j is symbols [src_beg[j], src_beg[j] + len[j]) of the packed read at img[src_off[j]:], to frame[dst_off[j]:].  The selection
    names its units here (ids, or beg and end): the arrays have one value each."""
    if kind == "quiva":                                      # (a .dexqv image has no packed reads to lay out)
        raise KeyError(kind)
    k = _kind(kind)
    ids, beg, end, n = _subset_selection(ids, beg, end)
    if n is None:
        raise ValueError("subset_layout: give ids, or beg and end (the arrays that come back have one value a unit)")
    lib, ln = L.load(), C.c_size_t()
    with _Outs(lib, 5) as (frame, *arr):
        rc = lib.dx_file_subset_layout(k, img, len(img), _ptr(ids), _ptr(beg), _ptr(end), n, C.byref(frame), C.byref(ln),
                                       *[C.byref(a) for a in arr])
        if rc != 0:
            raise _error(rc, _words(lib, None))
        out = {"frame": _text(frame, ln)}
        for name, a, t in zip(("src_off", "src_beg", "len", "dst_off"), arr, (np.uint64, np.uint32, np.uint32, np.uint64)):
            out[name] = _take(a, t, n)
        return out


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """dx_crc32_combine (host): zlib's crc32_combine -- crc32(A + B) from crc32(A), crc32(B) and len(B)"""
    return L.load().dx_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, int(len_b))


def text_options(kind, text: bytes):
    """dx_file_text_options (host): (upper, width) that give `text` back, as dx_file_verify reads them off it"""
    k, upper, width = _kind(kind), C.c_int(), C.c_uint32()
    rc = L.load().dx_file_text_options(k, text, len(text), C.byref(upper), C.byref(width))
    if rc != 0:
        raise L.DexGPUError(rc, "the text does not index")
    return bool(upper.value), width.value


def qv_build(hist, tot, params, lossy=False) -> L.QVCoding:
    """Create_QVcoding (QV.c:1029-1169) on the host."""
    lib, h, c = L.load(), _hist(hist), L.QVCoding()
    rc = lib.dx_qv_build(C.byref(h), int(tot), C.byref(params), int(lossy), C.byref(c))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_qv_build")
    return c


def qv_out_bound(hist, n, coding, lossy=False) -> int:
    """dx_qv_out_bound: bytes (without framing) the batch whose raw histograms are `hist` can encode to at most."""
    lib, h = L.load(), _hist(hist)
    return int(lib.dx_qv_out_bound(C.byref(h), int(n), C.byref(coding), int(lossy)))


def qv_write_coding(coding, prefix: bytes) -> bytes:
    lib = L.load()
    n = C.c_size_t()
    lib.dx_qv_write_coding(C.byref(coding), prefix, len(prefix), None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value)
    rc = lib.dx_qv_write_coding(C.byref(coding), prefix, len(prefix), buf, n.value, C.byref(n))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_qv_write_coding")
    return buf.raw[:n.value]


def qv_read_coding(img: bytes):
    """-> (coding, flip, prefix, consumed)"""
    lib = L.load()
    c, flip, used = L.QVCoding(), C.c_int(), C.c_size_t()
    pre = C.create_string_buffer(len(img) + 1)
    rc = lib.dx_qv_read_coding(img, len(img), C.byref(c), C.byref(flip), pre, len(img) + 1, C.byref(used))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_qv_read_coding")
    return c, flip.value, pre.value, used.value


def qv_walk(img: bytes, index=False):
    """Host boundary walk of a bare .dexqv image -> dict of numpy arrays + coding (QVIndex copy); index=True: with the
    group index of dx_qv_walk_indexed (gidx words, gidx_off, gidx_none)."""
    lib = L.load()
    x = L.QVIndex()
    p, nb = _host_bytes(img)
    rc = lib.dx_qv_walk_indexed(p, nb, C.byref(x), int(bool(index)))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_qv_walk")
    try:
        n = x.n
        extra = {}
        if index:
            w = int(x.gidx_words)
            extra = {"gidx": (np.ctypeslib.as_array(x.gidx, (w,)).copy() if w and x.gidx else np.zeros(0, np.uint32)),   # (an image without records: NULL)
                     "gidx_off": np.ctypeslib.as_array(x.gidx_off, (n + 1,)).copy(), "gidx_none": int(x.gidx_none)}
        return {**extra, "n": n,
                "rec_off": np.ctypeslib.as_array(x.rec_off, (n + 1,)).copy(),
                "hdr_off": np.ctypeslib.as_array(x.hdr_off, (n + 1,)).copy(),
                "seg": np.ctypeslib.as_array(x.seg, (max(n, 1), 5))[:n].copy(),
                "len": np.ctypeslib.as_array(x.len, (max(n, 1),))[:n].copy(),
                "hdr4": np.ctypeslib.as_array(x.hdr4, (max(n, 1), 4))[:n].copy(),
                "prefix": bytes(x.prefix), "newv": x.newv, "flip": x.flip,
                "delChar": x.coding.delChar, "subChar": x.coding.subChar}
    finally:
        lib.dx_qv_index_free(C.byref(x))


def qv_walk_records(buf, start, rlen, coding, flip=False):
    """dx_qv_walk_records (host, no GPU): the five segment sizes of the records that start at buf[start[i]] (no framing bytes,
    rlen[i] symbols a line) -> uint32 [n, 5].  Raises DexGPUError (DX_E_FORMAT, .bad_entry = the first such i) when a record
    does not end inside buf."""
    lib = L.load()
    start = np.ascontiguousarray(start, dtype=np.uint64)
    rlen = np.ascontiguousarray(rlen, dtype=np.uint32)
    assert len(start) == len(rlen)
    bp, nb = _host_bytes(buf)
    seg = np.zeros((len(start), 5), np.uint32)
    bad = C.c_uint64()
    rc = lib.dx_qv_walk_records(bp, nb, start.ctypes.data, rlen.ctypes.data, len(start), C.byref(coding), int(bool(flip)),
                                seg.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _error(rc, f"dx_qv_walk_records: entry {bad.value}", bad_entry=_index(bad))
    return seg


def frame_headers(hdr4, cnr4=None, lwell=0):
    """-> (blob uint8, off uint64 [n+1], last well)"""
    lib = L.load()
    hdr4 = np.ascontiguousarray(hdr4, dtype=np.int32)
    n = len(hdr4)
    kind = 0 if cnr4 is None else 1
    if cnr4 is not None:
        cnr4 = np.ascontiguousarray(cnr4, dtype=np.uint16)
    bound = lib.dx_frame_bound(hdr4.ctypes.data, n, lwell, kind)
    blob = np.zeros(bound + 16, np.uint8)
    off = np.zeros(n + 1, np.uint64)
    lw = C.c_int32(lwell)
    rc = lib.dx_frame_headers(hdr4.ctypes.data, cnr4.ctypes.data if kind else None, n, kind, C.byref(lw),
                              blob.ctypes.data, off.ctypes.data)
    if rc != 0:
        raise L.DexGPUError(rc, "dx_frame_headers")
    return blob[: int(off[n])], off, lw.value


def index_quiva(text: bytes):
    """-> (off uint64, len uint32, hdr4 int32 [n,4], prefix_len)"""
    lib = L.load()
    cnt, pl, line, code = C.c_uint64(), C.c_size_t(), C.c_uint64(), C.c_int()
    rc = lib.dx_index_quiva(text, len(text), 0, None, None, None, C.byref(cnt), C.byref(pl), C.byref(line), C.byref(code))
    if rc != 0:
        raise L.DexGPUError(rc, f"line {line.value}: DX_IDX code {code.value}")
    n = cnt.value
    off, ln, hdr = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 4), np.int32)
    lib.dx_index_quiva(text, len(text), n, off.ctypes.data, ln.ctypes.data, hdr.ctypes.data, C.byref(cnt),
                       C.byref(pl), C.byref(line), C.byref(code))
    return off, ln, hdr, pl.value


def index_seq(text: bytes, arrow=False):
    """-> (off, tlen, nsym, hdr4, cnr4, prefix_len)"""
    lib = L.load()
    cnt, pl, line, code = C.c_uint64(), C.c_size_t(), C.c_uint64(), C.c_int()
    rc = lib.dx_index_seq(int(arrow), text, len(text), 0, None, None, None, None, None, C.byref(cnt), C.byref(pl),
                          C.byref(line), C.byref(code))
    if rc != 0:
        raise L.DexGPUError(rc, f"line {line.value}: DX_IDX code {code.value}")
    n = cnt.value
    off, tl, ns = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hdr, cnr = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.uint16)
    lib.dx_index_seq(int(arrow), text, len(text), n, off.ctypes.data, tl.ctypes.data, ns.ctypes.data,
                     hdr.ctypes.data, cnr.ctypes.data, C.byref(cnt), C.byref(pl), C.byref(line), C.byref(code))
    return off, tl, ns, hdr, cnr, pl.value


def undexqv_plan_size(img: bytes) -> int:
    """Size of the text dx_file_undexqv would produce, from the host walk alone (no GPU, no context)."""
    lib = L.load()
    plan, total = C.c_void_p(), C.c_size_t()
    rc = lib.dx_file_undexqv_plan(img, len(img), C.byref(plan), C.byref(total))
    if rc != 0:
        raise L.DexGPUError(rc, "dx_file_undexqv_plan")
    lib.dx_file_undexqv_plan_free(plan)
    return total.value
