"""What dx_diff_ranges, dx_code_diff and dx_file_compare are to compute, stated in numpy on host arrays and on two TEXTS -- the
reference of tests/test_gpu_diff.py and tests/test_gpu_compare.py.  Nothing here calls the library."""
import numpy as np

NONE32 = 0xFFFFFFFF


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _tally(differ, first, sums, maxs, kind, nkinds):
    """per-unit figures -> what the call gives back"""
    differ = np.asarray(differ, np.uint32); first = np.asarray(first, np.uint32)
    kind = np.zeros(len(differ), np.uint8) if kind is None else np.asarray(kind, np.uint8)
    out = {"rec_differ": differ, "rec_first": first}
    out["differ"] = np.array([int(differ[kind == k].astype(np.uint64).sum()) for k in range(nkinds)], np.uint64)
    out["units"] = np.array([int((differ[kind == k] != 0).sum()) for k in range(nkinds)], np.uint64)
    out["sum_abs"] = np.array([sum(s for s, q in zip(sums, kind) if q == k) for k in range(nkinds)], np.uint64)
    out["max_abs"] = np.array([max([m for m, q in zip(maxs, kind) if q == k], default=0) for k in range(nkinds)], np.uint64)
    hit = np.flatnonzero(differ)
    out["first"] = (int(hit[0]), int(first[hit[0]])) if len(hit) else None
    return out


def diff_ranges(a, a_off, b, b_off, ln, kind=None, nkinds=1, a_and=None):
    """unit j: a[a_off[j] .. + ln[j]) & a_and[kind[j]] against b[b_off[j] .. + ln[j]) -> {"rec_differ", "rec_first" (per unit),
    "differ", "units", "sum_abs", "max_abs" (per kind), "first": (unit, position) or None}"""
    a = np.frombuffer(bytes(a), np.uint8); b = np.frombuffer(bytes(b), np.uint8)
    differ, first, sums, maxs = [], [], [], []
    for j in range(len(ln)):
        n, ao, bo = int(ln[j]), int(a_off[j]), int(b_off[j])
        m = 0xFF if a_and is None else int(a_and[0 if kind is None else int(kind[j])])
        x = (a[ao:ao + n] & m).astype(np.int64); y = b[bo:bo + n].astype(np.int64)
        assert len(x) == n and len(y) == n, "a reference unit outside its buffer"
        d = np.flatnonzero(x != y)
        differ.append(len(d)); first.append(int(d[0]) if len(d) else NONE32)
        sums.append(int(np.abs(x - y).sum())); maxs.append(int(np.abs(x - y).max()) if n else 0)
    return _tally(differ, first, sums, maxs, kind, nkinds)


def symbols(packed, at, n):
    """the first n symbols of the packed read at byte `at` (DB.c:319-338: four a byte, the first in the top two bits)"""
    raw = np.frombuffer(bytes(packed), np.uint8)[at:at + (n + 3) // 4]
    assert len(raw) == (n + 3) // 4, "a reference read outside its buffer"
    return np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[:n]


def code_diff(a, a_boff, b, b_boff, ln):
    """unit j: symbols [0, ln[j]) of the packed read at a + a_boff[j] against those at b + b_boff[j]; the pad bits of the last byte
    belong to no symbol -> {"rec_differ", "rec_first", "symbols", "units", "first"}"""
    differ, first = [], []
    for j in range(len(ln)):
        d = np.flatnonzero(symbols(a, int(a_boff[j]), int(ln[j])) != symbols(b, int(b_boff[j]), int(ln[j])))
        differ.append(len(d)); first.append(int(d[0]) if len(d) else NONE32)
    t = _tally(differ, first, [0] * len(ln), [0] * len(ln), None, 1)
    return {"rec_differ": t["rec_differ"], "rec_first": t["rec_first"], "symbols": int(t["differ"][0]), "units": int(t["units"][0]),
            "first": t["first"]}


def packed_reads(img, arrow=False):
    """the records of a .dexta / .dexar image of either key (0x55aa; dexta's legacy 0x33cc) and either byte order, walked as
    undexta.c:138-271 does it -> (offsets of the packed reads, their symbols)"""
    key = int.from_bytes(img[:2], "little")
    order = "little" if key in (0x55AA, 0x33CC) else "big"
    legacy = key in (0x33CC, 0xCC33)
    assert key in (0x55AA, 0xAA55, 0x33CC, 0xCC33) and not (legacy and arrow)
    w = 2 if legacy else 4
    at, off, ln = 6 + int.from_bytes(img[2:6], order), [], []
    while at < len(img):
        while img[at] == 255:
            at += 1
        at += 1
        beg, end = int.from_bytes(img[at:at + w], order), int.from_bytes(img[at + w:at + 2 * w], order)
        at += 2 * w + (2 if legacy else 8 if arrow else 4)
        off.append(at); ln.append(end - beg)
        at += (end - beg + 3) // 4
    return np.array(off, np.uint64), np.array(ln, np.uint32)


# ---- the file report, from two texts -----------------------------------------------------------------------------------------------
def _header(line):
    """>prefix/well/beg_end RQ=0.qv | SN=a,b,c,d -> (prefix, (well, beg, end, rest))"""
    name, _, rest = line[1:].partition(b" ")
    prefix, well, span = name.rsplit(b"/", 2)
    beg, end = span.split(b"_")
    if rest.startswith(b"RQ=0."):
        extra = (int(rest[5:]),)
    else:
        extra = tuple(int(round(float(v) * 100)) for v in rest[3:].split(b","))
    return prefix, (int(well), int(beg), int(end)) + extra


def records(kind, text):
    """a text -> [(prefix, header fields, [lines as uint8 arrays])]: one line of symbols for fasta / arrow (case folded, the line
    breaks taken out), five for quiva (the tag line in lower case)"""
    lines = text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n")
    out = []
    if kind == "quiva":
        for i in range(0, len(lines), 6):
            prefix, h = _header(lines[i])
            body = [np.frombuffer(l, np.uint8) for l in lines[i + 1:i + 6]]
            body[1] = np.frombuffer(lines[i + 2].lower(), np.uint8)
            out.append((prefix, h, body))
        return out
    starts = [i for i, l in enumerate(lines) if l.startswith(b">")] + [len(lines)]
    for s, e in zip(starts, starts[1:]):
        prefix, h = _header(lines[s])
        out.append((prefix, h, [np.frombuffer(b"".join(lines[s + 1:e]).lower(), np.uint8)]))
    return out


LOSSY_AND = (0xFF, 0xFF, 0xFE, 0xFC, 0xFF)          # what dexqv -l keeps of the del, tag, ins, mrg, sub lines (QV.c:1406-1415)


def report(kind, text_a, text_b, lossy=False):
    """dx_file_compare's report, as Context.compare(per_record=True) returns it, from the two TEXTS"""
    ra, rb = records(kind, text_a), records(kind, text_b)
    lines = 5 if kind == "quiva" else 1
    both = min(len(ra), len(rb))
    out = {"lines": lines, "records_a": len(ra), "records_b": len(rb),
           "prefix_differs": bool(ra and rb and ra[0][0] != rb[0][0]),
           "headers_differ": 0, "first_header": None, "lengths_differ": 0, "first_length": None,
           "records_differ": 0, "first_record": None, "first_line": None, "first_column": None}
    differ, recs, sums, maxs = ([0] * lines for _ in range(4))
    rec = np.zeros((both, lines), np.uint32)
    for i in range(both):
        (_, ha, la), (_, hb, lb) = ra[i], rb[i]
        if ha != hb:
            out["headers_differ"] += 1
            out["first_header"] = i if out["first_header"] is None else out["first_header"]
        if len(la[0]) != len(lb[0]):
            out["lengths_differ"] += 1
            out["first_length"] = i if out["first_length"] is None else out["first_length"]
        n = min(len(la[0]), len(lb[0]))
        for q in range(lines):
            x = (la[q][:n] & (LOSSY_AND[q] if lossy else 0xFF)).astype(np.int64); y = lb[q][:n].astype(np.int64)
            d = np.flatnonzero(x != y)
            rec[i, q] = len(d)
            if len(d):
                differ[q] += len(d); recs[q] += 1
                if kind == "quiva":
                    sums[q] += int(np.abs(x - y).sum()); maxs[q] = max(maxs[q], int(np.abs(x - y).max()))
                if out["first_record"] is None:
                    out["first_record"], out["first_line"], out["first_column"] = i, q, int(d[0])
        out["records_differ"] += int(rec[i].any())
    out["differ"], out["line_records"] = np.array(differ, np.uint64), np.array(recs, np.uint64)
    out["sum_abs"], out["max_abs"] = np.array(sums, np.uint64), np.array(maxs, np.uint64)
    out["rec_differ"] = rec
    out["same"] = (len(ra) == len(rb) and not out["prefix_differs"] and out["headers_differ"] == 0 and out["lengths_differ"] == 0
                   and out["records_differ"] == 0)
    return out


def assert_same_report(got, want):
    """field by field, arrays by value"""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])
