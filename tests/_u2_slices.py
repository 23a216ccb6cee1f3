"""The text tests/test_u2_slices_host.py and tests/test_gpu_u2_slices.py pack: the shapes at which the slice loop of the packed-read
drivers (csrc/dx_file_u2.c) would show a wrong offset or a wrong carve of its record arrays."""
import numpy as np

BIG, EMPTY = 20, (0, 12, 13, 39)
PLANT = "GGCCAATTGGCCAT"          # at both ends of the long record and of the records beside the empty ones: where a slice begins or ends


def synthetic(n=40, seed=5):
    """n .fasta records of 30 .. 1500 letters: the first and the last empty, two empty ones side by side, and one of 20000 letters,
    whose 5000 packed bytes alone exceed a budget of 4096 -> (the text, the n records' lengths).  The reference's dexta refuses a text
    whose last line is a header (dexta.c:165-172), so the text has one record more, of four letters, which image() cuts off again."""
    rng = np.random.default_rng(seed)
    out, lens = [], []
    for i in range(n):
        ln = 0 if i in EMPTY else 20000 if i == BIG else int(rng.integers(30, 1501))
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, ln))
        if i == BIG or any(abs(i - e) == 1 for e in EMPTY) and ln:
            s = PLANT + s[14:ln - 14] + PLANT
        out.append(f">u2s/{7 + 2 * i}/0_{ln} RQ=0.850" + "".join("\n" + s[k:k + 70] for k in range(0, ln, 70)))
        lens.append(ln)
    out.append(f">u2s/{7 + 2 * n}/0_4 RQ=0.850\nACGT")
    return ("\n".join(out) + "\n").encode(), lens


def image(pack, text):
    """the image `pack` (a dexta) makes of synthetic()'s text, without its last record: a well byte, beg, end and qv, one byte of reads"""
    img = pack(text)
    return img[:len(img) - (1 + 12 + 1)]


def slices(lens, cap, framing=13):
    """how many slices of whole records the image's reads go in under a cap of `cap` bytes of image (0: one): as many records as span
    at most `cap` bytes from the first one's reads to the last one's end, and one at least; framing: a well byte, beg, end and qv"""
    if cap == 0:
        return 1 if lens else 0
    count, i = 0, 0
    while i < len(lens):
        span, j = (lens[i] + 3) // 4, i + 1
        while j < len(lens) and span + framing + (lens[j] + 3) // 4 <= cap:
            span += framing + (lens[j] + 3) // 4
            j += 1
        count, i = count + 1, j
    return count
