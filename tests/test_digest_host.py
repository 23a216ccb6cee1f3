"""The digest's host side (no GPU): the C-ABI of dx_crc32_* / dx_file_digest, and dx_crc32_combine against zlib.crc32."""
import ctypes
import itertools
import os
import re
import zlib

import numpy as np
import pytest

from dextractor_amd import _lib as L
from dextractor_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 65535, 65536, 1 << 20]


def test_abi_has_the_digest():
    hdr = open(os.path.join(ROOT, "include", "dexgpu.h")).read()
    lib = L.load()
    for name in ("dx_crc32_ranges", "dx_crc32_fold", "dx_crc32_combine", "dx_file_digest"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in dexgpu.h"
        assert hasattr(lib, name), f"{name} is not exported by libdexgpu.so"
        assert name in L.SIGNATURES
    assert "dx_digest" in hdr
    for name in ("crc32_ranges", "crc32_fold", "digest"):
        assert callable(getattr(api.Context, name, None)), name
    assert callable(getattr(api, "crc32_combine", None))
    assert "DEXGPU_DIGEST" in open(os.path.join(ROOT, "dextractor_amd", "csrc", "dx_env.h")).read()


def test_digest_layout_matches_the_header():
    """dx_digest as ctypes sees it: two 32-bit fields, then two 64-bit ones, no padding"""
    assert [f for f, _ in L.Digest._fields_] == ["crc32", "reserved", "bytes", "records"]
    assert ctypes.sizeof(L.Digest) == 24
    assert (L.Digest.crc32.offset, L.Digest.reserved.offset, L.Digest.bytes.offset, L.Digest.records.offset) == (0, 4, 8, 16)


@pytest.fixture(scope="module")
def blocks():
    """per length two random blocks and their CRCs"""
    rng = np.random.default_rng(20261018)
    out = {}
    for n in LENGTHS:
        a, b = rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out[n] = (a, zlib.crc32(a), b, zlib.crc32(b))
    return out


def test_the_check_value():
    assert zlib.crc32(b"123456789") == 0xCBF43926
    assert api.crc32_combine(zlib.crc32(b"1234"), zlib.crc32(b"56789"), 5) == 0xCBF43926


def test_combine_is_zlibs_for_all_pairings(blocks):
    for la, lb in itertools.product(LENGTHS, LENGTHS):
        a, ca, _, _ = blocks[la]
        _, _, b, cb = blocks[lb]
        assert api.crc32_combine(ca, cb, lb) == zlib.crc32(a + b), (la, lb)
    a, ca, _, _ = blocks[1 << 20]
    assert zlib.crc32(b"") == 0
    assert api.crc32_combine(0, ca, len(a)) == ca                              # A empty
    assert api.crc32_combine(ca, 0, 0) == ca                                   # B empty
    assert api.crc32_combine(0, 0, 0) == 0


def test_combine_is_associative_over_a_three_way_split(blocks):
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()
    whole = zlib.crc32(data)
    for i, j in [(0, 0), (0, 1), (1, 1), (1, 2), (77, 65613), (4096, 4096), (100000, 299999), (299999, 300000), (300000, 300000)]:
        x, y, z = data[:i], data[i:j], data[j:]
        cx, cy, cz = zlib.crc32(x), zlib.crc32(y), zlib.crc32(z)
        left = api.crc32_combine(api.crc32_combine(cx, cy, len(y)), cz, len(z))
        right = api.crc32_combine(cx, api.crc32_combine(cy, cz, len(z)), len(y) + len(z))
        assert left == right == whole, (i, j)


def test_combine_takes_lengths_beyond_32_bits():
    """x^(8 n) for n >= 2^32 by the same chain of squares: (A, B of 2^32 + 5 zero bytes) in one step and in two"""
    ca = zlib.crc32(b"dextractor")
    zeros = bytes(1 << 20)
    cz = 0
    for _ in range(16):                                                         # the CRC of 16 MiB of zeros, by zlib
        cz = zlib.crc32(zeros, cz)
    big = cz
    for _ in range(8):                                                          # ... doubled eight times: 2^32 zeros
        big = api.crc32_combine(big, big, (1 << 24) << _)
    n = (1 << 32) + 5
    tail = zlib.crc32(bytes(5))
    czn = api.crc32_combine(big, tail, 5)                                       # the CRC of n zeros
    one = api.crc32_combine(ca, czn, n)
    two = api.crc32_combine(api.crc32_combine(ca, big, 1 << 32), tail, 5)
    assert one == two


def test_text_options_are_the_ones_that_give_the_goldens_back():
    """dx_file_text_options (what DEXGPU_DIGEST=1 dexta / dexar / dexqv digest with): the undex* flags tests/golden/cases.json names"""
    import _oracle as O
    assert api.text_options("fasta", O.golden("ta_small.fasta")) == (True, 80)
    assert api.text_options("fasta", O.golden("ta_lower_w60.fasta")) == (False, 60)
    assert api.text_options("arrow", O.golden("ar_small.arrow")) == (False, 80)
    assert api.text_options("quiva", O.golden("qv_mid.quiva")) == (True, 0)
    with pytest.raises(L.DexGPUError) as e:
        api.text_options("fasta", b"not a fasta file\n")
    assert e.value.code == -3
