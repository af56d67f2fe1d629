"""The partitioned contains at 2048 regions of 2^21 bits, probed by clusters of two workgroups.

Stage 1 (one 1024-thread block per CU, 1024-key tiles) buckets (bit index, key id) pairs by
2^21-bit region through 2048 line buffers; the two workgroups of a probe cluster hold the two
2^20-bit slices of a region in LDS.  The cases are the places where this geometry can go wrong
and the older one (1024 regions of 2^22 bits, 512-key tiles, clusters of four) could not: sizes
at the region boundary, the largest region count (2^32 - 3 bits: every line buffer and list entry
in use), batches at the 1024-key tile and at one tile per block plus one, line buffers carried
over tiles, a multi-round flush with 128 line groups per step, and the miss-record overflow.

The scheme is tests/test_contains_onepass_gpu.py's: mode 1 forced through rbx_tune, per-key flags
and the count equal oracle.OracleBloom's, the same in mode 0 (the direct kernel), mode 2 restored.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from redisson_amd import Arena
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

REGION = 1 << 21
N_BIG = 200_000


@functools.lru_cache(maxsize=None)
def _tile(fill_permille):
    """1 MiB of Redis-order bitmap bytes with the given share of set bits (read-only)."""
    rng = np.random.default_rng(0x2048 + fill_permille)
    t = np.packbits(rng.random(8 << 20) < fill_permille / 1000.0)
    t.setflags(write=False)
    return t


def _blob(size, fill_permille):
    nbytes = (size + 7) // 8
    blob = np.tile(_tile(fill_permille), (nbytes + (1 << 20) - 1) >> 20)[:nbytes].copy()
    if size % 8:  # bits past `size` stay clear (Redis order: bit i is 0x80 >> (i & 7) of byte i >> 3)
        blob[-1] &= (0xFF00 >> (size % 8)) & 0xFF
    return blob


def _check(client, name, size, k, mat, fill_permille=80, nadd=None):
    """Filter of `size` bits at the given fill plus the first `nadd` keys of `mat`; containsEach
    and contains of `mat` in mode 1, containsEach in mode 0, all against the oracle."""
    n = len(mat)
    nadd = (n + 1) // 2 if nadd is None else nadd
    blob = _blob(size, fill_permille)
    f = client.getBloomFilter(name)
    f.tryInitRaw(size, k)
    f.importBitmap(blob.tobytes())
    ref = O.OracleBloom(size, k)
    ref.bitmap[: len(blob)] = blob
    ref.redis_len = len(blob)
    del blob
    if nadd:
        f.add(Arena.fixed(mat[:nadd]))
        ref.add(*O.fixed_arena(mat[:nadd]))
    cr, pr = ref.contains(*O.fixed_arena(mat), per_key=True)
    probe = Arena.fixed(mat)
    try:
        assert L.lib().rbx_tune(b"contains_partition", 1) == 0
        c1, p1 = f.containsEach(probe)
        c1b = f.contains(probe)
        assert L.lib().rbx_tune(b"contains_partition", 0) == 0
        c0, p0 = f.containsEach(probe)
    finally:
        L.lib().rbx_tune(b"contains_partition", 2)
    f.delete()
    assert c0 == cr and np.array_equal(p0, pr)
    assert c1 == cr and np.array_equal(p1, pr)
    assert c1b == cr
    return cr


def _keys(seed, n, klen=32):
    return np.random.default_rng(seed).integers(0, 256, size=(n, klen), dtype=np.uint8)


@pytest.mark.parametrize("k", [7, 16])
@pytest.mark.parametrize("size", [REGION, REGION + 1, 3 * REGION - 3])
def test_regions_boundary_sizes(client, fresh, size, k):
    """Exactly one region, one bit more (a second region of one bit, the exact-modulo path) and a
    partial third region: both slices of a two-workgroup cluster hold pairs, and the last region's
    second slice may lie past the bitmap's end."""
    present = _check(client, fresh, size, k, _keys(size % 1009 + k, N_BIG))
    assert present >= N_BIG // 2


def test_regions_all_2048_buckets(client, fresh):
    """2^32 - 3 bits are 2048 regions (nb == kBkMaxBuckets): every line buffer and list entry of
    stage 1 is in use and the probe's 128 clusters walk 16 regions each.  The filter holds only the
    tiled blob, at fill 0.5: half the keys pass bit 0 (~290 pairs per region), ~0.8% are present."""
    size = (1 << 32) - 3
    present = _check(client, fresh, size, 7, _keys(2048, N_BIG), fill_permille=500, nadd=0)
    assert 0 < present < N_BIG // 20


@pytest.mark.parametrize("n", [1024, 1025, 256 * 1024 + 1])
def test_regions_tiling(client, fresh, n):
    """Exactly one 1024-key tile, one key more (a second block with one key), and 257 tiles on 256
    persistent blocks: block 0 runs a second tile of one key while 255 blocks run one."""
    _check(client, fresh, 1 << 27, 7, _keys(n % 1013, n))


def test_regions_tile_carry(client, fresh):
    """600,000 keys at k = 16 are 586 tiles on 256 blocks (two or three each): line buffers, list
    parity and segment offsets carry from tile to tile."""
    _check(client, fresh, 1 << 27, 16, _keys(586, 600_000))


@pytest.mark.parametrize("size", [REGION, 1 << 30])
def test_regions_repeated_key(client, fresh, size):
    """One added key repeated 5,000 times in a row: whole 1024-key tiles put their 6,144 pairs into
    at most k - 1 buckets, so the flush runs many rounds (128 line groups per step) and the segments
    overflow into the direct probe."""
    mat = _keys(size % 983, N_BIG)
    mat[50_000:55_000] = mat[3]
    _check(client, fresh, size, 7, mat)


def test_regions_miss_record_overflow(client, fresh):
    """Fill 0.5 at k = 16, absent keys, one region of two slices: ~375k clear bits per slice
    overflow the probe's LDS record list (6,400) into the direct atomicOr path."""
    _check(client, fresh, REGION, 16, _keys(79, N_BIG), fill_permille=500, nadd=0)
