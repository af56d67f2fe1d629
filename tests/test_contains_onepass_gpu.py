"""The one-pass partitioned contains (contains_partitioned.hip) against the oracle.

Stage 1 buckets (bit index, key id) pairs by 2^22-bit region through one line buffer per bucket
and writes them into per-block segments; a cluster of four probe workgroups holds the four
2^20-bit slices of a region in LDS and tests the region's pairs there.  Forced on (mode 1) for
filters and batches far below the sizes the default (mode 2) uses it for, so that every path runs:
less than one slice, one region, a partial last region on the modulo path, many regions; both
stage-1 instantiations (k <= 8, k > 8); the fixed-length and the generic hash; a partial tile,
fewer than 512 blocks, and exactly 512 with more than one tile each; the multi-round flush, the
segment overflow and the miss-record overflow.  Per-key flags and the count equal
oracle.OracleBloom's in mode 1 and in mode 0 (the direct kernel).

The cases are a covering set, not the full product: the filter size decides the region / slice
geometry, k the pairs per key, the key length only the hash, the batch size only the tiling, and no
kernel branches on a combination of them.  So every (size, k) pair runs at the largest batch, and
the other key lengths and batch sizes run at sizes that take each geometry path.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from redisson_amd import Arena
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

SIZES = [1 << 16, 1 << 22, 3 * (1 << 22) - 3, 1 << 27, 1 << 30]
KS = [2, 7, 8, 9, 16]
N_BIG = 200_000


@functools.lru_cache(maxsize=None)
def _tile(fill_permille):
    """1 MiB of Redis-order bitmap bytes with the given share of set bits (read-only)."""
    rng = np.random.default_rng(0x7117 + fill_permille)
    t = np.packbits(rng.random(8 << 20) < fill_permille / 1000.0)
    t.setflags(write=False)
    return t


def _blob(size, fill_permille):
    nbytes = (size + 7) // 8
    blob = np.tile(_tile(fill_permille), (nbytes + (1 << 20) - 1) >> 20)[:nbytes].copy()
    if size % 8:  # bits past `size` stay clear (Redis order: bit i is 0x80 >> (i & 7) of byte i >> 3)
        blob[-1] &= (0xFF00 >> (size % 8)) & 0xFF
    return blob


def _check(client, name, size, k, mat, fill_permille=80, nadd=None, repeat=1):
    """Filter of `size` bits at the given fill plus the first `nadd` keys of `mat`; contains(mat)
    in mode 1 (`repeat` times) and mode 0 against the oracle."""
    n = len(mat)
    nadd = (n + 1) // 2 if nadd is None else nadd
    blob = _blob(size, fill_permille)
    f = client.getBloomFilter(name)
    f.tryInitRaw(size, k)
    f.importBitmap(blob.tobytes())
    ref = O.OracleBloom(size, k)
    ref.bitmap[: len(blob)] = blob
    ref.redis_len = len(blob)
    if nadd:
        f.add(Arena.fixed(mat[:nadd]))
        ref.add(*O.fixed_arena(mat[:nadd]))
    cr, pr = ref.contains(*O.fixed_arena(mat), per_key=True)
    probe = Arena.fixed(mat)
    got = []
    try:
        assert L.lib().rbx_tune(b"contains_partition", 1) == 0
        for _ in range(repeat):
            got.append(f.containsEach(probe))
        got.append((f.contains(probe), None))
        assert L.lib().rbx_tune(b"contains_partition", 0) == 0
        c0, p0 = f.containsEach(probe)
    finally:
        L.lib().rbx_tune(b"contains_partition", 2)
    f.delete()
    assert c0 == cr and np.array_equal(p0, pr)
    for c1, p1 in got:
        assert c1 == cr
        assert p1 is None or np.array_equal(p1, pr)
    return cr


def _keys(seed, n, klen):
    return np.random.default_rng(seed).integers(0, 256, size=(n, klen), dtype=np.uint8)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("size", SIZES)
def test_onepass_sizes_and_k(client, fresh, size, k):
    """Every region geometry with every k, 200,000 32-byte keys (196 or 391 stage-1 blocks)."""
    present = _check(client, fresh, size, k, _keys(size % 997 + k, N_BIG, 32))
    assert present >= N_BIG // 2


@pytest.mark.parametrize("klen", [16, 33])
@pytest.mark.parametrize("size,k", [(1 << 22, 7), (3 * (1 << 22) - 3, 16), (1 << 30, 9), (1 << 30, 2)])
def test_onepass_key_lengths(client, fresh, size, k, klen):
    """16-byte keys (fixed-length hash) and 33-byte keys (the generic-length hash path)."""
    _check(client, fresh, size, k, _keys(klen * 31 + k, N_BIG, klen))


@pytest.mark.parametrize("n", [1, 63, 1024, 1025])
@pytest.mark.parametrize("size,k", [(1 << 16, 7), (3 * (1 << 22) - 3, 8), (1 << 30, 7), (1 << 27, 16)])
def test_onepass_small_batches(client, fresh, size, k, n):
    """A single key, a partial wave, exactly one tile (two at k > 8) and one key more: blocks with
    a partial tile, far fewer than 512 blocks, regions without any pair."""
    _check(client, fresh, size, k, _keys(n * 13 + k, n, 32))


def test_onepass_more_than_one_tile_per_block(client, fresh):
    """600,000 keys at k = 16 are 1,172 tiles on 512 persistent blocks: line buffers and segment
    offsets carry from tile to tile."""
    _check(client, fresh, 1 << 27, 16, _keys(5, 600_000, 32))


def test_onepass_miss_record_overflow(client, fresh):
    """Fill 0.5 at k = 16, absent keys, one region: ~190k clear bits per slice overflow the probe's
    LDS record list (6,400) into the direct atomicOr path."""
    _check(client, fresh, 1 << 22, 16, _keys(77, N_BIG, 32), fill_permille=500, nadd=0)


@pytest.mark.parametrize("size", [1 << 22, 1 << 30])
def test_onepass_repeated_key(client, fresh, size):
    """One added key repeated 5,000 times in a row: whole tiles put all their pairs into k - 1
    buckets, far more than a line buffer's eight (many flush rounds) and than a segment holds
    (overflow into the direct probe)."""
    mat = _keys(size % 991, N_BIG, 32)
    mat[50_000:55_000] = mat[3]
    _check(client, fresh, size, 7, mat)


def test_onepass_same_call_three_times(client, fresh):
    """The same 200,000-key call three times gives identical (the oracle's) flags."""
    _check(client, fresh, 1 << 30, 7, _keys(404, N_BIG, 32), repeat=3)
