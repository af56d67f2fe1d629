"""The partitioned contains on 5-byte entries (redisson_amd/csrc/bk_entry.h).

Stage 1 writes an entry as a 21-bit offset inside its region and a 19-bit key index local to the stage-1
block, q = tile iteration * 1024 + thread, twelve entries to a 64-byte line; the probe rebuilds the
chunk's key id from q, the segment's block and the grid when a bit is clear.  The cases are the places
where this format can go wrong and 8-byte (bit index, key id) pairs could not: every high bit of q (a
block's 512th tile, reached on a small batch through rbx_tune "contains_stage1_grid"), the split into
chunks at grid * 2^19 keys, segments that end just before, at and just after a line boundary, a full line
followed by a stale-tailed partial one, and the default grid at k = 16.

The scheme is tests/test_contains_regions_gpu.py's: mode 1 forced through rbx_tune, per-key flags and the
count equal oracle.OracleBloom's, the same in mode 0 (the direct kernel), mode 2 and the grid restored.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from redisson_amd import Arena
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

TILE = 1024
GRID_DEFAULT = 256


@functools.lru_cache(maxsize=None)
def _tile(fill_permille):
    """1 MiB of Redis-order bitmap bytes with the given share of set bits (read-only)."""
    rng = np.random.default_rng(0x5B + fill_permille)
    t = np.packbits(rng.random(8 << 20) < fill_permille / 1000.0)
    t.setflags(write=False)
    return t


def _blob(size, fill_permille):
    nbytes = (size + 7) // 8
    if fill_permille == 0:
        return np.zeros(nbytes, dtype=np.uint8)
    blob = np.tile(_tile(fill_permille), (nbytes + (1 << 20) - 1) >> 20)[:nbytes].copy()
    if size % 8:
        blob[-1] &= (0xFF00 >> (size % 8)) & 0xFF
    return blob


def _keys(seed, n, klen=32):
    return np.random.default_rng(seed).integers(0, 256, size=(n, klen), dtype=np.uint8)


def _check(client, name, size, k, mat, fill_permille, added, grid=GRID_DEFAULT):
    """Filter of `size` bits at the given fill plus the keys `added`; containsEach and contains of `mat` in
    mode 1 at the given stage-1 grid, containsEach in mode 0, all against the oracle."""
    blob = _blob(size, fill_permille)
    f = client.getBloomFilter(name)
    f.tryInitRaw(size, k)
    f.importBitmap(blob.tobytes())
    ref = O.OracleBloom(size, k)
    ref.bitmap[: len(blob)] = blob
    ref.redis_len = len(blob)
    del blob
    if len(added):
        f.add(Arena.fixed(added))
        ref.add(*O.fixed_arena(added))
    cr, pr = ref.contains(*O.fixed_arena(mat), per_key=True)
    probe = Arena.fixed(mat)
    try:
        assert L.lib().rbx_tune(b"contains_stage1_grid", grid) == 0
        assert L.lib().rbx_tune(b"contains_partition", 1) == 0
        c1, p1 = f.containsEach(probe)
        c1b = f.contains(probe)
        assert L.lib().rbx_tune(b"contains_partition", 0) == 0
        c0, p0 = f.containsEach(probe)
    finally:
        L.lib().rbx_tune(b"contains_partition", 2)
        L.lib().rbx_tune(b"contains_stage1_grid", GRID_DEFAULT)
    f.delete()
    assert c0 == cr and np.array_equal(p0, pr)
    bad = np.flatnonzero(p1 != pr)
    assert bad.size == 0, (bad.size, bad[:8])
    assert c1 == cr and c1b == cr
    return cr, pr


@pytest.mark.parametrize("extra", [0, TILE])
def test_entries5_every_high_bit_of_q(client, fresh, extra):
    """Two stage-1 blocks of 512 tiles each: q runs over all of [0, 2^19).  At fill 0.5 about half the keys
    pass bit 0 and most of those record a miss, so a key rebuilt wrongly is a wrong flag (on that key and on
    the one named instead).  With 1024 more keys the batch is past 2 * 2^19 and splits into two chunks."""
    n = 2 * 512 * TILE + extra
    mat = _keys(0x919 + extra, n)
    present, flags = _check(client, fresh, 1 << 27, 7, mat, 500, mat[: n // 2], grid=2)
    assert present >= n // 2
    assert not flags[n // 2:].all()  # the second half is mostly absent: its misses are what names keys


def _repeat_case(client, fresh, r, positions, n):
    """k = 2 (one entry per surviving key), an empty filter holding one added key, that key at `positions` among
    otherwise absent keys: its bucket's segment in the block(s) that hash those positions holds exactly the
    repeats, every other segment nothing (an absent key fails bit 0 unless it shares that one bit)."""
    mat = _keys(0x12 + r + n, n)
    key = mat[0].copy()
    mat[0] = mat[1] ^ 0x55  # the added key appears only where the case puts it
    mat[positions] = key
    present, flags = _check(client, fresh, 1 << 27, 2, mat, 0, key[None, :])
    assert flags[positions].all()
    assert present >= r


@pytest.mark.parametrize("r", [1, 11, 12, 13, 24, 25])
def test_entries5_line_boundaries_one_tile(client, fresh, r):
    """r repeats inside one tile: r entries in one segment, i.e. a partial line, exactly one or two full lines
    (the block-end store then has nothing left), and full lines followed by a partial one."""
    positions = 5 * TILE + 7 + 3 * np.arange(r)  # tile 5: block 5, its first tile
    _repeat_case(client, fresh, r, positions, 8 * TILE + 1)


@pytest.mark.parametrize("r", [1, 11, 12, 13, 24, 25])
def test_entries5_line_boundaries_three_tiles(client, fresh, r):
    """The repeats spread over the three tiles of block 0 (tiles 0, 256 and 512 of 513): the line buffer is
    carried from tile to tile, a full line is flushed in a later tile than it was begun in, and the partial
    line stored at the block's end holds stale entries of the flushed one past its count."""
    n = 2 * 256 * TILE + TILE
    tiles = np.array([0, 256, 512])
    positions = tiles[np.arange(r) % 3] * TILE + 11 + 5 * (np.arange(r) // 3)
    _repeat_case(client, fresh, r, positions, n)


def test_entries5_default_grid_k16(client, fresh):
    """Three tiles per block on the default grid (the last of one key) at k = 16: fifteen entries per
    surviving key, q in three tile iterations, every block's segments ending in partial lines."""
    n = 256 * 2 * TILE + 1
    mat = _keys(0x16, n)
    present, _ = _check(client, fresh, 1 << 27, 16, mat, 80, mat[: (n + 1) // 2])
    assert present >= n // 2
