"""Ranged BITCOUNT / BITPOS on the GPU (rbx_bitset_count_range / _pos and their batches, bitrange_kernels.hip):
every reply equals the brute-force model of bitrange_model.py, on the direct path and through the block
directory, from host and from device arrays."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import bitrange_model as M
from redisson_amd import RedisException
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

DEFAULTS = {"bitrange_dir": 2, "bitrange_pos_chunk": 256 << 10, "bitrange_chain_max": 128 << 10}
BLOCK = 4096  # a directory block, bytes


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k in knobs:
            L.lib().rbx_tune(k.encode(), DEFAULTS[k])


def put(client, name, data: bytes):
    bs = client.getBitSet(name)
    bs.setBytes(data)
    return bs


def dev_arrays(*arrays):
    import torch

    out = [None if a is None else torch.from_numpy(np.asarray(a, np.int64)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def count_dev(client, bs, starts, ends, unit):
    import torch

    d_s, d_e = dev_arrays(starts, ends)
    d_out = torch.full((max(len(starts), 1),), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bs.countRangesDev(d_s.data_ptr(), d_e.data_ptr(), len(starts), d_out.data_ptr(), unit)
    client.synchronize()
    return d_out.cpu().numpy()[: len(starts)].astype(np.uint64)


def pos_dev(client, bs, bit, starts, ends, unit):
    import torch

    d_s, d_e = dev_arrays(starts, ends)
    d_out = torch.full((max(len(starts), 1),), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bs.posRangesDev(bit, d_s.data_ptr(), None if d_e is None else d_e.data_ptr(), len(starts), d_out.data_ptr(), unit)
    client.synchronize()
    return d_out.cpu().numpy()[: len(starts)]


def check_batches(client, bs, data, starts, ends, unit, device=False):
    """count, pos 1 and pos 0 of one batch, and -- BYTE -- the pos forms without ends"""
    assert np.array_equal(bs.countRanges(starts, ends, unit), M.count_ranges(data, starts, ends, unit))
    if device:
        assert np.array_equal(count_dev(client, bs, starts, ends, unit), M.count_ranges(data, starts, ends, unit))
    for bit in (1, 0):
        want = M.pos_ranges(data, bit, starts, ends, unit)
        assert np.array_equal(bs.posRanges(bit, starts, ends, unit), want), bit
        if device:
            assert np.array_equal(pos_dev(client, bs, bit, starts, ends, unit), want), bit
        if unit == M.BYTE:
            want = M.pos_ranges(data, bit, starts)
            assert np.array_equal(bs.posRanges(bit, starts), want), bit
            if device:
                assert np.array_equal(pos_dev(client, bs, bit, starts, None, unit), want), bit


def check_singles(bs, data, pairs, unit):
    for s, e in pairs:
        s, e = int(s), int(e)
        assert bs.bitCount(s, e, unit) == M.bitcount(data, s, e, unit), (s, e, unit)
        for bit in (1, 0):
            assert bs.bitPos(bit, s, e, unit) == M.bitpos(data, bit, s, e, unit), (bit, s, e, unit)
            if unit == M.BYTE:
                assert bs.bitPos(bit, s) == M.bitpos(data, bit, s), (bit, s)


# ---- 1. every interval of a small string ---------------------------------------------------------------------
SMALL = np.random.default_rng(0xB17).bytes(40)
PAIRS = np.array([(lo, hi) for lo in range(320) for hi in range(lo, 320)], np.int64)  # 51,360 queries
_small_want = {}


def small_want():
    """the model's replies, computed once for both directory settings"""
    if not _small_want:
        lo, hi = PAIRS[:, 0], PAIRS[:, 1]
        _small_want["count"] = M.count_ranges(SMALL, lo, hi, M.BIT)
        for bit in (1, 0):
            _small_want[bit] = M.pos_ranges(SMALL, bit, lo, hi, M.BIT)
    return _small_want


@pytest.mark.parametrize("use_dir", [0, 1])
def test_every_interval_of_40_bytes(client, fresh, use_dir):
    """every first-vector and last-vector mask, and both masks in one vector (40 bytes = 2.5 vectors)"""
    assert len(PAIRS) == 51_360
    bs = put(client, fresh, SMALL)
    want = small_want()
    lo, hi = PAIRS[:, 0], PAIRS[:, 1]
    with tuned(bitrange_dir=use_dir):
        assert np.array_equal(bs.countRanges(lo, hi, "BIT"), want["count"])
        assert np.array_equal(count_dev(client, bs, lo, hi, "BIT"), want["count"])
        for bit in (1, 0):
            assert np.array_equal(bs.posRanges(bit, lo, hi, "BIT"), want[bit])
            assert np.array_equal(pos_dev(client, bs, bit, lo, hi, "BIT"), want[bit])
    assert bs.toByteArray() == SMALL
    bs.delete()


def test_every_seventh_interval_as_single_calls(client, fresh):
    bs = put(client, fresh, SMALL)
    want = small_want()
    for i in range(0, len(PAIRS), 7):
        lo, hi = int(PAIRS[i, 0]), int(PAIRS[i, 1])
        assert bs.bitCount(lo, hi, "BIT") == want["count"][i], (lo, hi)
        assert bs.bitPos(1, lo, hi, "BIT") == want[1][i], (lo, hi)
        assert bs.bitPos(0, lo, hi, "BIT") == want[0][i], (lo, hi)
    # one query through the batch entry points takes the single kernels too
    assert bs.countRanges([3], [200], "BIT")[0] == M.bitcount(SMALL, 3, 200, M.BIT)
    assert count_dev(client, bs, [3], [200], "BIT")[0] == M.bitcount(SMALL, 3, 200, M.BIT)
    for bit in (1, 0):
        assert bs.posRanges(bit, [3], [200], "BIT")[0] == M.bitpos(SMALL, bit, 3, 200, M.BIT)
        assert pos_dev(client, bs, bit, [3], [200], "BIT")[0] == M.bitpos(SMALL, bit, 3, 200, M.BIT)
        assert pos_dev(client, bs, bit, [1], None, "BYTE")[0] == M.bitpos(SMALL, bit, 1)
        assert pos_dev(client, bs, bit, [50], [60], "BYTE")[0] == -1  # an empty range: no kernel
    assert count_dev(client, bs, [-10], [-20], "BYTE")[0] == 0
    bs.delete()


# ---- 2. lengths around the vector and the block, four kinds of string --------------------------------------
LENGTHS = [1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 12_293]  # 12,293 = three blocks + 5


def strings_of(n: int):
    """(label, bytes): all zero, all ones, random, and one bit set / cleared at the first, the last and each
    block-edge position"""
    zeros, ones = bytes(n), b"\xff" * n
    yield "zeros", zeros
    yield "ones", ones
    yield "random", np.random.default_rng(n).bytes(n)
    edges = {0, 8 * n - 1}
    for b in range(1, (n + BLOCK - 1) // BLOCK + 1):
        edges |= {p for p in (8 * BLOCK * b - 1, 8 * BLOCK * b) if p < 8 * n}
    for p in sorted(edges):
        a = np.zeros(n, np.uint8)
        a[p >> 3] = 0x80 >> (p & 7)
        yield f"set{p}", a.tobytes()
        yield f"clear{p}", (~a).tobytes()


def queries_of(n: int, unit: int):
    """(starts, ends): every pair of values at and around the ends of the string, negative and past-the-end ones,
    the middle and the block edges"""
    t = 8 * n if unit == M.BIT else n
    blk = 8 * BLOCK if unit == M.BIT else BLOCK
    vals = {0, 1, 2, -1, -2, t - 1, t, t + 3, -t, -t - 2, -t + 1, t // 2, t // 3, -(t // 2), 1 << 40, -(1 << 40)}
    vals |= {v for b in range(1, 4) for v in (b * blk - 1, b * blk, b * blk + 1) if v < t}
    vals = sorted(vals)
    pairs = [(s, e) for s in vals for e in vals]
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_kinds(client, fresh, n):
    rng = np.random.default_rng(n + 1)
    bs = client.getBitSet(fresh)
    for label, data in strings_of(n):
        bs.setBytes(data)
        for unit in (M.BYTE, M.BIT):
            starts, ends = queries_of(n, unit)
            for use_dir in (0, 1):
                with tuned(bitrange_dir=use_dir):
                    check_batches(client, bs, data, starts, ends, unit, device=label == "random")
            pick = rng.choice(len(starts), 6, replace=False)
            check_singles(bs, data, zip(starts[pick], ends[pick]), unit)
        assert bs.bitPos(1) == M.bitpos(data, 1) and bs.bitPos(0) == M.bitpos(data, 0), label
        assert bs.bitCount(0, -1) == bs.cardinality() == M.bitcount(data, 0, -1), label
        assert bs.toByteArray() == data, label
    bs.delete()


# ---- 3. the directory's binary search ------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [1, 0])
@pytest.mark.parametrize("where", ["last block", "block 1", "nowhere"])
def test_directory_binary_search(client, fresh, bit, where):
    """the only wanted bit lies three blocks on, one block on, or nowhere; every search starts in block 0"""
    n = 12_293
    a = np.full(n, 0x00 if bit else 0xFF, np.uint8)
    p = {"last block": 8 * n - 3, "block 1": 8 * BLOCK + 8 * 1000 + 5, "nowhere": None}[where]
    if p is not None:
        a[p >> 3] ^= 0x80 >> (p & 7)
    data = a.tobytes()
    bs = put(client, fresh, data)
    byte_starts = np.array([0, 1, 100, 4095, -n], np.int64)
    bit_starts = np.array([0, 5, 127, 128, 32_767], np.int64)
    for use_dir in (1, 0):
        with tuned(bitrange_dir=use_dir):
            got = bs.posRanges(bit, byte_starts)
            assert np.array_equal(got, M.pos_ranges(data, bit, byte_starts))
            assert set(got.tolist()) == {p if p is not None else (-1 if bit else 8 * n)}
            # ends at, just before and just after the hit, at block edges and at the string's end
            for unit, starts in ((M.BIT, bit_starts), (M.BYTE, byte_starts)):
                t = 8 * n if unit == M.BIT else n
                q = (p if p is not None else t // 2) // (1 if unit == M.BIT else 8)
                blk = 8 * BLOCK if unit == M.BIT else BLOCK
                for end in (-1, t - 1, t + 9, q - 1, q, q + 1, blk - 1, blk, 2 * blk - 1, 2 * blk, 3 * blk - 1, 3 * blk):
                    ends = np.full(starts.size, end, np.int64)
                    assert np.array_equal(bs.posRanges(bit, starts, ends, unit), M.pos_ranges(data, bit, starts, ends, unit)), \
                        (unit, end)
                    assert np.array_equal(bs.countRanges(starts, ends, unit), M.count_ranges(data, starts, ends, unit)), \
                        (unit, end)
    bs.delete()


# ---- 4. one search over many chunks --------------------------------------------------------------------------
def test_single_search_across_257_chunks(client, fresh):
    n = (1 << 20) + 37
    last = 8 * n - 1
    bs = client.getBitSet(fresh)
    with tuned(bitrange_pos_chunk=4096):  # 256 whole chunks and one of 37 bytes
        for bit in (1, 0):
            for p in (8 * 17 + 3, 8 * (128 * 4096 + 9) + 6, 8 * (256 * 4096 + 30) + 1, last, None):
                a = np.full(n, 0x00 if bit else 0xFF, np.uint8)
                if p is not None:
                    a[p >> 3] ^= 0x80 >> (p & 7)
                data = a.tobytes()
                bs.setBytes(data)
                none = -1 if bit else 8 * n
                assert bs.bitPos(bit) == (p if p is not None else none), (bit, p)
                assert bs.bitPos(bit, 1) == M.bitpos(data, bit, 1), (bit, p)
                assert bs.bitPos(bit, 0, -1) == (p if p is not None else -1), (bit, p)
                assert bs.bitPos(bit, 0, -2) == (p if p is not None and p < last - 7 else -1), (bit, p)
                if p is not None:  # a start just behind the hit, an end just before it
                    assert bs.bitPos(bit, p + 1, last, "BIT") == -1
                    assert bs.bitPos(bit, 3, max(p - 1, 3), "BIT") == (-1 if p > 3 else p)
                    assert bs.bitPos(bit, p, p, "BIT") == p
                ones = (1 if p is not None else 0) if bit else 8 * n - (1 if p is not None else 0)
                assert bs.bitCount(0, -1) == ones == bs.cardinality()
                assert bs.bitCount(1, n - 2) == M.bitcount(data, 1, n - 2)
                assert bs.bitCount(5, last - 5, "BIT") == M.bitcount(data, 5, last - 5, M.BIT)
        # two hits: the lower one wins whichever chunk is scanned first
        a = np.zeros(n, np.uint8)
        a[700_000] = 0x01
        a[20_000] = 0x10
        bs.setBytes(a.tobytes())
        assert bs.bitPos(1) == 8 * 20_000 + 3 and bs.bitPos(1, 20_001) == 8 * 700_000 + 7
    data = np.random.default_rng(4).bytes(n)
    bs.setBytes(data)
    for chunk in (4096, 65_536, DEFAULTS["bitrange_pos_chunk"], 1 << 20):
        with tuned(bitrange_pos_chunk=chunk):
            assert bs.bitPos(1, 1000) == M.bitpos(data, 1, 1000) and bs.bitPos(0, -9) == M.bitpos(data, 0, -9)
    assert bs.bitCount(0, -1) == M.bitcount(data, 0, -1) == bs.cardinality()
    assert bs.bitCount(3, 1_000_003, "BIT") == M.bitcount(data, 3, 1_000_003, M.BIT)
    bs.delete()


def test_single_search_claims_chunks_beyond_the_grid(client, fresh):
    """2,305 chunks of 4 KiB against a grid of at most 2,048 workgroups: chunks 2,048 and up are claimed through
    the ticket word.  The hit lies in a chunk the grid owns, in claimed chunks, in the last, partial chunk, and
    nowhere; with the hit low, the claims are abandoned behind it."""
    chunk, grid = 4096, 2048
    n = 2304 * chunk + 37
    assert n // chunk + 1 > grid + 256
    last = 8 * n - 1
    bs = client.getBitSet(fresh)
    spots = {"grid's chunk 3": 8 * (3 * chunk + 77) + 2, "grid's last chunk": 8 * (2047 * chunk + 4095) + 7,
             "first claimed chunk": 8 * (2048 * chunk) + 0, "claimed chunk 2200": 8 * (2200 * chunk + 1234) + 5,
             "partial chunk": 8 * (2304 * chunk + 20) + 4, "last bit": last, "nowhere": None}
    with tuned(bitrange_pos_chunk=chunk):
        for bit in (1, 0):
            for where, p in spots.items():
                a = np.full(n, 0x00 if bit else 0xFF, np.uint8)
                if p is not None:
                    a[p >> 3] ^= 0x80 >> (p & 7)
                bs.setBytes(a.tobytes())
                none = -1 if bit else 8 * n
                assert bs.bitPos(bit) == (p if p is not None else none), (bit, where)
                assert bs.bitPos(bit, 0, -1) == (p if p is not None else -1), (bit, where)
                # a start that shifts every chunk edge; 2,280 chunks are left
                assert bs.bitPos(bit, 100_003) == (p if p is not None and p >= 8 * 100_003 else none), (bit, where)
                if p is not None:
                    assert bs.bitPos(bit, p + 1, last, "BIT") == -1, (bit, where)
                    assert bs.bitPos(bit, 3, max(p - 1, 3), "BIT") == -1, (bit, where)
                    assert bs.bitPos(bit, 0, p, "BIT") == p, (bit, where)
        # two hits in claimed chunks, and one in the grid's part before them: the lowest wins
        a = np.zeros(n, np.uint8)
        a[2300 * chunk + 9] = 0x01
        a[2100 * chunk + 50] = 0x10
        bs.setBytes(a.tobytes())
        assert bs.bitPos(1) == 8 * (2100 * chunk + 50) + 3
        assert bs.bitPos(1, 2100 * chunk + 51) == 8 * (2300 * chunk + 9) + 7
        a[1500 * chunk] = 0x80
        bs.setBytes(a.tobytes())
        assert bs.bitPos(1) == 8 * 1500 * chunk and bs.bitPos(1, 1) == 8 * 1500 * chunk
        # random bytes from the claimed part on, against the model
        data = np.random.default_rng(5).bytes(n)
        bs.setBytes(data)
        tail = data[2048 * chunk:]
        for bit in (1, 0):
            assert bs.bitPos(bit) == M.bitpos(data[:64], bit)
            assert bs.bitPos(bit, 2048 * chunk + 5) == 8 * 2048 * chunk + M.bitpos(tail, bit, 5)
    bs.delete()


# ---- 5. the path choice ----------------------------------------------------------------------------------------
def test_path_choice_answers_the_same(client, fresh):
    """dir = 2 decides by bytes read (S > L + n * 8192) and by the longest range (M > bitrange_chain_max); batches
    on each side of both rules answer as under 0 and 1"""
    n = 64 << 10
    data = np.random.default_rng(8).bytes(n)
    bs = put(client, fresh, data)
    small = (np.arange(4, dtype=np.int64) * 9000 + 3, np.arange(4, dtype=np.int64) * 9000 + 1026)  # S = 4 KiB: walk
    whole = (np.array([0, 1, 2, 3], np.int64), np.array([-1, -2, -3, -4], np.int64))  # S = 4 L > L + 32 KiB: directory
    one_long = (np.array([0, 10, 20_000], np.int64), np.array([5, 10, 29_000], np.int64))  # M = 9,001 bytes
    for starts, ends, knobs, directory in ((*small, {}, 0), (*whole, {}, 1), (*one_long, {"bitrange_chain_max": 9001}, 0),
                                           (*one_long, {"bitrange_chain_max": 9000}, 1)):
        covered = [M.normalise(int(s), int(e), M.BYTE, n) for s, e in zip(starts, ends)]
        covered = [(r[1] - r[0] + 1) // 8 for r in covered if r is not None]
        with tuned(**knobs):  # the batch is on the side of the rule it was built for
            assert L.lib().rbx_bench_bitrange_path(n, len(starts), sum(covered), max(covered)) == directory
        got = []
        for use_dir in (2, 0, 1):
            with tuned(bitrange_dir=use_dir, **knobs):
                got.append((bs.countRanges(starts, ends), bs.posRanges(1, starts, ends), bs.posRanges(0, starts, ends),
                            bs.posRanges(0, starts), count_dev(client, bs, starts, ends, "BYTE"),
                            pos_dev(client, bs, 1, starts, ends, "BYTE")))
        want = (M.count_ranges(data, starts, ends), M.pos_ranges(data, 1, starts, ends), M.pos_ranges(data, 0, starts, ends),
                M.pos_ranges(data, 0, starts), M.count_ranges(data, starts, ends), M.pos_ranges(data, 1, starts, ends))
        for g in got:
            assert all(np.array_equal(x, y) for x, y in zip(g, want))
    bs.delete()


# ---- 6. keys -----------------------------------------------------------------------------------------------------
def test_missing_empty_and_wrong_type_keys(client, fresh):
    starts, ends = np.array([0, -5, 2], np.int64), np.array([-1, 3, 1], np.int64)
    bs = client.getBitSet(fresh)
    for use_dir in (0, 1, 2):
        with tuned(bitrange_dir=use_dir):
            # a missing key: 0 ones, no set bit, and clear bits from position 0
            assert bs.bitCount(0, -1) == 0 and bs.bitPos(1) == -1 and bs.bitPos(0) == 0 and bs.bitPos(0, 3, 9) == 0
            assert bs.countRanges(starts, ends).tolist() == [0, 0, 0]
            assert bs.posRanges(1, starts, ends).tolist() == [-1, -1, -1] and bs.posRanges(0, starts).tolist() == [0, 0, 0]
            assert count_dev(client, bs, starts, ends, "BYTE").tolist() == [0, 0, 0]
            assert pos_dev(client, bs, 1, starts, ends, "BIT").tolist() == [-1, -1, -1]
            assert pos_dev(client, bs, 0, starts, None, "BYTE").tolist() == [0, 0, 0]
            assert not bs.isExists()
    # an existing empty string is not a missing key: every range is empty
    bs.setBytes(b"")
    assert bs.isExists() and bs.size() == 0
    assert bs.bitCount(0, -1) == 0 and bs.bitPos(1) == -1 and bs.bitPos(0) == -1 and bs.bitPos(0, 0, -1, "BIT") == -1
    assert bs.countRanges(starts, ends).tolist() == [0, 0, 0]
    for bit in (1, 0):
        assert bs.posRanges(bit, starts, ends).tolist() == [-1, -1, -1] and bs.posRanges(bit, starts).tolist() == [-1, -1, -1]
        assert pos_dev(client, bs, bit, starts, ends, "BYTE").tolist() == [-1, -1, -1]
        assert pos_dev(client, bs, bit, starts[:1], None, "BYTE").tolist() == [-1]
    assert count_dev(client, bs, starts, ends, "BIT").tolist() == [0, 0, 0]
    assert bs.isExists() and bs.toByteArray() == b""
    bs.delete()
    # the argument errors reach no key
    with pytest.raises(RedisException, match="must be 1 or 0"):
        bs.bitPos(2)
    with pytest.raises(RedisException, match="syntax error"):
        bs.bitPos(1, 0, None, "BIT")
    with pytest.raises(RedisException, match="syntax error"):
        bs.posRanges(1, starts, None, "BIT")
    # other types: an HLL string and a filter's config hash
    client.getHyperLogLog(fresh + ":hll").add(b"x")
    f = client.getBloomFilter(fresh + ":bf")
    assert f.tryInit(1000, 0.01)
    for name in (fresh + ":hll", "{" + fresh + ":bf}:config"):
        other = client.getBitSet(name)
        for call in (lambda: other.bitCount(0, -1), lambda: other.bitPos(1), lambda: other.countRanges(starts, ends),
                     lambda: other.posRanges(0, starts), lambda: count_dev(client, other, starts, ends, "BYTE"),
                     lambda: pos_dev(client, other, 1, starts, ends, "BYTE")):
            with pytest.raises(RedisException, match="WRONGTYPE"):
                call()
    # a Bloom filter's key is a bit set
    f.add([b"k%d" % i for i in range(500)])
    fb = client.getBitSet(fresh + ":bf")
    assert fb.bitCount(0, -1) == f.bitcount() == fb.countRanges([0, 0], [-1, -1])[0] > 0
    assert fb.bitPos(1) == M.bitpos(fb.toByteArray(), 1)
    f.delete()
    client.getHyperLogLog(fresh + ":hll").delete()


def test_reads_leave_the_key_alone(client, fresh):
    data = np.random.default_rng(3).bytes(5000)
    bs = put(client, fresh, data)
    assert bs.expire(600_000)
    expires = bs.getExpireTime()
    starts, ends = np.array([0, 4990, -3, 70_000], np.int64), np.array([9999, 9000, -1, 80_000], np.int64)
    for use_dir in (0, 1):
        with tuned(bitrange_dir=use_dir):
            check_batches(client, bs, data, starts, ends, M.BYTE, device=True)
            check_batches(client, bs, data, starts * 8, ends * 8, M.BIT, device=True)
    check_singles(bs, data, zip(starts, ends), M.BYTE)
    assert bs.toByteArray() == data and bs.size() == 8 * len(data) and bs.getExpireTime() == expires
    bs.delete()
    # n = 0 sends nothing: no key appears, whatever the arrays are
    empty = np.zeros(0, np.int64)
    assert bs.countRanges(empty, empty).size == 0 and bs.posRanges(1, empty).size == 0
    nm, _keep = L.name_struct(fresh)
    assert L.lib().rbx_bitset_count_ranges_dev(client.ctx, nm, None, None, 0, 0, None, None) == L.RBX_OK
    assert L.lib().rbx_bitset_pos_ranges_dev(client.ctx, nm, 0, None, None, 0, 0, None, None) == L.RBX_OK
    out = C.c_int64()
    assert L.lib().rbx_bitset_pos(client.ctx, nm, 1, 3, 0, 0, 0, C.byref(out)) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_bitset_pos(client.ctx, nm, 1, 2, 0, 0, 2, C.byref(out)) == L.RBX_E_ILLEGAL_ARGUMENT
    assert not bs.isExists()
