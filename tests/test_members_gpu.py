"""Set-bit enumeration and the java.util.BitSet exchange on the GPU (rbx_bitset_members / _as_words / _set_words,
members_kernels.hip): every output equals members_model.py in full -- positions, written, total, and the memory behind
the page untouched -- from host and from device arrays."""
import ctypes as C

import numpy as np
import pytest

import members_model as M
from redisson_amd import IllegalArgumentException, RedisException
from redisson_amd import _lib as L
from redisson_amd.client import BloomHandle, _config_name

pytestmark = pytest.mark.gpu

BLOCK = 4096  # a directory block, bytes
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8195, 3 * 4096 + 5]
BIG = (32 << 20) + 4096  # 8,193 directory blocks: past one pass of the directory's scan
SENTINEL = 0xDEADBEEFDEADBEEF
ALL = M.ALL


def put(client, name, data: bytes):
    bs = client.getBitSet(name)
    bs.setBytes(data)
    return bs


def fills(n: int, seed: int = 1) -> dict:
    """the strings of n bytes the kernels can go wrong on"""
    rng = np.random.default_rng(seed + n)
    out = {"zero": bytes(n), "ff": b"\xff" * n, "half": rng.bytes(n)}
    sparse = np.zeros(n, np.uint8)
    k = max(1, n // 512) if n else 0  # one bit in 4096
    sparse[rng.integers(0, max(n, 1), k)] |= (0x80 >> rng.integers(0, 8, k)).astype(np.uint8)
    out["sparse"] = sparse.tobytes()
    if n:
        out["first"] = b"\x80" + bytes(n - 1)
        out["last"] = bytes(n - 1) + b"\x01"
        third = np.frombuffer(rng.bytes(n), np.uint8).copy()
        third[(np.arange(n) // BLOCK) % 3 != 1] = 0  # ones only in every third block
        out["third"] = third.tobytes()
    return out


def raw_members(client, name, nargs=0, start=0, end=0, unit=M.BYTE, skip=0, cap=ALL, room=0):
    """the C call with `room` entries of output and a sentinel behind them -> (page, written, total)"""
    nm, _keep = L.name_struct(name)
    out = np.full(room + 1, SENTINEL, np.uint64)
    written, total = C.c_uint64(77), C.c_uint64(77)
    rc = L.lib().rbx_bitset_members(client.ctx, nm, nargs, start, end, unit, skip, cap,
                                    out.ctypes.data_as(L.u64p) if cap else None, C.byref(written), C.byref(total))
    assert rc == L.RBX_OK, (rc, L.last_error())
    assert written.value <= room and (out[written.value:] == SENTINEL).all()
    return out[: written.value].copy(), int(written.value), int(total.value)


def dev_members(client, bs, cap, room, stream=None, **kw):
    """membersDev into `room` entries with a sentinel behind -> (page, written, total)"""
    import torch

    d_out = torch.full((room + 1,), -2, dtype=torch.int64, device="cuda")
    d_counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bs.membersDev(d_out.data_ptr() if cap else None, cap, d_counts.data_ptr(), stream=stream, **kw)
    torch.cuda.synchronize()
    written, total = (int(x) for x in d_counts.cpu().numpy())
    out = d_out.cpu().numpy()
    assert written <= room and (out[written:] == -2).all()
    return out[:written].astype(np.uint64), written, total


def check_whole(client, name, data, want=None):
    """members() of the whole string, its total against cardinality(), and asBitSet()"""
    bs = client.getBitSet(name)
    want = M.all_members(data) if want is None else want
    got = bs.members()
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    page, written, total = raw_members(client, name, room=want.size)
    assert np.array_equal(page, want) and written == total == want.size == bs.cardinality()
    assert raw_members(client, name, cap=0)[1:] == (0, want.size)  # count only


# ---- one key: lengths and fills ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_fills(client, fresh, n):
    for fill, data in fills(n).items():
        put(client, fresh, data)
        check_whole(client, fresh, data)
        words = client.getBitSet(fresh).asBitSet()
        assert words.dtype == np.uint64 and np.array_equal(words, M.as_words_fast(data)), (n, fill)
    if n == 0:
        assert client.getBitSet(fresh).size() == 0 and client.getBitSet(fresh).isExists()  # an imported empty string


def big_string(fill: str) -> bytes:
    """The fills of the 8,193-block string whose whole member list stays small: a page of 2^28 ones is 2 GiB of output
    and as much of model, so the random half fill and the all-ones fill of this length are checked by pages
    (test_dense_fills_of_8193_blocks_by_pages), and "every third block" keeps its dense blocks at both ends only."""
    a = np.zeros(BIG, np.uint8)
    rng = np.random.default_rng(3)
    if fill == "sparse":  # one bit in 4096
        k = BIG // 512
        a[rng.integers(0, BIG, k)] |= (0x80 >> rng.integers(0, 8, k)).astype(np.uint8)
    elif fill == "first":
        a[0] = 0x80
    elif fill == "last":
        a[-1] = 0x01
    else:  # dense blocks far apart: every third block of the first and of the last 20
        for blk in [b for b in range(BIG // BLOCK) if b % 3 == 1 and (b < 20 or b >= BIG // BLOCK - 20)]:
            a[blk * BLOCK: (blk + 1) * BLOCK] = np.frombuffer(rng.bytes(BLOCK), np.uint8)
    return a.tobytes()


@pytest.mark.parametrize("fill", ["sparse", "first", "last", "third"])
def test_a_string_of_8193_blocks(client, fresh, fill):
    data = big_string(fill)
    put(client, fresh, data)
    want = M.all_members(data)
    check_whole(client, fresh, data, want)
    if fill == "sparse":
        assert np.array_equal(client.getBitSet(fresh).asBitSet(), M.as_words_fast(data))
    # an interval that starts and ends inside far-apart blocks
    lo, hi = 5 * 8 * BLOCK + 77, 8 * BIG - 8 * BLOCK - 13
    got = client.getBitSet(fresh).members(lo, hi, "BIT")
    assert np.array_equal(got, want[(want >= lo) & (want <= hi)])
    assert got.size == client.getBitSet(fresh).bitCount(lo, hi, "BIT")


@pytest.mark.parametrize("fill", ["ff", "half"])
def test_dense_fills_of_8193_blocks_by_pages(client, fresh, fill):
    """the dense store path and the block skipping past one pass of the scan, with a small output"""
    data = b"\xff" * BIG if fill == "ff" else np.random.default_rng(5).bytes(BIG)
    bs = put(client, fresh, data)
    ones_of_byte = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)
    cum = np.cumsum(ones_of_byte[np.frombuffer(data, np.uint8)], dtype=np.int64)  # the ones up to and with each byte
    total = int(cum[-1])
    assert bs.cardinality() == total
    for skip in (0, total // 2 + 17, total - 50_000):
        n = min(100_000, total - skip)
        b0, b1 = int(np.searchsorted(cum, skip + 1)), int(np.searchsorted(cum, skip + n))  # the bytes of the page's ends
        before = int(cum[b0 - 1]) if b0 else 0
        inside = 8 * b0 + np.flatnonzero(M.bits_of(data[b0: b1 + 1]))
        want = inside[skip - before: skip - before + n].astype(np.uint64)
        assert want.size == n
        page, written, tot = raw_members(client, fresh, skip=skip, cap=100_000, room=100_000)
        assert tot == total and written == n and np.array_equal(page, want), skip
        page, written, tot = dev_members(client, bs, 100_000, 100_000, skip=skip)
        assert tot == total and written == n and np.array_equal(page, want), skip
    if fill == "half":
        return
    assert bs.members(skip=total - 3).tolist() == [total - 3, total - 2, total - 1]
    assert bs.members(skip=total).size == 0 and bs.members(skip=total + 5, limit=9).size == 0


# ---- one key: intervals and pages ----------------------------------------------------------------------------
DATA3 = np.random.default_rng(0xFEED).bytes(3 * BLOCK + 5)
INTERVALS = [
    (3, 20, M.BIT), (35, 35, M.BIT), (120, 140, M.BIT), (127, 128, M.BIT), (8 * BLOCK - 8, 8 * BLOCK + 12, M.BIT),
    (8 * BLOCK - 1, 8 * BLOCK, M.BIT), (1, 8 * 3 * BLOCK + 39, M.BIT), (1, 5, M.BYTE), (15, 16, M.BYTE),
    (BLOCK - 6, BLOCK + 4, M.BYTE), (BLOCK, 2 * BLOCK - 1, M.BYTE), (0, -1, M.BYTE), (-100, -1, M.BYTE),
    (-5000, -3, M.BIT), (-1, -1, M.BIT), (-(1 << 62), 1 << 62, M.BIT), (5, 4, M.BYTE), (-1, -2, M.BIT), (-20000, -30000, M.BYTE),
    (1 << 40, 1 << 41, M.BIT), (3 * BLOCK + 4, 3 * BLOCK + 9, M.BYTE),
]


def test_intervals(client, fresh):
    bs = put(client, fresh, DATA3)
    for start, end, unit in INTERVALS:
        want = M.all_members(DATA3, 2, start, end, unit)
        got = bs.members(start, end, unit)
        assert np.array_equal(got, want), (start, end, unit)
        assert want.size == bs.bitCount(start, end, unit), (start, end, unit)
        for skip, cap in [(1, 3), (want.size // 2, 70), (want.size, 4)]:
            page, written, total = raw_members(client, fresh, 2, start, end, unit, skip, cap, room=cap)
            assert total == want.size and np.array_equal(page, want[skip: skip + cap]), (start, end, unit, skip, cap)
    # the same intervals over the short strings, whose last vector is partial
    for n in (1, 17, 4097):
        data = fills(n)["half"]
        put(client, fresh, data)
        for start, end, unit in INTERVALS:
            assert np.array_equal(bs.members(start, end, unit), M.all_members(data, 2, start, end, unit)), (n, start, end)


def test_pages_at_every_edge(client, fresh):
    data = fills(8195)["half"]
    bs = put(client, fresh, data)
    want = M.all_members(data)
    total = want.size
    bits = M.bits_of(data)
    at_word, at_vec, at_block = (int(bits[:p].sum()) for p in (32, 128, 8 * BLOCK))
    edges = [0, 1, 5, at_word - 1, at_word, at_vec - 1, at_vec, at_vec + 1, at_block - 1, at_block, at_block + 1,
             total - 1, total, total + 7]
    for skip in edges:
        for end in edges:
            if end < skip:
                continue
            cap = end - skip
            page, written, tot = raw_members(client, fresh, skip=skip, cap=cap, room=cap)
            assert tot == total and np.array_equal(page, want[skip: skip + cap]), (skip, cap)
    # inside an interval too: ranks count from the interval's first one
    lo, hi = 8 * BLOCK - 100, 8 * BLOCK + 4000
    sub = want[(want >= lo) & (want <= hi)]
    for skip, cap in [(0, 10), (49, 3), (sub.size - 2, 10)]:
        page, _, tot = raw_members(client, fresh, 2, lo, hi, M.BIT, skip, cap, room=cap)
        assert tot == sub.size and np.array_equal(page, sub[skip: skip + cap])
    # consecutive pages make the whole list
    pages = [bs.members(skip=s, limit=1000) for s in range(0, total + 1000, 1000)]
    assert np.array_equal(np.concatenate(pages), want) and pages[-1].size == 0
    assert bs.members(limit=0).size == 0


def test_positions_past_32_bits(client, fresh):
    x = [0, 1 << 31, (1 << 32) - 1]
    bs = client.getBitSet(fresh)
    bs.setIndexes(x)  # a 512 MiB string
    assert bs.size() == 1 << 32 and bs.cardinality() == 3
    assert bs.members().tolist() == x
    assert bs.members(1 << 31, -1, "BIT").tolist() == x[1:]
    assert bs.members((1 << 31) + 1, -2, "BIT").size == 0
    assert bs.members(skip=2).tolist() == x[2:]
    nm, _keep = L.name_struct(fresh)  # the words in use, and the first two of them
    words, n = np.full(3, SENTINEL, np.uint64), C.c_uint64()
    assert L.lib().rbx_bitset_as_words(client.ctx, nm, words.ctypes.data_as(L.u64p), 2, C.byref(n)) == L.RBX_OK
    assert n.value == 1 << 26 and words.tolist() == [1, 0, SENTINEL]
    bs.delete()


def test_members_after_set_indexes(client, fresh):
    rng = np.random.default_rng(77)
    x = rng.integers(0, 200_000, 5000)
    bs = client.getBitSet(fresh)
    bs.setIndexes(x)
    assert bs.members().tolist() == sorted(set(int(v) for v in x))
    assert bs.toString() == "{" + ", ".join(str(v) for v in sorted(set(int(v) for v in x))) + "}"
    assert client.getBitSet(fresh + "none").toString() == "{}"


def test_dev_forms_on_another_stream(client, fresh):
    import torch

    st = torch.cuda.Stream()
    data = fills(3 * BLOCK + 5)["half"]
    bs = put(client, fresh, data)
    want = M.all_members(data)
    for kw, w in [({}, want), ({"start": 100, "end": -100, "unit": "BIT"}, M.all_members(data, 2, 100, -100, M.BIT))]:
        for skip, cap in [(0, w.size), (0, w.size + 10), (17, 1000), (w.size - 3, 10), (w.size + 1, 10)]:
            page, written, total = dev_members(client, bs, cap, cap, stream=st.cuda_stream, skip=skip, **kw)
            assert total == w.size and np.array_equal(page, w[skip: skip + cap]), (kw, skip, cap)
        assert dev_members(client, bs, 0, 0, stream=st.cuda_stream, **kw)[1:] == (0, w.size)
    # a missing key and an empty string: the counts are written, nothing else
    assert dev_members(client, client.getBitSet(fresh + "none"), 5, 5, stream=st.cuda_stream)[1:] == (0, 0)
    assert dev_members(client, put(client, fresh + "e", b""), 5, 5, stream=st.cuda_stream)[1:] == (0, 0)
    # the words
    d_words = torch.full((want.size,), -2, dtype=torch.int64, device="cuda")
    d_n = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    model = M.as_words_fast(data)
    for cap in (model.size + 5, model.size, 3, 0):
        d_words.fill_(-2)
        torch.cuda.synchronize()
        bs.asBitSetDev(d_words.data_ptr() if cap else None, cap, d_n.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
        got = d_words.cpu().numpy()
        m = min(cap, model.size)
        assert int(d_n.cpu()[0]) == model.size and np.array_equal(got[:m].astype(np.uint64), model[:m])
        assert (got[m:] == -2).all()
    client.getBitSet(fresh + "none").asBitSetDev(None, 0, d_n.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert int(d_n.cpu()[0]) == 0
    # setBitSet from device words
    w = torch.from_numpy(model.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    tw = client.getBitSet(fresh + "tw")
    tw.setBitSetDev(w.data_ptr(), model.size, stream=st.cuda_stream)
    client.synchronize()
    torch.cuda.synchronize()
    assert tw.toByteArray() == M.bytes_of_words_fast(model)
    tw.setBitSetDev(None, 0, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert tw.toByteArray() == b"\0"


# ---- errors and what a read leaves alone ---------------------------------------------------------------------
def test_errors_and_read_only(client, fresh):
    f = client.getBloomFilter(fresh + "bf")
    assert f.tryInit(1000, 0.01)
    h = client.getHyperLogLog(fresh + "hll")
    h.add(b"x")
    for wrong in (_config_name(fresh + "bf"), fresh + "hll"):
        with pytest.raises(RedisException):
            client.getBitSet(wrong).members()
        with pytest.raises(RedisException):
            client.getBitSet(wrong).asBitSet()
        nm, _keep = L.name_struct(wrong)
        w, t = C.c_uint64(), C.c_uint64()
        assert L.lib().rbx_bitset_members(client.ctx, nm, 0, 0, 0, 0, 0, 0, None, C.byref(w), C.byref(t)) == L.RBX_E_WRONGTYPE
    data = fills(4097)["half"]
    bs = put(client, fresh, data)
    nm, _keep = L.name_struct(fresh)
    w, t = C.c_uint64(), C.c_uint64()
    out = np.zeros(8, np.uint64)
    for nargs, unit in [(1, 0), (3, 0), (-1, 0), (0, 2), (2, -1)]:
        assert L.lib().rbx_bitset_members(client.ctx, nm, nargs, 0, -1, unit, 0, 8, out.ctypes.data_as(L.u64p), C.byref(w),
                                          C.byref(t)) == L.RBX_E_ILLEGAL_ARGUMENT, (nargs, unit)
    assert L.lib().rbx_bitset_members(client.ctx, nm, 0, 0, 0, 0, 0, 8, None, C.byref(w),
                                      C.byref(t)) == L.RBX_E_ILLEGAL_ARGUMENT  # NULL out with cap > 0
    with pytest.raises(IllegalArgumentException):
        bs.members(1, None)
    with pytest.raises(IllegalArgumentException):
        bs.members(0, -1, "WORD")
    # nothing is created, grown or touched
    assert bs.expire(3_600_000)
    when = bs.getExpireTime()
    none = client.getBitSet(fresh + "none")
    for b in (bs, none):
        b.members(), b.members(3, 900, "BIT", skip=2, limit=5), b.asBitSet(), b.toString()
    assert not none.isExists()
    assert bs.toByteArray() == data and bs.size() == 8 * len(data) and bs.getExpireTime() == when
    f.delete(), h.delete()


# ---- set(BitSet) against rbx_bitset_import_n of the model's bytes on a twin key -------------------------------
def words_cases():
    rng = np.random.default_rng(0x5E7)
    cases = [[], [0, 0], [1], [1 << 6], [1 << 7], [1 << 8], [1 << 63], [0, 1], [1 << 63, 1 << 63], [5, 0, 0, 0]]
    cases += [rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + 1 for n in (2, 3, 511, 512, 513, 1537)]
    sparse = np.zeros(2000, np.uint64)
    sparse[[3, 700, 1999]] = [1 << 17, 1, 1 << 40]
    return cases + [sparse, np.concatenate([sparse, np.zeros(100, np.uint64)])]


def test_set_bitset_equals_import_of_the_models_bytes(client, fresh):
    a, b = client.getBitSet(fresh + "a"), client.getBitSet(fresh + "b")
    for words in words_cases():
        want = M.bytes_of_words_fast(words)
        for pre in (None, b"\xff" * 5000):  # a missing key, and a longer string before
            for bs in (a, b):
                bs.delete()
                if pre is not None:
                    bs.setBytes(pre)
                    assert bs.expire(3_600_000)
            a.setBitSet(words)
            b.setBytes(want)
            assert a.toByteArray() == b.toByteArray() == want
            assert a.size() == b.size() == 8 * len(want)
            assert a.remainTimeToLive() == b.remainTimeToLive()
            assert np.array_equal(a.asBitSet(), M.as_words_fast(want))
            # no stale tail and zero padding: a later bit past the old end shows zeros between
            for bs in (a, b):
                bs.set(8 * 5000 + 77)
            tail = bytearray(max(5010, len(want)))
            tail[: len(want)] = want
            tail[5009] |= 0x80 >> 5
            assert a.toByteArray() == b.toByteArray() == bytes(tail)
    a.setBitSet([])
    assert a.toByteArray() == b"\0" and a.size() == 8  # the empty BitSet stores one zero byte


def test_set_bitset_on_other_types_and_bloom_keys(client, fresh):
    """whatever import_n does to a key of another type, a Bloom filter's bits and its config floor, set_words does"""
    words = np.array([0xF0F0, 1 << 63, 7], np.uint64)
    want = M.bytes_of_words_fast(words)
    results = []
    for how in ("words", "bytes"):
        name = fresh + how
        f = client.getBloomFilter(name)
        assert f.tryInit(1000, 0.01)
        f.add([b"k%d" % i for i in range(50)])
        handle = BloomHandle(client, name)
        bs = client.getBitSet(name)
        hl = client.getBitSet(name + "hll")
        client.getHyperLogLog(name + "hll").add(b"x")
        outcome = []
        for target in (bs, hl):
            try:
                target.setBitSet(words) if how == "words" else target.setBytes(want)
                outcome.append((target.toByteArray(), target.size()))
            except RedisException as e:
                outcome.append(type(e).__name__)
        bs.set(f.getSize() - 1)  # inside the config's |size|: the allocation covers it either way
        outcome.append(bs.toByteArray())
        outcome.append(bool(f.contains(b"k1")))
        handle.close()
        results.append(outcome)
    assert results[0] == results[1]
    assert results[0][0] == (want, 8 * len(want))


def test_set_bitset_refuses_a_bit_java_cannot_count(client, fresh):
    import torch

    bs = put(client, fresh, b"\x42")
    w = torch.zeros(1 << 25, dtype=torch.int64, device="cuda")
    w[-1] = -(1 << 63)  # bit 2^31 - 1
    torch.cuda.synchronize()
    with pytest.raises(IllegalArgumentException):
        bs.setBitSetDev(w.data_ptr(), 1 << 25)
    assert bs.toByteArray() == b"\x42"
    w[-1] = 1 << 62  # bit 2^31 - 2: the last one length() can report
    torch.cuda.synchronize()
    bs.setBitSetDev(w.data_ptr(), 1 << 25)
    assert bs.size() == 8 << 28 and bs.cardinality() == 1 and bs.members().tolist() == [(1 << 31) - 2]
    with pytest.raises(IllegalArgumentException):
        bs.setBitSet(np.zeros((1 << 25) + 1, np.uint64) + 1)
    bs.delete()


# ---- many keys: rbx_bitset_members_stream ----------------------------------------------------------------------
from redisson_amd import RBatch, bitset_members_stream_call, bitset_members_stream_dev  # noqa: E402
import contextlib  # noqa: E402

KNOBS = {"members_lanes": 16, "members_short_max": 4096, "members_tile": 65536, "members_chunk": 1 << 25}


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k in knobs:
            L.lib().rbx_tune(k.encode(), KNOBS[k])


def last_call():
    out = (C.c_uint32 * 4)()
    assert L.lib().rbx_bench_members_last(out) == 0
    return dict(zip(("short", "long", "tiles", "waits"), out))


def raw_stream(client, names, cmd_key, rows, cap, room):
    """the C call with `room` entries of output and a sentinel behind them -> (rc, off, out[:room + 1], status, total)"""
    from redisson_amd.client import _members_cmds_array

    key = np.ascontiguousarray(cmd_key, np.uint32)
    arr = _members_cmds_array(list(rows))
    names_arr, _keep = L.names_array(names)
    n = key.size
    off, status, total = np.full(n + 2, SENTINEL, np.uint64), np.full(n + 1, 0x5A, np.uint8), C.c_uint64(77)
    out = np.full(room + 1, SENTINEL, np.uint64)
    rc = L.lib().rbx_bitset_members_stream(client.ctx, names_arr, len(names), key.ctypes.data_as(L.u32p), arr, n, cap,
                                           off.ctypes.data_as(L.u64p), out.ctypes.data_as(L.u64p) if cap else None,
                                           status.ctypes.data_as(L.u8p), C.byref(total))
    assert off[n + 1] == SENTINEL and status[n] == 0x5A
    return rc, off[: n + 1], out, status[:n], int(total.value)


def check_stream(client, want, names, cmd_key, rows, caps=(None,)):
    """the host call against want = M.stream(...) of the same input (computed once by the test), all outputs in full,
    for each cap (None: exactly the total)"""
    w_off, w_out, w_status, w_failed = want
    total = int(w_off[-1])
    for cap in caps:
        cap = total if cap is None else cap
        rc, off, out, status, tot = raw_stream(client, names, cmd_key, rows, cap, cap)
        assert rc == (L.RBX_E_WRONGTYPE if w_failed else L.RBX_OK), (rc, L.last_error())
        assert tot == total and np.array_equal(off, w_off) and np.array_equal(status, w_status)
        m = min(total, cap)
        assert np.array_equal(out[:m], w_out[:m]) and (out[m:] == SENTINEL).all(), cap  # untouched past min(total, cap)
    return total


def small_world(client, fresh, nstr=5000, seed=11):
    """nstr strings of 0 .. 64 bytes, missing names, a duplicate name, an HLL key and a {name}:config key"""
    rng = np.random.default_rng(seed)
    strings, names = {}, []
    for j in range(nstr):
        name = "%s:%d" % (fresh, j)
        names.append(name)
        if j % 17 == 3:
            strings[name] = None  # missing
            continue
        n = int(rng.integers(0, 65))
        data = rng.bytes(n) if j % 5 else bytes(np.frombuffer(rng.bytes(n), np.uint8) & np.frombuffer(rng.bytes(n), np.uint8))
        put(client, name, data)
        strings[name] = data
    names.append(names[7])  # two names with equal bytes are one key
    f = client.getBloomFilter(fresh + "bf")
    assert f.tryInit(100, 0.01)
    client.getHyperLogLog(fresh + "hll").add(b"x")
    for wrong in (_config_name(fresh + "bf"), fresh + "hll"):
        names.append(wrong)
        strings[wrong] = M.WRONG
    return strings, names, rng


def random_rows(rng, n, nkeys, maxlen=64):
    key = rng.integers(0, nkeys, n)
    rows = []
    for _ in range(n):
        nargs = int(rng.integers(0, 2)) * 2
        unit = int(rng.integers(0, 2))
        t = maxlen * (8 if unit else 1)
        start, end = (int(x) for x in rng.integers(-t - 3, t + 4, 2))
        # (picked by index: an array of these values would be float64, and 2^64 - 1 would not survive it)
        skip = (0, 0, 0, 1, 7, 63, 200, 1 << 40, ALL)[int(rng.integers(0, 9))]
        limit = (None, None, None, 0, 1, 3, 64, ALL - 1, ALL)[int(rng.integers(0, 9))]
        rows.append((nargs, start, end, unit, skip, limit))
    return key, rows


def cleanup(client, fresh, names):
    client.getBloomFilter(fresh + "bf").delete()
    client.getHyperLogLog(fresh + "hll").delete()
    for nm in names[:-3]:
        client.getBitSet(nm).delete()


def test_stream_over_5000_small_strings(client, fresh):
    strings, names, rng = small_world(client, fresh)
    key, rows = random_rows(rng, 12_000, len(names))
    key[:2] = [len(names) - 1, len(names) - 2]  # the wrong-type keys are used
    key[2:4] = [7, len(names) - 3]  # and both names of one key
    want = M.stream(strings, names, key, rows)
    total = check_stream(client, want, names, key, rows, caps=(None, 0, 1))
    check_stream(client, want, names, key, rows, caps=(total - 1, total + 9, total // 2))
    assert last_call()["long"] == 0
    # the keys are as they were, and nothing was created for the missing names
    for nm in names[:60]:
        bs = client.getBitSet(nm)
        assert bs.isExists() == (strings[nm] is not None) and bs.toByteArray() == (strings[nm] or b"")
    # every lane-group width and several chunks, on the same input
    for lanes in (4, 8, 32, 64):
        with tuned(members_lanes=lanes):
            check_stream(client, want, names, key, rows)
    with tuned(members_chunk=700):
        check_stream(client, want, names, key, rows, caps=(None, total // 3))
        assert last_call()["waits"] == -(-12_000 // 700)
    # n = 0 sends nothing
    rc, off, out, status, tot = raw_stream(client, names, [], [], 5, 5)
    assert rc == L.RBX_OK and off.tolist() == [0] and tot == 0 and (out == SENTINEL).all()
    # the caller's own errors
    for bad_key, bad_row in [([len(names)], [(0, 0, 0, 0, 0, None)]), ([0], [(1, 0, 0, 0, 0, None)]),
                             ([0], [(3, 0, 0, 0, 0, None)]), ([0], [(2, 0, 0, 2, 0, None)])]:
        assert raw_stream(client, names, bad_key, bad_row, 5, 5)[0] == L.RBX_E_ILLEGAL_ARGUMENT
    cleanup(client, fresh, names)


def test_stream_with_long_strings_on_the_tiles(client, fresh):
    strings, names, rng = small_world(client, fresh, nstr=300, seed=12)
    big = []
    for j, n in enumerate(((1 << 20) + 5, (1 << 20) + 5, (1 << 20) + 5, 8195)):
        a = np.frombuffer(rng.bytes(n), np.uint8) & np.frombuffer(rng.bytes(n), np.uint8)
        if j == 1:
            a = a & np.frombuffer(rng.bytes(n), np.uint8) & np.frombuffer(rng.bytes(n), np.uint8)  # sparser
        if j == 2:
            a = np.where((np.arange(n) // BLOCK) % 3 == 1, 0xFF, 0).astype(np.uint8)  # full and empty blocks
        name = "%s:big%d" % (fresh, j)
        put(client, name, a.tobytes())
        strings[name] = a.tobytes()
        names.insert(j, name)
        big.append(name)
    key, rows = random_rows(rng, 2000, len(names))
    nb = 8 * ((1 << 20) + 5)
    extra = [(0, (0, 0, 0, 0, 0, None)), (1, (0, 0, 0, 0, 0, None)), (2, (0, 0, 0, 0, 5, 100_000)),
             (0, (2, 777, nb - 999, 1, 123_456, 70_000)), (1, (2, 5000, -5000, 0, 0, 1000)), (2, (2, -70_000, -1, 0, 99, None)),
             (0, (0, 0, 0, 0, 1 << 40, None)), (1, (0, 0, 0, 0, 3, 0)), (2, (0, 0, 0, 0, nb // 3 - 50, 100)),
             (3, (0, 0, 0, 0, 0, None)), (3, (2, 100, -100, 1, 77, 30_000)), (0, (2, 4096, 4096 + 4095, 0, 10, 20))]
    for pos, (k, row) in zip(range(5, 2000, 150), extra):
        key[pos], rows[pos] = k, row
    want = M.stream(strings, names, key, rows)
    total = check_stream(client, want, names, key, rows, caps=(None, 1000))
    assert last_call()["long"] >= 9 and last_call()["tiles"] > 100
    # each side of the short / long threshold, small tiles, other widths and several chunks, on the same input
    with tuned(members_short_max=64, members_tile=4096):
        check_stream(client, want, names, key, rows)
        assert last_call()["long"] > 12
    with tuned(members_short_max=16384, members_lanes=64):
        check_stream(client, want, names, key, rows)
    with tuned(members_chunk=333, members_lanes=4, members_tile=1 << 20):
        check_stream(client, want, names, key, rows, caps=(total // 2,))
    for nm in big:
        assert client.getBitSet(nm).toByteArray() == strings[nm]
        client.getBitSet(nm).delete()
    cleanup(client, fresh, [n for n in names if n not in big])


def test_stream_dev_on_another_stream(client, fresh):
    import torch

    from redisson_amd.client import _members_cmds_array

    strings, names, rng = small_world(client, fresh, nstr=200, seed=13)
    name = fresh + ":big"
    data = rng.bytes(70_001)
    put(client, name, data)
    strings[name] = data
    names.insert(0, name)
    key, rows = random_rows(rng, 1500, len(names))
    key[10], rows[10] = 0, (0, 0, 0, 0, 0, None)
    key[11], rows[11] = 0, (2, 9, -9, 0, 1000, 5000)
    w_off, w_out, w_status, w_failed = M.stream(strings, names, key, rows)
    arr = _members_cmds_array(rows)
    d_cmds = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    d_key = torch.from_numpy(np.asarray(key, np.int32)).cuda()
    st = torch.cuda.Stream()
    for cap in (int(w_off[-1]), 100, 0):
        d_off = torch.full((len(rows) + 2,), -2, dtype=torch.int64, device="cuda")
        d_out = torch.full((cap + 1,), -2, dtype=torch.int64, device="cuda")
        d_status = torch.full((len(rows) + 1,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(RedisException):  # the wrong-type commands failed alone; the others ran
            bitset_members_stream_dev(client, names, d_key.data_ptr(), d_cmds.data_ptr(), len(rows), cap, d_off.data_ptr(),
                                      d_out.data_ptr() if cap else None, d_status.data_ptr(), stream=st.cuda_stream)
        assert w_failed
        torch.cuda.synchronize()
        off, out, status = d_off.cpu().numpy(), d_out.cpu().numpy(), d_status.cpu().numpy()
        assert np.array_equal(off[:-1].astype(np.uint64), w_off) and off[-1] == -2
        assert np.array_equal(status[:-1], w_status) and status[-1] == 0x5A
        assert np.array_equal(out[:cap].astype(np.uint64), w_out[:cap]) and out[cap] == -2
    client.getBitSet(name).delete()
    cleanup(client, fresh, names[1:])


def test_batch_members_async(client, fresh):
    calls = []

    def counting(names, keys, rows):
        calls.append(len(rows))
        return bitset_members_stream_call(client, names, keys, rows)

    batch = RBatch(client, members_stream_call=counting)
    a, b = batch.getBitSet(fresh + "a"), batch.getBitSet(fresh + "b")
    futures = [a.setAsync(5), a.membersAsync(), a.setAsync(900), b.setAsync(3), a.membersAsync(), b.membersAsync(),
               a.membersAsync(0, 0, "BYTE"), a.membersAsync(skip=1, limit=5), batch.getBitSet(fresh + "none").membersAsync()]
    run = [(a if j % 2 else b).membersAsync(skip=j % 3) for j in range(1000)]
    batch.execute()
    got = [f.get() for f in futures[:1] + futures[2:4]] + [f.get().tolist() for f in futures[1:2] + futures[4:]]
    assert got == [False, False, False, [5], [5, 900], [3], [5], [900], []]  # each sees the writes before it
    assert calls == [1, 1005]  # the run of 1,000 and the five before it: one stream call
    assert [f.get().tolist() for f in run[:4]] == [[3], [900], [], [5, 900]]
    # through createBatch(), and a key of another type fails alone
    client.getHyperLogLog(fresh + "hll").add(b"x")
    batch = client.createBatch()
    f1, f2 = batch.getBitSet(fresh + "hll").membersAsync(), batch.getBitSet(fresh + "a").membersAsync()
    with pytest.raises(RedisException):
        batch.execute()
    assert f2.get().tolist() == [5, 900]
    with pytest.raises(RedisException):
        f1.get()
    for nm in ("a", "b"):
        client.getBitSet(fresh + nm).delete()
    client.getHyperLogLog(fresh + "hll").delete()


# ---- the two read streams against each other, through the tiers they share ------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("lanes", [4, 64])
def test_range_stream_counts_equal_members_stream_yields(client, fresh, lanes, form):
    """Every BITCOUNT reply of the range stream is the members stream's yield off[i + 1] - off[i] (skip 0, no limit) of
    the same interval, and both are the models'; both streams list the same commands with the same tiles."""
    import bitstring_model as BM
    import rangestream_model as RM
    import test_rangestream_gpu as RS
    import torch

    from redisson_amd.client import _members_cmds_array

    SHORT_MAX, TILE, CHUNK = 64, 4096, 2
    rng = np.random.default_rng(29)
    missing, small, large = fresh + "none", fresh + "s", fresh + "l"
    strings = {missing: None, small: rng.bytes(100), large: rng.bytes(3 * 4096 + 17)}
    for nm, data in strings.items():
        RS.put(client, nm, data)
    names = [missing, small, large]
    # (key, nargs, start, end, unit, the interval's bits [lo, hi] or None): a short command between the two long ones
    cmds = [(2, 0, 0, 0, M.BYTE, (0, 8 * (3 * 4096 + 17) - 1)),  # the whole long string
            (1, 2, 3, 40, M.BYTE, (24, 8 * 41 - 1)),
            (2, 2, 5, 8 * (2 * 4096) + 3, M.BIT, (5, 8 * (2 * 4096) + 3)),
            (0, 0, 0, 0, M.BYTE, None),  # the missing key
            (1, 2, 50, 10, M.BYTE, None)]  # an empty interval
    key = [c[0] for c in cmds]
    m_rows = [(nargs, start, end, unit, 0, None) for _k, nargs, start, end, unit, _iv in cmds]
    r_rows = [(RM.COUNT, 0, nargs, start, end, unit) for _k, nargs, start, end, unit, _iv in cmds]
    # what the tiers are to do, from the intervals and the knobs alone
    is_long = [iv is not None and (iv[1] >> 3) - (iv[0] >> 3) + 1 > SHORT_MAX for *_c, iv in cmds]
    tiles = sum(((iv[1] >> 7) - (iv[0] >> 7)) // (TILE // 16) + 1 for *_c, iv in (c for c, lg in zip(cmds, is_long) if lg))
    chunks = [is_long[i:i + CHUNK] for i in range(0, len(cmds), CHUNK)]
    assert is_long == [True, False, True, False, False] and tiles == 4 + 3 and len(chunks) == 3
    assert sum(any(ch) for ch in chunks) == 2  # the two long commands fall in different chunks

    w_off, _w_out, _w_status, w_failed = M.stream(strings, names, key, m_rows)
    ks = RS.model_of({k: v for k, v in strings.items() if v})
    rc_model, w_counts, _st, _kinds = RM.apply_stream(ks, names, key, r_rows)
    assert rc_model == RM.OK and not w_failed
    assert w_counts == np.diff(w_off.astype(np.int64)).tolist()  # the two models agree

    with RS.tuned(short_max=SHORT_MAX, tile=TILE, rangestream_chunk=CHUNK, rangestream_lanes=lanes):
        rc, counts, status = RS.RUNNERS[form](client, names, key, r_rows)
        r_last = RS.last()
    assert rc == L.RBX_OK and status == [0] * len(cmds), L.last_error()
    with tuned(members_short_max=SHORT_MAX, members_tile=TILE, members_chunk=CHUNK, members_lanes=lanes):
        if form == "host":
            rc, off, _out, m_status, total = raw_stream(client, names, key, m_rows, int(w_off[-1]), int(w_off[-1]))
            assert rc == L.RBX_OK and total == int(w_off[-1]) and not m_status.any()
        else:
            d_cmds = torch.frombuffer(bytearray(bytes(_members_cmds_array(m_rows))), dtype=torch.uint8).cuda()
            d_key = torch.from_numpy(np.asarray(key, np.int32)).cuda()
            d_off = torch.full((len(cmds) + 1,), -2, dtype=torch.int64, device="cuda")
            d_out = torch.full((int(w_off[-1]) + 1,), -2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            bitset_members_stream_dev(client, names, d_key.data_ptr(), d_cmds.data_ptr(), len(cmds), int(w_off[-1]),
                                      d_off.data_ptr(), d_out.data_ptr(), None)
            client.synchronize()
            off = d_off.cpu().numpy().astype(np.uint64)
        m_last = last_call()
    print("counts", counts, "yields", np.diff(off.astype(np.int64)).tolist(), "model", w_counts, "range last", r_last,
          "members last", m_last)
    assert np.array_equal(off, w_off)
    assert counts == np.diff(off.astype(np.int64)).tolist() == w_counts
    n_long = sum(is_long)
    assert (m_last["short"], m_last["long"], m_last["tiles"]) == (len(cmds) - n_long, n_long, tiles) == tuple(r_last[:3])
    assert m_last["waits"] == len(chunks)  # one wait per chunk (the host form's second run publishes the same)
    # the range stream's host form waits once more in each chunk that listed a command, for the replies behind the tiles
    assert r_last[3] == len(chunks) + (sum(any(ch) for ch in chunks) if form == "host" else 0)
    for nm in (small, large):
        client.getBitSet(nm).delete()
