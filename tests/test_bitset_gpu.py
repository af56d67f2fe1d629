"""RBitSet on the GPU (rbx_bitset_*, bitset_kernels.hip): every reply, length and exported byte is
compared exactly with the numpy model of Redis strings in bitset_model.py.
T/ = /root/reference/redisson/src/test/java/org/redisson/"""
import ctypes as C
import itertools

import numpy as np
import pytest

from bitset_model import MAX_OFFSET, RedisString, bitop, bits_of
from redisson_amd import BloomHandle, RedisException, device_keys
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

OPS = {"and": L.RBX_BITOP_AND, "or": L.RBX_BITOP_OR, "xor": L.RBX_BITOP_XOR, "not": L.RBX_BITOP_NOT}
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4099]  # 0 = a missing key


def raw_op(client, op, dest, srcs):
    """BITOP op dest srcs.. through the C ABI -> (return code, reply)"""
    d, _k1 = L.name_struct(dest)
    arr, _k2 = L.names_array(srcs)
    out = C.c_uint64(12345)
    rc = L.lib().rbx_bitset_op(client.ctx, OPS[op], d, arr, len(srcs), C.byref(out))
    return rc, int(out.value)


def put(client, name, data: bytes):
    """SET name data; empty data = leave the key missing"""
    if data:
        client.getBitSet(name).setBytes(data)


def capacity_of(nbytes: int) -> int:
    """bytes the engine allocates for a string of nbytes (a multiple of 256, at least 256)"""
    return max(256, (nbytes + 255) & ~255)


def check_string(client, name, want: bytes):
    """GET name == want, and the allocation behind it is zero: a SETBIT 0 of the allocation's last
    bit stretches the string over the padding in place, which must then read as zeros."""
    b = client.getBitSet(name)
    assert b.toByteArray() == want
    assert b.size() == 8 * len(want)
    cap = capacity_of(len(want))
    if 0 < len(want) < cap:  # (a string that fills its allocation has no padding)
        assert b.set(8 * cap - 1, False) is False
        assert b.toByteArray() == want + bytes(cap - len(want))


def drop(client, *names):
    for n in names:
        client.getBitSet(n).delete()


# ---- 1. reference vectors (T/RedissonBitSetTest.java, as data) ---------------------------------
def test_reference_length(client, fresh):  # testLength :68-94
    bs = client.getBitSet(fresh)
    bs.setRange(0, 5)
    bs.clearRange(0, 1)
    assert bs.length() == 5
    bs.clear()
    bs.set(28)
    bs.set(31)
    assert bs.length() == 32
    bs.clear()
    bs.set(3)
    bs.set(7)
    assert bs.length() == 8
    bs.clear()
    bs.set(3)
    bs.set(120)
    bs.set(121)
    assert bs.length() == 122
    bs.clear()
    bs.set(0)
    assert bs.length() == 1
    # the script's own corners: a zero last byte answers 1 (bit 0 set) or fails; so does a missing key
    bs.set(15, False)
    assert bs.toByteArray() == b"\x80\x00" and bs.length() == 1
    bs.set(0, False)
    with pytest.raises(RedisException, match="bit offset"):
        bs.length()
    bs.clear()
    with pytest.raises(RedisException, match="bit offset"):
        bs.length()


def test_reference_clear_not_set(client, fresh):
    bs = client.getBitSet(fresh)
    bs.setRange(0, 8)  # testClear :96-102
    bs.clearRange(0, 3)
    assert bits_of(bs.toByteArray()) == [3, 4, 5, 6, 7]
    bs.clear()
    assert not bs.isExists()
    bs.set(3)  # testNot :104-111
    bs.set(5)
    bs.not_()
    assert bits_of(bs.toByteArray()) == [0, 1, 2, 4, 6, 7]
    bs.clear()
    assert bs.set(3) is False  # testSet :113-137
    assert bs.set(5) is False
    assert bs.set(5) is True
    assert bits_of(bs.toByteArray()) == [3, 5]
    bs.setBytes(bytes([0x40, 0x20]))  # toByteArrayReverse of java.util.BitSet {1, 10}: 11 / 8 + 1 bytes
    assert bits_of(client.getBitSet(fresh).toByteArray()) == [1, 10]
    bs2 = client.getBitSet(fresh + "2")
    bs2.setIndexes([1, 3, 5, 7], True)
    assert bits_of(client.getBitSet(fresh + "2").toByteArray()) == [1, 3, 5, 7]
    bs2.setIndexes([3, 5], False)
    assert bits_of(client.getBitSet(fresh + "2").toByteArray()) == [1, 7]
    drop(client, fresh, fresh + "2")


def test_reference_setget_range_and(client, fresh):
    bs = client.getBitSet(fresh)  # testSetGet :139-152
    assert bs.cardinality() == 0 and bs.size() == 0
    assert bs.set(10, True) is False
    assert bs.set(31, True) is False
    assert bs.get(0) is False and bs.get(31) is True and bs.get(10) is True
    assert bs.cardinality() == 2 and bs.size() == 32
    bs.clear()
    bs.setRange(3, 10)  # testSetRange :154-160
    assert bs.cardinality() == 7 and bs.size() == 16
    bs.clear()
    bs1, bs2 = client.getBitSet(fresh + "1"), client.getBitSet(fresh + "2")  # testAnd :178-197
    bs1.setRange(3, 5)
    assert bs1.cardinality() == 2 and bs1.size() == 8
    bs2.set(4)
    bs2.set(10)
    bs1.and_(bs2.getName())
    assert bs1.get(3) is False and bs1.get(4) is True and bs1.get(5) is False and bs2.get(10) is True
    assert bs1.cardinality() == 1 and bs1.size() == 16
    drop(client, fresh + "1", fresh + "2")


def test_reference_index_range_and_the_offset_limit(client, fresh):
    """testIndexRange :59-66 (one 512 MiB key), then the batch rule at the limit on the same key:
    set(from, to) with to > 2^32 applies [from, 2^32) and reports the error of the rest."""
    bs = client.getBitSet(fresh)
    top = 2147483647 * 2
    try:
        assert bs.get(top) is False
        assert not bs.isExists()
        assert bs.set(top) is False
        assert bs.get(top) is True
        assert bs.size() == MAX_OFFSET and bs.cardinality() == 1 and bs.length() == top + 1
        with pytest.raises(RedisException, match="bit offset"):
            bs.setRange(MAX_OFFSET - 70, MAX_OFFSET + 5)
        assert bs.cardinality() == 70 and bs.get(MAX_OFFSET - 1) and bs.get(MAX_OFFSET - 70)
        assert not bs.get(MAX_OFFSET - 71) and bs.length() == MAX_OFFSET
        for call in (lambda: bs.get(MAX_OFFSET), lambda: bs.set(MAX_OFFSET), lambda: bs.set(MAX_OFFSET, False),
                     lambda: bs.setRange(MAX_OFFSET, MAX_OFFSET + 9)):
            with pytest.raises(RedisException, match="bit offset"):
                call()
        assert bs.cardinality() == 70
    finally:
        bs.delete()


# ---- 2. BITOP: lengths and source counts ------------------------------------------------------
@pytest.mark.parametrize("op", ["and", "or", "xor"])
def test_bitop_lengths_and_source_counts(client, fresh, op):
    rng = np.random.default_rng(0xB170 + OPS[op])
    pick = itertools.cycle(rng.permutation(LENGTHS).tolist())  # 96 draws: every length is used, eight times
    for nsrc in (1, 2, 3, 9, 17):
        for rep in range(3):
            srcs = [rng.bytes(next(pick)) for _ in range(nsrc)]
            names = [f"{fresh}:s{i}" for i in range(nsrc)]
            for n, s in zip(names, srcs):
                put(client, n, s)
            want = bitop(op, srcs)
            rc, reply = raw_op(client, op, fresh + ":d", names)
            assert rc == 0 and reply == len(want), (nsrc, rep, [len(s) for s in srcs])
            check_string(client, fresh + ":d", want)
            assert client.getBitSet(fresh + ":d").isExists() == bool(want)
            for n, s in zip(names, srcs):  # the sources are untouched
                assert client.getBitSet(n).toByteArray() == s
            drop(client, fresh + ":d", *names)


def test_bitop_not_lengths(client, fresh):
    rng = np.random.default_rng(0xB173)
    for ln in LENGTHS:
        s = rng.bytes(ln)
        put(client, fresh + ":s", s)
        rc, reply = raw_op(client, "not", fresh + ":d", [fresh + ":s"])
        assert rc == 0 and reply == ln
        check_string(client, fresh + ":d", bitop("not", [s]))  # the padding stays zero, not ones
        # in place, as RBitSet.not() runs it
        bs = client.getBitSet(fresh + ":s")
        bs.not_()
        check_string(client, fresh + ":s", bitop("not", [s]))
        assert bs.isExists() == bool(ln)
        drop(client, fresh + ":d", fresh + ":s")
    rc, _ = raw_op(client, "not", fresh + ":d", [fresh + ":a", fresh + ":b"])
    assert rc == L.RBX_E_REDIS and "single source" in L.last_error()


# ---- 3. BITOP: where the destination stands ---------------------------------------------------
@pytest.mark.parametrize("op", ["and", "or", "xor"])
def test_bitop_destination_positions(client, fresh, op):
    rng = np.random.default_rng(0xD357 + OPS[op])
    for nsrc, pos, dest_len in ((3, None, 17), (3, 0, 257), (3, 0, 4), (3, 2, 255), (3, 2, 4099), (17, 10, 16),
                                (17, 10, 4099), (17, 10, 0), (2, 0, 0)):
        lens = [int(x) for x in rng.choice(LENGTHS, size=nsrc)]
        lens[0] = max(lens[0], 300)  # a result longer than most destinations: dest also has to grow
        if pos is not None:
            lens[pos] = dest_len
        srcs = [rng.bytes(n) for n in lens]
        names = [f"{fresh}:s{i}" for i in range(nsrc)]
        dest = fresh + ":d" if pos is None else names[pos]
        for n, s in zip(names, srcs):
            put(client, n, s)
        if pos is None:
            put(client, dest, rng.bytes(dest_len))  # an unrelated previous value
        want = bitop(op, srcs)
        rc, reply = raw_op(client, op, dest, names)
        assert rc == 0 and reply == len(want), (nsrc, pos, lens)
        check_string(client, dest, want)
        for i, (n, s) in enumerate(zip(names, srcs)):
            if i != pos:
                assert client.getBitSet(n).toByteArray() == s
        drop(client, fresh + ":d", *names)


def test_bitop_shorter_result_clears_the_old_destination(client, fresh):
    d = client.getBitSet(fresh + ":d")
    d.setBytes(b"\xff" * 4099)
    put(client, fresh + ":a", b"\x0f\xf0\xaa")
    put(client, fresh + ":b", b"\xff\x3c")
    rc, reply = raw_op(client, "and", fresh + ":d", [fresh + ":a", fresh + ":b"])
    assert rc == 0 and reply == 3
    assert d.toByteArray() == b"\x0f\x30\x00" and d.size() == 24
    assert d.set(32_000) is False
    assert d.toByteArray() == b"\x0f\x30\x00" + bytes(3997) + b"\x80"
    assert d.cardinality() == 7
    drop(client, fresh + ":d", fresh + ":a", fresh + ":b")


def test_bitop_all_sources_missing_deletes_the_destination(client, fresh):
    d = client.getBitSet(fresh + ":d")
    for op in ("and", "or", "xor"):
        d.setBytes(b"\x01\x02\x03")
        assert d.isExists()
        rc, reply = raw_op(client, op, fresh + ":d", [fresh + ":m1", fresh + ":m2", fresh + ":m3"])
        assert rc == 0 and reply == 0
        assert not d.isExists() and d.toByteArray() == b"" and d.size() == 0
    # through the object API the destination is its own first source: an op over missing keys keeps it
    d.setBytes(b"\x01\x02\x03")
    d.or_(fresh + ":m1")
    assert d.toByteArray() == b"\x01\x02\x03"
    d.and_(fresh + ":m1")
    assert d.toByteArray() == b"\x00\x00\x00" and d.isExists()
    d.delete()


# ---- 4. BITOP: the grid-stride loop takes a second trip ----------------------------------------
def test_bitop_past_one_grid_sweep(client, fresh):
    """2048 blocks x 256 lanes x 16 bytes = 8 MiB per sweep: three sources of 8 MiB + 5 bytes."""
    n = 2048 * 256 * 16 + 5
    rng = np.random.default_rng(0x6121D)
    srcs = [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(3)]
    names = [f"{fresh}:s{i}" for i in range(3)]
    for nm, s in zip(names, srcs):
        client.getBitSet(nm).setBytes(s.tobytes())
    try:
        for op, fn in (("xor", np.bitwise_xor), ("and", np.bitwise_and), ("or", np.bitwise_or)):
            rc, reply = raw_op(client, op, fresh + ":d", names)
            assert rc == 0 and reply == n
            got = np.frombuffer(client.getBitSet(fresh + ":d").toByteArray(), np.uint8)
            assert np.array_equal(got, fn(fn(srcs[0], srcs[1]), srcs[2])), op
        # in place over itself, and the padding behind the odd tail
        client.getBitSet(names[0]).xor(names[1], names[2])
        check_string(client, names[0], (srcs[0] ^ srcs[1] ^ srcs[2]).tobytes())
    finally:
        drop(client, fresh + ":d", *names)


# ---- 5. ranges ----------------------------------------------------------------------------------
POINTS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256]


@pytest.mark.parametrize("value", [1, 0])
@pytest.mark.parametrize("start", ["empty", "ones"])
def test_set_range_every_pair(client, fresh, start, value):
    bs = client.getBitSet(fresh)
    init = b"\xff" * 64 if start == "ones" else None
    for frm, to in itertools.combinations_with_replacement(POINTS, 2):
        model = RedisString(init)
        if init:
            bs.setBytes(init)
        model.set_range(frm, to, value)
        bs.setRange(frm, to, bool(value))
        assert bs.toByteArray() == model.bytes(), (frm, to)
        assert bs.isExists() == (model.data is not None), (frm, to)  # the empty range creates nothing
        assert bs.cardinality() == model.bitcount()
        if model.data is not None:
            check_string(client, fresh, model.bytes())
        bs.delete()
    # from > to is empty too
    bs.setRange(9, 3, bool(value))
    assert not bs.isExists()


# ---- 6. index batches ---------------------------------------------------------------------------
def test_index_batches(client, fresh):
    rng = np.random.default_rng(0x1DE5)
    bs = client.getBitSet(fresh)
    model = RedisString()
    idx = rng.integers(0, 100_000, size=10_000)
    idx[:500] = idx[500:1000]  # duplicates for certain
    model.set_indexes(idx, 1)
    bs.setIndexes(idx, True)
    assert bs.toByteArray() == model.bytes() and bs.cardinality() == model.bitcount()
    sub = rng.choice(idx, size=3000, replace=False)
    model.set_indexes(sub, 0)
    bs.setIndexes(sub, False)
    assert bs.toByteArray() == model.bytes() and bs.cardinality() == model.bitcount()
    # reads: inside the string, past its end, past its allocation
    q = np.concatenate([rng.integers(0, 100_000, size=5000), rng.integers(100_000, 1 << 22, size=500),
                        np.array([0, 8 * model.strlen() - 1, 8 * model.strlen(), MAX_OFFSET - 1])])
    got = bs.getIndexes(q)
    assert got.dtype == bool and np.array_equal(got, model.get_indexes(q))
    assert got[:5000].any() and not got[5000:5500].any()
    assert bs.toByteArray() == model.bytes()  # a read grows nothing
    # n = 0 is a no-op
    bs.setIndexes([], True)
    assert bs.getIndexes([]).size == 0 and bs.toByteArray() == model.bytes()
    # an index of 2^32 fails the whole batch: nothing changes
    for value in (True, False):
        with pytest.raises(RedisException, match="bit offset"):
            bs.setIndexes([5, MAX_OFFSET, 7], value)
    with pytest.raises(RedisException, match="bit offset"):
        bs.getIndexes([5, MAX_OFFSET])
    assert bs.toByteArray() == model.bytes()
    bs.delete()
    # on a missing key: reads are zeros and create nothing, n = 0 and a failed batch create nothing
    assert not bs.getIndexes(q).any() and not bs.isExists()
    bs.setIndexes(np.zeros(0, np.int64), False)
    with pytest.raises(RedisException, match="bit offset"):
        bs.setIndexes([5, MAX_OFFSET], True)
    assert not bs.isExists()
    # a clear-only batch leaves a zero string of the right length
    bs.setIndexes([3, 100, 17], False)
    assert bs.toByteArray() == bytes(13) and bs.isExists()
    assert bs.clearBit(200) is False and bs.toByteArray() == bytes(26)
    bs.delete()


def test_index_batches_device_forms(client, fresh):
    import torch

    rng = np.random.default_rng(0xDE71CE)
    idx = rng.integers(0, 100_000, size=10_000)
    sub = rng.choice(idx, size=3000, replace=False)
    q = np.concatenate([rng.integers(0, 100_000, size=5000), rng.integers(100_000, 1 << 22, size=500)])
    host, dev = client.getBitSet(fresh + ":h"), client.getBitSet(fresh + ":d")
    d_idx, d_sub, d_q = (torch.from_numpy(a.astype(np.int64)).cuda() for a in (idx, sub, q))
    d_out = torch.full((q.size,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev.getIndexesDev(d_q.data_ptr(), q.size, d_out.data_ptr())  # a missing key: zeros
    client.synchronize()
    assert not d_out.cpu().numpy().any() and not dev.isExists()
    host.setIndexes(idx, True)
    dev.setIndexesDev(d_idx.data_ptr(), idx.size, True)
    assert dev.toByteArray() == host.toByteArray()
    host.setIndexes(sub, False)
    dev.setIndexesDev(d_sub.data_ptr(), sub.size, False)
    assert dev.toByteArray() == host.toByteArray()
    dev.getIndexesDev(d_q.data_ptr(), q.size, d_out.data_ptr())
    client.synchronize()
    assert np.array_equal(d_out.cpu().numpy().astype(bool), host.getIndexes(q))
    # n = 0, and an index of 2^32: nothing changes
    dev.setIndexesDev(d_idx.data_ptr(), 0, True)
    d_bad = torch.from_numpy(np.array([5, MAX_OFFSET], np.int64)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RedisException, match="bit offset"):
        dev.setIndexesDev(d_bad.data_ptr(), 2, True)
    with pytest.raises(RedisException, match="bit offset"):
        dev.getIndexesDev(d_bad.data_ptr(), 2, d_out.data_ptr())
    assert dev.toByteArray() == host.toByteArray()
    # a clear-only batch on a missing key
    drop(client, fresh + ":d")
    dev.setIndexesDev(d_sub.data_ptr(), sub.size, False)
    assert dev.toByteArray() == bytes((int(sub.max()) >> 3) + 1)
    drop(client, fresh + ":h", fresh + ":d")


# ---- 7. Bloom interop -----------------------------------------------------------------------------
def test_bloom_union_through_the_bit_set(client, fresh):
    import torch

    names = [fresh + s for s in ("A", "B", "C")]
    fa, fb, fc = (client.getBloomFilter(n) for n in names)
    for f in (fa, fb, fc):
        assert f.tryInit(10_000, 0.01)
    rng = np.random.default_rng(0xB100)
    mat = rng.integers(0, 256, size=(4000, 16), dtype=np.uint8)  # 4000 distinct 16-byte keys
    ka, kb = [r.tobytes() for r in mat[:2000]], [r.tobytes() for r in mat[2000:]]
    fa.add(ka)
    fb.add(kb)
    fc.add(ka + kb)
    h = BloomHandle(client, names[0])  # opened before the OR
    assert fa.exportBitmap() != fc.exportBitmap()
    client.getBitSet(names[0]).or_(names[1])
    assert fa.exportBitmap() == fc.exportBitmap()
    assert fa.contains(ka + kb) == 4000
    assert fa.count() == fc.count()
    assert client.getBitSet(names[0]).cardinality() == fc.bitcount()
    d_keys = torch.from_numpy(mat).cuda()
    d_out = torch.zeros(4000, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.contains_dev(device_keys(d_keys.data_ptr(), 4000, 16), d_cnt.data_ptr(), d_out.data_ptr())
    client.synchronize()
    assert d_cnt.item() == 4000 and d_out.cpu().numpy().all()
    h.close()
    # clear() is DEL of the bitmap alone: the config stays and the filter is empty
    client.getBitSet(names[0]).clear()
    assert fa.isExists() and fa.getSize() == fc.getSize()
    cnt, flags = fa.containsEach(ka + kb)
    assert cnt == 0 and not flags.any()
    for f in (fa, fb, fc):
        f.delete()


# ---- 8. types and timeouts ----------------------------------------------------------------------
def test_bitop_wrong_types_leave_the_destination(client, fresh):
    f = client.getBloomFilter(fresh + "F")
    assert f.tryInit(100, 0.03)
    cfg = "{" + fresh + "F}:config"
    hll = client.getHyperLogLog(fresh + "H")
    assert hll.addAll([b"a", b"b"])
    d = client.getBitSet(fresh + "D")
    d.setBytes(b"\x12\x34\x56")
    put(client, fresh + "S", b"\xff" * 9)
    for bad in (cfg, fresh + "H"):
        for srcs in ([bad], [fresh + "S", bad], [fresh + "D", fresh + "S", bad]):
            rc, _ = raw_op(client, "or", fresh + "D", srcs)
            assert rc == L.RBX_E_WRONGTYPE and "WRONGTYPE" in L.last_error(), (bad, srcs)
            assert d.toByteArray() == b"\x12\x34\x56"
        rc, _ = raw_op(client, "or", bad, [fresh + "S"])  # as the destination
        assert rc == L.RBX_E_WRONGTYPE
        with pytest.raises(RedisException, match="WRONGTYPE"):
            client.getBitSet(bad).set(1)
        with pytest.raises(RedisException, match="WRONGTYPE"):
            client.getBitSet(bad).get(1)
    assert f.getSize() == 729 and hll.count() == 2  # both still what they were
    f.delete()
    hll.delete()
    drop(client, fresh + "D", fresh + "S")


def test_timeouts_bitop_drops_setbit_keeps(client, fresh):
    d = client.getBitSet(fresh + "D")
    put(client, fresh + "S", b"\x01\x02")
    assert d.remainTimeToLive() == -2
    d.set(3)
    assert d.remainTimeToLive() == -1
    assert d.expire(3_600_000)
    for write in (lambda: d.set(77), lambda: d.clearBit(3), lambda: d.setRange(5, 900), lambda: d.clearRange(1, 9),
                  lambda: d.setIndexes([1, 5000], True), lambda: d.setIndexes([2], False)):
        write()  # SETBIT-style writes keep the timeout, also when the string has to grow
        assert 0 < d.remainTimeToLive() <= 3_600_000
    d.or_(fresh + "S")
    assert d.remainTimeToLive() == -1  # BITOP stores its result without KEEPTTL
    assert d.expire(3_600_000)
    d.rename(fresh + "E")  # RENAME keeps it
    assert d.getName() == fresh + "E" and 0 < d.remainTimeToLive() <= 3_600_000
    assert not client.getBitSet(fresh + "D").isExists()
    d.not_()
    assert d.remainTimeToLive() == -1
    drop(client, fresh + "E", fresh + "S")
