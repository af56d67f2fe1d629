"""RBitSet's typed fields on the GPU (rbx_bitset_field*, bitfield_kernels.hip): every reply and every
exported byte is compared for equality with the big-integer model of BITFIELD in bitfield_model.py.
T/ = /root/reference/redisson/src/test/java/org/redisson/"""
import numpy as np
import pytest

import bitfield_model as M
from redisson_amd import BloomHandle, IllegalArgumentException, RedisException, device_keys
from redisson_amd import _lib as L

pytestmark = pytest.mark.gpu

OPS = {M.GET: L.RBX_FIELD_GET, M.SET: L.RBX_FIELD_SET, M.INCRBY: L.RBX_FIELD_INCRBY}
TYPES = [(s, sg) for s in (1, 5, 7, 8, 31, 32, 33) for sg in (False, True)] + [(63, False), (64, True)]
OFFSETS = [0, 1, 2, 3, 4, 5, 6, 7, 27, 30, 59, 60, 63, 2040, 2047]
I64_MAX = (1 << 63) - 1


def single(bs, op, signed, size, offset, value=0):
    if op == M.GET:
        return bs.getSigned(size, offset) if signed else bs.getUnsigned(size, offset)
    if op == M.SET:
        return bs.setSigned(size, offset, value) if signed else bs.setUnsigned(size, offset, value)
    return bs.incrementAndGetSigned(size, offset, value) if signed else bs.incrementAndGetUnsigned(size, offset, value)


def batch_host(bs, op, signed, size, offs, vals, replies=True):
    if op == M.GET:
        return bs.getFields(size, offs, signed)
    fn = bs.setFields if op == M.SET else bs.incrementFields
    return fn(size, offs, vals, signed, replies)


def batch_dev(client, bs, op, signed, size, offs, vals, replies=True):
    import torch

    n = len(offs)
    d_offs = torch.from_numpy(np.asarray(offs, np.uint64).astype(np.int64).reshape(-1)).cuda()
    d_vals = None if vals is None else torch.from_numpy(np.asarray(vals, np.int64).reshape(-1)).cuda()
    d_rep = torch.full((max(n, 1),), 77, dtype=torch.int64, device="cuda") if replies else None
    torch.cuda.synchronize()
    rp = None if d_rep is None else d_rep.data_ptr()
    if op == M.GET:
        bs.getFieldsDev(size, d_offs.data_ptr(), n, rp, signed)
    elif op == M.SET:
        bs.setFieldsDev(size, d_offs.data_ptr(), d_vals.data_ptr(), n, rp, signed)
    else:
        bs.incrementFieldsDev(size, d_offs.data_ptr(), d_vals.data_ptr(), n, rp, signed)
    client.synchronize()
    return None if d_rep is None else d_rep.cpu().numpy()[:n]


def check_padding(bs, want: bytes):
    """GET == want, and what lies behind the string is zero: a SETBIT 0 further on stretches the string
    over its padding (in place, or through a copy of the whole allocation), which must read as zeros."""
    assert bs.toByteArray() == want
    assert bs.size() == 8 * len(want)
    far = len(want) + 700
    assert bs.set(8 * far - 1, False) is False
    assert bs.toByteArray() == want + bytes(far - len(want))


def both_forms(client, fresh, start: bytes, op, signed, size, offs, vals, replies=True):
    """The batch through the host form and the device form, each on its own copy of `start`
    (empty = a missing key): replies and strings equal the model's.  Returns the string after."""
    want, want_rep = M.fields(start, op, signed, size, offs, vals)
    for tag in ("h", "d"):
        bs = client.getBitSet(fresh + tag)
        bs.delete()
        if start:
            bs.setBytes(start)
        got = (batch_host(bs, op, signed, size, offs, vals, replies) if tag == "h"
               else batch_dev(client, bs, op, signed, size, offs, vals, replies))
        if replies:
            assert got.dtype == np.int64 and got.tolist() == want_rep, (tag, op, signed, size)
        else:
            assert got is None
        assert bs.toByteArray() == want, (tag, op, signed, size)
        assert bs.isExists() == (len(want) > 0)
        if want:
            check_padding(bs, want)
        bs.delete()
    return want


# ---- 1. reference vectors (T/RedissonBitSetTest.java:15-57) ---------------------------------------
def test_reference_vectors(client, fresh):
    bs = client.getBitSet(fresh + "U")  # testUnsigned
    assert bs.setUnsigned(8, 1, 120) == 0
    assert bs.toByteArray() == bytes.fromhex("3c00") and bs.size() == 16
    assert bs.incrementAndGetUnsigned(8, 1, 1) == 121
    assert bs.getUnsigned(8, 1) == 121
    bs.delete()
    bs = client.getBitSet(fresh + "S")  # testSigned
    assert bs.setSigned(8, 1, -120) == 0
    assert bs.toByteArray() == bytes.fromhex("4400")
    assert bs.incrementAndGetSigned(8, 1, 1) == -119
    assert bs.getSigned(8, 1) == -119
    assert bs.toByteArray() == bytes.fromhex("4480") and bs.size() == 16
    bs.delete()
    bs = client.getBitSet(fresh + "B")  # testIncrement
    assert bs.setByte(2, 12) == 0
    assert bs.getByte(2) == 12 and bs.toByteArray() == bytes.fromhex("0300")
    assert bs.incrementAndGetByte(2, 12) == 24
    assert bs.getByte(2) == 24 and bs.toByteArray() == bytes.fromhex("0600") and bs.size() == 16
    bs.delete()
    bs = client.getBitSet(fresh + "L")  # testSetGetNumber
    assert bs.setLong(2, 12) == 0
    assert bs.getLong(2) == 12
    assert bs.toByteArray() == bytes(7) + bytes.fromhex("0300") and bs.size() == 72
    bs.delete()
    bs = client.getBitSet(fresh + "H")
    assert bs.setShort(2, 2312) == 0
    assert bs.getShort(2) == 2312 and bs.toByteArray() == bytes.fromhex("024200") and bs.size() == 24
    bs.delete()
    bs = client.getBitSet(fresh + "I")
    assert bs.setInteger(2, 323241) == 0
    assert bs.getInteger(2) == 323241 and bs.toByteArray() == bytes.fromhex("00013baa40") and bs.size() == 40
    assert bs.get_integer(2) == 323241 and bs.increment_and_get_integer(2, -1) == 323240  # the snake_case aliases
    bs.delete()


def test_java_argument_ranges(client, fresh):
    bs = client.getBitSet(fresh)
    for call in (lambda: bs.setByte(0, 128), lambda: bs.setByte(0, -129), lambda: bs.incrementAndGetByte(0, 128),
                 lambda: bs.setShort(0, 1 << 15), lambda: bs.incrementAndGetShort(0, -(1 << 15) - 1),
                 lambda: bs.setInteger(0, 1 << 31), lambda: bs.incrementAndGetInteger(0, -(1 << 31) - 1),
                 lambda: bs.setLong(0, 1 << 63), lambda: bs.incrementAndGetLong(0, -(1 << 63) - 1),
                 lambda: bs.setSigned(8, 0, 1 << 63), lambda: bs.setUnsigned(8, 0, 1 << 63)):
        with pytest.raises(IllegalArgumentException):
            call()
    for call in (lambda: bs.getSigned(65, 0), lambda: bs.setSigned(65, 0, 1), lambda: bs.incrementAndGetSigned(65, 0, 1)):
        with pytest.raises(IllegalArgumentException, match="greater than 64 bits"):
            call()
    for call in (lambda: bs.getUnsigned(64, 0), lambda: bs.setUnsigned(64, 0, 1),
                 lambda: bs.incrementAndGetUnsigned(64, 0, 1), lambda: bs.setFields(64, [0], [1], signed=False)):
        with pytest.raises(IllegalArgumentException, match="greater than 63 bits"):
            call()
    for call in (lambda: bs.getSigned(0, 0), lambda: bs.setUnsigned(0, 0, 1), lambda: bs.incrementAndGetSigned(-3, 0, 1),
                 lambda: bs.getFields(0, [0])):
        with pytest.raises(RedisException, match="Invalid bitfield type"):
            call()
    for call in (lambda: bs.getByte(1 << 32), lambda: bs.setByte(1 << 32, 1), lambda: bs.incrementAndGetByte(-1, 1),
                 lambda: bs.setByte((1 << 32) - 7, 1), lambda: bs.getLong((1 << 32) - 63)):
        with pytest.raises(RedisException, match="bit offset is not an integer or out of range"):
            call()
    assert not bs.isExists()


# ---- 2. single calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["missing", "random"])
def test_single_calls(client, fresh, start):
    rng = np.random.default_rng(0xF1E1D)
    for size, signed in TYPES:
        for offset in OFFSETS:
            bs = client.getBitSet(fresh)
            data = b"" if start == "missing" else rng.bytes(250)  # one 256-byte allocation; 2040.. grows it
            if data:
                bs.setBytes(data)
            v = int(rng.integers(-(1 << 63), 1 << 63, dtype=np.int64))
            inc = int(rng.integers(-(1 << 63), 1 << 63, dtype=np.int64))
            for op, value in ((M.SET, v), (M.GET, 0), (M.INCRBY, inc)):
                data, want = M.field(data, op, signed, size, offset, value)
                assert single(bs, op, signed, size, offset, value) == want, (size, signed, offset, op)
                assert bs.toByteArray() == data, (size, signed, offset, op)
            check_padding(bs, data)
            bs.delete()


def test_single_call_wraps(client, fresh):
    bs = client.getBitSet(fresh)
    cases = [  # (signed, size, start value, increment)
        (False, 8, 255, 1), (True, 8, 127, 1), (True, 64, I64_MAX, 1), (False, 63, I64_MAX, 1),
        (False, 8, 3, -5), (False, 63, 0, -1), (False, 5, 1, -(1 << 63)), (True, 7, -64, -1)]
    data = b""
    for k, (signed, size, v0, inc) in enumerate(cases):
        offset = 3 + 70 * k
        for op, value in ((M.SET, v0), (M.INCRBY, inc), (M.GET, 0)):
            data, want = M.field(data, op, signed, size, offset, value)
            assert single(bs, op, signed, size, offset, value) == want, (signed, size, op)
    assert single(bs, M.GET, False, 8, 3) == 0 and single(bs, M.GET, True, 8, 73) == -128
    assert single(bs, M.GET, True, 64, 143) == -(1 << 63) and single(bs, M.GET, False, 63, 213) == 0
    # SET of a value wider than the field keeps value mod 2^size
    for signed, size, value in ((False, 4, 0x1F5), (True, 4, 0x1F5), (False, 12, -1), (True, 33, I64_MAX), (True, 1, 3)):
        data, want = M.field(data, M.SET, signed, size, 1001, value)
        assert single(bs, M.SET, signed, size, 1001, value) == want
        data, want = M.field(data, M.GET, signed, size, 1001)
        assert single(bs, M.GET, signed, size, 1001) == want
    check_padding(bs, data)
    bs.delete()


def test_get_creates_nothing_incrby_zero_creates(client, fresh):
    bs = client.getBitSet(fresh)
    for size, signed, offset in ((8, True, 0), (64, True, 2), (63, False, 5000), (1, False, (1 << 32) - 1)):
        assert single(bs, M.GET, signed, size, offset) == 0
        assert bs.getFields(size, [offset, 0], signed).tolist() == [0, 0]
        assert not bs.isExists() and bs.size() == 0
    for size, signed, offset in ((8, True, 0), (64, True, 2), (63, False, 5000), (3, False, 30)):
        assert single(bs, M.INCRBY, signed, size, offset, 0) == 0
        want = M.field(b"", M.INCRBY, signed, size, offset, 0)[0]
        assert len(want) == ((offset + size - 1) >> 3) + 1
        assert bs.isExists() and bs.toByteArray() == want
        bs.delete()
    # a GET past the end of an existing string grows nothing either
    bs.setBytes(b"\xff\xff\xff")
    assert bs.getSigned(16, 16) == -256 and bs.getUnsigned(16, 20) == 0xF000 and bs.getLong(4000) == 0
    assert bs.toByteArray() == b"\xff\xff\xff"
    bs.delete()


# ---- 3. batches --------------------------------------------------------------------------------
NS = [1, 2, 255, 256, 257, 4096]


@pytest.mark.parametrize("n", NS)
def test_batch_get_unaligned(client, fresh, n):
    rng = np.random.default_rng(n)
    data = rng.bytes(300)  # a 512-byte allocation: offsets reach past the string and past the allocation
    for size, signed in ((1, False), (7, True), (13, False), (32, True), (33, True), (63, False), (64, True)):
        offs = rng.integers(0, 6000, n).astype(np.uint64)
        offs[0] = 300 * 8 - size // 2 - 1  # across the string's end
        offs[-1] = 512 * 8 - 1 if n > 1 else offs[-1]  # across the allocation's end
        assert both_forms(client, fresh, data, M.GET, signed, size, offs, None) == data
        both_forms(client, fresh, b"", M.GET, signed, size, offs, None)  # a missing key: zeros, no key


@pytest.mark.parametrize("op", [M.SET, M.INCRBY])
@pytest.mark.parametrize("size", [3, 4, 8, 12, 16, 32, 64])
def test_batch_aligned_with_replies(client, fresh, op, size):
    signed = size == 64 or size == 12
    rng = np.random.default_rng(size * 10 + op)
    data = rng.bytes(100)
    slots = rng.choice(200, 64, replace=False)  # 64 distinct slots: long runs that cross block boundaries
    for n in NS:
        offs = (rng.choice(slots, n) * size).astype(np.uint64)
        vals = rng.integers(-(1 << 63), 1 << 63, n, dtype=np.int64)
        both_forms(client, fresh, data, op, signed, size, offs, vals)
    both_forms(client, fresh, b"", op, signed, size, (rng.choice(slots, 257) * size).astype(np.uint64),
               rng.integers(-9, 9, 257))  # a missing key
    both_forms(client, fresh, data, op, signed, size, (rng.choice(slots, 257) * size).astype(np.uint64),
               rng.integers(-9, 9, 257), replies=False)


@pytest.mark.parametrize("op", [M.SET, M.INCRBY])
def test_batch_one_slot_and_no_duplicates(client, fresh, op):
    rng = np.random.default_rng(41 + op)
    data = rng.bytes(64)
    for size, signed in ((12, False), (16, True), (64, True)):
        vals = rng.integers(-(1 << 63), 1 << 63, 4096, dtype=np.int64)
        both_forms(client, fresh, data, op, signed, size, np.full(4096, 5 * size, np.uint64), vals)
        both_forms(client, fresh, data, op, signed, size, (rng.permutation(4096) * size).astype(np.uint64), vals)


@pytest.mark.parametrize("size", [1, 2, 4, 8, 16, 32, 64])
def test_batch_increment_without_replies(client, fresh, size):
    """65,536 increments over 16 slots: many lanes contend on one word and the counters wrap."""
    rng = np.random.default_rng(size)
    data = rng.bytes(40)
    slots = rng.choice(max(32, 640 // size), 16, replace=False)  # some inside the 40-byte string, some past it
    offs = (rng.choice(slots, 65536) * size).astype(np.uint64)
    incs = rng.integers(-(1 << 63), 1 << 63, 65536, dtype=np.int64) if size > 16 else rng.integers(-300, 300, 65536)
    both_forms(client, fresh, data, M.INCRBY, size == 64, size, offs, incs, replies=False)
    both_forms(client, fresh, b"", M.INCRBY, True, size, offs[:257], incs[:257], replies=False)


@pytest.mark.parametrize("op", [M.SET, M.INCRBY])
def test_batch_unaligned_overlapping_is_serial(client, fresh, op):
    rng = np.random.default_rng(7 + op)
    offs = (3 * np.arange(257)).astype(np.uint64)  # size 8: each field overlaps its neighbours
    vals = rng.integers(-(1 << 63), 1 << 63, 257, dtype=np.int64)
    for signed in (False, True):
        both_forms(client, fresh, rng.bytes(50), op, signed, 8, offs, vals)
        both_forms(client, fresh, b"", op, signed, 8, offs[::-1].copy(), vals)
        both_forms(client, fresh, rng.bytes(50), op, signed, 8, offs, vals, replies=False)


def test_batch_order(client, fresh):
    assert both_forms(client, fresh, b"\xfe", M.INCRBY, False, 8, [0, 0, 0], [1, 1, 1]) == b"\x01"
    bs = client.getBitSet(fresh)
    bs.setBytes(b"\xfe")
    assert bs.incrementFields(8, [0, 0, 0], [1, 1, 1], signed=False).tolist() == [255, 0, 1]
    bs.setBytes(b"\x03")
    assert bs.setFields(8, [0, 0], [5, 9], signed=False).tolist() == [3, 5]
    assert bs.toByteArray() == b"\x09"
    assert bs.set_fields(8, [0], [1], replies=False) is None and bs.get_fields(8, [0]).tolist() == [1]
    bs.delete()


# ---- 4. all-or-nothing, types, the empty batch -------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_illegal_offset_fails_the_whole_batch(client, fresh, form):
    bs = client.getBitSet(fresh)
    run = (lambda *a: batch_host(bs, *a)) if form == "host" else (lambda *a: batch_dev(client, bs, *a))
    vals = np.arange(256, dtype=np.int64)
    for last in (1 << 32, (1 << 32) - 7, (1 << 63) + 8):
        offs = (np.arange(256) * 8).astype(np.uint64)
        offs[-1] = last
        for op in (M.SET, M.INCRBY, M.GET):
            with pytest.raises(RedisException, match="bit offset is not an integer or out of range"):
                run(op, True, 8, offs, vals)
            assert not bs.isExists()
    bs.setBytes(b"\x12\x34")
    for op in (M.SET, M.INCRBY):
        with pytest.raises(RedisException, match="bit offset"):
            run(op, True, 8, offs, vals)
        assert bs.toByteArray() == b"\x12\x34"
    bs.delete()


def test_wrong_types_and_the_empty_batch(client, fresh):
    f = client.getBloomFilter(fresh + "F")
    assert f.tryInit(100, 0.03)
    hll = client.getHyperLogLog(fresh + "H")
    assert hll.addAll([b"a", b"b"])
    for bad in ("{" + fresh + "F}:config", fresh + "H"):
        bs = client.getBitSet(bad)
        for call in (lambda: bs.getByte(0), lambda: bs.setByte(0, 1), lambda: bs.incrementAndGetByte(0, 1),
                     lambda: bs.getFields(8, [0, 8]), lambda: bs.setFields(8, [0, 8], [1, 2]),
                     lambda: bs.incrementFields(8, [0, 8], [1, 2], replies=False),
                     lambda: bs.incrementFields(8, [0, 3], [1, 2]),
                     lambda: batch_dev(client, bs, M.SET, True, 8, [0, 8], [1, 2])):
            with pytest.raises(RedisException, match="WRONGTYPE"):
                call()
    assert f.getSize() == 729 and hll.count() == 2  # both still what they were
    f.delete()
    hll.delete()
    bs = client.getBitSet(fresh)
    empty = np.zeros(0, np.uint64)
    for op in (M.GET, M.SET, M.INCRBY):
        got = batch_host(bs, op, True, 8, empty, np.zeros(0, np.int64))
        assert got.size == 0 and got.dtype == np.int64
        assert batch_dev(client, bs, op, True, 8, empty, np.zeros(0, np.int64)).size == 0
        nm, _keep = L.name_struct(fresh)
        assert L.lib().rbx_bitset_fields(client.ctx, nm, OPS[op], 1, 8, None, None, 0, None) == L.RBX_OK
        assert not bs.isExists()


# ---- 5. neighbours -----------------------------------------------------------------------------
def test_neighbours_keep_their_bytes(client, fresh):
    rng = np.random.default_rng(5)
    data = rng.bytes(4099)
    slots = rng.choice(2 * 4099, 500, replace=False)
    offs = (rng.choice(slots, 4096) * 4).astype(np.uint64)
    after = both_forms(client, fresh, data, M.INCRBY, False, 4, offs, rng.integers(1, 16, 4096), replies=False)
    touched = np.zeros(4099, bool)
    touched[np.unique(offs // 8).astype(np.int64)] = True
    a, b = np.frombuffer(after, np.uint8), np.frombuffer(data, np.uint8)
    assert (a[~touched] == b[~touched]).all() and len(after) == 4099
    for o in np.unique(offs):  # the other u4 of a touched byte
        other = int(o) ^ 4
        if other not in offs:
            assert M.field(after, M.GET, False, 4, other)[1] == M.field(data, M.GET, False, 4, other)[1]


def test_growth_leaves_zeros_between_the_lengths(client, fresh):
    """4,099 bytes of 0xFF shrink to the 3 bytes of a BITOP AND inside the same allocation; a field
    write past them grows the string over bytes that must read as zero, not as the old 0xFF."""
    bs, three = client.getBitSet(fresh), client.getBitSet(fresh + "3")
    bs.setBytes(b"\xff" * 4099)
    three.setBytes(b"\x0f\xff\xf0")
    dest, _k1 = L.name_struct(fresh)
    srcs, _k2 = L.names_array([fresh + "3"])
    assert L.lib().rbx_bitset_op(client.ctx, L.RBX_BITOP_AND, dest, srcs, 1, None) == L.RBX_OK
    old = bs.toByteArray()
    assert old == b"\x0f\xff\xf0"
    assert bs.setUnsigned(8, 32000, 1) == 0
    want = M.field(old, M.SET, False, 8, 32000, 1)[0]
    assert len(want) == 4001 and want[3:4000] == bytes(3997)
    assert bs.toByteArray() == want
    assert bs.incrementAndGetSigned(13, 80001, -1) == -1  # past the allocation as well
    want = M.field(want, M.INCRBY, True, 13, 80001, -1)[0]
    assert len(want) == 10002 and want[4001:10000] == bytes(5999)
    check_padding(bs, want)
    bs.delete()
    three.delete()


# ---- 6. interplay ------------------------------------------------------------------------------
def test_u1_set_batch_equals_set_indexes(client, fresh):
    rng = np.random.default_rng(61)
    idx = rng.integers(0, 50_000, 4096).astype(np.uint64)
    a, b = client.getBitSet(fresh + "a"), client.getBitSet(fresh + "b")
    for v in (1, 0):
        sub = idx if v else idx[::3].copy()
        a.setIndexes(sub, bool(v))
        assert b.setFields(1, sub, np.full(sub.size, v), signed=False, replies=False) is None
        assert a.toByteArray() == b.toByteArray() and a.size() == b.size()
    a.delete()
    b.delete()


def test_bloom_handle_sees_in_place_set_byte(client, fresh):
    import torch

    f = client.getBloomFilter(fresh)
    assert f.tryInit(100, 0.03)  # 729 bits: 92 bytes in a 256-byte allocation
    rng = np.random.default_rng(0xB17)
    mat = rng.integers(0, 256, size=(1000, 16), dtype=np.uint8)
    f.add([mat[0].tobytes()])
    h = BloomHandle(client, fresh)  # opened before the writes
    d_keys = torch.from_numpy(mat).cuda()
    d_out = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.contains_dev(device_keys(d_keys.data_ptr(), 1000, 16), d_cnt.data_ptr(), d_out.data_ptr())
    client.synchronize()
    assert 1 <= d_cnt.item() < 1000
    bs = client.getBitSet(fresh)
    for byte in range(92):
        bs.setByte(8 * byte, -1)
    assert bs.toByteArray() == b"\xff" * 92
    d_cnt.zero_()
    torch.cuda.synchronize()
    h.contains_dev(device_keys(d_keys.data_ptr(), 1000, 16), d_cnt.data_ptr(), d_out.data_ptr())
    client.synchronize()
    assert d_cnt.item() == 1000 and d_out.cpu().numpy().all()
    h.close()
    f.delete()


def test_timeout_survives_field_writes(client, fresh):
    d = client.getBitSet(fresh)
    assert d.setByte(0, 1) == 0
    assert d.remainTimeToLive() == -1
    assert d.expire(3_600_000)
    for write in (lambda: d.setSigned(7, 3, 9), lambda: d.incrementAndGetUnsigned(5, 9000, 3),
                  lambda: d.setFields(8, [0, 80_000], [1, 2]), lambda: d.incrementFields(16, [16, 16], [1, 2], replies=False),
                  lambda: d.incrementFields(8, [3, 5], [1, 2]), lambda: d.getLong(5)):
        write()  # also when the string has to grow
        assert 0 < d.remainTimeToLive() <= 3_600_000
    d.delete()


# ---- 7. the last legal field ---------------------------------------------------------------------
def test_last_legal_field(client, fresh):
    bs = client.getBitSet(fresh)
    try:
        assert bs.setByte((1 << 32) - 8, 7) == 0
        assert bs.getByte((1 << 32) - 8) == 7
        assert bs.size() == 1 << 32
        assert bs.getFields(8, [(1 << 32) - 8, (1 << 32) - 16, 0]).tolist() == [7, 0, 0]
        assert bs.incrementFields(4, [(1 << 32) - 4], [-8], signed=False).tolist() == [15]
        assert bs.getUnsigned(8, (1 << 32) - 8) == 15 and bs.cardinality() == 4
        with pytest.raises(RedisException, match="bit offset"):
            bs.setByte((1 << 32) - 7, 1)
    finally:
        bs.delete()
