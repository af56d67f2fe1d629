"""BITFIELD under OVERFLOW SAT / FAIL and Spring Data's bitField on the GPU (rbx_bitset_fields_ov*,
rbx_bitset_bitfield, bitfield_kernels.hip): after every write the whole exported string, the replies and the
nil mask are compared for equality with the big-integer model of bitfield_overflow_model.py.  Strings start
from a 0xA5 pattern so that a clobbered neighbour shows, and what lies behind a string must stay zero."""
import ctypes as C

import numpy as np
import pytest

import bitfield_overflow_model as M
from redisson_amd import BloomHandle, IllegalArgumentException, RedisException, device_keys
from redisson_amd import _lib as L
from redisson_amd.client import _check
from redisson_amd.spring_data import (BitFieldGet, BitFieldIncrBy, BitFieldSet, BitFieldType, Offset,
                                      RedissonConnection)
from test_bitfield_gpu import OFFSETS, TYPES, check_padding

pytestmark = pytest.mark.gpu

MODE_NAMES = {M.WRAP: "WRAP", M.SAT: "SAT", M.FAIL: "FAIL"}
I64_MIN, I64_MAX = M.I64_MIN, M.I64_MAX


def pattern(n: int) -> bytes:
    return b"\xa5" * n


def i64(values) -> np.ndarray:
    return np.array([int(v) for v in values], dtype=np.int64)


def run_host(bs, op, signed, size, mode, offs, vals, replies):
    """-> (replies or None, nil mask or None) through RBitSet's host form"""
    fn = bs.setFields if op == M.SET else bs.incrementFields
    got = fn(size, offs, vals, signed, replies, overflow=MODE_NAMES[mode])
    if mode == M.FAIL:
        return got
    return got, None


def run_dev(client, bs, op, signed, size, mode, offs, vals, replies):
    """the same through the device form; the nil mask is asked for under every mode but WRAP"""
    import torch

    n = len(offs)
    d_offs = torch.from_numpy(np.asarray(offs, np.uint64).astype(np.int64).reshape(-1)).cuda()
    d_vals = torch.from_numpy(np.asarray(vals, np.int64).reshape(-1)).cuda()
    d_rep = torch.full((max(n, 1),), 77, dtype=torch.int64, device="cuda") if replies else None
    d_nil = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda") if mode != M.WRAP else None
    torch.cuda.synchronize()
    fn = bs.setFieldsDev if op == M.SET else bs.incrementFieldsDev
    fn(size, d_offs.data_ptr(), d_vals.data_ptr(), n, None if d_rep is None else d_rep.data_ptr(), signed,
       overflow=MODE_NAMES[mode], d_nil=None if d_nil is None else d_nil.data_ptr())
    client.synchronize()
    return (None if d_rep is None else d_rep.cpu().numpy()[:n],
            None if d_nil is None else d_nil.cpu().numpy()[:n].astype(bool))


def tune(client, knob: int):
    assert L.lib().rbx_tune(b"bitfield_sat_atomic", knob) == 0


def both_forms(client, fresh, start: bytes, op, signed, size, mode, offs, vals, replies=True, knobs=(1,)):
    """The batch through the host and the device form, under each setting of bitfield_sat_atomic, each on its
    own copy of `start` (empty = a missing key): strings, replies and nil masks equal the model's.  Returns
    the string after."""
    want, want_rep = M.fields(start, op, signed, size, mode, offs, vals)
    want_nil = [r is None for r in want_rep]
    want_num = [0 if r is None else r for r in want_rep]
    try:
        for knob in knobs:
            tune(client, knob)
            for tag in ("h", "d"):
                bs = client.getBitSet(fresh + tag)
                bs.delete()
                if start:
                    bs.setBytes(start)
                rep, nil = (run_host(bs, op, signed, size, mode, offs, vals, replies) if tag == "h"
                            else run_dev(client, bs, op, signed, size, mode, offs, vals, replies))
                where = (tag, knob, op, signed, size, mode)
                if replies:
                    assert rep.dtype == np.int64 and rep.tolist() == want_num, where
                else:
                    assert rep is None
                if nil is not None:
                    assert nil.tolist() == (want_nil if mode == M.FAIL else [False] * len(want_nil)), where
                assert bs.toByteArray() == want, where
                assert bs.isExists() == (len(want) > 0)
                if want:
                    check_padding(bs, want)
                bs.delete()
    finally:
        tune(client, 1)
    return want


def raw_bitfield(client, name, rows, with_nil=True):
    """rbx_bitset_bitfield on rows of (op, signed, size, mode, offset, value) -> replies, None for nil"""
    arr = (L.RbxFieldCmd * max(len(rows), 1))()
    for a, (op, signed, size, mode, offset, value) in zip(arr, rows):
        a.op, a.is_signed, a.size, a.overflow, a.offset, a.value = op, int(signed), size, mode, offset, value
    rep = np.full(max(len(rows), 1), 77, np.int64)
    nil = np.full(max(len(rows), 1), 77, np.uint8)
    nm, _keep = L.name_struct(name)
    _check(L.lib().rbx_bitset_bitfield(client.ctx, nm, arr, len(rows), rep.ctypes.data_as(L.i64p),
                                       nil.ctypes.data_as(L.u8p) if with_nil else None))
    if not with_nil:
        return rep[: len(rows)].tolist()
    assert set(nil[: len(rows)].tolist()) <= {0, 1}
    assert all(r == 0 for r, z in zip(rep[: len(rows)], nil) if z)
    return [None if z else int(r) for r, z in zip(rep[: len(rows)], nil)]


# ---- 1. the vectors of the Redis documentation (recalled; known answers) -------------------------
def test_redis_documentation_vectors(client, fresh):
    bs = client.getBitSet(fresh)
    u2 = (False, 2)
    step = [(M.INCRBY, *u2, M.WRAP, 100, 1), (M.INCRBY, *u2, M.SAT, 102, 1)]
    got = [raw_bitfield(client, fresh, step) for _ in range(4)]
    assert got == [[1, 1], [2, 2], [3, 3], [0, 3]]
    assert bs.toByteArray() == bytes(12) + b"\x03"
    assert raw_bitfield(client, fresh, [(M.INCRBY, *u2, M.FAIL, 102, 1)]) == [None]
    check_padding(bs, bytes(12) + b"\x03")
    bs.delete()
    assert raw_bitfield(client, fresh, [(M.INCRBY, True, 5, M.WRAP, 100, 1), (M.GET, False, 4, M.WRAP, 0, 0)]) == [1, 0]
    assert bs.toByteArray() == M.bitfield(b"", [(M.INCRBY, True, 5, M.WRAP, 100, 1)])[0]
    bs.delete()


# ---- 2. the saturating atomic path ---------------------------------------------------------------
SAT_TYPES = [(1, False), (2, False), (4, False), (8, False), (16, False), (32, False),
             (8, True), (16, True), (32, True), (64, True)]


def sat_batch(size: int, signed: bool, sign: int):
    """4,096 increments of one sign over 16 slots, slots 15 and 16 among them (for u4: bits 60..67, the last
    field of one word and the first of the next).  Eight heavy slots take almost all of them and saturate;
    light slot j takes j % 3, small ones."""
    rng = np.random.default_rng(size * 4 + signed * 2 + (sign > 0))
    others = [s for s in rng.permutation(40).tolist() if s not in (15, 16)][:14]
    heavy, light = [15] + others[:7], [16] + others[7:]
    lo, hi = M.bounds(signed, size)
    m = max(1, hi // 64)
    slots = [s for j, s in enumerate(light) for _ in range(j % 3)]
    slots += rng.choice(heavy, 4096 - len(slots) - 1).tolist()
    incs = [sign * int(v) for v in rng.integers(1, m + 1, len(slots), dtype=np.int64)]
    order = rng.permutation(len(slots))
    slots, incs = [slots[i] for i in order], [incs[i] for i in order]
    slots.insert(2048, heavy[1])  # the largest step there is
    incs.insert(2048, (I64_MAX if sign > 0 else I64_MIN) if size == 64 else sign * (hi - lo))
    return np.array(slots, np.uint64) * np.uint64(size), i64(incs), heavy, light


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("size,signed", SAT_TYPES)
def test_saturating_increments_without_replies(client, fresh, size, signed, sign):
    offs, incs, heavy, light = sat_batch(size, signed, sign)
    assert len(offs) == 4096 and (incs > 0).all() == (sign > 0) and (incs < 0).all() == (sign < 0)
    start = pattern(330)
    after = both_forms(client, fresh, start, M.INCRBY, signed, size, M.SAT, offs, incs, replies=False, knobs=(1, 0))
    lo, hi = M.bounds(signed, size)
    bound = hi if sign > 0 else lo
    final = {s: M._read(after, signed, size, s * size) for s in heavy + light}
    assert all(final[s] == bound for s in heavy)
    assert any(final[s] != bound for s in light)  # some slots saturate and some do not
    assert after != M.fields(start, M.INCRBY, signed, size, M.WRAP, offs, incs)[0]
    # a missing key, and a batch with zero increments among the others
    both_forms(client, fresh, b"", M.INCRBY, signed, size, M.SAT, offs[:257], incs[:257], replies=False, knobs=(1, 0))
    zeros = incs.copy()
    zeros[::3] = 0
    both_forms(client, fresh, start, M.INCRBY, signed, size, M.SAT, offs, zeros, replies=False, knobs=(1, 0))


@pytest.mark.parametrize("n", [1, 2, 255, 1000, 1001])
def test_device_arrays_that_start_at_an_odd_element(client, fresh, n):
    """the sign check reads two elements per load from 16-byte aligned arrays, and one at a time from any other"""
    import torch

    offs, incs, _h, _l = sat_batch(8, False, 1)
    bs = client.getBitSet(fresh)
    for skip, mixed in ((0, False), (1, False), (0, True), (1, True)):
        o, v = offs[: n + skip].copy(), incs[: n + skip].copy()
        if mixed:
            v[-1] = -v[-1]  # the one negative increment is the last element: the odd one out when n is odd
        d_offs, d_vals = torch.from_numpy(o.astype(np.int64)).cuda(), torch.from_numpy(v).cuda()
        bs.setBytes(pattern(330))
        torch.cuda.synchronize()
        bs.incrementFieldsDev(8, d_offs.data_ptr() + 8 * skip, d_vals.data_ptr() + 8 * skip, n, None, signed=False,
                              overflow="SAT")
        client.synchronize()
        assert bs.toByteArray() == M.fields(pattern(330), M.INCRBY, False, 8, M.SAT, o[skip:], v[skip:])[0], (skip, mixed)
    bs.delete()


# ---- 3. batches whose result depends on the order ------------------------------------------------
def test_mixed_signs_under_sat_keep_the_order(client, fresh):
    start = bytes([250]) * 64
    offs = np.repeat(np.arange(64, dtype=np.uint64) * 8, 2)
    incs = i64([10, -10] * 64)
    want = M.fields(start, M.INCRBY, False, 8, M.SAT, offs, incs)[0]
    assert want == bytes([245]) * 64
    assert M.fields(start, M.INCRBY, False, 8, M.SAT, offs[::-1], incs[::-1])[0] == bytes([250]) * 64  # the order shows
    for replies in (False, True):
        assert both_forms(client, fresh, start, M.INCRBY, False, 8, M.SAT, offs, incs, replies, knobs=(1, 0)) == want
    # one negative increment at the end of a positive batch is enough
    incs2 = i64([10, 10] * 63 + [10, -10])
    both_forms(client, fresh, start, M.INCRBY, False, 8, M.SAT, offs, incs2, replies=False, knobs=(1, 0))


def test_fail_keeps_the_order(client, fresh):
    start = bytes([250]) * 64
    offs = np.repeat(np.arange(64, dtype=np.uint64) * 8, 2)
    incs = i64([5, 3] * 64)
    want, rep = M.fields(start, M.INCRBY, False, 8, M.FAIL, offs, incs)
    assert want == bytes([255]) * 64 and rep[:2] == [255, None]
    assert M.fields(start, M.INCRBY, False, 8, M.FAIL, offs[::-1], incs[::-1])[0] == bytes([253]) * 64
    for replies in (True, False):
        assert both_forms(client, fresh, start, M.INCRBY, False, 8, M.FAIL, offs, incs, replies, knobs=(1, 0)) == want


# ---- 4. the grouped path with replies ------------------------------------------------------------
def wide_values(rng, op, signed, size, n):
    """values around the type's range: some sub-commands overflow on either side and some do not"""
    lo, hi = M.bounds(signed, size)
    span = max(2, (hi - lo) // 3) if op == M.INCRBY else 2 * (hi - lo) + 2
    vals = [(int(rng.integers(0, 1 << 62)) * (2 * span + 1) >> 62) - span for _ in range(n)]  # uniform in [-span, span]
    return i64(max(I64_MIN, min(I64_MAX, v)) for v in vals)


@pytest.mark.parametrize("mode", [M.SAT, M.FAIL])
@pytest.mark.parametrize("op", [M.SET, M.INCRBY])
def test_grouped_path_with_replies(client, fresh, op, mode):
    rng = np.random.default_rng(100 + 10 * op + mode)
    for size, signed in TYPES:
        slots = rng.choice(60, 32, replace=False)
        offs = (rng.choice(slots, 2000) * size).astype(np.uint64)
        vals = wide_values(rng, op, signed, size, 2000)
        want, rep = M.fields(pattern(100), op, signed, size, mode, offs, vals)
        if mode == M.FAIL and (size, signed) != (64, True):
            assert any(r is None for r in rep) and any(r is not None for r in rep), (size, signed)
        both_forms(client, fresh, pattern(100), op, signed, size, mode, offs, vals)
    both_forms(client, fresh, b"", op, True, 12, mode, offs[:257] // 64 * 12, vals[:257])  # a missing key


# ---- 5. the serial path --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [M.SAT, M.FAIL])
@pytest.mark.parametrize("op", [M.SET, M.INCRBY])
def test_serial_path_on_overlapping_fields(client, fresh, op, mode):
    rng = np.random.default_rng(500 + 10 * op + mode)
    for size, signed in TYPES:
        offs = rng.choice(OFFSETS, 200).astype(np.uint64)
        offs[0] = 3  # never aligned for size > 1 ... and size 1 is the aligned edge of the same call
        vals = wide_values(rng, op, signed, size, 200)
        both_forms(client, fresh, pattern(100), op, signed, size, mode, offs, vals)
        both_forms(client, fresh, pattern(100), op, signed, size, mode, offs, vals, replies=False)


# ---- 6. growth and errors ------------------------------------------------------------------------
def test_a_failing_batch_still_sizes_the_key(client, fresh):
    bs = client.getBitSet(fresh)
    rep, nil = bs.incrementFields(8, [0], [300], signed=False, overflow="FAIL")
    assert rep.tolist() == [0] and nil.tolist() == [True]
    assert bs.isExists() and bs.toByteArray() == b"\x00"
    bs.delete()
    both_forms(client, fresh, b"", M.INCRBY, False, 8, M.FAIL, [0, 40, 3], [300, 300, 256])  # serial
    both_forms(client, fresh, b"", M.INCRBY, False, 8, M.FAIL, [0, 40, 8], [300, 300, 256])  # grouped
    assert raw_bitfield(client, fresh, [(M.INCRBY, False, 8, M.FAIL, 16, 300), (M.GET, True, 3, M.WRAP, 900, 0)]) == [None, 0]
    assert bs.toByteArray() == bytes(3)  # the GET grows nothing
    check_padding(bs, bytes(3))
    bs.delete()


@pytest.mark.parametrize("mode", [M.SAT, M.FAIL])
def test_errors_leave_nothing_behind(client, fresh, mode):
    bs = client.getBitSet(fresh)
    vals = np.arange(256, dtype=np.int64)
    for last in (1 << 32, (1 << 32) - 7):
        offs = (np.arange(256) * 8).astype(np.uint64)
        offs[-1] = last
        for op in (M.SET, M.INCRBY):
            for run in (lambda: run_host(bs, op, True, 8, mode, offs, vals, True),
                        lambda: run_dev(client, bs, op, True, 8, mode, offs, vals, True),
                        lambda: raw_bitfield(client, fresh, [(op, True, 8, mode, 0, 1), (M.GET, False, 3, 0, 0, 0),
                                                             (op, True, 8, mode, last, 1)])):
                with pytest.raises(RedisException, match="bit offset is not an integer or out of range"):
                    run()
                assert not bs.isExists()
    # types: Redisson's limits on the batch, Redis's alone on the list
    with pytest.raises(IllegalArgumentException, match="greater than 63 bits"):
        bs.setFields(64, [0], [1], signed=False, overflow=MODE_NAMES[mode])
    for signed, size in ((False, 64), (True, 65), (True, 0)):
        with pytest.raises(RedisException, match="Invalid bitfield type"):
            raw_bitfield(client, fresh, [(M.SET, True, 8, mode, 0, 1), (M.SET, signed, size, mode, 0, 1)])
    # modes
    with pytest.raises(IllegalArgumentException, match="OVERFLOW"):
        bs.incrementFields(8, [0], [1], overflow="CLAMP")
    nm, _keep = L.name_struct(fresh)
    one_off, one_val = (C.c_uint64 * 1)(0), (C.c_int64 * 1)(1)
    rep, nil = (C.c_int64 * 1)(), (C.c_uint8 * 1)()
    lib = L.lib()
    for bad in (3, -1):
        assert lib.rbx_bitset_fields_ov(client.ctx, nm, M.INCRBY, 0, 8, bad, one_off, one_val, 1, rep, nil) == \
            L.RBX_E_ILLEGAL_ARGUMENT
        assert lib.rbx_bitset_fields_ov_dev(client.ctx, nm, M.INCRBY, 0, 8, bad, 8, 8, 1, None, None, None) == \
            L.RBX_E_ILLEGAL_ARGUMENT
    with pytest.raises(IllegalArgumentException, match="OVERFLOW"):
        raw_bitfield(client, fresh, [(M.SET, True, 8, 3, 0, 1), (M.GET, True, 8, 0, 0, 0)])
    # FAIL with replies needs nil; without replies, and under the other modes, it does not
    rc = lib.rbx_bitset_fields_ov(client.ctx, nm, M.INCRBY, 0, 8, M.FAIL, one_off, one_val, 1, rep, None)
    assert rc == L.RBX_E_ILLEGAL_ARGUMENT and "nil" in L.last_error()
    with pytest.raises(IllegalArgumentException, match="nil"):
        raw_bitfield(client, fresh, [(M.INCRBY, True, 8, M.FAIL, 0, 1), (M.GET, True, 4, 0, 0, 0)], with_nil=False)
    assert not bs.isExists()
    assert lib.rbx_bitset_fields_ov(client.ctx, nm, M.INCRBY, 0, 8, M.FAIL, one_off, one_val, 1, None, None) == L.RBX_OK
    assert lib.rbx_bitset_fields_ov(client.ctx, nm, M.INCRBY, 0, 8, M.SAT, one_off, one_val, 1, rep, None) == L.RBX_OK
    assert rep[0] == 2 and raw_bitfield(client, fresh, [(M.GET, False, 8, M.FAIL, 0, 0)], with_nil=False) == [2]
    bs.delete()
    # n = 0 sends nothing
    assert lib.rbx_bitset_fields_ov(client.ctx, nm, M.INCRBY, 0, 8, mode, None, None, 0, None, None) == L.RBX_OK
    assert lib.rbx_bitset_bitfield(client.ctx, nm, None, 0, None, None) == L.RBX_OK
    assert RedissonConnection(client).bitField(fresh.encode(), []) == []
    rep0, nil0 = bs.incrementFields(8, np.zeros(0, np.uint64), np.zeros(0, np.int64), overflow="FAIL")
    assert rep0.size == 0 and nil0.size == 0 and not bs.isExists()


def test_wrong_types_are_refused_unchanged(client, fresh):
    f = client.getBloomFilter(fresh + "F")
    assert f.tryInit(100, 0.03)
    hll = client.getHyperLogLog(fresh + "H")
    assert hll.addAll([b"a", b"b"])
    for bad in ("{" + fresh + "F}:config", fresh + "H"):
        bs = client.getBitSet(bad)
        for call in (lambda: bs.setFields(8, [0, 8], [1, 2], overflow="SAT"),
                     lambda: bs.incrementFields(8, [0, 8], [1, 2], replies=False, overflow="SAT"),
                     lambda: bs.incrementFields(8, [0, 3], [1, 2], overflow="FAIL"),
                     lambda: run_dev(client, bs, M.SET, True, 8, M.FAIL, [0, 8], [1, 2], True),
                     lambda: raw_bitfield(client, bad, [(M.SET, True, 8, M.SAT, 0, 1), (M.GET, False, 3, 0, 0, 0)]),
                     lambda: raw_bitfield(client, bad, [(M.GET, True, 8, 0, 0, 0), (M.GET, False, 3, 0, 0, 0)])):
            with pytest.raises(RedisException, match="WRONGTYPE"):
                call()
    assert f.getSize() == 729 and hll.count() == 2  # both still what they were
    f.delete()
    hll.delete()


def test_bloom_handle_sees_an_in_place_saturating_set(client, fresh):
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
    # an unsigned SET of -1 overflows upwards: SAT stores 255
    bs.setFields(8, [8 * b for b in range(92)], [-1] * 92, signed=False, replies=False, overflow="SAT")
    assert bs.toByteArray() == b"\xff" * 92
    d_cnt.zero_()
    torch.cuda.synchronize()
    h.contains_dev(device_keys(d_keys.data_ptr(), 1000, 16), d_cnt.data_ptr(), d_out.data_ptr())
    client.synchronize()
    assert d_cnt.item() == 1000 and d_out.cpu().numpy().all()
    h.close()
    f.delete()


# ---- 7. WRAP through the new entry answers as the old one ------------------------------------------
def wrap_pair(client, fresh, start, op, signed, size, offs, vals, replies):
    lib = L.lib()
    offs = np.ascontiguousarray(offs, np.uint64)
    vals = np.ascontiguousarray(vals, np.int64)
    out = []
    for tag in ("o", "n"):
        bs = client.getBitSet(fresh + tag)
        bs.setBytes(start)
        rep = np.full(len(offs), 77, np.int64) if replies else None
        nil = np.full(len(offs), 77, np.uint8)
        nm, _keep = L.name_struct(fresh + tag)
        args = (offs.ctypes.data_as(L.u64p), vals.ctypes.data_as(L.i64p), len(offs),
                None if rep is None else rep.ctypes.data_as(L.i64p))
        if tag == "o":
            _check(lib.rbx_bitset_fields(client.ctx, nm, op, int(signed), size, *args))
        else:
            _check(lib.rbx_bitset_fields_ov(client.ctx, nm, op, int(signed), size, M.WRAP, *args,
                                            nil.ctypes.data_as(L.u8p)))
            assert not nil.any()
        out.append((bs.toByteArray(), None if rep is None else rep.tolist()))
        bs.delete()
    assert out[0] == out[1], (op, signed, size)
    assert out[0][0] == M.fields(start, op, signed, size, M.WRAP, offs, vals)[0]


def test_wrap_equals_the_entry_without_a_mode(client, fresh):
    for size, signed in SAT_TYPES:
        for sign in (1, -1):
            offs, incs, _h, _l = sat_batch(size, signed, sign)
            wrap_pair(client, fresh, pattern(330), M.INCRBY, signed, size, offs, incs, False)
    rng = np.random.default_rng(77)
    for size, signed in TYPES:
        for op in (M.SET, M.INCRBY):
            offs = (rng.choice(32, 2000) * size).astype(np.uint64)
            wrap_pair(client, fresh, pattern(100), op, signed, size, offs, wide_values(rng, op, signed, size, 2000), True)


# ---- 8. mixed lists and RedissonConnection.bitField --------------------------------------------------
def random_list(rng, n):
    rows = []
    for _ in range(n):
        signed = bool(rng.integers(0, 2))
        size = int(rng.integers(1, 65 if signed else 64))
        op = int(rng.integers(0, 3))
        mode = int(rng.integers(0, 3))
        offset = int(rng.integers(0, 150))  # any alignment; some reach past the 16 bytes and grow the string
        lo, hi = M.bounds(signed, size)
        kind = int(rng.integers(0, 3))
        value = (int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64)) if kind == 0 else
                 int(rng.integers(-4, 5)) if kind == 1 else
                 max(I64_MIN, min(I64_MAX, [lo, hi, hi - lo, lo - hi, hi + 1, lo - 1][int(rng.integers(0, 6))])))
        rows.append((op, signed, size, mode, offset, value))
    return rows


def test_mixed_lists_against_the_model(client, fresh):
    rng = np.random.default_rng(0xB17F1E1D)
    bs = client.getBitSet(fresh)
    for k in range(200):
        rows = random_list(rng, int(rng.integers(1, 33)))
        start = b"" if k % 10 == 0 else rng.bytes(16)
        bs.delete()
        if start:
            bs.setBytes(start)
        want, want_rep = M.bitfield(start, rows)
        assert raw_bitfield(client, fresh, rows) == want_rep, (k, rows)
        assert bs.toByteArray() == want and bs.isExists() == (len(want) > 0), (k, rows)
        if want and k % 20 == 1:
            check_padding(bs, want)
    bs.delete()


@pytest.mark.parametrize("mode", [M.WRAP, M.SAT, M.FAIL])
def test_a_homogeneous_list_takes_the_batch_path(client, fresh, mode):
    rng = np.random.default_rng(mode)
    bs = client.getBitSet(fresh)
    offs = rng.choice(64, 4096) * 8
    vals = rng.integers(-40, 60, 4096)
    rows = [(M.INCRBY, False, 8, mode, int(o), int(v)) for o, v in zip(offs, vals)]
    bs.setBytes(pattern(100))
    want, want_rep = M.bitfield(pattern(100), rows)
    assert raw_bitfield(client, fresh, rows) == want_rep
    check_padding(bs, want)
    gets = [(M.GET, True, 8, int(m), int(o), 0) for o, m in zip(offs, rng.integers(0, 3, 4096))]  # GET ignores the mode
    assert raw_bitfield(client, fresh, gets) == M.bitfield(want, gets)[1]
    bs.delete()


def test_spring_data_bit_field(client, fresh):
    conn = RedissonConnection(client)
    key = fresh.encode()
    bs = client.getBitSet(fresh)
    u8, i5, u2 = BitFieldType(False, 8), BitFieldType(True, 5), BitFieldType(False, 2)
    # the reference appends OVERFLOW after the INCRBY that carries it: it governs what FOLLOWS
    assert conn.bitField(key, [BitFieldIncrBy(u8, 0, 200, "SAT"), BitFieldIncrBy(u8, 0, 100)]) == [200, 255]
    assert bs.toByteArray() == b"\xff"
    bs.delete()
    assert conn.bitField(key, [BitFieldIncrBy(u8, 0, 300, "SAT")]) == [44]  # alone, it runs under WRAP
    assert bs.toByteArray() == b"\x2c"
    assert conn.bitField(key, [BitFieldIncrBy(u8, 0, 1, "FAIL"), BitFieldSet(u8, 0, 256), BitFieldGet(u8, 0),
                               BitFieldIncrBy(u8, 0, 255, "SAT"), BitFieldIncrBy(u8, 0, 255),
                               BitFieldIncrBy(u8, 0, 1, "WRAP"), BitFieldIncrBy(u8, 0, 1)]) == \
        [45, None, 45, None, 255, 255, 0]
    assert bs.toByteArray() == b"\x00"
    # '#N' is N * bits
    assert conn.bitField(key, [BitFieldSet(i5, Offset(2, zero_based=False), -1), BitFieldGet(i5, 10),
                               BitFieldGet(u2, Offset(6, zero_based=False))]) == [0, -1, 3]
    assert bs.toByteArray() == b"\x00\x3e"
    assert conn.bit_field(key, [BitFieldGet(u8, 8)]) == [0x3e]
    # no size check before Redis's
    for bad in (BitFieldType(False, 64), BitFieldType(True, 65), BitFieldType(True, 0)):
        with pytest.raises(RedisException, match="Invalid bitfield type"):
            conn.bitField(key, [BitFieldGet(u8, 0), BitFieldGet(bad, 0)])
    with pytest.raises(RedisException, match="bit offset"):
        conn.bitField(key, [BitFieldSet(u8, 0, 9), BitFieldSet(u8, Offset(1 << 29, zero_based=False), 1)])
    assert bs.toByteArray() == b"\x00\x3e"
    bs.delete()
