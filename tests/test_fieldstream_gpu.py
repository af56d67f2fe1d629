"""The ordered BITFIELD stream over many keys on the GPU (rbx_bitset_field_stream[_dev],
fieldstream_kernels.hip), RBatch's typed fields and Spring Data's pipeline: every reply, every status, every
final string and length, and the existence and timeout of every key are compared for equality with the model
of fieldstream_model.py, under the auto rule and each forced path (fieldstream_path 1 one lane, 2 sorted by
word, 3 sorted by key) wherever the path is not the point."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import fieldstream_model as M
from redisson_amd import RedisException
from redisson_amd import _lib as L
from redisson_amd.client import _config_name, _field_cmds_array
from redisson_amd.spring_data import BitFieldGet, BitFieldIncrBy, BitFieldSet, BitFieldType, RedissonConnection

pytestmark = pytest.mark.gpu

G, S, I = M.GET, M.SET, M.INCRBY
W, SAT, FAIL = M.WRAP, M.SAT, M.FAIL
DEFAULTS = {"fieldstream_path": 0, "fieldstream_serial_max": 64, "fieldstream_chunk": 1 << 25}
PATHS = [0, 1, 2, 3]
FORMS = ["host", "dev"]
SERIAL, WORDS, KEYS, GATHER, ATOMIC = 1, 2, 3, 4, 5  # rbx_bench_fieldstream_last_path


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0


def last_path() -> int:
    return L.lib().rbx_bench_fieldstream_last_path()


def run_host(client, names, key, cmds, replies=True, status=True, stream=None):
    n = len(key)
    k = np.asarray(key, np.uint32)
    arr = _field_cmds_array(list(cmds))
    rep = np.full(max(n, 1), 77, np.int64) if replies else None
    st = np.full(max(n, 1), 77, np.uint8) if status else None
    names_arr, _keep = L.names_array(names)
    rc = L.lib().rbx_bitset_field_stream(client.ctx, names_arr, len(names), k.ctypes.data_as(L.u32p), arr, n,
                                         rep.ctypes.data_as(L.i64p) if replies else None,
                                         st.ctypes.data_as(L.u8p) if status else None)
    return rc, (rep[:n].tolist() if replies else None), (st[:n].tolist() if status else None)


def run_dev(client, names, key, cmds, replies=True, status=True, stream=None):
    """the device form over torch tensors, enqueued on the context's stream"""
    import torch

    n = len(key)
    d_key = torch.from_numpy(np.asarray(key, np.uint32).view(np.int32).copy()).cuda()
    raw = np.frombuffer(bytes(_field_cmds_array(list(cmds))), np.uint8)[: 24 * max(n, 1)].copy()
    d_cmds = torch.from_numpy(raw).cuda()
    d_rep = torch.full((max(n, 1),), 77, dtype=torch.int64, device="cuda") if replies else None
    d_st = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda") if status else None
    torch.cuda.synchronize()
    arr, _keep = L.names_array(names)
    rc = L.lib().rbx_bitset_field_stream_dev(client.ctx, arr, len(names), d_key.data_ptr(), d_cmds.data_ptr(), n,
                                             None if d_rep is None else d_rep.data_ptr(),
                                             None if d_st is None else d_st.data_ptr(), stream)
    client.synchronize()
    return (rc, None if d_rep is None else d_rep.cpu().numpy()[:n].tolist(),
            None if d_st is None else d_st.cpu().numpy()[:n].tolist())


RUNNERS = {"host": run_host, "dev": run_dev}


def put(client, name: str, data):
    """the key holds `data` (None: it is missing)"""
    bs = client.getBitSet(name)
    bs.delete()
    if data is not None:
        bs.setBytes(bytes(data))


def check_state(client, names, model, where=None):
    for name in dict.fromkeys(names):
        bs = client.getBitSet(name)
        want = model.strings.get(name.encode())
        assert bs.toByteArray() == bytes(want or b""), (name, where)
        assert bs.size() == 8 * len(want or b""), (name, where)
        assert bs.isExists() == (want is not None), (name, where)


def check_batch(client, names, start, key, cmds, path, form="host", wrong=(), replies=True, **knobs):
    """`start`: name -> bytes or None.  Runs the batch under the path and checks code, replies, status and
    strings against the model; returns (replies, status)."""
    for name, data in start.items():
        put(client, name, data)
    model = M.FieldStreamModel({k.encode(): v for k, v in start.items() if v is not None}, wrong=[w.encode() for w in wrong])
    want_rc, want, want_st = model.run([n.encode() for n in names], key, cmds)
    with tuned(fieldstream_path=path, **knobs):
        rc, got, st = RUNNERS[form](client, names, key, cmds, replies)
    assert rc == want_rc, (path, form, L.last_error())
    if replies:
        assert got == want, (path, form)
    assert st == want_st, (path, form)
    check_state(client, [n for n in names if n not in wrong], model, (path, form))
    return got, st


# ---- 1. one field, in order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", [W, SAT, FAIL])
def test_one_field_in_order(client, fresh, path, mode):
    a = fresh + "a"
    cmds = [(S, 0, 8, mode, 8, 200), (I, 0, 8, mode, 8, 100), (G, 0, 8, mode, 8, 0), (I, 0, 8, mode, 8, -250)]
    got, st = check_batch(client, [a], {a: None}, [0] * 4, cmds, path)
    assert (got, st) == {W: ([0, 44, 44, 50], [0] * 4), SAT: ([0, 255, 255, 5], [0] * 4),
                         FAIL: ([0, 0, 200, 0], [0, 1, 0, 1])}[mode]


# ---- 2. the key id is part of the cell; equal names are one key -------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_same_offset_on_two_keys_interleaved(client, fresh, path, form):
    a, b = fresh + "a", fresh + "b"
    names = [a, b, a]  # the third entry repeats the first key's bytes
    key = [0, 1, 2, 1, 0, 2, 1, 0, 1, 2] * 8  # 80 commands: past the one lane's limit under the auto rule
    cmds = [((S, I, G, I)[i % 4], i % 2, 16, (W, SAT, FAIL)[i % 3], 16, 1000 * i - 30000) for i in range(80)]
    check_batch(client, names, {a: None, b: b"\x00\x00\x10\x01"}, key, cmds, path, form)
    if path == 0:
        assert last_path() == WORDS


# ---- 3. fields of several sizes sharing two words ---------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_fields_sharing_a_word(client, fresh, path):
    a = fresh + "w"
    rng = np.random.default_rng(303)
    cmds = []
    for _ in range(128):
        size = int(rng.choice([4, 8, 16, 32]))
        cmds.append((int(rng.integers(0, 3)), int(rng.integers(0, 2)), size, int(rng.integers(0, 3)),
                     size * int(rng.integers(0, 128 // size)), int(rng.integers(-70000, 70000))))
    check_batch(client, [a], {a: bytes([0xA5, 0x3C, 0xFF, 0x00] * 4)}, [0] * 128, cmds, path)
    if path in (0, 2):
        assert last_path() == WORDS


# ---- 4. word edges: a straddling field routes the auto rule to the key cells ---------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_word_edges_and_the_straddle(client, fresh, form):
    a, b = fresh + "a", fresh + "b"
    edge = [(I, 0, 8, W, 56, 3), (S, 1, 8, SAT, 64, -5), (G, 0, 16, W, 48, 0), (I, 1, 16, FAIL, 64, 40000)]
    straddle = [(S, 0, 8, W, 60, 0xAB), (G, 0, 8, W, 56, 0), (G, 0, 8, W, 64, 0), (I, 0, 8, SAT, 60, 100)]
    start = {a: bytes(range(1, 21)), b: None}
    answers = {}
    for label, tail in (("contained", edge), ("straddling", edge + straddle)):
        key = [i % 2 for i in range(96)] + [0] * len(tail)
        cmds = [((I, S, G)[i % 3], 0, 8, W, 8 * (i % 12), i) for i in range(96)] + tail
        for path in PATHS:
            answers[label, path] = check_batch(client, [a, b], start, key, cmds, path, form)
            if path in (0, 2):
                assert last_path() == (WORDS if label == "contained" else KEYS), (label, path)
        assert all(answers[label, p] == answers[label, 0] for p in PATHS)


# ---- 5. the allocation's edge (allocations are multiples of 256 bytes) ---------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_the_allocations_last_bit_growth_across_it_and_a_get_past_it(client, fresh, path):
    a = fresh + "a"
    start = {a: bytes(range(256))}
    # fields ending at bit 2047, the last of a 256-byte allocation: in place
    inside = [(I, 0, 16, W, 2032, 7), (S, 1, 64, W, 1984, -2), (G, 0, 1, W, 2047, 0), (I, 0, 63, SAT, 1985, 5)]
    check_batch(client, [a], start, [0] * 4, inside, path)
    assert len(client.getBitSet(a).toByteArray()) == 256
    # a GET wholly past the allocation reads zero and grows nothing
    got, _ = check_batch(client, [a], start, [0] * 3, [(G, 1, 64, W, 2048, 0), (G, 0, 13, W, 100_000, 0), (G, 0, 8, W, 2044, 0)], path)
    assert got == [0, 0, 0xF0] and len(client.getBitSet(a).toByteArray()) == 256
    # a field across the boundary grows the string by one byte; the old bytes stay
    check_batch(client, [a], start, [0] * 3, [(I, 0, 16, W, 2040, 0x0102), (G, 0, 8, W, 2048, 0), (S, 0, 5, FAIL, 2050, 99)], path)
    grown = client.getBitSet(a).toByteArray()
    assert len(grown) == 257 and grown[:255] == bytes(range(255)) and grown[255:] == b"\x00\x02"


# ---- 6. creation, growth and a kept timeout ---------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_growth_creation_and_timeout(client, fresh, path):
    new, ghost, slab, ttl = (fresh + s for s in ("new", "ghost", "slab", "ttl"))
    start = {new: None, ghost: None, slab: bytes(range(256)), ttl: b"\x01"}
    names = [new, ghost, slab, ttl]
    key = [0, 1, 1, 2, 2, 3, 3]
    cmds = [(I, 0, 8, W, 2400, 0), (G, 1, 32, W, 0, 0), (G, 0, 8, W, 99999, 0), (S, 1, 16, W, 32000, -1), (G, 0, 8, W, 2040, 0),
            (I, 0, 4, SAT, 68, 9), (G, 0, 8, W, 0, 0)]
    for name, data in start.items():
        put(client, name, data)
    assert client.getBitSet(ttl).expire(1_000_000)
    model = M.FieldStreamModel({k.encode(): v for k, v in start.items() if v is not None})
    want = model.run([n.encode() for n in names], key, cmds)
    with tuned(fieldstream_path=path):
        got = run_host(client, names, key, cmds)
    assert got == want and got[0] == L.RBX_OK
    check_state(client, names, model)
    assert client.getBitSet(new).toByteArray() == bytes(301)  # an INCRBY by 0 creates and grows
    assert not client.getBitSet(ghost).isExists()
    grown = client.getBitSet(slab).toByteArray()
    assert len(grown) == 4002 and grown[:256] == bytes(range(256)) and grown[-2:] == b"\xff\xff"
    assert 0 < client.getBitSet(ttl).remainTimeToLive() <= 1_000_000
    assert client.getBitSet(ttl).toByteArray() == b"\x01" + bytes(7) + b"\x09"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_a_nil_on_a_missing_key_leaves_the_sized_string(client, fresh, path, form):
    a = fresh + "a"
    got, st = check_batch(client, [a], {a: None}, [0], [(I, 0, 8, FAIL, 0, 300)], path, form)
    assert (got, st) == ([0], [1]) and client.getBitSet(a).toByteArray() == b"\x00"


# ---- 7. failures ---------------------------------------------------------------------------------------------
def other_types(client, fresh):
    """a Bloom filter's {name}:config hash and an HLL, with what shows that neither was touched"""
    f = client.getBloomFilter(fresh + "x")
    assert f.tryInit(100, 0.03)
    h = client.getHyperLogLog(fresh + "hll")
    h.addAll([b"e%d" % i for i in range(50)])
    return _config_name(fresh + "x"), fresh + "hll", f, h, (f.getSize(), h.count(), h.exportString())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_failed_commands_fail_alone_and_the_first_decides_the_code(client, fresh, path, form):
    cfg, hll, f, h, before = other_types(client, fresh)
    s, only = fresh + "s", fresh + "only"
    names = [s, cfg, hll, only]
    key = [0, 3, 3, 3, 1, 2, 0, 0, 3, 2]
    cmds = [(S, 0, 8, W, 0, 9), (S, 0, 64, W, 0, 1), (I, 1, 65, SAT, 0, 1), (S, 1, 0, W, 0, 1),  # u64, i65, size 0
            (G, 0, 8, W, 0, 0), (I, 0, 8, W, 0, 1),  # a config hash, an HLL
            (G, 0, 8, W, 0, 0), (S, 0, 16, W, (1 << 32) - 15, 1), (I, 0, 8, FAIL, 1 << 32, 1),  # past the limit
            (G, 0, 8, W, 1 << 32, 0)]  # past the limit on a key of another type: the offset is looked at first
    got, st = check_batch(client, names, {s: None, only: None}, key, cmds, path, form, wrong=[cfg, hll])
    assert st == [0, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0xFF, 0xFF, 0xFF] and got == [0] * 6 + [9, 0, 0, 0]
    assert "Invalid bitfield type" in L.last_error()
    assert not client.getBitSet(only).isExists() and client.getBitSet(s).toByteArray() == b"\x09"
    assert (f.getSize(), h.count(), h.exportString()) == before
    # each kind first in turn: the first failure in array order decides the code and the message
    for order, code, text in (([4, 1, 7], L.RBX_E_WRONGTYPE, "WRONGTYPE"), ([7, 4, 1], L.RBX_E_REDIS, "bit offset"),
                              ([0, 9, 5], L.RBX_E_REDIS, "bit offset"), ([3, 8, 5], L.RBX_E_REDIS, "Invalid bitfield type")):
        with tuned(fieldstream_path=path):
            rc, _rep, st = RUNNERS[form](client, names, [key[i] for i in order], [cmds[i] for i in order])
        assert rc == code and text in L.last_error(), order
        assert st == [0 if i == 0 else 0xFF for i in order]
    assert not client.getBitSet(only).isExists()
    assert (f.getSize(), h.count(), h.exportString()) == before


@pytest.mark.parametrize("path", PATHS)
def test_the_last_offset_is_legal(client, fresh, path):
    a = fresh + "top"
    put(client, a, None)
    top = 1 << 32
    cmds = [(G, 0, 8, W, top - 8, 0), (I, 0, 8, W, top - 8, 5), (G, 1, 64, W, top - 64, 0), (S, 0, 1, W, top - 1, 0),
            (G, 0, 63, W, top - 63, 0), (G, 0, 8, W, top - 7, 0)]
    with tuned(fieldstream_path=path):
        rc, got, st = run_host(client, [a], [0] * 6, cmds)
    assert rc == L.RBX_E_REDIS and got == [0, 5, 5, 1, 4, 0] and st == [0, 0, 0, 0, 0, 0xFF]
    bs = client.getBitSet(a)
    assert bs.size() == top and bs.cardinality() == 1
    bs.delete()


@pytest.mark.parametrize("form", FORMS)
def test_caller_errors_change_nothing(client, fresh, form):
    a, b = fresh + "a", fresh + "b"
    put(client, a, b"\x0f")
    put(client, b, None)
    run = RUNNERS[form]
    ok = (S, 0, 8, W, 0, 1)
    for path in PATHS:
        with tuned(fieldstream_path=path):
            for key, bad in (([1, 0, 2], ok), ([1, 0, 1], (3, 0, 8, W, 0, 1)), ([1, 0, 1], (S, 0, 8, 3, 0, 1)),
                             ([1, 0, 1], (S, 2, 8, W, 0, 1))):  # cmd_key == nkeys, op 3, overflow 3, is_signed 2
                assert run(client, [a, b], key, [ok, ok, bad])[0] == L.RBX_E_ILLEGAL_ARGUMENT, (path, key, bad)
            # OVERFLOW FAIL with replies needs status; without replies, or under another mode, it does not
            assert run(client, [a, b], [1, 1], [ok, (I, 0, 8, FAIL, 0, 1)], True, False)[0] == L.RBX_E_ILLEGAL_ARGUMENT
            assert "status" in L.last_error()
    assert client.getBitSet(a).toByteArray() == b"\x0f" and not client.getBitSet(b).isExists()
    assert run(client, [a, b], [1, 1], [ok, (I, 0, 8, FAIL, 0, 300)], False, False)[0] == L.RBX_OK
    assert run(client, [a, b], [1], [(I, 0, 8, SAT, 0, 300)], True, False)[:2] == (L.RBX_OK, [255])
    assert run(client, [a, b], [1], [(G, 0, 8, FAIL, 0, 0)], True, False)[:2] == (L.RBX_OK, [255])  # a GET has no mode
    assert client.getBitSet(b).toByteArray() == b"\xff"
    put(client, b, None)
    assert run(client, [a, b], [], [])[0] == L.RBX_OK  # n == 0
    assert not client.getBitSet(b).isExists()


def test_null_arrays_are_the_callers_error(client, fresh):
    import torch

    b = fresh + "b"
    put(client, b, None)
    arr, _keep = L.names_array([b])
    key = np.zeros(2, np.uint32)
    cmds = _field_cmds_array([(S, 0, 8, W, 0, 1)] * 2)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    lib = L.lib()
    assert lib.rbx_bitset_field_stream(client.ctx, arr, 1, None, cmds, 2, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_stream(client.ctx, arr, 1, key.ctypes.data_as(L.u32p), None, 2, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_stream(client.ctx, None, 1, key.ctypes.data_as(L.u32p), cmds, 2, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_stream_dev(client.ctx, arr, 1, None, d.data_ptr(), 2, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_stream_dev(client.ctx, arr, 1, d.data_ptr(), None, 2, None, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert lib.rbx_bitset_field_stream(client.ctx, arr, 1, None, None, 0, None, None) == L.RBX_OK
    assert not client.getBitSet(b).isExists()
    # replies == NULL and status == NULL are legal
    assert lib.rbx_bitset_field_stream(client.ctx, arr, 1, key.ctypes.data_as(L.u32p), cmds, 2, None, None) == L.RBX_OK
    assert client.getBitSet(b).toByteArray() == b"\x01"


# ---- 8. one long run among other commands ---------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_a_long_run_on_one_field(client, fresh, path):
    a, b = fresh + "a", fresh + "b"
    rng = np.random.default_rng(606)
    key, cmds = [], []
    for i in range(2048):
        key += [0, int(rng.integers(0, 2))]
        cmds += [((I, G, S, I)[i % 4], 1, 16, (W, SAT, FAIL)[i % 3], 4096, 20000 - 150 * (i % 300)),
                 (int(rng.integers(0, 3)), 0, 8, W, 8 * int(rng.integers(0, 400)), int(rng.integers(0, 256)))]
    assert len(cmds) == 4096
    _got, st = check_batch(client, [a, b], {a: b"\xff" * 600, b: None}, key, cmds, path)
    assert st.count(1) == 130  # the nils of the FAIL steps, worked out with the model on the CPU


# ---- 9. chunk edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("straddle", [False, True])
def test_chunk_edges(client, fresh, straddle):
    a, b = fresh + "a", fresh + "b"
    rng = np.random.default_rng(707)
    n = 200
    key = rng.integers(0, 2, n).tolist()
    cmds = [(int(rng.integers(0, 3)), 0, 8, int(rng.integers(0, 3)), 8 * int(rng.integers(0, 30)), int(rng.integers(-200, 200)))
            for _ in range(n)]
    for i in list(range(0, n, 7)) + list(range(60, 70)) + list(range(124, 132)):  # one cell across both chunk edges
        key[i], cmds[i] = 1, ((I, I, G, S)[i % 4], 0, 8, (W, SAT, FAIL)[i % 3], 72, 90 + i)
    if straddle:
        cmds[3] = (S, 0, 8, W, 60, 0x5A)
    start = {a: b"\x5a" * 20, b: None}
    chunked = check_batch(client, [a, b], start, key, cmds, 2, fieldstream_chunk=64)
    assert last_path() == (KEYS if straddle else WORDS)
    by_key = check_batch(client, [a, b], start, key, cmds, 3, fieldstream_chunk=64)
    whole = check_batch(client, [a, b], start, key, cmds, 2)
    serial = check_batch(client, [a, b], start, key, cmds, 1, fieldstream_chunk=64)
    assert chunked == by_key == whole == serial


# ---- 10. the compare-and-swap path ---------------------------------------------------------------------------
def atomic_batch(size, n=4096, nkeys=40, seed=1010):
    rng = np.random.default_rng(seed + size)
    key = rng.integers(0, nkeys, n).tolist()
    slots = rng.integers(0, 24, n)  # few slots per key: many duplicates
    lo, hi = -(1 << 62), 1 << 62
    cmds = [(I, int(size == 64 or rng.integers(0, 2)), size, W, size * int(s), int(rng.integers(lo, hi))) for s in slots]
    return key, cmds


@pytest.mark.parametrize("size", [8, 16, 64])
@pytest.mark.parametrize("form", FORMS)
def test_the_atomic_path_against_the_model_and_the_one_lane(client, fresh, size, form):
    names = [fresh + "k%d" % i for i in range(40)] + [fresh + "k0"]
    key, cmds = atomic_batch(size)
    key[5] = key[77] = 40  # the repeated name
    rng = np.random.default_rng(size)
    start = {nm: (None if i % 3 == 0 else rng.bytes(int(rng.integers(0, 300)))) for i, nm in enumerate(names[:40])}
    check_batch(client, names, start, key, cmds, 0, form, replies=False)
    assert last_path() == ATOMIC
    auto = {nm: client.getBitSet(nm).toByteArray() for nm in names}
    check_batch(client, names, start, key, cmds, 1, form, replies=False)
    assert last_path() == SERIAL and auto == {nm: client.getBitSet(nm).toByteArray() for nm in names}


@pytest.mark.parametrize("short", ["replies", "a SET", "a GET", "SAT", "FAIL", "two sizes", "unaligned", "size 5"])
def test_one_condition_short_of_the_atomic_path_is_still_exact(client, fresh, short):
    names = [fresh + "k%d" % i for i in range(40)]
    key, cmds = atomic_batch(8, n=1024)
    at = 517
    op, signed, size, mode, _offset, value = cmds[at]
    offset = 16  # inside the first word, whatever is added below
    if short == "size 5":  # u5 / i5 at multiples of 5: no divisor of 64 (the field at 60 straddles two words)
        cmds = [(o, sg, 5, m, off // 8 * 5, v) for o, sg, _sz, m, off, v in cmds]
    else:
        cmds[at] = {"replies": (op, signed, size, mode, offset, value), "a SET": (S, signed, size, mode, offset, value),
                    "a GET": (G, signed, size, mode, offset, 0), "SAT": (op, signed, size, SAT, offset, value),
                    "FAIL": (op, signed, size, FAIL, offset, value),
                    "two sizes": (op, signed, 16, mode, offset, value),  # a u16 over two of the u8 fields
                    "unaligned": (op, signed, size, mode, offset + 4, value)}[short]
    start = {nm: (None if i % 3 == 0 else bytes([i]) * 30) for i, nm in enumerate(names)}
    check_batch(client, names, start, key, cmds, 0, replies=(short == "replies"))
    assert last_path() == (KEYS if short == "size 5" else WORDS)


# ---- 11. the summary pass's per-key maxima ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one key", "stretches", "interleaved"])
def test_lengths_of_many_writes_per_key(client, fresh, shape):
    """The summary pass folds a key's field ends in lanes and waves before its atomicMax: ascending ends (every
    command raises its key's maximum) on one key, on three keys in stretches and on three keys in turn; more
    commands than one grid-stride sweep of the pass (512 workgroups of 256), so keys of up to 137 KiB.  The
    fields are pairwise distinct, so the expected strings are laid out directly."""
    n = 140_000
    names = [fresh + s for s in "abc"]
    key = np.array({"one key": [1] * n, "stretches": [(i // 1000) % 3 for i in range(n)],
                    "interleaved": [i % 3 for i in range(n)]}[shape], np.uint32)
    values = (np.arange(n) * 7 + 1) & 0xFF
    for nm in names:
        put(client, nm, None)
    cmds = (L.RbxFieldCmd * n)()
    raw = np.frombuffer(cmds, dtype=np.dtype([("offset", "<u8"), ("value", "<i8"), ("op", "u1"), ("is_signed", "u1"),
                                              ("size", "u1"), ("overflow", "u1"), ("pad", "u1", 4)]))
    raw["offset"], raw["value"], raw["op"], raw["size"] = np.arange(n) * 8, values, S, 8
    names_arr, _keep = L.names_array(names)
    rep = np.full(n, 77, np.int64)
    st = np.full(n, 77, np.uint8)
    for replies in (True, False):
        rc = L.lib().rbx_bitset_field_stream(client.ctx, names_arr, 3, key.ctypes.data_as(L.u32p), cmds, n,
                                             rep.ctypes.data_as(L.i64p) if replies else None, st.ctypes.data_as(L.u8p))
        assert rc == L.RBX_OK and last_path() == WORDS
        assert not st.any()
        if replies:
            assert not rep.any()  # the keys were missing: every SET replies the old value 0
        for k, nm in enumerate(names):
            mine = np.nonzero(key == k)[0]
            want = np.zeros(int(mine.max()) + 1 if mine.size else 0, np.uint8)
            want[mine] = values[mine]
            assert client.getBitSet(nm).toByteArray() == want.tobytes(), (shape, nm)
            assert client.getBitSet(nm).isExists() == bool(mine.size)
        rep[:] = 77
        st[:] = 77


# ---- 12. seeded random batches over seven keys ------------------------------------------------------------------
def random_keys(client, prefix):
    """the entries of M.KEYS: names, the start strings of the bit strings, the wrong-type names, and the Bloom
    filter and the HLL with what shows that their own state was not touched"""
    rng = np.random.default_rng(808)
    names = [prefix + k for k in M.KEYS]
    start = {names[0]: rng.bytes(40), names[1]: rng.bytes(100), names[2]: b"", names[3]: None, names[6]: None}
    for name, data in start.items():
        put(client, name, data)
    assert client.getBitSet(names[1]).expire(1_000_000)
    f = client.getBloomFilter(names[4])
    f.delete()
    assert f.tryInit(150, 0.03)
    f.add([b"m%d" % i for i in range(60)])
    start[names[4]] = client.getBitSet(names[4]).toByteArray()
    assert len(start[names[4]]) > 0
    h = client.getHyperLogLog(names[M.HLL])
    h.delete()
    h.addAll([b"e%d" % i for i in range(50)])
    return names, start, [names[M.HLL]], (f, h, (f.getSize(), f.getHashIterations(), h.count(), h.exportString()))


@pytest.mark.parametrize("contained", [False, True])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_random_batches(client, fresh, path, form, contained):
    for seed in M.SEEDS:
        key, cmds = M.random_batch(seed, contained)
        names, start, wrong, (f, h, before) = random_keys(client, fresh + "%d" % seed)
        model = M.FieldStreamModel({k.encode(): v for k, v in start.items() if v is not None}, wrong=[w.encode() for w in wrong])
        want = model.run([n.encode() for n in names], key, cmds)
        with tuned(fieldstream_path=path):
            got = RUNNERS[form](client, names, key, cmds, **({"stream": client.stream()} if form == "dev" else {}))
        assert got[0] == want[0] != L.RBX_OK, (seed, L.last_error())
        assert {"type": "Invalid bitfield type", "offset": "bit offset", "wrong": "WRONGTYPE"}[model.first_failure] in L.last_error()
        assert got[2] == want[2] and got[1] == want[1], seed
        if path in (0, 2):
            assert last_path() == (WORDS if contained else KEYS)
        check_state(client, [n for n in names if n not in wrong], model, (seed, path, form))
        assert not client.getBitSet(names[M.GHOST]).isExists()
        assert 0 < client.getBitSet(names[1]).remainTimeToLive() <= 1_000_000
        assert client.getBitSet(names[0]).remainTimeToLive() == -1
        assert (f.getSize(), f.getHashIterations(), h.count(), h.exportString()) == before


# ---- 13. equivalence with single calls ---------------------------------------------------------------------------
def test_equivalent_to_single_calls(client, fresh):
    """The same commands through rbx_bitset_bitfield, one sub-command per call, on a second set of keys: replies,
    nil, each command's code and message (so the order of the three checks), the first failure, and the strings."""
    key, cmds = M.random_batch(M.SEEDS[0], n=400)
    # the order of the checks, pinned: a bad type past the limit on a key of another type, and each pair
    key += [M.HLL] * 3 + [0]
    cmds += [(S, 0, 64, W, 1 << 32, 1), (S, 0, 8, W, 1 << 32, 1), (S, 0, 64, W, 0, 1), (S, 1, 65, W, (1 << 32) - 3, 1)]
    names, _start, _wrong, _x = random_keys(client, fresh + "s")
    twins, _start2, _wrong2, _y = random_keys(client, fresh + "t")
    rc, got, st = run_host(client, names, key, cmds)
    stream_msg = L.last_error()
    first = None
    for i, (k, cmd) in enumerate(zip(key, cmds)):
        nm, _keep = L.name_struct(twins[k].encode())
        reply, nil = C.c_int64(0), C.c_uint8(0)
        one = L.lib().rbx_bitset_bitfield(client.ctx, nm, _field_cmds_array([cmd]), 1, C.byref(reply), C.byref(nil))
        if one != L.RBX_OK:
            first = first or (one, L.last_error())
            assert st[i] == 0xFF and got[i] == 0, (i, cmd, L.last_error())
        else:
            assert (st[i], got[i]) == (nil.value, reply.value), (i, cmd)
    assert first is not None and (rc, stream_msg) == first
    for name, twin in zip(names, twins):
        if name.endswith("hll"):
            continue
        a, b = client.getBitSet(name), client.getBitSet(twin)
        assert a.toByteArray() == b.toByteArray() and a.isExists() == b.isExists()


# ---- 14. RBatch ---------------------------------------------------------------------------------------------
def test_rbatch_typed_fields(client, fresh):
    a, b = fresh + "u:1", fresh + "u:2"
    put(client, a, None)
    put(client, b, b"\x00\x00\x00\x07")
    batch = client.createBatch()
    ba, bb = batch.getBitSet(a), batch.getBitSet(b)
    f = [ba.incrementAndGetIntegerAsync(0, 1), bb.incrementAndGetIntegerAsync(0, 1), ba.setAsync(40), ba.getByteAsync(40),
         ba.incrementAndGetShortAsync(16, -2), ba.getIntegerAsync(0), bb.setUnsignedAsync(4, 4, 15), bb.getLongAsync(0),
         ba.getAsync(40), ba.incrementAndGetUnsignedAsync(3, 61, 9), ba.setSignedAsync(5, 59, -16),  # one call so far
         ba.cardinalityAsync(), ba.setLongAsync(64, -1), ba.getSignedAsync(64, 64), bb.setByteAsync(8, -128), bb.getShortAsync(0)]
    res = batch.execute()
    want = [1, 8, False, -128, -1, 0xFFFF, 0, 0x0F000008 << 32, True, 1, 1, 18, 0, -1, 0, 0x0F80]
    assert res.getResponses() == want and [x.get() for x in f] == want
    assert client.getBitSet(a).toByteArray() == bytes([0, 0, 0xFF, 0xFF, 0, 0x80, 0, 0x10]) + b"\xff" * 8
    assert client.getBitSet(b).toByteArray() == b"\x0f\x80\x00\x08"


def test_rbatch_raises_the_first_error_after_every_command_ran(client, fresh):
    cfg, _hll, _f, _h, _before = other_types(client, fresh)
    a = fresh + "a"
    put(client, a, None)
    batch = client.createBatch()
    ba = batch.getBitSet(a)
    f0 = ba.setByteAsync(0, 5)
    f1 = ba.incrementAndGetIntegerAsync(1 << 32, 1)
    f2 = batch.getBitSet(cfg).getByteAsync(0)
    f3 = ba.getUnsignedAsync(0, 0)
    f4 = ba.setAsync(1 << 32)
    f5 = ba.incrementAndGetByteAsync(0, 2)
    f6 = ba.cardinalityAsync()
    with pytest.raises(RedisException, match="bit offset is not an integer or out of range"):
        batch.execute()
    assert (f0.get(), f5.get(), f6.get()) == (0, 7, 3)
    for fut, text in ((f1, "bit offset"), (f2, "WRONGTYPE"), (f3, "Invalid bitfield type"), (f4, "bit offset")):
        with pytest.raises(RedisException, match=text):
            fut.get()
    assert client.getBitSet(a).toByteArray() == b"\x07"


# ---- 15. Spring Data's pipeline ---------------------------------------------------------------------------------
def test_spring_data_pipeline(client, fresh):
    conn = RedissonConnection(client)
    u8, i16 = BitFieldType(False, 8), BitFieldType(True, 16)

    def commands(c, a, b):
        return [c.bitField(a, [BitFieldIncrBy(u8, 0, 200)]), c.setBit(a, 9, True), c.bitField(b, [BitFieldSet(i16, 16, -2)]),
                c.bitField(a, [BitFieldGet(u8, 8)]), c.getBit(b, 16), c.bitField(a, [BitFieldIncrBy(u8, 0, 100, "FAIL")]),
                c.bitCount(a),  # splits the run
                c.bitField(a, [BitFieldIncrBy(u8, 0, 1, "FAIL"), BitFieldIncrBy(u8, 0, 250), BitFieldGet(u8, 0)]),  # a nil
                c.bitField(b, [BitFieldGet(i16, 16)]), c.strLen(b)]

    keys = [(fresh + s).encode() for s in ("pa", "pb", "qa", "qb")]
    for k in keys:
        put(client, k.decode(), b"\x01\x02" if k.endswith(b"b") else None)
    conn.openPipeline()
    assert commands(conn, keys[0], keys[1]) == [None] * 10
    piped = conn.closePipeline()
    plain = commands(conn, keys[2], keys[3])
    assert piped == plain == [[200], False, [0], [0x40], True, [44], 4, [45, None, 45], [-2], 4]
    for p, q in ((keys[0], keys[2]), (keys[1], keys[3])):
        assert client.getBitSet(p.decode()).toByteArray() == client.getBitSet(q.decode()).toByteArray()
    # a failing command fails alone; the first failure is raised after every command ran
    cfg = _config_name(fresh + "x")
    assert client.getBloomFilter(fresh + "x").tryInit(100, 0.03)
    conn.openPipeline()
    conn.bitField(keys[0], [BitFieldSet(u8, 0, 7)])
    conn.bitField(cfg.encode(), [BitFieldGet(u8, 0)])
    conn.bitField(keys[0], [BitFieldGet(BitFieldType(False, 64), 0)])
    conn.bitField(keys[0], [BitFieldIncrBy(u8, 0, 1)])
    with pytest.raises(RedisException, match="WRONGTYPE"):
        conn.closePipeline()
    assert client.getBitSet(keys[0].decode()).toByteArray()[:1] == b"\x08"
