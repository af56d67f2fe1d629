"""The ordered GETBIT / SETBIT stream over many keys on the GPU (rbx_bitset_stream[_dev],
bitstream_kernels.hip), RBatch and Spring Data's pipeline: every reply, every final string, and the existence
and timeout of every key are compared for equality with the model of bitstream_model.py, under the forced
one-lane path (bitstream_path 1) and the forced sorted path (2) wherever the path is not the point."""
import contextlib

import numpy as np
import pytest

import bitstream_model as M
from oracle import oracle as O
from redisson_amd import IllegalStateException, RedisException
from redisson_amd import _lib as L
from redisson_amd.client import _config_name, bitset_stream_call
from redisson_amd.spring_data import RedissonConnection

pytestmark = pytest.mark.gpu

G, S0, S1 = M.GETBIT, M.SETBIT0, M.SETBIT1
DEFAULTS = {"bitstream_path": 0, "bitstream_serial_max": 64, "bitstream_chunk": 1 << 25}
PATHS = [1, 2]


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            assert L.lib().rbx_tune(k.encode(), v) == 0


def run_host(client, names, key, op, idx, replies=True):
    rc, _msg, out = bitset_stream_call(client, names, key, op, idx, replies)
    return rc, (None if out is None else out.tolist())


def run_dev(client, names, key, op, idx, replies=True, stream=None):
    """the device form over torch tensors, enqueued on the context's stream"""
    import torch

    n = len(key)
    d_key = torch.from_numpy(np.asarray(key, np.uint32).view(np.int32).copy()).cuda()
    d_op = torch.from_numpy(np.asarray(op, np.uint8).copy()).cuda()
    d_idx = torch.from_numpy(np.asarray(idx, np.uint64).view(np.int64).copy()).cuda()
    d_rep = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda") if replies else None
    torch.cuda.synchronize()
    arr, _keep = L.names_array(names)
    rc = L.lib().rbx_bitset_stream_dev(client.ctx, arr, len(names), d_key.data_ptr(), d_op.data_ptr(), d_idx.data_ptr(), n,
                                       None if d_rep is None else d_rep.data_ptr(), stream)
    client.synchronize()
    return rc, (None if d_rep is None else d_rep.cpu().numpy()[:n].tolist())


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
        assert bs.isExists() == (want is not None), (name, where)


def check_batch(client, names, start, key, op, idx, path, form="host", wrong=(), replies=True, **knobs):
    """`start`: name -> bytes or None.  Runs the batch under the path and checks code, replies and strings
    against the model; returns the replies."""
    for name, data in start.items():
        put(client, name, data)
    model = M.StreamModel({k.encode(): v for k, v in start.items() if v is not None}, wrong=[w.encode() for w in wrong])
    want_rc, want = model.run([n.encode() for n in names], key, op, idx)
    with tuned(bitstream_path=path, **knobs):
        rc, got = RUNNERS[form](client, names, key, op, idx, replies)
    assert rc == want_rc, (path, form, L.last_error())
    if replies:
        assert got == want, (path, form)
    check_state(client, [n for n in names if n not in wrong], model, (path, form))
    return got


# ---- 1. one bit, in order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_one_bit_in_order(client, fresh, path):
    a = fresh + "a"
    got = check_batch(client, [a], {a: None}, [0] * 7, [G, S1, G, S1, S0, G, S1], [5] * 7, path)
    assert got == [0, 0, 1, 1, 1, 0, 0]
    bs = client.getBitSet(a)
    assert bs.get(5) is True and bs.size() == 8 and bs.toByteArray() == b"\x04"


# ---- 2. the key id is part of the group key; equal names are one key ---------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_same_index_on_two_keys_interleaved(client, fresh, path, form):
    a, b = fresh + "a", fresh + "b"
    names = [a, b, a]  # the third entry repeats the first key's bytes
    key = [0, 1, 2, 1, 0, 2, 1, 0, 1, 2]
    op = [S1, G, G, S1, S0, G, G, S1, S0, G]
    got = check_batch(client, names, {a: None, b: b"\x00\x00\x10"}, key, op, [19] * 10, path, form)
    assert got == [0, 1, 1, 1, 1, 0, 1, 0, 1, 1]


# ---- 3. 64 commands from distinct lanes on the bits of two adjacent words ---------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_shared_words(client, fresh, path):
    a = fresh + "w"
    rng = np.random.default_rng(303)
    idx = (32 + rng.permutation(64)).tolist()
    op = rng.integers(0, 3, 64).tolist()
    assert {G, S0, S1} == set(op)
    start = bytes([0xA5, 0x3C, 0xFF, 0x00] * 4)
    check_batch(client, [a], {a: start}, [0] * 64, op, idx, path)


# ---- 4. growth and creation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_growth_creation_and_timeout(client, fresh, path):
    new, ghost, slab, ttl = (fresh + s for s in ("new", "ghost", "slab", "ttl"))
    old = bytes(range(256))
    put(client, ttl, b"\x01")
    start = {new: None, ghost: None, slab: old, ttl: b"\x01"}
    names = [new, ghost, slab, ttl]
    key, op, idx = [0, 1, 1, 2, 2, 3, 3], [S0, G, G, S1, G, S1, G], [2400, 0, 99999, 1 << 20, 2047, 70, 7]
    for name, data in start.items():
        put(client, name, data)
    assert client.getBitSet(ttl).expire(1_000_000)
    model = M.StreamModel({k.encode(): v for k, v in start.items() if v is not None})
    want_rc, want = model.run([n.encode() for n in names], key, op, idx)
    with tuned(bitstream_path=path):
        rc, got = run_host(client, names, key, op, idx)
    assert (rc, got) == (want_rc, want) and rc == L.RBX_OK
    check_state(client, names, model)
    assert client.getBitSet(new).toByteArray() == bytes(301)
    assert not client.getBitSet(ghost).isExists()
    grown = client.getBitSet(slab).toByteArray()
    assert len(grown) == (1 << 17) + 1 and grown[:256] == old and grown[-1] == 0x80
    assert 0 < client.getBitSet(ttl).remainTimeToLive() <= 1_000_000
    assert client.getBitSet(ttl).toByteArray() == b"\x01" + bytes(7) + b"\x02"


@pytest.mark.parametrize("shape", ["one key", "stretches", "interleaved"])
def test_lengths_of_many_setbits_per_key(client, fresh, shape):
    """The summary pass folds a key's SETBIT indexes in lanes and waves before its atomicMax: ascending indexes
    (every command raises its key's maximum) on one key, on three keys in stretches and on three keys in turn;
    more commands than one grid-stride sweep of the pass (512 workgroups of 256)."""
    n = 140_000
    names = [fresh + s for s in "abc"]
    key = {"one key": [1] * n, "stretches": [(i // 1000) % 3 for i in range(n)],
           "interleaved": [i % 3 for i in range(n)]}[shape]
    idx = [3 * i + 5 for i in range(n)]
    op = [S0 if i % 5 == 0 else S1 for i in range(n)]
    check_batch(client, names, {nm: None for nm in names}, key, op, idx, 0)
    check_batch(client, names, {nm: None for nm in names}, key, [S1] * n, idx, 0, replies=False)


# ---- 5. failures ---------------------------------------------------------------------------------------------
def other_types(client, fresh):
    """a Bloom filter's {name}:config hash and an HLL, with what shows that neither was touched"""
    f = client.getBloomFilter(fresh + "x")
    assert f.tryInit(100, 0.03)
    h = client.getHyperLogLog(fresh + "hll")
    h.addAll([b"e%d" % i for i in range(50)])
    return _config_name(fresh + "x"), fresh + "hll", f, h, (f.getSize(), h.count(), h.exportString())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_failed_commands_fail_alone(client, fresh, path, form):
    cfg, hll, f, h, before = other_types(client, fresh)
    s, only = fresh + "s", fresh + "only"
    names = [s, cfg, hll, only]
    key = [0, 0, 3, 1, 2, 0, 0, 2]
    op = [S1, S1, S1, G, S1, G, G, G]
    idx = [3, 1 << 32, 1 << 32, 9, 9, 3, (1 << 32) - 1, 1 << 33]
    got = check_batch(client, names, {s: None, only: None}, key, op, idx, path, form, wrong=[cfg, hll])
    assert got == [0, 0xFF, 0xFF, 0xFF, 0xFF, 1, 0, 0xFF]
    assert "bit offset is not an integer or out of range" in L.last_error()
    assert not client.getBitSet(only).isExists() and client.getBitSet(s).toByteArray() == b"\x10"
    assert (f.getSize(), h.count(), h.exportString()) == before
    # the same commands with the wrong-type ones first: the first failure in array order decides the code
    order = [3, 4, 0, 1, 2, 5, 6, 7]
    with tuned(bitstream_path=path):
        rc, got2 = RUNNERS[form](client, names, [key[i] for i in order], [op[i] for i in order], [idx[i] for i in order])
    assert rc == L.RBX_E_WRONGTYPE and "WRONGTYPE" in L.last_error()
    assert got2 == [0xFF, 0xFF, 1, 0xFF, 0xFF, 1, 0, 0xFF]
    with tuned(bitstream_path=path):
        rc, _ = RUNNERS[form](client, names, [key[i] for i in range(8)], op, idx)
    assert rc == L.RBX_E_REDIS
    assert (f.getSize(), h.count(), h.exportString()) == before


@pytest.mark.parametrize("path", PATHS)
def test_the_last_offset_is_legal(client, fresh, path):
    a = fresh + "top"
    put(client, a, None)
    with tuned(bitstream_path=path):
        rc, got = run_host(client, [a], [0, 0, 0, 0], [G, S1, G, S0], [(1 << 32) - 1] * 4)
    assert rc == L.RBX_OK and got == [0, 0, 1, 1]
    bs = client.getBitSet(a)
    assert bs.size() == 1 << 32 and bs.cardinality() == 0
    bs.delete()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_caller_errors_change_nothing(client, fresh, form):
    a, b = fresh + "a", fresh + "b"
    put(client, a, b"\x0f")
    put(client, b, None)
    run = RUNNERS[form]
    for path in (0, 1, 2):
        with tuned(bitstream_path=path):
            assert run(client, [a, b], [1, 0, 2], [S1, S1, S1], [1, 2, 3])[0] == L.RBX_E_ILLEGAL_ARGUMENT  # cmd_key == nkeys
            assert run(client, [a, b], [1, 0, 1], [S1, S1, 3], [1, 2, 3])[0] == L.RBX_E_ILLEGAL_ARGUMENT  # cmd_op == 3
    assert client.getBitSet(a).toByteArray() == b"\x0f" and not client.getBitSet(b).isExists()
    assert run(client, [a, b], [], [], [])[0] == L.RBX_OK  # n == 0
    assert not client.getBitSet(b).isExists()


def test_null_arrays_are_the_callers_error(client, fresh):
    import torch

    b = fresh + "b"
    put(client, b, None)
    arr, _keep = L.names_array([b])
    key, op, idx = np.zeros(2, np.uint32), np.full(2, S1, np.uint8), np.array([1, 2], np.uint64)
    ptrs = [key.ctypes.data_as(L.u32p), op.ctypes.data_as(L.u8p), idx.ctypes.data_as(L.u64p)]
    d = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for missing in range(3):
        args = [None if i == missing else p for i, p in enumerate(ptrs)]
        assert L.lib().rbx_bitset_stream(client.ctx, arr, 1, *args, 2, None) == L.RBX_E_ILLEGAL_ARGUMENT
        dargs = [None if i == missing else d.data_ptr() for i in range(3)]
        assert L.lib().rbx_bitset_stream_dev(client.ctx, arr, 1, *dargs, 2, None, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_bitset_stream(client.ctx, None, 1, *ptrs, 2, None) == L.RBX_E_ILLEGAL_ARGUMENT
    assert L.lib().rbx_bitset_stream(client.ctx, arr, 1, None, None, None, 0, None) == L.RBX_OK
    assert not client.getBitSet(b).isExists()


# ---- 6. one long run among other commands ---------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_a_long_run_on_one_bit(client, fresh, path):
    a, b = fresh + "a", fresh + "b"
    rng = np.random.default_rng(606)
    key, op, idx = [], [], []
    for i in range(3000):
        key += [0, int(rng.integers(0, 2))]
        op += [[S1, G, S0, G][i % 4], int(rng.integers(0, 3))]
        idx += [4097, int(rng.integers(0, 50_000))]
    got = check_batch(client, [a, b], {a: b"\xff" * 600, b: None}, key, op, idx, path)
    assert got[0:8:2] == [1, 1, 1, 0]  # bit 4097 starts set: SET1, GET, SET0, GET


# ---- 7. chunk edges ---------------------------------------------------------------------------------------------
def test_chunk_edges(client, fresh):
    a, b = fresh + "a", fresh + "b"
    rng = np.random.default_rng(707)
    n = 2500
    key = rng.integers(0, 2, n).tolist()
    op = rng.integers(0, 3, n).tolist()
    idx = rng.integers(0, 300, n).tolist()
    for i in list(range(0, n, 7)) + list(range(990, 1010)) + list(range(1990, 2010)):  # one cell across both edges
        key[i], idx[i] = 1, 77
    start = {a: b"\x5a" * 20, b: None}
    chunked = check_batch(client, [a, b], start, key, op, idx, 2, bitstream_chunk=1000)
    whole = check_batch(client, [a, b], start, key, op, idx, 2)
    serial = check_batch(client, [a, b], start, key, op, idx, 1, bitstream_chunk=1000)
    assert chunked == whole == serial


# ---- 8. a seeded random batch ---------------------------------------------------------------------------------
NKEYS, NCMD, LOW = 16, 20_000, 1024


def random_commands(seed, n=NCMD, ops=(G, S0, S1)):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, NKEYS, n).tolist()
    op = rng.choice(ops, n).tolist()
    idx = rng.integers(0, LOW, n)
    far = rng.choice(n, 20, replace=False)
    idx[far] = rng.integers(LOW, (1 << 22) + 1, 20)
    return key, op, idx.tolist()


def random_keys(client, prefix):
    """16 keys: 4 missing, 12 random strings of 0 to 160 bytes, one with a timeout, one a Bloom filter's bitmap.
    -> names, the start strings, the filter"""
    rng = np.random.default_rng(808)
    names = [prefix + "k%d" % i for i in range(NKEYS)]
    start = {}
    for i, name in enumerate(names):
        start[name] = None if i % 4 == 3 else rng.bytes(int(rng.integers(0, 161)))
        put(client, name, start[name])
    assert client.getBitSet(names[5]).expire(1_000_000)
    f = client.getBloomFilter(names[9])
    f.delete()
    assert f.tryInit(150, 0.03)  # 1,095 bits: within the 160 bytes, and more than a batch of SETBIT 1s leaves set
    f.add([b"m%d" % i for i in range(60)])
    start[names[9]] = client.getBitSet(names[9]).toByteArray()
    assert len(start[names[9]]) > 0
    return names, start, f


def check_random(client, prefix, key, op, idx, path, form, replies=True):
    names, start, f = random_keys(client, prefix)
    model = M.StreamModel({k.encode(): v for k, v in start.items() if v is not None})
    want_rc, want = model.run([n.encode() for n in names], key, op, idx)
    with tuned(bitstream_path=path):
        rc, got = RUNNERS[form](client, names, key, op, idx, replies, **({"stream": client.stream()} if form == "dev" else {}))
    assert rc == want_rc == L.RBX_OK, (path, form)
    if replies:
        assert got == want, (path, form)
    check_state(client, names, model, (path, form))
    assert 0 < client.getBitSet(names[5]).remainTimeToLive() <= 1_000_000
    assert all(client.getBitSet(n).remainTimeToLive() == -1 for n in names if n != names[5] and n.encode() in model.strings)
    ones = sum(bin(b).count("1") for b in model.strings[names[9].encode()])
    assert ones < f.getSize()
    assert f.count() == O.lib().orc_bloom_count_estimate(ones, f.getSize(), f.getHashIterations())
    return got, model


def test_random_batch_input_has_the_collisions_it_is_meant_to():
    key, op, idx = random_commands(8)
    seen, repeats = set(), 0
    last_set1, set1_then_set0 = set(), set()
    for k, o, i in zip(key, op, idx):
        repeats += (k, i) in seen
        seen.add((k, i))
        if o == S1:
            last_set1.add((k, i))
        elif o == S0 and (k, i) in last_set1:
            set1_then_set0.add((k, i))
    assert sum(i >= LOW for i in idx) == 20 and max(idx) <= 1 << 22
    # pigeonhole: 19,980 commands on 16 x 1,024 cells address at least 3,596 cells again (the bound asked for is 3,576)
    assert repeats >= NCMD - 20 - NKEYS * LOW == 3596 >= 3576
    assert len(set1_then_set0) >= 100


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_random_batch(client, fresh, path, form):
    key, op, idx = random_commands(8)
    check_random(client, fresh, key, op, idx, path, form)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_fast_paths_match_the_model_and_the_one_lane(client, fresh, form):
    # gather: GETBITs only; scatter: SETBIT 1 only and no replies -- each under the auto rule and under path 1
    key, _, idx = random_commands(9)
    gets, sets = [G] * NCMD, [S1] * NCMD
    auto, _m = check_random(client, fresh + "g0", key, gets, idx, 0, form)
    lane, _m = check_random(client, fresh + "g1", key, gets, idx, 1, form)
    assert auto == lane and set(auto) == {0, 1}
    _, m0 = check_random(client, fresh + "s0", key, sets, idx, 0, form, replies=False)
    _, m1 = check_random(client, fresh + "s1", key, sets, idx, 1, form, replies=False)
    assert list(m0.strings.values()) == list(m1.strings.values()) and len(m0.strings) == NKEYS
    # SETBIT 0 only, without replies: the other scatter
    check_random(client, fresh + "c0", key, [S0] * NCMD, idx, 0, form, replies=False)


# ---- 9. equivalence with single calls ---------------------------------------------------------------------------
def test_equivalent_to_single_calls(client, fresh):
    key, op, idx = random_commands(10, 500)
    names, start, _f = random_keys(client, fresh + "s")
    twins, _start, _f2 = random_keys(client, fresh + "t")
    rc, got = run_host(client, names, key, op, idx)
    assert rc == L.RBX_OK
    sets = [client.getBitSet(t) for t in twins]
    singles = [int(sets[k].get(i) if o == G else sets[k].set(i, o == S1)) for k, o, i in zip(key, op, idx)]
    assert got == singles
    for name, twin in zip(names, twins):
        a, b = client.getBitSet(name), client.getBitSet(twin)
        assert a.toByteArray() == b.toByteArray() and a.isExists() == b.isExists()


# ---- 10. RBatch ---------------------------------------------------------------------------------------------
def test_rbatch(client, fresh):
    a, b, c = (fresh + s for s in "abc")
    put(client, a, b"\x80")
    put(client, b, None)
    put(client, c, b"\x00\xff")
    batch = client.createBatch()
    ba, bb, bc = batch.getBitSet(a), batch.getBitSet(b), batch.getBitSet(c)
    f = [ba.getAsync(0), bb.setAsync(12), bc.clearBitAsync(8), bb.getAsync(12),  # one call
         bb.setAsync(3), bb.cardinalityAsync(), bb.setAsync(4),                   # a count between two sets
         bc.setRangeAsync(0, 8), bc.sizeAsync(), ba.clearAsync(), ba.getAsync(0), bb.cardinalityAsync()]
    res = batch.execute()
    assert res.getResponses() == [True, False, True, True, False, 2, False, None, 16, None, False, 3]
    assert [x.get() for x in f] == res.getResponses()
    assert client.getBitSet(b).toByteArray() == b"\x18\x08" and client.getBitSet(c).toByteArray() == b"\xff\x7f"
    assert not client.getBitSet(a).isExists()
    with pytest.raises(IllegalStateException, match="Batch already executed!"):
        batch.execute()
    with pytest.raises(IllegalStateException, match="Batch already executed!"):
        ba.getAsync(1)


def test_rbatch_raises_the_first_error_after_every_command_ran(client, fresh):
    cfg, _hll, _f, _h, _before = other_types(client, fresh)
    a = fresh + "a"
    put(client, a, None)
    batch = client.createBatch()
    ba = batch.getBitSet(a)
    f0 = ba.setAsync(1)
    f1 = ba.setAsync(1 << 32)
    f2 = batch.getBitSet(cfg).getAsync(0)
    f3 = batch.getBitSet(cfg).cardinalityAsync()
    f4 = ba.setAsync(2)
    f5 = ba.cardinalityAsync()
    with pytest.raises(RedisException, match="bit offset is not an integer or out of range"):
        batch.execute()
    assert (f0.get(), f4.get(), f5.get()) == (False, False, 2)
    for fut, text in ((f1, "bit offset"), (f2, "WRONGTYPE"), (f3, "WRONGTYPE")):
        with pytest.raises(RedisException, match=text):
            fut.get()
    assert client.getBitSet(a).toByteArray() == b"\x60"


# ---- 11. Spring Data's pipeline ---------------------------------------------------------------------------------
def test_spring_data_pipeline(client, fresh):
    conn = RedissonConnection(client)

    def commands(c, a, b):
        return [c.setBit(a, 5, True), c.getBit(a, 5), c.setBit(b, 5, True), c.bitCount(a), c.setBit(a, 5, False),
                c.getBit(b, 5), c.getBit(a, 5), c.setBit(b, 900, False), c.bitCount(b), c.strLen(b), c.bitCount(b, 0, 0)]

    keys = [(fresh + s).encode() for s in ("pa", "pb", "qa", "qb")]
    for k in keys:
        put(client, k.decode(), b"\x01\x02" if k.endswith(b"b") else None)
    assert not conn.isPipelined() and conn.closePipeline() == []
    conn.openPipeline()
    assert conn.isPipelined()
    assert commands(conn, keys[0], keys[1]) == [None] * 11
    assert conn.isPipelined()
    piped = conn.closePipeline()
    assert not conn.isPipelined()
    plain = commands(conn, keys[2], keys[3])
    assert piped == plain == [False, True, False, 1, True, True, False, False, 3, 113, 2]
    for p, q in ((keys[0], keys[2]), (keys[1], keys[3])):
        assert client.getBitSet(p.decode()).toByteArray() == client.getBitSet(q.decode()).toByteArray()
