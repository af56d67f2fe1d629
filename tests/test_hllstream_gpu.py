"""rbx_hll_stream on the GPU against hllstream_model: after every call the replies, the status bytes and the return
code, then every key's GET in the as-stored encoding (header included), its registers (the dense GET) and its TTL
state.  Unless a test says otherwise it runs under rbx_tune "hllstream_path" 0, 1 and 2, which must agree with the
model and so with each other."""
import ctypes as C

import numpy as np
import pytest

import hll_driver as D
import hll_elements as E
import hll_model as HM
import hllstream_model as M
from hll_model import BITS, BLOOM, WRONGTYPE, Keyspace
from hllstream_model import FAILED, NONE, PFADD, PFCOUNT
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WRONG_MSG = "WRONGTYPE Key is not a valid HyperLogLog string value."


@pytest.fixture(params=[0, 1, 2], ids=["auto", "rounds", "grouped"])
def path(request):
    from redisson_amd import _lib as L

    assert L.lib().rbx_tune(b"hllstream_path", request.param) == 0
    yield request.param
    assert L.lib().rbx_tune(b"hllstream_path", 0) == 0


def last():
    from redisson_amd import _lib as L

    out = (C.c_uint32 * 4)()
    assert L.lib().rbx_bench_hllstream_last(out) == 0
    return list(out)  # phases, runs by rounds, runs grouped, grouped chunks


def at(register, count, serial=1, length=16):
    return ("at", serial, ((register, count, length),))


class Engine:
    """the stream through librbx.so beside the model; keys are prefix + key, BITS is a bit string and BLOOM the
    {name}:config hash of a Bloom filter"""

    def __init__(self, client, prefix):
        self.client, self.prefix, self.ks = client, prefix, Keyspace()
        self.bits = client.getBitSet(self.name(BITS))
        self.bits.set(5, True)
        self.bloom = client.getBloomFilter(prefix + "bloom")
        assert self.bloom.tryInitRaw(3001, 5)

    def name(self, key) -> str:
        return "{%sbloom}:config" % self.prefix if key == BLOOM else self.prefix + key

    def hll(self, key):
        return self.client.getHyperLogLog(self.name(key))

    def apply(self, cmd):
        """a setup command of hll_driver's form on both sides"""
        getattr(self.ks, cmd[0])(*cmd[1:])
        if cmd[0] == "set":
            self.hll(cmd[2]).importString(cmd[3])
        elif cmd[0] == "expire":
            assert self.hll(cmd[2]).expire(D.TTL_MS)
        else:
            raise AssertionError(cmd)

    def arrays(self, cmds, names=None):
        names = list(dict.fromkeys(k for k, _, _ in cmds)) if names is None else names
        parts = [[bytes(r) for r in HM.materialize(spec)] for _k, _op, spec in cmds]
        seg = np.zeros(len(cmds) + 1, np.uint64)
        seg[1:] = np.cumsum([len(p) for p in parts])
        return names, [names.index(k) for k, _, _ in cmds], [op for _, op, _ in cmds], seg, [e for p in parts for e in p]

    def call(self, cmds, names=None, dev=False):
        from redisson_amd import _lib as L
        from redisson_amd import hll_stream_call

        names, key, op, seg, elements = self.arrays(cmds, names)
        real = [self.name(k) for k in names]
        if dev:
            return self.call_dev(real, key, op, seg, elements)
        rc, msg, replies, status = hll_stream_call(self.client, real, key, op, seg, elements)
        assert rc in (L.RBX_OK, L.RBX_E_WRONGTYPE) and (msg == WRONG_MSG) == (rc != L.RBX_OK), (rc, msg)
        return (WRONGTYPE if rc else None), [int(x) for x in replies], [int(x) for x in status]

    def call_dev(self, real, key, op, seg, elements):
        import torch

        from redisson_amd import _lib as L
        from redisson_amd import device_keys
        from redisson_amd.client import hll_stream_dev_call

        buf, offs = O.arena(elements)
        d_bytes = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        torch.cuda.synchronize()
        keys = device_keys(d_bytes.data_ptr(), len(elements), 0, d_offs.data_ptr())
        rc, msg, replies, status = hll_stream_dev_call(self.client, real, key, op, seg, keys)
        assert rc in (L.RBX_OK, L.RBX_E_WRONGTYPE) and (msg == WRONG_MSG) == (rc != L.RBX_OK), (rc, msg)
        return (WRONGTYPE if rc else None), [int(x) for x in replies], [int(x) for x in status]

    def run(self, cmds, names=None, dev=False):
        """one stream call on both sides, everything compared"""
        want = M.stream(self.ks, cmds)
        got = self.call(cmds, names, dev)
        assert got == want, D.first_difference(list(got), list(want))
        self.check()
        return got

    def check(self, keys=M.KEYS + ("z", "y", "x", "w", "v")):
        for key in keys:
            h, k = self.hll(key), self.ks.keys.get(key)
            if k is None:
                assert not h.isExists() and h.exportString("stored") == b"", key
                continue
            got, want = h.exportString("stored"), k.string()
            assert got == want, (key, D.first_difference(got, want))
            assert h.exportDense() == HM.header(0, k.card) + O.hll_dense_pack(k.h.regs), key
            t = h.remainTimeToLive()
            assert (0 < t <= D.TTL_MS) if k.ttl else t == -1, (key, t)
        assert self.bits.get(5) and self.bits.cardinality() == 1 and self.bloom.isExists()
        assert self.bloom.getSize() == 3001

    def close(self):
        for key in M.KEYS + ("z", "y", "x", "w", "v"):
            self.hll(key).delete()
        self.bits.delete()
        self.bloom.delete()


@pytest.fixture
def eng(client, fresh):
    e = Engine(client, fresh)
    yield e
    e.close()


# ---- one key, one register ---------------------------------------------------------------------------------------
def test_one_register_counts_in_order(eng, path):
    eng.run([("a", PFADD, NONE)])
    five = [at(9, c, i) for i, c in enumerate((3, 5, 4, 5, 6))]
    assert eng.run([("a", PFADD, s) for s in five])[1] == [1, 1, 0, 0, 1]
    assert eng.run([("b", PFADD, ("cat",) + tuple(five))])[1] == [1]
    assert eng.run([("c", PFADD, ("cat",) + tuple(five)), ("c", PFADD, ("cat",) + tuple(five))])[1] == [1, 0]
    same = at(700, 2, 77)
    assert eng.run([("d", PFADD, same), ("d", PFADD, same)])[1] == [1, 0]
    eng.run([("a", PFADD, at(9, 6, 5)), ("a", PFADD, at(9, 7, 6)), ("a", PFCOUNT, NONE)])


def test_a_run_of_equal_cells_crosses_workgroups(eng, path):
    eng.apply(("set", "obj", "b", HM.header(0, 5) + O.hll_dense_pack(np.zeros(HM.REGS, np.uint8))))
    rng = np.random.default_rng(3)
    counts = [int(c) for c in rng.choice((1, 2, 3, 4, 5, 6, 7, 9, 12, 40), size=1500)]
    counts.sort(key=lambda c: c + int(rng.integers(0, 6)))  # rising on the whole, with ties and dips
    got = eng.run([("b", PFADD, at(4000, c, i)) for i, c in enumerate(counts)])
    assert 3 <= sum(got[1]) <= 40
    two = [("b", PFADD, at(8190 + (i & 1), 1 + (i * 5) % 11 + i // 90, i)) for i in range(1200)]
    assert sum(eng.run(two)[1]) >= 4


def test_key_counts_equal_names_and_interleaving(eng, path):
    keys = ("a", "b", "c", "d", "e")
    for n in (1, 2, 3, 5):
        cmds = [(keys[i % n], PFADD, ("low", 100 * n + i, 3)) for i in range(4 * n + 3)]
        cmds += [(keys[i % n], PFCOUNT, NONE) for i in range(n)]
        eng.run(cmds, names=list(keys[:n]))
    # two equal names are one key: the commands alternate between the two entries
    from redisson_amd import hll_stream_call

    specs = [at(50 + i % 3, 1 + i % 4, i) for i in range(10)]
    want = M.stream(eng.ks, [("a", PFADD, s) for s in specs] + [("a", PFCOUNT, NONE)])
    elements = [HM.materialize(s)[0] for s in specs]
    rc, _msg, replies, status = hll_stream_call(eng.client, [eng.name("a"), eng.name("b"), eng.name("a")],
                                                [0, 2] * 5 + [2], [PFADD] * 10 + [PFCOUNT], list(range(11)) + [10], elements)
    assert (rc, [int(x) for x in replies], [int(x) for x in status]) == (0, want[1], want[2])
    eng.check()


def test_empty_adds_missing_counts_and_phases(eng, path):
    assert eng.run([("z", PFCOUNT, NONE), ("a", PFADD, NONE), ("a", PFADD, NONE), ("y", PFCOUNT, NONE)])[1] == [0, 1, 0, 0]
    assert last()[0] == 1
    eng.run([("a", PFADD, at(4, 2)), ("a", PFCOUNT, NONE), ("a", PFADD, at(5, 2)), ("a", PFCOUNT, NONE), ("a", PFADD, at(6, 1))])
    assert last()[0] == 3  # the leading add, then one phase per (count, add) pair
    keys = ("a", "b", "c", "d", "e")
    eng.run([(k, PFADD, ("low", 7 + i, 2)) for i, k in enumerate(keys * 2)] + [(k, PFCOUNT, NONE) for k in keys])
    assert last()[0] == 2


def test_count_add_count_on_one_key(eng, path):
    """A phase ends before a PFCOUNT that names a key an earlier PFADD of the phase names, and a count reads the
    state before its phase: a count and the add after it share a phase, so count, add, count on one key is two
    phases (a count pass, an add run, a count pass); three (count, add) pairs after a leading add are four."""
    eng.run([("a", PFADD, at(1, 1))])
    assert eng.run([("a", PFCOUNT, NONE), ("a", PFADD, at(3, 2)), ("a", PFCOUNT, NONE)])[1] == [1, 1, 2]
    assert last()[0] == len(M.phases([("a", PFCOUNT, NONE), ("a", PFADD, NONE), ("a", PFCOUNT, NONE)])) == 2
    eng.run([("a", PFADD, at(2, 1)), ("a", PFCOUNT, NONE), ("a", PFADD, at(7, 1)), ("a", PFCOUNT, NONE), ("a", PFADD, NONE),
             ("a", PFCOUNT, NONE)])
    assert last()[0] == 4


def test_the_cached_cardinality(eng, path):
    eng.apply(("set", "obj", "a", HM.header(1, 4321) + bytes([0x7F, 0xFF])))  # valid and wrong
    assert eng.run([("a", PFCOUNT, NONE), ("a", PFADD, NONE), ("a", PFCOUNT, NONE)])[1] == [4321, 0, 4321]
    assert eng.run([("a", PFADD, at(8, 2)), ("a", PFADD, at(8, 2, 2)), ("a", PFADD, at(8, 1, 3))])[1] == [1, 0, 0]
    assert eng.ks.keys["a"].card == HM.INVALID | 4321
    assert eng.run([("a", PFCOUNT, NONE), ("a", PFADD, at(8, 2, 4)), ("a", PFCOUNT, NONE)])[1] == [1, 0, 1]
    assert eng.ks.keys["a"].card == 1


# ---- sparse strings ----------------------------------------------------------------------------------------------
def test_promotion_by_value_in_the_middle_command(eng, path):
    cmds = [("a", PFADD, ("low", 1, 5)), ("b", PFADD, ("low", 2, 5)), ("a", PFADD, at(100, 33)), ("b", PFADD, ("low", 3, 5)),
            ("a", PFADD, ("low", 4, 6)), ("a", PFADD, at(101, 2, 9)), ("a", PFCOUNT, NONE)]
    eng.run(cmds)
    assert eng.ks.keys["a"].dense and not eng.ks.keys["b"].dense
    eng.run([("a", PFADD, ("low", 5, 6)), ("b", PFADD, at(5, 40)), ("b", PFADD, ("low", 6, 3))])
    assert eng.ks.keys["b"].dense


def test_promotion_by_bytes(eng, path):
    eng.run([("a", PFADD, ("rows", 1, 300)), ("b", PFADD, ("low", 1, 4)), ("a", PFADD, ("rows", 2, 300))])
    assert not eng.ks.keys["a"].dense
    eng.run([("a", PFADD, ("rows", 3, 400)), ("b", PFADD, ("low", 2, 4)), ("a", PFADD, ("rows", 4, 400)),
             ("a", PFADD, ("rows", 5, 400)), ("a", PFADD, ("low", 9, 4))])  # 1,800 elements: past 3,000 bytes in command 2
    assert eng.ks.keys["a"].dense and not eng.ks.keys["b"].dense


def test_a_string_that_is_not_normalized_is_replayed_across_commands(eng, path):
    eng.apply(("set", "obj", "c", D.odd_string(2)))
    regs = [40, 47, 41, 46, 42, 45, 43, 44, 48, 39, 38, 49]
    parts = [("at", 10 + i, tuple((r, 2, 16) for r in regs[3 * i:3 * i + 3])) for i in range(4)]
    cmds = []
    for i, p in enumerate(parts):
        cmds += [("c", PFADD, p), ("a", PFADD, ("low", 30 + i, 3))]
    events = []
    M.stream(M.copy_keyspace(eng.ks), cmds, events)
    assert sum(ev.count(("replay",)) for ev in events) >= 4  # element by element, not the shortcut
    eng.run(cmds)
    eng.run([("c", PFADD, ("at", 20, tuple((r, 3, 16) for r in regs[::2]))), ("c", PFCOUNT, NONE)])
    # a fresh key whose final registers hold a run longer than 4: replayed too, in command order
    eng.run([("d", PFADD, ("at", 21 + i, ((600 + r, 1, 16),))) for i, r in enumerate((3, 0, 5, 1, 4, 2, 6))])


# ---- failures --------------------------------------------------------------------------------------------------------
def test_wrong_type_commands_fail_alone(eng, path):
    cmds = [("a", PFADD, at(1, 1)), (BITS, PFADD, at(2, 2)), ("z", PFCOUNT, NONE), (BLOOM, PFCOUNT, NONE), (BITS, PFCOUNT, NONE),
            (BLOOM, PFADD, ("low", 1, 3)), ("a", PFADD, at(1, 2, 2)), ("a", PFCOUNT, NONE), (BLOOM, PFADD, NONE)]
    got = eng.run(cmds)
    assert got == (WRONGTYPE, [1, 0, 0, 0, 0, 0, 1, 1, 0], [0, FAILED, 0, FAILED, FAILED, FAILED, 0, 0, FAILED])
    assert eng.run([(BLOOM, PFADD, at(1, 1)), ("b", PFADD, NONE)])[0] == WRONGTYPE
    assert eng.run([(BITS, PFCOUNT, NONE)]) == (WRONGTYPE, [0], [FAILED])


def test_caller_errors_change_nothing(eng, path):
    from redisson_amd import Arena
    from redisson_amd import _lib as L

    eng.run([("a", PFADD, at(1, 1))])
    lib, ctx = L.lib(), eng.client.ctx
    names, _keep = L.names_array([eng.name("a"), eng.name("z")])
    elems = [E.element(5, 2), E.element(6, 2)]
    arena = Arena(elems)

    def call(key, op, seg, n=None, nkeys=2, arrays=(True, True, True), elements=arena):
        k, o, s = np.array(key, np.uint32), np.array(op, np.uint8), np.array(seg, np.uint64)
        replies, status = np.full(len(key) + 1, 7, np.uint64), np.full(len(key) + 1, 7, np.uint8)
        rc = lib.rbx_hll_stream(ctx, names, nkeys, k.ctypes.data_as(L.u32p) if arrays[0] else None,
                                o.ctypes.data_as(L.u8p) if arrays[1] else None, s.ctypes.data_as(L.u64p) if arrays[2] else None,
                                len(key) if n is None else n, elements.ptr() if elements is not None else None,
                                replies.ctypes.data_as(L.u64p), status.ctypes.data_as(L.u8p))
        return rc

    bad = [call([0, 2], [0, 0], [0, 1, 2]), call([0, 1], [0, 2], [0, 1, 2]), call([1, 1], [0, 0], [0, 2, 1]),
           call([1, 1], [0, 0], [0, 1, 1]), call([1, 1], [0, 0], [1, 1, 2]), call([1, 0], [0, 1], [0, 1, 2]),
           call([1, 1], [0, 0], [0, 1, 2], arrays=(False, True, True)), call([1, 1], [0, 0], [0, 1, 2], arrays=(True, False, True)),
           call([1, 1], [0, 0], [0, 1, 2], arrays=(True, True, False)), call([1, 1], [0, 0], [0, 1, 2], elements=None),
           call([1], [0], [0, 2], nkeys=1)]
    assert bad == [L.RBX_E_ILLEGAL_ARGUMENT] * len(bad)
    assert call([], [], [0], n=0, arrays=(False, False, False), elements=None) == L.RBX_OK  # n = 0 sends nothing
    eng.check()
    assert call([1, 1, 0], [0, 0, 1], [0, 1, 2, 2]) == L.RBX_OK  # and the same arrays in order run
    M.stream(eng.ks, [("z", PFADD, ("lit", (elems[0],))), ("z", PFADD, ("lit", (elems[1],))), ("a", PFCOUNT, NONE)])
    eng.check()


# ---- chunks, the device form ---------------------------------------------------------------------------------------
def test_chunks_of_256_elements_and_a_command_larger_than_a_chunk(eng):
    from redisson_amd import _lib as L

    assert L.lib().rbx_tune(b"hllstream_path", 2) == 0 and L.lib().rbx_tune(b"hllstream_chunk", 256) == 0
    try:
        cmds = []
        for i in range(12):  # 12 x 60 elements of key a with others between: three chunks of four commands
            cmds += [("a", PFADD, ("rows", 50 + i, 50)), ("b", PFADD, ("low", 80 + i, 10))]
        eng.run(cmds)
        assert last() == [1, 0, 1, 3]
        eng.run([("a", PFADD, ("rows", 70, 100)), ("c", PFADD, ("rows", 71, 1000)), ("a", PFADD, ("rows", 72, 100)),
                 ("c", PFADD, ("low", 73, 5)), ("c", PFCOUNT, NONE)])
        assert last() == [2, 0, 1, 2]  # the 1,000-element command went alone, by rounds, between two chunks
    finally:
        assert L.lib().rbx_tune(b"hllstream_path", 0) == 0 and L.lib().rbx_tune(b"hllstream_chunk", 1 << 25) == 0


def test_the_device_form_answers_as_the_host_form(eng, path):
    eng.apply(("set", "obj", "c", D.odd_string(4)))
    cmds = [("a", PFADD, ("low", 1, 4)), ("c", PFADD, ("crafted", 2, 5)), ("a", PFCOUNT, NONE), ("b", PFADD, NONE),
            ("a", PFADD, ("var", 3, 6)), ("c", PFADD, ("rows", 4, 3)), ("c", PFCOUNT, NONE), ("z", PFCOUNT, NONE)]
    eng.run(cmds, dev=True)
    eng.run(cmds + [(BITS, PFADD, at(1, 1))], dev=True)


# ---- seeded random streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", M.SEEDS)
def test_seeded_streams(eng, path, seed):
    for cmd in M.setup(seed):
        eng.apply(cmd)
    for cmds in M.seeded(seed):
        eng.run(cmds)


# ---- RBatch and the Spring Data pipeline against the engine ----------------------------------------------------------
def mixed(seed, n=300):
    """n commands over 5 keys: ('add', key, elements) / ('count', key) / ('merge', key, other) / ('bit', key)"""
    rng = np.random.default_rng([0xBA7C, seed])
    out = []
    for i in range(n):
        r, key = rng.random(), "abcde"[int(rng.integers(0, 5))]
        if r < 0.6:
            out.append(("add", key, tuple(E.element(int(rng.integers(0, 40)), int(rng.integers(1, 5)), 16, rng)
                                          for _ in range(int(rng.integers(0, 4))))))
        elif r < 0.9:
            out.append(("count", key))
        elif r < 0.95:
            out.append(("merge", key, "abcde"[int(rng.integers(0, 5))]))
        else:
            out.append(("bit", key))
    return out


def model_responses(ks, cmds):
    want, runs, prev = [], 0, None
    for c in cmds:
        if c[0] == "add":
            want.append(bool(ks.pfadd("obj", c[1], ("lit", c[2]))[0]))
        elif c[0] == "count":
            want.append(ks.pfcount("obj", c[1])[0])
        elif c[0] == "merge":
            want.append(ks.pfmerge("obj", c[1], (c[2],))[0])
        else:
            want.append(False)
        runs += c[0] in ("add", "count") and prev not in ("add", "count")
        prev = c[0]
    return want, runs


def test_rbatch_against_the_engine(eng):
    from redisson_amd import ByteArrayCodec, RBatch
    from redisson_amd.client import hll_stream_call

    cmds = mixed(1)
    want, runs = model_responses(eng.ks, cmds)
    calls = []

    def counted(*a):
        calls.append(len(a[1]))
        out = hll_stream_call(eng.client, *a)
        assert last()[0] >= 1
        return out

    b = RBatch(eng.client, hll_stream_call=counted)
    for c in cmds:
        h = b.getHyperLogLog(eng.name(c[1]), ByteArrayCodec())
        if c[0] == "add":
            h.addAllAsync(list(c[2]))
        elif c[0] == "count":
            h.countAsync()
        elif c[0] == "merge":
            h.mergeWithAsync(eng.name(c[2]))
        else:
            b.getBitSet(eng.name("bitsonly")).getAsync(3)
    assert b.execute().getResponses() == want
    assert len(calls) == runs and sum(calls) == sum(c[0] in ("add", "count") for c in cmds)
    eng.check()


def test_the_spring_data_pipeline_against_the_engine(eng, monkeypatch):
    import redisson_amd.spring_data as S

    cmds = mixed(2)
    want, runs = model_responses(eng.ks, cmds)
    calls = []
    real = S.hll_stream_call
    monkeypatch.setattr(S, "hll_stream_call", lambda *a: calls.append(len(a[2])) or real(*a))
    conn = S.RedissonConnection(eng.client)
    conn.openPipeline()
    for c in cmds:
        key = eng.name(c[1]).encode()
        if c[0] == "add":
            conn.pfAdd(key, *c[2])
        elif c[0] == "count":
            conn.pfCount(key)
        elif c[0] == "merge":
            conn.pfMerge(key, eng.name(c[2]).encode())
        else:
            conn.getBit(eng.name("bitsonly").encode(), 3)
    got = conn.closePipeline()
    assert got == [int(w) if isinstance(w, bool) and c[0] == "add" else w for w, c in zip(want, cmds)]
    assert len(calls) == runs
    eng.check()
