"""rbx_bitset_op_groups on the GPU against bitgroups_model: after every call the return code, the message, lens,
counts and status, then every touched key's bytes (toByteArray), existence and TTL state, and the phase count
through rbx_bench_bitgroups_last.  Every test runs under rbx_tune "bitgroups_tile" auto, 4096 and 65536, which must
agree with the model and so with each other."""
import ctypes as C

import numpy as np
import pytest

import bitgroups_driver as D
import bitgroups_model as M
from bitgroups_model import AND, NOT, OR, XOR

pytestmark = pytest.mark.gpu

T = D.T
LENGTHS = D.LENGTHS
HLL, CFG = "hll", "cfg"  # the two keys of another type
TTL_MS = 3_600_000


@pytest.fixture(params=[0, 4096, 65536], ids=["auto", "T4096", "T65536"])
def tile(request):
    from redisson_amd import _lib as L

    assert L.lib().rbx_tune(b"bitgroups_tile", request.param) == 0
    yield request.param
    assert L.lib().rbx_tune(b"bitgroups_tile", 0) == 0


def last():
    from redisson_amd import _lib as L

    out = (C.c_uint32 * 4)()
    assert L.lib().rbx_bench_bitgroups_last(out) == 0
    return list(out)  # phases, launches, tile of the last launch, groups on the device


def data(seed, n) -> bytes:
    return np.random.default_rng([0xB175, seed]).bytes(n)


class Engine:
    """the grouped call through librbx.so beside the model; keys are prefix + key, HLL is an HLL and CFG the
    {name}:config hash of a Bloom filter"""

    def __init__(self, client, prefix):
        self.client, self.prefix, self.ks = client, prefix, M.Keyspace()
        self.touched = set()
        assert client.getHyperLogLog(self.name(HLL)).add("x")
        self.bloom = client.getBloomFilter(prefix + "bloom")
        assert self.bloom.tryInitRaw(3001, 5)
        self.ks.hll |= {HLL, CFG}

    def name(self, key) -> str:
        return "{%sbloom}:config" % self.prefix if key == CFG else self.prefix + key

    def bitset(self, key):
        self.touched.add(key)
        return self.client.getBitSet(self.name(key))

    def set(self, key, value: bytes, timeout=False):
        """SET key value (b"": DEL), then a timeout"""
        if value:
            self.bitset(key).setBytes(value)
            self.ks._put(key, value, "set")
        else:
            self.bitset(key).delete()
            self.ks._put(key, None)
        if timeout and value:
            assert self.bitset(key).expire(TTL_MS)
            self.ks.timeout.add(key)

    def check(self, keys=None):
        for key in sorted(self.touched if keys is None else keys):
            b = self.client.getBitSet(self.name(key))
            want = self.ks.data.get(key, b"")
            got = b.toByteArray()
            assert got == want, (key, len(got), len(want), first_difference(got, want))
            ttl = b.remainTimeToLive()
            state = "missing" if ttl == -2 else "none" if ttl == -1 else "set"
            assert state == self.ks.ttl("conn", key)[0], (key, ttl)
            assert b.isExists() == (key in self.ks.data), key

    def call(self, names, ops, dests, groups, check=None):
        """one rbx_bitset_op_groups call on both sides, everything compared, the phase count too; names: keys"""
        from redisson_amd import _lib as L
        from redisson_amd import bitset_op_groups_call

        self.touched.update(k for k in names if k not in (HLL, CFG))
        phases = M.expected_phases(self.ks, names, ops, dests, groups)
        want = M.apply_groups(self.ks, names, ops, dests, groups)
        rc, msg, lens, counts, status = bitset_op_groups_call(self.client, [self.name(k) for k in names], ops, dests,
                                                              groups)
        code = {L.RBX_OK: M.OK, L.RBX_E_WRONGTYPE: M.E_WRONGTYPE, L.RBX_E_REDIS: M.E_REDIS,
                L.RBX_E_ILLEGAL_ARGUMENT: M.E_ILLEGAL_ARGUMENT}[rc]
        assert code == want[0], (rc, msg, want[0])
        if code != M.E_ILLEGAL_ARGUMENT:
            assert msg == M.message(code), msg
            got = ([int(x) for x in lens], [int(x) for x in counts], [int(x) for x in status])
            for what, g, w in zip(("lens", "counts", "status"), got, want[1:]):
                assert g == w, (what, first_difference(g, w))
            assert last()[0] == phases, (last(), phases)
        self.check(check)
        return want

    def cleanup(self):
        for key in self.touched:
            self.client.getBitSet(self.name(key)).delete()
        self.client.getHyperLogLog(self.name(HLL)).delete()
        self.bloom.delete()


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), None, None


@pytest.fixture
def eng(client, fresh, tile):
    e = Engine(client, fresh)
    yield e
    e.cleanup()


def length_keys(eng):
    """one key per length of LENGTHS: L0 (missing) .. L11 (3T + 5 bytes)"""
    keys = ["L%d" % i for i in range(len(LENGTHS))]
    for i, (k, n) in enumerate(zip(keys, LENGTHS)):
        eng.set(k, data(i, n))
    return keys


# ---- every length, op and source count -------------------------------------------------------------------------------------
def test_every_length_op_and_source_count(eng):
    keys = length_keys(eng)
    nl = len(keys)
    names = keys + ["d%d" % i for i in range(60)]
    # each length alone, as the longest source: a copy (OR) into a fresh destination, its NOT, and both counted only
    ops, dests, groups = [], [], []
    for i in range(nl):
        ops += [OR, NOT, OR, NOT]
        dests += [nl + 2 * i, nl + 2 * i + 1, None, None]
        groups += [[i]] * 4
    eng.call(names, ops, dests, groups)
    # 1, 2, 8, 9 and 17 sources of mixed lengths inside one group, under every op, stored and counted only; the
    # stride walks the lengths so that a group holds short, vector-edge and tile-edge strings together
    ops, dests, groups, d = [], [], [], nl + 24
    for op in (AND, OR, XOR):
        for nsrc in (1, 2, 8, 9, 17):
            for start in (0, 5, 11):
                srcs = [(start + 5 * j) % nl for j in range(nsrc)]
                ops += [op, op]
                dests += [d, None]
                groups += [srcs, srcs]
                d += 1 if start == 11 else 0
            # (one destination per (op, nsrc): written three times in a row, a phase each)
    eng.call(names, ops, dests, groups)


def test_a_longer_destination_shrinks_and_its_old_tail_reads_zero(eng):
    eng.set("big", b"\xFF" * (3 * T + 5))
    eng.set("a", data(1, 17))
    eng.set("b", data(2, 33))
    _rc, lens, counts, _status = eng.call(["big", "a", "b"], [XOR], [0], [[1, 2]])
    assert lens == [33] and eng.ks.strlen("big") == 33
    # the string grows again in place: what the longer value held must read as zero
    eng.bitset("big").set(8 * (3 * T + 4) + 7, True)
    eng.ks.setbit("obj", "big", 8 * (3 * T + 4) + 7, 1)
    eng.check()
    assert eng.client.getBitSet(eng.name("big")).cardinality() == counts[0] + 1


def test_destination_among_its_sources_and_growth_past_the_allocation(eng):
    for k, n in (("d1", 17), ("d2", 17), ("d3", 33), ("big", 3 * T + 5), ("mid", T + 1)):
        eng.set(k, data(len(k) + n, n))
    names = ["d1", "d2", "d3", "big", "mid"]
    # first and last among the sources; d1 and d2 (17 bytes in a 256-byte block) must grow to 3T + 5 while being read
    eng.call(names, [XOR, OR, AND, NOT], [0, 1, 2, 4], [[0, 3], [3, 4, 1], [2, 4, 2], [4]])
    eng.call(names, [OR, XOR], [2, 0], [[3, 2], [0, 0]])  # d3 grows as its own last source; d1 ^ d1 is zeros
    assert eng.ks.data["d1"] == b"\0" * (3 * T + 5)


def test_timeouts_and_the_empty_result(eng):
    eng.set("gone", data(1, 40), timeout=True)
    eng.set("kept", data(2, 40), timeout=True)
    eng.set("src", data(3, 64), timeout=True)
    eng.set("empty-src", b"")
    names = ["gone", "kept", "src", "empty-src", "also-missing"]
    # AND over missing keys is the empty string: DEL gone (timeout and all); kept survives without its timeout
    _rc, lens, counts, _status = eng.call(names, [AND, OR, NOT], [0, 1, 4], [[3, 4], [2, 1], [3]])
    assert lens == [0, 64, 0] and counts[0] == 0
    assert eng.ks.ttl("conn", "gone")[0] == "missing" and eng.ks.ttl("conn", "kept")[0] == "none"
    assert eng.ks.ttl("conn", "src")[0] == "set"
    assert last()[3] == 1  # only the OR reached the device


def test_groups_without_a_destination_change_nothing(eng):
    keys = length_keys(eng)
    before = {k: eng.client.getBitSet(eng.name(k)).toByteArray() for k in keys}
    ops = [AND, OR, XOR, NOT, NOT, OR, AND]
    groups = [[4, 6, 11], [1, 9, 10], [2, 3, 8], [4], [0], [0], [4, 0]]  # keys[4] has 17 bytes: the padding must not count
    _rc, lens, counts, _status = eng.call(keys, ops, [None] * 7, groups)
    assert lens[3] == 17 and counts[3] == 17 * 8 - eng.client.getBitSet(eng.name(keys[4])).cardinality()
    assert lens[4:] == [0, 0, 17] and counts[4:] == [0, 0, 0]
    assert before == {k: eng.client.getBitSet(eng.name(k)).toByteArray() for k in keys}
    assert last()[0] == 1


# ---- failures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", [HLL, CFG])
def test_wrong_types_fail_alone_between_dependent_groups(eng, wrong):
    eng.set("a", data(1, 33))
    eng.set("b", data(2, 17))
    names = ["a", "b", "t", "u", wrong]
    # t <- a | b; (fails: wrong source); (fails: wrong destination); u <- t ^ a; (fails: counted only); count u
    rc, lens, _counts, status = eng.call(names, [OR, OR, AND, XOR, OR, OR], [2, 2, 4, 3, None, None],
                                         [[0, 1], [0, 4], [0], [2, 0], [4], [3]])
    assert rc == M.E_WRONGTYPE and status == [0, 0xFF, 0xFF, 0, 0xFF, 0] and lens == [33, 0, 0, 33, 0, 33]
    assert last()[0] == 2  # the dependants still see each other: read after write, the failed ones close nothing


def test_not_with_two_sources_fails_alone_with_the_redis_error(eng):
    eng.set("a", data(1, 33))
    eng.set("b", data(2, 17))
    rc, _lens, _counts, status = eng.call(["a", "b", "d", HLL], [NOT, NOT, OR], [2, 2, 2], [[0], [0, 1], [3]])
    assert rc == M.E_REDIS and status == [0, 0xFF, 0xFF]
    rc, *_ = eng.call(["a", "b", "d", HLL], [OR, NOT], [2, 2], [[3], [0, 1]])
    assert rc == M.E_WRONGTYPE  # the first failing group's code


def test_caller_errors_change_nothing(eng):
    keys = length_keys(eng)
    snapshot = {k: eng.client.getBitSet(eng.name(k)).toByteArray() for k in keys + ["new"]}
    names = keys + ["new"]
    for ops, dests, groups in (([OR, 4], [12, 12], [[1], [2]]), ([OR, OR], [12, 12], [[1], []]),
                               ([OR, OR], [12, 12], [[1], [13]]), ([OR, OR], [12, 13], [[1], [2]])):
        rc, *_ = eng.call(names, ops, dests, groups)
        assert rc == M.E_ILLEGAL_ARGUMENT
        assert snapshot == {k: eng.client.getBitSet(eng.name(k)).toByteArray() for k in names}
        assert not eng.client.getBitSet(eng.name("new")).isExists()


# ---- many groups of very different sizes in one launch; dependent chains ------------------------------------------------------
def test_one_large_group_beside_500_small_ones(eng):
    big = ["B%d" % i for i in range(3)]
    for i, k in enumerate(big):
        eng.set(k, data(100 + i, (1 << 20) - (0, 1, 17)[i]))
    small = ["s%d" % i for i in range(40)]
    for i, k in enumerate(small):
        eng.set(k, data(i, (1, 15, 16, 17, 31, 32, 33)[i % 7]))
    names = big + small + ["D"] + ["d%d" % i for i in range(250)]
    rng = np.random.default_rng(5)
    ops, dests, groups = [], [], []
    for i in range(500):
        if i == 250:  # in the middle: the binary search crosses from the small groups' tiles into its tiles and back
            ops.append(XOR), dests.append(43), groups.append([0, 1, 2])
        ops.append(int(rng.integers(0, 3)))
        dests.append(44 + i // 2 if i % 2 else None)
        groups.append([3 + int(k) for k in rng.integers(0, 40, size=int(rng.integers(1, 4)))])
    eng.call(names, ops, dests, groups, check=["D"] + names[44:])
    assert last()[:2] == [1, 1] and last()[3] == 501


def test_a_chain_of_64_is_64_phases(eng):
    keys = ["c%d" % i for i in range(65)]
    for i, k in enumerate(keys):
        eng.set(k, data(i, LENGTHS[1 + i % 11]))
    eng.call(keys, [OR] * 64, list(range(1, 65)), [[i, i + 1] for i in range(64)])
    assert last()[0] == 64
    assert eng.ks.strlen("c64") == 3 * T + 5


def test_the_cohort_pipeline_is_one_phase_and_one_temporary_is_a_phase_each(eng):
    eng.set("a", data(1, T + 1))
    eng.set("b", data(2, T - 1))
    names = ["a", "b"] + ["t%d" % i for i in range(20)]
    ops, dests, groups = [AND, OR] * 20, [], []
    for i in range(20):
        dests += [2 + i, None]
        groups += [[0, 1], [2 + i]]
    eng.call(names, ops, dests, groups)
    assert last()[0] == 1 and last()[1] == 1 and last()[3] == 20  # the counts are forwarded
    eng.call(names, ops, [2, None] * 20, [[0, 1], [2]] * 20)
    assert last()[0] == 20


# ---- a Bloom filter's bitmap as the destination, with an open handle -------------------------------------------------------------
def test_an_open_bloom_handle_sees_a_grouped_or(client, fresh, tile):
    import torch

    from redisson_amd import BloomHandle, bitset_op_groups_call, device_keys
    from redisson_amd import _lib as L

    rng = np.random.default_rng(0xB17)
    mat = rng.integers(0, 256, size=(2000, 16), dtype=np.uint8)
    filters = [client.getBloomFilter(fresh + n) for n in ("grouped", "twin", "other")]
    for f in filters:
        assert f.tryInit(3000, 0.03)
    for f in filters[:2]:
        f.add([m.tobytes() for m in mat[:300]])
    filters[2].add([m.tobytes() for m in mat[300:900]])
    h, twin = BloomHandle(client, fresh + "grouped"), BloomHandle(client, fresh + "twin")  # opened before the ORs
    rc, _msg, lens, counts, _status = bitset_op_groups_call(client, [fresh + "grouped", fresh + "other"], [OR, OR],
                                                            [0, None], [[0, 1], [0]])
    assert rc == L.RBX_OK and lens[0] == lens[1] and counts[0] == counts[1]
    assert client.getBitSet(fresh + "twin")._op(L.RBX_BITOP_OR, [fresh + "other"]) == lens[0]
    assert client.getBitSet(fresh + "twin").cardinality() == counts[0]
    d_keys = torch.from_numpy(mat).cuda()
    outs = []
    for handle in (h, twin):
        d_out = torch.zeros(2000, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        handle.contains_dev(device_keys(d_keys.data_ptr(), 2000, 16), d_cnt.data_ptr(), d_out.data_ptr())
        client.synchronize()
        outs.append((d_cnt.item(), d_out.cpu().numpy()))
    assert outs[0][0] == outs[1][0] >= 900 and (outs[0][1] == outs[1][1]).all() and outs[0][1][:900].all()
    h.close()
    twin.close()
    for f in filters:
        f.delete()


# ---- the seeded random driver --------------------------------------------------------------------------------------------------
def test_seeded_random_calls(eng):
    calls = D.seeded_calls()
    total = sum(len(ops) for _r, ops, _d, _g in calls)
    assert D.failing_groups(calls) <= total // 10  # the plan stays a test of BITOPs, not of failures
    names = ["k%d" % i for i in range(D.NKEYS)] + [HLL, CFG]
    for n, (resets, ops, dests, groups) in enumerate(calls):
        for key, length, seed, timeout in resets:
            eng.set(names[key], np.random.default_rng(seed).bytes(length), timeout)
        touched = {names[d] for d in dests if d is not None and d < D.NKEYS} | {names[k] for k, *_ in resets}
        eng.call(names, ops, dests, groups, check=None if n % 50 == 49 else touched)
    eng.check()


# ---- RBatch and the Spring Data pipeline end to end ------------------------------------------------------------------------------
def cohort_days(eng, days=9):  # 36 pairs, of which the first 30
    keys = ["day%d" % i for i in range(days)]
    for i, k in enumerate(keys):
        eng.set(k, data(i, T + 17 * i))
    pairs = [(i, j) for i in range(days) for j in range(i + 1, days)]
    return keys, pairs[:30]


def test_rbatch_cohort_pipeline_is_one_launch(eng):
    keys, pairs = cohort_days(eng)
    want = []
    for n, (i, j) in enumerate(pairs):
        t = "pair%d" % n
        eng.touched.add(t)
        eng.ks.bitop("obj", t, "and", (t, keys[i], keys[j]))
        want += [None, eng.ks.cardinality("obj", t)[0]]
    b = eng.client.createBatch()
    for n, (i, j) in enumerate(pairs):
        t = b.getBitSet(eng.name("pair%d" % n))
        t.andAsync(eng.name(keys[i]), eng.name(keys[j]))
        t.cardinalityAsync()
    assert b.execute().getResponses() == want
    assert last()[:2] == [1, 1] and last()[3] == 30
    eng.check()


def test_spring_data_cohort_pipeline_is_one_launch(eng):
    from redisson_amd.spring_data import RedissonConnection

    keys, pairs = cohort_days(eng)
    want = []
    for n, (i, j) in enumerate(pairs):
        t = "pair%d" % n
        eng.touched.add(t)
        want += [eng.ks.bitop("conn", t, "and", (keys[i], keys[j]))[0], eng.ks.cardinality("conn", t)[0]]
    conn = RedissonConnection(eng.client)
    conn.openPipeline()
    for n, (i, j) in enumerate(pairs):
        t = eng.name("pair%d" % n).encode()
        conn.bitOp("AND", t, eng.name(keys[i]).encode(), eng.name(keys[j]).encode())
        conn.bitCount(t)
    assert conn.closePipeline() == want
    assert last()[:2] == [1, 1] and last()[3] == 30
    eng.check()
