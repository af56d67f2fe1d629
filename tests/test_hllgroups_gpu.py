"""rbx_hll_count_groups / rbx_hll_merge_groups on the GPU against hllgroups_model: after every call the counts, the
status bytes and the return code, then every key's GET in the as-stored encoding (header included), its registers
(the dense GET) and its TTL state.  Every test runs under rbx_tune "hllgroups_split" auto and under every P, which
must agree with the model and so with each other."""
import ctypes as C

import numpy as np
import pytest

import hll_driver as D
import hll_elements as E
import hll_model as HM
import hllgroups_model as G
import hllstream_model as SM
from hll_model import BITS, BLOOM, INVALID, REGS, WRONGTYPE, Keyspace
from hllgroups_model import FAILED, at
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WRONG_MSG = "WRONGTYPE Key is not a valid HyperLogLog string value."
EXTRA = tuple("x%d" % i for i in range(40))  # further keys of single tests


@pytest.fixture(params=[0, 1, 2, 4, 8, 16], ids=["auto", "P1", "P2", "P4", "P8", "P16"])
def split(request):
    from redisson_amd import _lib as L

    assert L.lib().rbx_tune(b"hllgroups_split", request.param) == 0
    yield request.param
    assert L.lib().rbx_tune(b"hllgroups_split", 0) == 0


def last():
    from redisson_amd import _lib as L

    out = (C.c_uint32 * 4)()
    assert L.lib().rbx_bench_hllgroups_last(out) == 0
    return list(out)  # phases, launches, split of the last launch, groups on the device


def dense(regs, card=INVALID) -> bytes:
    return HM.header(0, card) + O.hll_dense_pack(np.asarray(regs, np.uint8))


def sparse(regs, card=INVALID) -> bytes:
    return HM.header(1, card) + O.hll_sparse_pack(np.asarray(regs, np.uint8))


def some_regs(seed, n=200, top=6):
    rng = np.random.default_rng([0x9E95, seed])
    regs = np.zeros(REGS, np.uint8)
    regs[rng.integers(0, REGS, size=n)] = rng.integers(1, top + 1, size=n)
    return regs


class Engine:
    """the grouped calls through librbx.so beside the model; keys are prefix + key, BITS is a bit string and BLOOM
    the {name}:config hash of a Bloom filter"""

    def __init__(self, client, prefix):
        self.client, self.prefix, self.ks = client, prefix, Keyspace()
        self.touched = set()
        self.bits = client.getBitSet(self.name(BITS))
        self.bits.set(5, True)
        self.bloom = client.getBloomFilter(prefix + "bloom")
        assert self.bloom.tryInitRaw(3001, 5)

    def name(self, key) -> str:
        return "{%sbloom}:config" % self.prefix if key == BLOOM else self.prefix + key

    def hll(self, key):
        self.touched.add(key)
        return self.client.getHyperLogLog(self.name(key))

    def apply(self, cmd):
        """a setup command of hll_driver's form on both sides"""
        from redisson_amd import hll_stream

        getattr(self.ks, cmd[0])(*cmd[1:])
        if cmd[0] == "set":
            self.hll(cmd[2]).importString(cmd[3])
        elif cmd[0] == "expire":
            assert self.hll(cmd[2]).expire(D.TTL_MS)
        elif cmd[0] == "delete":
            self.hll(cmd[2]).delete()
        elif cmd[0] == "pfadd":
            elements = [bytes(e) for e in HM.materialize(cmd[3])]
            self.touched.add(cmd[2])
            hll_stream(self.client, [self.name(cmd[2])], [0], [SM.PFADD], [0, len(elements)], elements)
        else:
            raise AssertionError(cmd)

    def _rc(self, rc, msg):
        from redisson_amd import _lib as L

        assert rc in (L.RBX_OK, L.RBX_E_WRONGTYPE) and (msg == WRONG_MSG) == (rc != L.RBX_OK), (rc, msg)
        return WRONGTYPE if rc else None

    def counts(self, groups, names=None):
        """one rbx_hll_count_groups call on both sides, everything compared"""
        from redisson_amd import hll_count_groups_call

        groups = [tuple(g) for g in groups]
        names = list(dict.fromkeys(k for g in groups for k in g)) if names is None else names
        self.touched.update(k for k in names if not G.wrong(k))
        want = G.count_groups(self.ks, groups)
        rc, msg, out, status = hll_count_groups_call(self.client, [self.name(k) for k in names],
                                                     [[names.index(k) for k in g] for g in groups])
        got = (self._rc(rc, msg), [int(x) for x in out], [int(x) for x in status])
        assert got == want, D.first_difference(list(got), list(want))
        self.check()
        return got

    def merges(self, merges, names=None):
        """one rbx_hll_merge_groups call on both sides, everything compared, the phase count too"""
        from redisson_amd import hll_merge_groups_call

        merges = [(d, tuple(s)) for d, s in merges]
        names = list(dict.fromkeys(k for d, s in merges for k in (d,) + s)) if names is None else names
        self.touched.update(k for k in names if not G.wrong(k))
        want = G.merge_groups(self.ks, merges)
        rc, msg, status = hll_merge_groups_call(self.client, [self.name(k) for k in names],
                                                [names.index(d) for d, _ in merges],
                                                [[names.index(k) for k in s] for _, s in merges])
        got = (self._rc(rc, msg), [int(x) for x in status])
        assert got == want, D.first_difference(list(got), list(want))
        assert last()[0] == len(G.merge_phases(merges)), (last(), G.merge_phases(merges))
        self.check()
        return got

    def check(self):
        for key in sorted(self.touched):
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
        for key in self.touched:
            self.client.getHyperLogLog(self.name(key)).delete()
        self.bits.delete()
        self.bloom.delete()


@pytest.fixture
def eng(client, fresh):
    e = Engine(client, fresh)
    yield e
    e.close()


# ---- counts ----------------------------------------------------------------------------------------------------------
def test_group_sizes_around_the_unroll_and_group_counts(eng, split):
    keys = EXTRA[:33]
    for i, k in enumerate(keys):
        if i % 3 == 0:
            eng.apply(("set", "obj", k, dense(some_regs(i, 300, 40))))
        elif i % 3 == 1:
            eng.apply(("set", "obj", k, sparse(some_regs(i, 40, 5))))
        else:
            eng.apply(("pfadd", "obj", k, ("low", 900 + i, 5)))
    groups = [keys[:n] for n in (1, 2, 3, 4, 5, 9, 33)]
    got = eng.counts(groups)
    assert last()[1] == 1 and last()[3] == 7 and len(set(got[1])) >= 5
    assert last()[2] == (split or 16)
    eng.counts([keys[4:13]])  # ngroups = 1
    eng.counts([keys[i:i + 1 + i % 4] for i in range(7)])  # 7: keys in many groups
    many = [tuple(keys[(i * 7 + j * 3) % 33] for j in range(2 + i % 5)) for i in range(300)]  # 300: more than one block row
    eng.counts(many)
    assert last()[2] == (split or 1) and last()[3] == 300
    eng.counts([(keys[0], keys[0]), (keys[1], keys[2], keys[1]), (keys[0],)])  # a key twice in one group


def test_one_entry_against_the_same_key_twice_on_a_wrong_valid_cache(eng, split):
    eng.apply(("set", "obj", "k0", sparse(some_regs(1, 30, 3), card=4321)))  # valid and wrong
    got = eng.counts([("k0",), ("k0", "k0"), ("k0",)])
    assert got[1][0] == got[1][2] == 4321 and got[1][1] == O.hll_count(some_regs(1, 30, 3)) != 4321
    assert eng.ks.keys["k0"].card == 4321


def test_sparse_and_dense_members_missing_keys_and_an_empty_key(eng, split):
    eng.apply(("set", "obj", "k0", dense(some_regs(2, 500, 45))))
    eng.apply(("pfadd", "obj", "k1", ("low", 7, 6)))
    eng.apply(("pfadd", "obj", "k2", SM.NONE))  # exists, empty
    got = eng.counts([("k0", "k1"), ("k8", "k9"), ("k9",), ("k2",), ("k2", "k9"), ("k1", "k9", "k0", "k2"), ("k2", "k2")])
    assert got[1][1] == got[1][2] == got[1][3] == got[1][4] == got[1][6] == 0 and got[1][0] == got[1][5] > 0
    assert set(eng.ks.keys) == {"k0", "k1", "k2"}
    eng.counts([("k8", "k9"), ("k9", "k9")])  # nothing reaches the device
    assert last()[1] == 0 and last()[3] == 0


def test_registers_at_the_ends_and_at_every_slice_boundary(eng, split):
    edges = sorted({0, REGS - 1} | {b + d for b in range(1024, REGS, 1024) for d in (-1, 0, 1)})
    a = [E.element(r, 1 + i % 7) for i, r in enumerate(edges[0::2])]
    b = [E.element(r, 1 + i % 5) for i, r in enumerate(edges[1::2])]
    eng.apply(("pfadd", "obj", "k0", ("lit", tuple(a))))
    eng.apply(("pfadd", "obj", "k1", ("lit", tuple(b))))
    eng.apply(("pfadd", "obj", "k2", ("lit", (E.element(0, 9), E.element(REGS - 1, 9)))))
    got = eng.counts([("k0", "k1"), ("k0",), ("k1", "k2"), ("k2", "k0", "k1")])
    assert got[1][0] == len(edges) and got[1][1] == len(a)
    regs = np.zeros(REGS, np.uint8)  # and as a dense string: each slice's first and last byte is counted once
    regs[edges] = 3
    eng.apply(("set", "obj", "k3", dense(regs)))
    eng.counts([("k3", "k2"), ("k3", "k3")])


def test_the_tau_branch_and_fifty_everywhere_but_one(eng, split):
    a, b = some_regs(3, 400, 50), some_regs(4, 400, 50)
    a[777] = 51
    eng.apply(("set", "obj", "k0", dense(a)))
    eng.apply(("set", "obj", "k1", dense(b)))
    assert int(b.max()) <= 50 and int(np.delete(a, 777).max()) <= 50
    eng.counts([("k0", "k1"), ("k1",), ("k0",), ("k1", "k1")])
    lo, hi = np.full(REGS, 50, np.uint8), np.full(REGS, 50, np.uint8)
    lo[REGS // 2:] = 0
    hi[:REGS // 2] = 0
    hi[9999] = 0
    eng.apply(("set", "obj", "k2", dense(lo)))
    eng.apply(("set", "obj", "k3", dense(hi)))
    got = eng.counts([("k2", "k3"), ("k3", "k2", "k0")])
    want = np.maximum(lo, hi)
    assert int((want == 0).sum()) == 1 and got[1][0] == O.hll_count(want)


def test_the_cache_rule(eng, split):
    eng.apply(("pfadd", "obj", "k0", ("low", 3, 6)))
    eng.apply(("pfadd", "obj", "k1", ("low", 4, 6)))
    assert eng.ks.keys["k0"].card >> 63
    eng.counts([("k0", "k1"), ("k1", "k0", "k0")])  # unions store nothing
    assert eng.ks.keys["k0"].card >> 63 and eng.ks.keys["k1"].card >> 63
    first = eng.counts([("k0",), ("k1", "k0"), ("k0",)])  # the recount is stored (twice, the same value)
    assert last()[1] == 1 and last()[3] == 3 and not eng.ks.keys["k0"].card >> 63
    again = eng.counts([("k0",), ("k0",)])
    assert last()[1] == 0 and again[1] == [first[1][0]] * 2  # returned without a launch
    assert eng.ks.keys["k1"].card >> 63


def test_wrong_type_groups_fail_alone(eng, split):
    eng.apply(("pfadd", "obj", "k0", ("low", 5, 6)))
    eng.apply(("pfadd", "obj", "k1", ("low", 6, 6)))
    groups = [("k0", "k1"), (BITS, "k0"), ("k0", BLOOM, "k1"), (BLOOM,), ("k0",), ("k1", "k0", BITS), ("k9", "k1")]
    got = eng.counts(groups)
    assert got[0] == WRONGTYPE and got[2] == [0, FAILED, FAILED, FAILED, 0, FAILED, 0]
    assert eng.counts([(BITS,)]) == (WRONGTYPE, [0], [FAILED])
    assert eng.counts([("k0",), ("k1", "k0")])[0] is None


def test_equal_names_are_one_key(eng, split):
    from redisson_amd import hll_count_groups_call, hll_merge_groups_call

    eng.apply(("pfadd", "obj", "k0", ("low", 8, 5)))
    eng.apply(("pfadd", "obj", "k1", ("low", 9, 5)))
    names = [eng.name("k0"), eng.name("k1"), eng.name("k0"), eng.name("k2")]
    want = G.count_groups(eng.ks, [("k0", "k1"), ("k0",), ("k0", "k0")])
    rc, _msg, out, status = hll_count_groups_call(eng.client, names, [[2, 1], [2], [0, 2]])
    assert (rc, [int(x) for x in out], [int(x) for x in status]) == (0, want[1], want[2])
    # k2 <- k0 then k0 (under its other entry) <- k1: a write after a read across two entries of one key
    merges = [("k2", ("k0",)), ("k0", ("k1",))]
    G.merge_groups(eng.ks, merges)
    rc, _msg, status = hll_merge_groups_call(eng.client, names, [3, 2], [[0], [1]])
    assert rc == 0 and list(status) == [0, 0] and last()[0] == 2
    eng.touched.add("k2")
    eng.check()


def test_caller_errors_change_nothing(eng, split):
    from redisson_amd import _lib as L

    eng.apply(("pfadd", "obj", "k0", at(1, 1)))
    lib, ctx = L.lib(), eng.client.ctx
    names, _keep = L.names_array([eng.name("k0"), eng.name("k9")])
    u64, u32 = (lambda *x: np.array(x, np.uint64)), (lambda *x: np.array(x, np.uint32))
    out, status = np.zeros(4, np.uint64), np.zeros(4, np.uint8)

    def count(off, key, n):
        return lib.rbx_hll_count_groups(ctx, names, 2, off.ctypes.data_as(L.u64p), key.ctypes.data_as(L.u32p), n,
                                        out.ctypes.data_as(L.u64p), status.ctypes.data_as(L.u8p))

    def merge(dest, off, key, n):
        return lib.rbx_hll_merge_groups(ctx, names, 2, dest.ctypes.data_as(L.u32p), off.ctypes.data_as(L.u64p),
                                        key.ctypes.data_as(L.u32p), n, status.ctypes.data_as(L.u8p))

    bad = [count(u64(0, 1, 1), u32(0), 2), count(u64(0, 1), u32(2), 1), count(u64(1, 2), u32(0, 1), 1),
           merge(u32(1, 2), u64(0, 1, 2), u32(0, 0), 2), merge(u32(1, 1), u64(0, 1, 2), u32(0, 2), 2),
           merge(u32(1, 1), u64(0, 2, 1), u32(0, 0), 2)]
    assert bad == [L.RBX_E_ILLEGAL_ARGUMENT] * len(bad)
    eng.touched.add("k9")
    eng.check()  # k9 was not created
    assert count(u64(0), u32(0), 0) == L.RBX_OK and merge(u32(0), u64(0), u32(0), 0) == L.RBX_OK


# ---- merges: the hazards ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_the_cases_the_wrong_models_miss(eng, split, case):
    setup, merges, groups = G.CASES[case]
    for cmd in setup:
        eng.apply(cmd)
    if merges:
        eng.merges(merges)
    if groups:
        eng.counts(groups)


def test_each_hazard_is_its_own_phase(eng, split):
    for i, k in enumerate(("k1", "k2", "k3")):
        eng.apply(("pfadd", "obj", k, ("low", 20 + i, 6)))
    eng.merges([("k0", ("k1",)), ("k4", ("k0",))])  # A <- B, C <- A
    assert last()[0] == 2
    eng.merges([("k5", ("k1",)), ("k1", ("k2",))])  # A <- B, B <- C
    assert last()[0] == 2
    eng.merges([("k6", ("k1",)), ("k6", ("k3",))])  # A <- B, A <- C
    assert last()[0] == 2
    eng.merges([("k7", ("k7", "k2"))])  # A <- A, B
    assert last()[:2] == [1, 1]
    eng.merges([("k8", ("k1",)), ("k9", ("k8",)), ("k10", ("k9", "k1")), ("k8", ("k3",))])
    assert last()[0] == 3  # the last one joins the third phase: k8 was written and read in earlier phases only


def test_three_hundred_independent_merges_are_one_phase(eng, split):
    src = EXTRA[:8]
    for i, k in enumerate(src):
        eng.apply(("set", "obj", k, dense(some_regs(40 + i, 300, 45))) if i % 2 else ("pfadd", "obj", k, ("low", 60 + i, 6)))
    merges = [("d%d" % i, tuple(src[(i + j) % 8] for j in range(1 + i % 4))) for i in range(300)]
    eng.merges(merges)
    assert last()[:2] == [1, 1] and last()[3] == 300 and last()[2] == (split or 1)
    eng.counts([("d%d" % i, "d%d" % (i + 1)) for i in range(0, 300, 7)])


# ---- merges: encodings -------------------------------------------------------------------------------------------------
def test_missing_destination_and_missing_sources(eng, split):
    eng.merges([("k0", ("k8", "k9")), ("k1", ())])
    for k in ("k0", "k1"):
        assert eng.ks.keys[k].card == INVALID and not eng.ks.keys[k].dense
    assert last()[1] == 0 and set(eng.ks.keys) == {"k0", "k1"}
    eng.apply(("set", "obj", "k2", sparse(some_regs(5, 20, 3), card=777)))
    eng.apply(("expire", "obj", "k2"))
    eng.merges([("k2", ()), ("k3", ("k2",))])
    assert eng.ks.keys["k2"].card == INVALID | 777 and eng.ks.keys["k2"].ttl  # the low 63 bits and the TTL stay


def test_sparse_into_sparse_stays_sparse_and_a_dense_source_promotes(eng, split):
    eng.apply(("pfadd", "obj", "k0", ("low", 11, 6)))
    eng.apply(("pfadd", "obj", "k1", ("low", 12, 6)))
    eng.apply(("set", "obj", "k2", D.odd_string(5)))  # not normalized: the write-back goes through hllSparseSet
    eng.merges([("k0", ("k1", "k2")), ("k3", ("k1",))])
    assert not eng.ks.keys["k0"].dense and not eng.ks.keys["k3"].dense
    eng.apply(("set", "obj", "k4", G.small_dense()))
    eng.apply(("expire", "obj", "k1"))
    eng.merges([("k1", ("k4",)), ("k5", ("k0", "k4")), ("k4", ("k0",))])
    assert eng.ks.keys["k1"].dense and eng.ks.keys["k5"].dense and eng.ks.keys["k1"].ttl


def test_promotion_by_the_write_back(eng, split):
    half_a, half_b = np.zeros(REGS, np.uint8), np.zeros(REGS, np.uint8)
    half_a[0:2000:2] = 1  # 1,000 VALs and 1,000 ZEROs: 2,000 bytes and an XZERO
    half_b[2000:4400:2] = 2  # 2,400 bytes and two XZEROs
    eng.apply(("set", "obj", "k0", sparse(half_a)))
    eng.apply(("set", "obj", "k1", sparse(half_b)))
    assert 16 + len(O.hll_sparse_pack(half_a)) <= 3000 and 16 + len(O.hll_sparse_pack(half_b)) <= 3000
    eng.merges([("k2", ("k0", "k1"))])  # the union passes 3,000 bytes
    assert eng.ks.keys["k2"].dense and not eng.ks.keys["k0"].dense
    hi = np.zeros(REGS, np.uint8)
    hi[[3, 9000]] = (2, 3)
    eng.apply(("set", "obj", "k3", sparse(hi)))
    eng.apply(("pfadd", "obj", "k4", at(4444, 33)))  # promoted by value: dense
    eng.apply(("pfadd", "obj", "k5", ("low", 13, 4)))
    assert eng.ks.keys["k4"].dense
    eng.merges([("k3", ("k5",)), ("k6", ("k3", "k4"))])
    assert not eng.ks.keys["k3"].dense and eng.ks.keys["k6"].dense


def test_wrong_type_merges_fail_alone_and_create_nothing(eng, split):
    eng.apply(("pfadd", "obj", "k0", ("low", 14, 5)))
    merges = [("k1", ("k0",)), (BITS, ("k0",)), ("k2", ("k0", BLOOM)), ("k3", (BITS,)), ("k1", ("k2",)), ("k4", ("k1",)),
              (BLOOM, ())]
    got = eng.merges(merges)
    assert got == (WRONGTYPE, [0, FAILED, FAILED, FAILED, 0, 0, FAILED])
    assert set(eng.ks.keys) == {"k0", "k1", "k4"}
    assert eng.merges([(BLOOM, ("k0",))]) == (WRONGTYPE, [FAILED]) and last()[0] == 0


# ---- seeded sequences ------------------------------------------------------------------------------------------------
def run_step(eng, step):
    from redisson_amd import hll_stream_call

    kind = step[0]
    if kind == "count":
        return eng.counts(step[1])
    if kind == "merge":
        return eng.merges(step[1])
    want = G.apply_step(eng.ks, step)
    if kind == "stream":
        cmds = step[1]
        names = list(dict.fromkeys(k for k, _, _ in cmds))
        eng.touched.update(k for k in names if not G.wrong(k))
        parts = [[bytes(r) for r in HM.materialize(spec)] for _k, _op, spec in cmds]
        seg = np.zeros(len(cmds) + 1, np.uint64)
        seg[1:] = np.cumsum([len(p) for p in parts])
        rc, msg, replies, status = hll_stream_call(eng.client, [eng.name(k) for k in names], [names.index(k) for k, _, _ in cmds],
                                                   [op for _, op, _ in cmds], seg, [e for p in parts for e in p])
        got = (eng._rc(rc, msg), [int(x) for x in replies], [int(x) for x in status])
        assert got == want, D.first_difference(list(got), list(want))
    elif kind == "countWith":
        assert eng.hll(step[1][0]).countWith(*[eng.name(k) for k in step[1][1:]]) == want[0]
    elif kind == "mergeWith":
        eng.hll(step[1]).mergeWith(*[eng.name(k) for k in step[2]])
        eng.touched.update(step[2])
    elif kind == "set":
        eng.hll(step[1]).importString(step[2])
    elif kind == "delete":
        assert eng.hll(step[1]).delete() == want[0]
    else:
        raise AssertionError(step)
    eng.check()


@pytest.mark.parametrize("seed", G.SEEDS)
def test_seeded_sequences(eng, split, seed):
    for cmd in G.setup(seed):
        eng.apply(cmd)
    for step in G.seeded(seed):
        run_step(eng, step)


# ---- RBatch and the Spring Data pipeline, end to end --------------------------------------------------------------------
def test_rbatch_and_the_pipeline_equal_the_commands_one_at_a_time(client, fresh, split):
    import redisson_amd.spring_data as S
    from redisson_amd import ByteArrayCodec, RBatch

    keys = "abcde"
    x = [E.element(10 + i, 1 + i % 3) for i in range(8)]

    def name(prefix, k):
        return fresh + prefix + k

    def singly(p):
        hll = lambda k: client.getHyperLogLog(name(p, k), ByteArrayCodec())  # noqa: E731
        return [hll("a").addAll(x[:3]), hll("a").count(), hll("a").countWith(name(p, "b")), hll("b").countWith(name(p, "a"), name(p, "z")),
                hll("a").countWith(name(p, "a")), hll("c").mergeWith(name(p, "a")), hll("d").mergeWith(name(p, "c"), name(p, "b")),
                hll("d").countWith(name(p, "e")), hll("b").addAll(x[3:])]

    def strings(p):
        return [client.getHyperLogLog(name(p, k)).exportString("stored") for k in keys]

    want = singly("one-")
    b = RBatch(client)
    hll = lambda k: b.getHyperLogLog(name("bat-", k), ByteArrayCodec())  # noqa: E731
    n = lambda k: name("bat-", k)  # noqa: E731
    hll("a").addAllAsync(x[:3]), hll("a").countAsync(), hll("a").countWithAsync(n("b")), hll("b").countWithAsync(n("a"), n("z"))
    hll("a").countWithAsync(n("a")), hll("c").mergeWithAsync(n("a")), hll("d").mergeWithAsync(n("c"), n("b"))
    hll("d").countWithAsync(n("e")), hll("b").addAllAsync(x[3:])
    assert b.execute().getResponses() == want
    assert last()[0] == 0 and last()[3] == 1  # the last grouped call was the one count after the merges
    assert strings("bat-") == strings("one-")

    conn = S.RedissonConnection(client)
    k = lambda key: name("pipe-", key).encode()  # noqa: E731
    conn.openPipeline()
    conn.pfAdd(k("a"), *x[:3]), conn.pfCount(k("a")), conn.pfCount(k("a"), k("b")), conn.pfCount(k("b"), k("a"), k("z"))
    conn.pfCount(k("a"), k("a")), conn.pfMerge(k("c"), k("a")), conn.pfMerge(k("d"), k("c"), k("b"))
    conn.pfCount(k("d"), k("e")), conn.pfAdd(k("b"), *x[3:])
    got = conn.closePipeline()
    assert got == [int(w) if isinstance(w, bool) else w for w in want]
    assert strings("pipe-") == strings("one-")
    for p in ("one-", "bat-", "pipe-"):
        for key in keys:
            client.getHyperLogLog(name(p, key)).delete()
