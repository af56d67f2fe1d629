"""A model of rbx_hll_count_groups and rbx_hll_merge_groups: the groups applied one command at a time, in array order,
to hll_model.Keyspace (Keyspace.pfcount / pfcount_multi / pfmerge are the specification), under the pipelined-batch
rule -- a group that names a key of another type fails alone, changes, stores and creates nothing, and the first
failure in array order decides the return code.  Also a restatement of the host's phase rule for merges, the
deliberately wrong models the CPU test must catch, and the seeded inputs the CPU and GPU tests share.  Shares no code
with the engine.

A count group is a tuple of keys (one key: the single-key PFCOUNT with the header cache; more: the union, counted by
entries).  A merge is (destination, (sources..))."""
import numpy as np

import hll_driver as D
import hll_model as M
import hllstream_model as SM
from hll_model import BITS, BLOOM, WRONGTYPE, Keyspace
from oracle import oracle as O

RAN, FAILED = 0, 0xFF
KEYS = tuple("k%d" % i for i in range(12))  # the twelve shared keys of a seeded sequence
SEEDS = tuple(range(6))
STEPS = 40


def wrong(*keys) -> bool:
    return any(k in (BITS, BLOOM) for k in keys)


def count_groups(ks: Keyspace, groups):
    """(return code kind, counts, status) of the groups one PFCOUNT at a time"""
    kind, counts, status = None, [], []
    for g in groups:
        g = tuple(g)
        reply, err = ks.pfcount("groups", g[0]) if len(g) == 1 else ks.pfcount_multi("groups", g[0], g[1:])
        if err is not None:
            assert err == WRONGTYPE
            kind = kind or WRONGTYPE
            counts.append(0)
            status.append(FAILED)
        else:
            counts.append(int(reply))
            status.append(RAN)
    return kind, counts, status


def merge_groups(ks: Keyspace, merges):
    """(return code kind, status) of the merges one PFMERGE at a time"""
    kind, status = None, []
    for dest, srcs in merges:
        _reply, err = ks.pfmerge("groups", dest, tuple(srcs))
        if err is not None:
            assert err == WRONGTYPE
            kind = kind or WRONGTYPE
            status.append(FAILED)
        else:
            status.append(RAN)
    return kind, status


def merge_phases(merges):
    """The host's rule restated: the indexes of the merges that run, phase by phase.  A merge closes the phase before
    it when its destination is a destination or a source of an earlier merge of the phase, or one of its sources is
    such a destination; its own destination among its own sources counts for nothing; a merge that fails alone is in
    no phase and closes none."""
    out, cur, written, read = [], [], set(), set()
    for i, (dest, srcs) in enumerate(merges):
        if wrong(dest, *srcs):
            continue
        others = {s for s in srcs if s != dest}
        if dest in written or dest in read or others & written:
            out.append(cur)
            cur, written, read = [], set(), set()
        cur.append(i)
        written.add(dest)
        read |= others
    if cur:
        out.append(cur)
    return out


state = SM.state
copy_keyspace = SM.copy_keyspace


# ---- deliberately wrong models ------------------------------------------------------------------------------------
class _CacheOnUnion(Keyspace):
    def pfcount_multi(self, via, key, others):
        reply, err = super().pfcount_multi(via, key, others)
        if err is None and key in self.keys:
            self.keys[key].card = reply
        return reply, err


class _NoInvalidationWithoutSources(Keyspace):
    sources = 0

    def pfmerge(self, via, key, srcs):
        self.sources = sum(s in self.keys for s in srcs)
        return super().pfmerge(via, key, srcs)

    def _after_merge(self, k):
        if self.sources:
            k.card |= M.INVALID


class _DenseFromDestination(Keyspace):
    def _use_dense(self, d, sources):
        return d.dense


def wrong_groups(defect: str, ks: Keyspace, merges=(), groups=()):
    """(merge result, count result, final state) of a wrong model on a copy of ks: the merges, then the counts
      'snapshot'  all merges in one phase, every source read as it stood before the call (ignores read after write)
      'no_war'    no write-after-read break: a source that a later merge of the call writes is read as it ends up
      'cache'     the cached cardinality stored on a union
      'no_inval'  no invalidation without an existing source
      'dest'      use_dense from the destination only"""
    cls = {"cache": _CacheOnUnion, "no_inval": _NoInvalidationWithoutSources, "dest": _DenseFromDestination}.get(defect, Keyspace)
    ks = copy_keyspace(ks, cls)
    if defect == "snapshot":
        before = copy_keyspace(ks)
        kind, status = None, []
        for dest, srcs in merges:
            if wrong(dest, *srcs):
                kind, status = kind or WRONGTYPE, status + [FAILED]
                continue
            status.append(RAN)
            tmp = ["\0src%d" % j for j in range(len(srcs))]
            for t, s in zip(tmp, srcs):  # the sources as they stood before the call, except the destination itself
                if s == dest or s not in before.keys:
                    continue
                ks.keys[t] = M.Hll(M.clone(before.keys[s].h), before.keys[s].card, False)
            ks.pfmerge("groups", dest, tuple(s if s == dest else t for t, s in zip(tmp, srcs)))
            for t in tmp:
                ks.keys.pop(t, None)
        merged = (kind, status)
    elif defect == "no_war":
        # a merge reads, for each source that a later merge writes, the value that source ends with
        final = copy_keyspace(ks)
        merge_groups(final, merges)
        kind, status = None, []
        for i, (dest, srcs) in enumerate(merges):
            if wrong(dest, *srcs):
                kind, status = kind or WRONGTYPE, status + [FAILED]
                continue
            status.append(RAN)
            later = {d for d, s in merges[i + 1:] if not wrong(d, *s)}
            tmp = ["\0src%d" % j for j in range(len(srcs))]
            names = []
            for t, s in zip(tmp, srcs):
                if s != dest and s in later and s in final.keys:
                    ks.keys[t] = M.Hll(M.clone(final.keys[s].h), final.keys[s].card, False)
                    names.append(t)
                else:
                    names.append(s)
            ks.pfmerge("groups", dest, tuple(names))
            for t in tmp:
                ks.keys.pop(t, None)
        merged = (kind, status)
    else:
        merged = merge_groups(ks, merges)
    counted = count_groups(ks, groups)
    return merged, counted, state(ks)


DEFECTS = ("snapshot", "no_war", "cache", "no_inval", "dest")


# ---- the hazards and encodings the GPU file runs, as data ----------------------------------------------------------
def at(register, count, serial=1, length=16):
    return ("at", serial, ((register, count, length),))


def small_dense(card=M.INVALID) -> bytes:
    """a dense string whose registers a sparse string could hold: only use_dense makes its merge dense"""
    regs = np.zeros(M.REGS, np.uint8)
    regs[[100, 101, 9000]] = (2, 2, 3)
    return M.header(0, card) + O.hll_dense_pack(regs)


# (setup commands, merges, counts after them): each wrong model differs from the model on at least one of these
CASES = {
    "raw": ([("pfadd", "obj", "k1", at(5, 3, 1)), ("pfadd", "obj", "k2", at(9, 2, 2))],
            [("k0", ("k1",)), ("k2", ("k0",))], []),
    "war": ([("pfadd", "obj", "k1", at(5, 3, 1)), ("pfadd", "obj", "k2", at(9, 2, 2))],
            [("k0", ("k1",)), ("k1", ("k2",))], []),
    "waw": ([("pfadd", "obj", "k1", at(5, 3, 1)), ("pfadd", "obj", "k2", at(9, 2, 2))],
            [("k0", ("k1",)), ("k0", ("k2",))], []),
    "self": ([("pfadd", "obj", "k0", at(5, 3, 1)), ("pfadd", "obj", "k1", at(9, 2, 2))],
             [("k0", ("k0", "k1"))], []),
    "union_cache": ([("pfadd", "obj", "k0", at(5, 3, 1)), ("pfadd", "obj", "k1", at(9, 2, 2))],
                    [], [("k0", "k1"), ("k0",), ("k0", "k0")]),
    "no_sources": ([("set", "obj", "k0", M.header(1, 77) + bytes([0x7F, 0xFF]))],
                   [("k0", ()), ("k1", ("k9",)), ("k0", ("k9", "k10"))], []),
    "dense_source": ([("pfadd", "obj", "k0", at(5, 3, 1)), ("set", "obj", "k1", small_dense())],
                     [("k0", ("k1",)), ("k2", ("k0",))], []),
}


def prepared(setup) -> Keyspace:
    ks = Keyspace()
    for cmd in setup:
        getattr(ks, cmd[0])(*cmd[1:])
    return ks


# ---- the seeded sequences ----------------------------------------------------------------------------------------
def setup(seed: int):
    """hll_driver command tuples that prepare a seed's keyspace: two dense strings and two sparse strings that are not
    normalized, with valid cached cardinalities that are wrong, one of them with a TTL; the other keys start missing"""
    return [("set", "obj", "k1", D.dense_string(seed)), ("set", "obj", "k2", D.odd_string(seed)),
            ("set", "obj", "k3", D.odd_string(seed + 3)), ("set", "obj", "k4", D.dense_string(seed + 7)),
            ("expire", "obj", "k2")]


def seeded(seed: int, steps: int = STEPS):
    """steps of ('count', groups) / ('merge', merges) / ('stream', cmds) / ('countWith', keys) / ('mergeWith', dest,
    srcs) / ('set', key, string) / ('delete', key) over KEYS + BITS + BLOOM"""
    rng = np.random.default_rng([0x6A0F5, seed])
    serial = [0]
    pool = KEYS + (BITS, BLOOM)

    def ser():
        serial[0] += 1
        return 500_000 + 1000 * seed + serial[0]

    def key(p_wrong=0.04):
        return pool[int(rng.integers(12, 14))] if rng.random() < p_wrong else KEYS[int(rng.integers(0, 12))]

    def spec():
        r = rng.random()
        if r < 0.15:
            return SM.NONE
        if r < 0.55:
            return ("low", ser(), int(rng.integers(1, 6)))
        if r < 0.8:
            return ("crafted", ser(), int(rng.integers(1, 6)))
        if r < 0.9:
            return ("rows", ser(), int(rng.choice((1, 300))))
        return at(int(rng.integers(0, M.REGS)), int(rng.choice((1, 33, 50, 51))), ser())

    out = []
    for _ in range(steps):
        r = rng.random()
        if r < 0.27:
            groups = [tuple(key() for _ in range(int(rng.choice((1, 1, 2, 3, 5, 9))))) for _ in range(int(rng.integers(1, 9)))]
            out.append(("count", groups))
        elif r < 0.55:
            merges = []
            for _ in range(int(rng.integers(1, 8))):
                dest = key(0.03)
                if merges and rng.random() < 0.5:  # a hazard on purpose: an earlier destination or source again
                    d0, s0 = merges[int(rng.integers(0, len(merges)))]
                    pick = rng.random()
                    srcs = tuple(key() for _ in range(int(rng.integers(0, 3))))
                    if pick < 0.35:
                        srcs += (d0,)
                    elif pick < 0.7 and s0:
                        dest = s0[0]
                    else:
                        dest = d0
                else:
                    srcs = tuple(key() for _ in range(int(rng.integers(0, 4))))
                merges.append((dest, srcs))
            out.append(("merge", merges))
        elif r < 0.72:
            cmds = []
            for _ in range(int(rng.integers(1, 7))):
                k = key()
                cmds.append((k, SM.PFCOUNT, SM.NONE) if rng.random() < 0.3 else (k, SM.PFADD, spec()))
            out.append(("stream", cmds))
        elif r < 0.8:
            out.append(("countWith", tuple(KEYS[int(i)] for i in rng.integers(0, 12, size=int(rng.integers(1, 4))))))
        elif r < 0.88:
            out.append(("mergeWith", KEYS[int(rng.integers(0, 12))],
                        tuple(KEYS[int(i)] for i in rng.integers(0, 12, size=int(rng.integers(0, 3))))))
        elif r < 0.95:
            k = KEYS[int(rng.integers(0, 12))]
            s = (D.dense_string, D.odd_string)[int(rng.integers(0, 2))](int(rng.integers(0, 50)))
            out.append(("set", k, s))
        else:
            out.append(("delete", KEYS[int(rng.integers(0, 12))]))
    return out


def apply_step(ks: Keyspace, step):
    """a seeded step on the model: what the engine must answer"""
    kind = step[0]
    if kind == "count":
        return count_groups(ks, step[1])
    if kind == "merge":
        return merge_groups(ks, step[1])
    if kind == "stream":
        return SM.stream(ks, step[1])
    if kind == "countWith":
        keys = step[1]
        return ks.pfcount("obj", keys[0]) if len(keys) == 1 else ks.pfcount_multi("obj", keys[0], keys[1:])
    if kind == "mergeWith":
        return ks.pfmerge("obj", step[1], step[2])
    if kind == "set":
        return ks.set("obj", step[1], step[2])
    if kind == "delete":
        return ks.delete("obj", step[1])
    raise AssertionError(step)


def union_count(ks: Keyspace, keys) -> int:
    mx = O.hll_new()
    for k in keys:
        mx = np.maximum(mx, ks.registers(k))
    return O.hll_count(mx)
