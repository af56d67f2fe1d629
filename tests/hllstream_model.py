"""A model of rbx_hll_stream: the commands applied one at a time, in array order, to hll_model.Keyspace (exact
headers, sparse strings built element by element), under the pipelined-batch rule -- a command on a key of another
type fails alone, changes and creates nothing, and the first failure in array order decides the return code.  Also a
restatement of the host's phase splitter, the deliberately wrong streams the CPU test must catch, and the seeded
streams the CPU and GPU tests share.  Shares no code with the engine.

A command is (key, op, spec): a key of hll_driver's (or BITS / BLOOM, the keys of another type), PFADD or PFCOUNT, and
an element spec of hll_model.materialize (("none",) for a PFCOUNT and for an empty PFADD)."""
import numpy as np

import hll_driver as D
import hll_model as M
from hll_model import BITS, BLOOM, WRONGTYPE, Keyspace
from oracle import oracle as O

PFADD, PFCOUNT = 0, 1
RAN, FAILED = 0, 0xFF
NONE = ("none",)
KEYS = ("a", "b", "c", "d", "e", "f")  # the six HLL keys of a seeded stream
SEEDS = tuple(range(40))


def wrong(key) -> bool:
    return key in (BITS, BLOOM)


def stream(ks: Keyspace, cmds, events=None):
    """(return code kind, replies, status) of the commands one at a time; events (a list) collects, per command,
    what the model noted"""
    kind, replies, status = None, [], []
    for key, op, spec in cmds:
        reply, err = ks.pfadd("stream", key, spec) if op == PFADD else ks.pfcount("stream", key)
        if events is not None:
            events.append(list(ks.events))
        if err is not None:
            assert err == WRONGTYPE
            kind = kind or WRONGTYPE
            replies.append(0)
            status.append(FAILED)
        else:
            replies.append(int(reply))
            status.append(RAN)
    return kind, replies, status


def phases(cmds):
    """The host's splitter restated: [(count indexes, add indexes), ...].  A phase is a maximal stretch in which no
    PFCOUNT names a key that an earlier PFADD of the stretch names; a command that fails alone is in neither list."""
    out, counts, adds, added = [], [], [], set()
    for i, (key, op, _spec) in enumerate(cmds):
        if wrong(key):
            continue
        if op == PFCOUNT and key in added:
            out.append((counts, adds))
            counts, adds, added = [], [], set()
        if op == PFADD:
            adds.append(i)
            added.add(key)
        else:
            counts.append(i)
    if counts or adds or not out:
        out.append((counts, adds))
    return out


def stream_by_phases(ks: Keyspace, cmds, counts_first=True):
    """the commands executed the engine's way: per phase its PFCOUNTs, then its PFADDs (counts_first=False: the
    wrong order)"""
    n = len(cmds)
    replies, status = [0] * n, [FAILED if wrong(k) else RAN for k, _, _ in cmds]
    for counts, adds in phases(cmds):
        for group in ((counts, adds) if counts_first else (adds, counts)):
            for i in group:
                key, op, spec = cmds[i]
                reply, err = ks.pfadd("stream", key, spec) if op == PFADD else ks.pfcount("stream", key)
                assert err is None
                replies[i] = int(reply)
    return (WRONGTYPE if FAILED in status else None), replies, status


def state(ks: Keyspace):
    """everything a test reads back: per key the stored string (header included), registers and TTL flag"""
    return {k: (v.string(), v.h.regs.tobytes(), v.ttl) for k, v in sorted(ks.keys.items())}


# ---- deliberately wrong streams -------------------------------------------------------------------------------
class _UnchangedInvalidates(Keyspace):
    def _invalidate(self, k, changed):
        k.card |= M.INVALID


class _RegisterOrder(Keyspace):
    def _elements(self, k, x):
        if k.dense or len(x) == 0:
            return x
        x = [bytes(r) for r in x]
        return sorted(x, key=lambda e: O.hll_patlen(e)[0])


def copy_keyspace(ks: Keyspace, cls=Keyspace) -> Keyspace:
    out = cls()
    for key, k in ks.keys.items():
        out.keys[key] = M.Hll(M.clone(k.h), k.card, k.ttl)
    return out


def wrong_stream(defect: str, ks: Keyspace, cmds):
    """(result, final state) of a wrong model:
      'start'    replies judged against the registers at the start of the stream
      'created'  created = 1 on every PFADD of a key the stream created
      'inval'    an unchanged PFADD sets the invalid bit
      'order'    a phase's counts run after its adds
      'failed'   a failed command creates its key
      'regorder' sparse elements applied in register order, not command order"""
    if defect == "order":
        ks = copy_keyspace(ks)
        return stream_by_phases(ks, cmds, counts_first=False), state(ks)
    if defect == "inval":
        ks = copy_keyspace(ks, _UnchangedInvalidates)
        return stream(ks, cmds), state(ks)
    if defect == "regorder":
        ks = copy_keyspace(ks, _RegisterOrder)
        return stream(ks, cmds), state(ks)
    start = copy_keyspace(ks)
    ks = copy_keyspace(ks)
    kind, replies, status = stream(ks, cmds)
    created = set()
    for i, (key, op, spec) in enumerate(cmds):
        if wrong(key):
            if defect == "failed":
                ks.keys[key] = M.Hll()
            continue
        if op != PFADD:
            continue
        if key not in start.keys:
            created.add(key)
        if defect == "created" and key in created:
            replies[i] = 1
        if defect == "start" and key in start.keys and M.count_of(spec):
            replies[i] = int(bool(M.clone(start.keys[key].h).pfadd(*M.oracle_arena(M.materialize(spec)))))
    return (kind, replies, status), state(ks)


DEFECTS = ("start", "created", "inval", "order", "failed", "regorder")


# ---- the seeded streams -----------------------------------------------------------------------------------------
def setup(seed: int):
    """the commands that prepare a seed's keyspace, as hll_driver command tuples (set / expire / pfcount): a dense
    string and a sparse string that is not normalized, both with a valid cached cardinality that is wrong; the other
    keys start missing"""
    return [("set", "obj", "b", D.dense_string(seed)), ("set", "obj", "c", D.odd_string(seed)),
            ("set", "obj", "d", D.odd_string(seed + 3)), ("expire", "obj", "c")]


def seeded(seed: int):
    """two streams of about 100 commands each over KEYS + BITS + BLOOM; the second carries on from the first's state"""
    rng = np.random.default_rng([0x5712EA, seed])
    serial = [0]

    def ser():
        serial[0] += 1
        return 100_000 + 1000 * seed + serial[0]

    def spec_for(key):
        r = rng.random()
        if r < 0.12:
            return NONE
        if key in "acd" and r < 0.37:  # a permuted run of adjacent registers: the string depends on the order
            base, count = 300 + 16 * int(rng.integers(0, 8)), int(rng.integers(1, 4))
            regs = base + rng.permutation(int(rng.integers(5, 10)))
            return ("at", ser(), tuple((int(x), count, 16) for x in regs))
        if key == "a":  # fresh and small: stays sparse, its string follows the elements' order
            return ("low", ser(), int(rng.integers(1, 5))) if r < 0.8 else ("crafted", ser(), int(rng.integers(1, 4)))
        if key == "e":  # crosses hll-sparse-max-bytes inside a stream
            return ("rows", ser(), int(rng.choice((1, 200, 400))))
        if key == "f" and r < 0.3:  # one register, rising counts: promotion by value at 33
            return ("at", ser(), ((77, int(rng.choice((1, 2, 3, 32, 33, 50))), 16),))
        if r < 0.6:
            return ("low", ser(), int(rng.integers(1, 7)))
        return ("crafted", ser(), int(rng.integers(1, 7)))

    out = []
    for half in range(2):
        cmds, prev, old = [], None, {}
        n = int(rng.integers(90, 111))
        while len(cmds) < n:
            r = rng.random()
            key = prev if prev is not None and r < 0.35 else (KEYS + (BITS, BLOOM))[int(rng.integers(0, 8))]
            if not wrong(key) and rng.random() < 0.12:  # a burst on one key: three or more PFADDs of one run
                for _ in range(3):
                    cmds.append((key, PFADD, spec_for(key)))
            if rng.random() < 0.28:
                cmds.append((key, PFCOUNT, NONE))
            else:
                spec = old[key] if key in old and rng.random() < 0.2 else spec_for(key)  # a repeat changes nothing
                old[key] = spec
                cmds.append((key, PFADD, spec))
            prev = key
        if half == 0:
            cmds[3:3] = [("b", PFCOUNT, NONE), ("c", PFCOUNT, NONE)]  # before any add: the cached values as they stand
        out.append(cmds)
    return out


def coverage(seeds=SEEDS) -> dict:
    """what the seeded streams contain, counted on the model alone"""
    got = {"three adds of one key in a run": 0, "promoted by value": 0, "promoted by bytes": 0, "replay": 0,
           "wrong cache hit": 0, "failed alone": 0, "empty add creates": 0}
    for seed in seeds:
        ks = Keyspace()
        for cmd in setup(seed):
            getattr(ks, cmd[0])(*cmd[1:])
        for cmds in seeded(seed):
            for _counts, adds in phases(cmds):
                keys = [cmds[i][0] for i in adds]
                got["three adds of one key in a run"] += any(keys.count(k) >= 3 for k in set(keys))
            for (key, op, spec), _ in zip(cmds, cmds):
                if op == PFADD and spec == NONE and not wrong(key) and key not in ks.keys:
                    got["empty add creates"] += 1
                events = []
                _kind, _r, status = stream(ks, [(key, op, spec)], events)
                got["failed alone"] += status[0] == FAILED
                for ev in events[0]:
                    got["promoted by value"] += ev == ("promoted", "value in pfadd")
                    got["promoted by bytes"] += ev == ("promoted", "bytes in pfadd")
                    got["replay"] += ev == ("replay",)
                    got["wrong cache hit"] += ev == ("cache hit", True)
    return got
