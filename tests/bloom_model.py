"""The keyspace model of the Bloom filter command sequences (bloom_driver.py): bitstring_model.Keyspace -- names,
strings, timeouts, the other type, RedisString -- extended by what RBloomFilter keeps beside the string.

A filter is two keys, as in the reference: `name` holds the Redis string its SETBITs write and `{name}:config` the
hash (size, hashIterations, expectedInsertions); either may exist without the other, each has a timeout of its own,
and DEL / RENAME / PEXPIRE / PERSIST go over both in RedissonBloomFilter's order.  A handle is (name, size, k) as
read when it was opened: it follows its NAME, and every call through it first checks that the name's config still
is (size, k) -- addConfigCheck.  An absent string reads as zeros and stays absent; only an add creates it.

Every command is `method(via, key, *args) -> (reply, error kind or None)`.  Hashing is oracle.bloom_hash_batch.
The replies of an add follow the one-command-at-a-time rule of Keyspace.bloom_add: key i is new when it sets a bit
that neither the string nor a key before it had set.  A multi call is its segments in order, a stream call its
commands in order, and neither has a rule of its own; a call that ends in an error changes nothing.

`events` collects what a command met (bloom_driver.stats counts them); the `_hooks` are where FaultyModelEngine
injects its defects.  Nothing here is read from the engine."""
import numpy as np

import bitset_model as SM
from bitstring_model import (BIT_OFFSET, ILLEGAL, NO_SUCH_KEY, NOT_INIT, REDIS, WRONGTYPE, Failed, Keyspace,  # noqa: F401
                             command)
from oracle import oracle as O

CONFIG, ARITH = "config has been changed", "/ by zero"
STREAM_KMAX = 32  # rbx_bloom_stream: k <= 32

_rng = np.random.default_rng(0xB100)
VAR = [_rng.bytes(int(n)) for n in _rng.integers(0, 41, size=3000)]  # lengths 0 .. 40 (two may be equal: the short ones)
VAR[0], VAR[1] = b"", b"\x00"
S16 = np.random.default_rng(0xB116).integers(0, 256, size=(2000, 16), dtype=np.uint8)
S32 = np.random.default_rng(0xB132).integers(0, 256, size=(1000, 32), dtype=np.uint8)
POOLS = {"v": len(VAR), "s16": len(S16), "s32": len(S32)}


def keys_of(spec):
    """spec = (pool, ids), or ("lit", keys) -> the keys as a list of bytes"""
    pool, ids = spec
    if pool == "lit":  # the keys themselves
        return list(ids)
    if pool == "v":
        return [VAR[i] for i in ids]
    mat = S16 if pool == "s16" else S32
    return [mat[i].tobytes() for i in ids]


def matrix_of(spec):
    """the fixed-stride pools as a uint8 matrix (None for the pool of varying lengths)"""
    pool, ids = spec
    if pool in ("v", "lit"):
        return None
    return np.ascontiguousarray((S16 if pool == "s16" else S32)[np.asarray(ids, np.int64).reshape(-1)])


def indexes(size, k, keys):
    """uint64[n, k]: the bit indexes of each key"""
    buf, offs = O.arena(list(keys))
    return O.bloom_hash_batch(buf, offs, k, size).astype(np.uint64)


class BloomKeyspace(Keyspace):
    def __init__(self):
        super().__init__()
        self.expected = {}        # name -> expectedInsertions of its config (0: tryInitRaw)
        self.cfg_timeout = set()  # names whose CONFIG key has a timeout
        self.handles = {}         # handle id -> (name, size, k)
        self.digests = {}         # name -> the string the last digest read saw
        self.events = []

    # ---- what Keyspace does for a string alone, over both keys -------------------------------------------
    def _put(self, key, new, how="write"):
        if new == b"" and how == "set":  # SET name "": the empty string exists
            self.data[key] = b""
            self.timeout.discard(key)
            return
        super()._put(key, new, how)

    def _present(self, key):
        return key in self.data or key in self.hll

    def _drop_config(self, key):
        self.cfg.pop(key, None)
        self.expected.pop(key, None)
        self.cfg_timeout.discard(key)

    def _drop_string(self, key):
        self.data.pop(key, None)
        self.hll.discard(key)
        self.timeout.discard(key)

    def _move_string(self, key, new):
        value, timed, hll = self.data.get(key), key in self.timeout, key in self.hll
        self._drop_string(key)
        self._drop_string(new)
        if hll:
            self.hll.add(new)
        else:
            self.data[new] = value
        if timed:
            self.timeout.add(new)

    def _move_config(self, key, new):
        cfg, exp, timed = self.cfg[key], self.expected[key], key in self.cfg_timeout
        self._drop_config(key)
        self._drop_config(new)
        self.cfg[new], self.expected[new] = cfg, exp
        if timed:
            self.cfg_timeout.add(new)

    @command
    def exists(self, via, key):
        return self._present(key) or key in self.cfg

    @command
    def size_in_memory(self, via, key):
        """compared as zero / non-zero only"""
        return self._present(key) or key in self.cfg

    @command
    def delete(self, via, key):
        had = self._present(key) or key in self.cfg
        self._deleted(key)
        self._drop_string(key)
        self._drop_config(key)
        return had

    @command
    def rename(self, via, key, new):
        """the script of renameAsync: the string if it exists, then the config (whose absence fails the script
        after the string has moved)"""
        if key == new:
            if key not in self.cfg:
                raise Failed(NO_SUCH_KEY)
            return None
        if self._present(key):
            self._move_string(key, new)
        if key not in self.cfg:
            raise Failed(NO_SUCH_KEY)
        self._rename_config(key, new)
        self.events.append(("renamed", key, new))
        return None

    @command
    def renamenx(self, via, key, new):
        if not self._present(key):
            raise Failed(NO_SUCH_KEY)
        if self._present(new):
            return False
        self._move_string(key, new)
        if key not in self.cfg:
            raise Failed(NO_SUCH_KEY)
        if new in self.cfg:
            return False
        self._rename_config(key, new)
        self.events.append(("renamed", key, new))
        return True

    @command
    def expire(self, via, key, when):
        """when: 'hour' = PEXPIRE of an hour on both keys, 'past' = PEXPIREAT 1, which deletes them"""
        had = self._present(key) or key in self.cfg
        if when == "past":
            self._deleted(key)
            self._drop_string(key)
            self._drop_config(key)
            return had
        if self._present(key):
            self.timeout.add(key)
        if key in self.cfg:
            self.cfg_timeout.add(key)
        return had

    @command
    def clear_expire(self, via, key):
        had = key in self.timeout or key in self.cfg_timeout
        self.timeout.discard(key)
        self.cfg_timeout.discard(key)
        return had

    @command
    def ttl(self, via, key):
        """PTTL name: the string's alone"""
        return "missing" if not self._present(key) else "set" if key in self.timeout else "none"

    def bitop_not(self, via, dest, src):
        return super().bitop_not("obj", dest, src)  # RBitSet.not_() returns nothing

    # ---- the config ------------------------------------------------------------------------------------------
    @command
    def try_init(self, via, key, n, p):
        size, k = O.bloom_optimal(n, p)
        return self._init(key, size, k, n)

    @command
    def init_raw(self, via, key, size, k):
        return self._init(key, size, k, 0)

    def _init(self, key, size, k, expected):
        if key in self.cfg:
            return False
        self.cfg[key], self.expected[key] = (size, k), expected
        self.events.append(("created", key, (size, k)))
        return True

    @command
    def config(self, via, key):
        if key not in self.cfg:
            raise Failed(NOT_INIT)
        return [*self.cfg[key], self.expected[key]]

    # ---- the hooks ---------------------------------------------------------------------------------------------
    def _deleted(self, key):
        """before DEL / an expiry in the past removes both keys"""

    def _rename_config(self, key, new):
        self._move_config(key, new)

    def _count_config(self, key):
        return self.cfg[key]

    def _add_flags(self, keys, was, first, k):
        """was[j]: bit j of the flattened indexes was set before the batch; first: the position of each distinct
        index's first occurrence"""
        flags = np.zeros(len(keys), bool)
        flags[first[~was[first]] // k] = True
        return flags

    def _lengthens(self, flags):
        return True

    def _read_view(self, key, how):
        """the string a contains reads; how: 'name', 'handle', 'multi' or 'stream'"""
        return self._get(key)

    def _contains_side_effect(self, key, idx):
        pass

    def _mismatch_writes(self, name, size, k, keys):
        pass

    def _imported(self, key, data):
        return data

    # ---- add / contains on one name with one (size, k) ------------------------------------------------------------
    def _add(self, name, size, k, keys, how):
        idx = indexes(size, k, keys)
        flat = idx.reshape(-1)
        before = self._get(name)
        was = SM.RedisString(self._read_view(name, how)).get_indexes(flat)
        _u, first = np.unique(flat, return_index=True)
        flags = self._add_flags(keys, was, first, k)
        s = SM.RedisString(before)
        s.set_indexes(flat, 1)
        new = s.bytes()
        if not self._lengthens(flags):
            new = new[:max(len(before or b""), 1)]
        self._put(name, new)
        self._note_add(name, keys, idx, was, flags, len(before or b""), len(new))
        return flags

    def _note_add(self, name, keys, idx, was, flags, len0, len1):
        k = idx.shape[1]
        if len(set(keys)) < len(keys):
            self.events.append(("duplicate", name))
        if not flags.any():
            self.events.append(("all present", name))
        if len1 > len0 and not flags[-1]:
            self.events.append(("lengthens, last key not new", name))
        zero = ~was.reshape(-1, k)  # keys whose zero bits are one index: two different keys on the same one
        lo = np.where(zero, idx, np.uint64(2**63)).min(axis=1)
        hi = np.where(zero, idx, np.uint64(0)).max(axis=1)
        only = {}
        for i in np.flatnonzero(zero.any(axis=1) & (lo == hi)):
            only.setdefault(int(lo[i]), set()).add(keys[i])
        if any(len(v) > 1 for v in only.values()):
            self.events.append(("shared zero bit", name))

    def _contains(self, name, size, k, keys, how):
        idx = indexes(size, k, keys)
        flags = SM.RedisString(self._read_view(name, how)).get_indexes(idx.reshape(-1)).reshape(-1, k).all(axis=1)
        self._contains_side_effect(name, idx)
        return flags

    @staticmethod
    def _reply(flags, per_key):
        return [int(flags.sum()), flags.astype(int).tolist() if per_key else None]

    # ---- by name: RBloomFilter, rbx_bloom_add / _contains and their async forms --------------------------------
    def _by_name(self, key, spec, per_key, cached, is_add):
        """cached: the (size, k) the caller holds, None = it reads the config first.  The order of the checks is
        the reference's: readConfig, addConfigCheck, the division by the collection's size, then the commands."""
        if cached is None:
            if key not in self.cfg:
                raise Failed(NOT_INIT)
            cached = self.cfg[key]
        if self.cfg.get(key) != tuple(cached):
            raise Failed(CONFIG)
        keys = keys_of(spec)
        if not keys:
            raise Failed(ARITH)
        self._get(key)  # WRONGTYPE
        size, k = cached
        flags = (self._add if is_add else self._contains)(key, size, k, keys, "name")
        return self._reply(flags, per_key)

    @command
    def _named(self, op, key, spec, per_key, cached):
        return self._by_name(key, spec, per_key, cached, op == "add")

    def _queued(self, op, key, spec, per_key, cached, more):
        """more: the (op, key, spec, per_key, cached) calls queued behind this one before any is waited for (the
        async forms); they run in that order, whatever the first one answers"""
        reply, err = self._named(op, key, spec, per_key, cached)
        if more:
            reply = [reply, [list(self._named(*m)) for m in more]]
        return reply, err

    def add(self, via, key, spec, per_key, cached=None, more=()):
        return self._queued("add", key, spec, per_key, cached, more)

    def contains(self, via, key, spec, per_key, cached=None, more=()):
        return self._queued("contains", key, spec, per_key, cached, more)

    # ---- handles ---------------------------------------------------------------------------------------------------
    @command
    def open(self, via, key, hid):
        if key not in self.cfg:
            raise Failed(NOT_INIT)
        self._get(key)
        self.handles[hid] = (key, *self.cfg[key])
        return list(self.cfg[key])

    @command
    def close(self, via, key, hid):
        del self.handles[hid]

    def _bound(self, hid, write=None):
        """addConfigCheck, then the type of what the name holds; write: the keys an add would have written"""
        name, size, k = self.handles[hid]
        if self.cfg.get(name) != (size, k):
            if write is not None and name in self.cfg and name not in self.hll:
                self._mismatch_writes(name, size, k, write)
            raise Failed(CONFIG)
        self._get(name)
        return name, size, k

    def handle_is_current(self, hid):
        name, size, k = self.handles[hid]
        return self.cfg.get(name) == (size, k) and name not in self.hll

    @command
    def add_dev(self, via, key, hid, spec, per_key, layout=None):
        keys = keys_of(spec)
        if not keys:
            raise Failed(ARITH)
        self.events.append(("handle call", self.handles[hid][0], hid))
        name, size, k = self._bound(hid, keys)
        return self._reply(self._add(name, size, k, keys, "handle"), per_key)

    @command
    def contains_dev(self, via, key, hid, spec, per_key, layout=None):
        keys = keys_of(spec)
        if not keys:
            raise Failed(ARITH)
        self.events.append(("handle call", self.handles[hid][0], hid))
        name, size, k = self._bound(hid)
        return self._reply(self._contains(name, size, k, keys, "handle"), per_key)

    # ---- many filters in one call -------------------------------------------------------------------------------
    def _segments(self, via, segs, is_add):
        """segs: ((handle id, spec), ...).  The host form refuses an empty segment before it looks at a handle;
        the device form runs it as nothing."""
        parts = [keys_of(spec) for _h, spec in segs]
        if via == "multi" and any(not p for p in parts):
            raise Failed(ARITH)
        bound = [self._bound(hid) for hid, _ in segs]
        names = [b[0] for b in bound]
        if len(set(names)) < len(names):
            self.events.append(("repeated tenant",))
        self.events.append(("multi", is_add, tuple(h for h, _ in segs), tuple(names),
                            tuple(n for n in names if n not in self.data)))
        counts, flags, seen = [], [], set()
        for (name, size, k), keys in zip(bound, parts):
            if not keys:
                counts.append(0)
                continue
            if is_add:
                f = self._multi_add(name, size, k, keys, name in seen)
            else:
                f = self._contains(name, size, k, keys, "multi")
            seen.add(name)
            counts.append(int(f.sum()))
            flags += f.astype(int).tolist()
        return counts, flags

    def _multi_add(self, name, size, k, keys, again):
        return self._add(name, size, k, keys, "multi")

    @command
    def add_multi(self, via, key, segs, per_key):
        counts, flags = self._segments(via, segs, True)
        return [counts, flags if per_key else None]

    @command
    def contains_multi(self, via, key, segs, per_key):
        counts, flags = self._segments(via, segs, False)
        return [counts, flags if per_key else None]

    @command
    def stream(self, via, key, hids, kf, ops, spec):
        """command i: ops[i] (1 add, 0 contains) of key i on handle hids[kf[i]]; reply: (flags, [present, new])"""
        bound = []
        for h in hids:  # handle by handle: its k, its config, the type under its name
            if self.handles[h][2] > STREAM_KMAX:
                raise Failed(ILLEGAL)
            bound.append(self._bound(h))
        keys = keys_of(spec)
        rows = [None] * len(keys)
        for f, (name, size, k) in enumerate(bound):  # one hashing call per filter
            at = [i for i, g in enumerate(kf) if g == f]
            for i, row in zip(at, indexes(size, k, [keys[i] for i in at]) if at else ()):
                rows[i] = row
        before = {name: SM.RedisString(self._get(name)) for name, _s, _k in bound}
        now = {name: SM.RedisString(self._get(name)) for name, _s, _k in bound}
        out, counts, added, wrote = [], [0, 0], set(), set()
        for f, op, key_, row in zip(kf, ops, keys, rows):
            name = bound[f][0]
            if op:
                flag = not now[name].get_indexes(row).all()
                now[name].set_indexes(row, 1)
                added.add((name, key_))
                wrote.add(name)
            else:
                again = (name, key_) in added
                flag = bool(self._stream_view(now, before, name, again).get_indexes(row).all())
                if again:
                    self.events.append(("stream add then contains",))
            out.append(int(flag))
            counts[1 if op else 0] += flag
        for name in wrote:
            self._put(name, now[name].bytes())
        return [out, counts]

    def _stream_view(self, now, before, name, added_before):
        return now[name]

    # ---- the string as a whole -----------------------------------------------------------------------------------
    @command
    def count(self, via, key):
        if key not in self.cfg:
            raise Failed(NOT_INIT)
        size, k = self._count_config(key)
        return int(O.lib().orc_bloom_count_estimate(SM.RedisString(self._get(key)).bitcount(), size, k))

    @command
    def bitcount(self, via, key):
        return SM.RedisString(self._get(key)).bitcount()

    @command
    def digest(self, via, key):
        """'first', 'same' or 'changed' against the read before it: the value itself is the engine's own"""
        now = self._get(key)
        reply = "first" if key not in self.digests else "same" if self.digests[key] == now else "changed"
        self.digests[key] = now
        return reply

    @command
    def export(self, via, key):
        return self._get(key) or b""

    @command
    def import_bitmap(self, via, key, data):
        """SET name data: whatever the name held, timeout included, is replaced (the config is another key)"""
        self.hll.discard(key)
        self._put(key, self._imported(key, bytes(data)), "set")
        self.events.append(("imported", key))
