"""One keyspace model for command sequences that mix the bit-command families on shared keys.

A bit-string key is a non-empty `bytes` value plus a "has a timeout" flag; one key may be an HLL (another
type, for WRONGTYPE replies); a name may carry a Bloom config (size, k).  The rules of the commands are those of
the four family models, which are called and not restated: bitset_model (SETBIT / GETBIT / index batches / range
fill / BITOP / the length script), bitfield_model (GET and the WRAP fields), bitfield_overflow_model (SAT / FAIL and
the mixed list) and bitrange_model (ranged BITCOUNT / BITPOS).  Bloom commands are oracle.bloom_hash_batch followed
by set_indexes / get_indexes, with OracleBloom's in-order first-setter rule for the per-key "new" flags.

Every command is `method(via, key, *args) -> (reply, error kind or None)`; `via` names the caller's form (object,
Spring Data connection, device arrays, Bloom handle) and changes nothing here.  A command that errors leaves the
model unchanged.  What this file adds of its own is key-level only: which writes keep a timeout (SETBIT-style
ones) and which drop it (BITOP, SET, DEL), RENAME, and the order "arguments, then the key's type"."""
import numpy as np

import bitfield_model as FM
import bitfield_overflow_model as OM
import bitrange_model as RM
import bitset_model as SM

WRONGTYPE, BIT_OFFSET, ILLEGAL, NO_SUCH_KEY, REDIS, NOT_INIT = \
    "WRONGTYPE", "bit offset", "illegal argument", "no such key", "redis error", "not initialized"

GET, SET, INCRBY = FM.GET, FM.SET, FM.INCRBY
MODES = {"WRAP": OM.WRAP, "SAT": OM.SAT, "FAIL": OM.FAIL}
UNITS = {"BYTE": RM.BYTE, "BIT": RM.BIT}
# the typed forms of RBitSet: (signed, size or None = the caller's)
FORMS = {"signed": (True, None), "unsigned": (False, None), "byte": (True, 8), "short": (True, 16),
         "integer": (True, 32), "long": (True, 64)}

POOL = np.random.default_rng(0xB100F).integers(0, 256, size=(2000, 16), dtype=np.uint8)  # the Bloom keys there are


class Failed(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def command(fn):
    """-> (reply, None) or (None, error kind); the family models' exceptions become kinds"""
    def run(self, *args):
        try:
            return fn(self, *args), None
        except Failed as e:
            return None, e.kind
        except FM.IllegalArgument:
            return None, ILLEGAL
        except (SM.RedisError, FM.RedisError, RM.RedisError) as e:
            return None, BIT_OFFSET if "bit offset" in str(e) else REDIS
    run.__name__ = fn.__name__
    return run


def resolve_modes(rows):
    """redisson_amd.spring_data.resolve_overflow over plain rows (op, signed, size, offset, value, overflow)"""
    from redisson_amd.spring_data import BitFieldGet, BitFieldIncrBy, BitFieldSet, BitFieldType, resolve_overflow

    cmds = []
    for op, signed, size, offset, value, overflow in rows:
        t = BitFieldType(signed, size)
        cmds.append(BitFieldGet(t, offset) if op == GET else BitFieldSet(t, offset, value) if op == SET
                    else BitFieldIncrBy(t, offset, value, overflow))
    return [MODES[m] for m in resolve_overflow(cmds)]


class Keyspace:
    def __init__(self):
        self.data = {}     # name -> non-empty bytes
        self.timeout = set()
        self.hll = set()
        self.cfg = {}      # name -> (size, k)

    # ---- the three places a defect can be injected (FaultyModelEngine) -----------------------------
    def _get(self, key):
        """the string, None for a missing key"""
        if key in self.hll:
            raise Failed(WRONGTYPE)
        return self.data.get(key)

    def _padded(self, key):
        """what a reader that may look past the string's end sees: the string (the rest reads as zero)"""
        return self._get(key)

    def _put(self, key, new, how="write"):
        """how: 'write' = SETBIT-style (keeps a timeout), 'bitop' / 'set' store a new value without one"""
        if not new:
            self.data.pop(key, None)
            self.timeout.discard(key)
            return
        self.data[key] = bytes(new)
        if how != "write":
            self.timeout.discard(key)

    def _handle_view(self, key):
        """the string an open Bloom handle reads"""
        return self._get(key)

    def strlen(self, key):
        return len(self.data.get(key, b""))

    # ---- single bits, index batches, ranges (bitset_model) -------------------------------------------
    def _string(self, key, padded=False):
        return SM.RedisString(self._padded(key) if padded else self._get(key))

    @command
    def setbit(self, via, key, i, value):
        s = self._string(key)
        old = s.setbit(i, value)
        self._put(key, s.bytes())
        return bool(old)

    @command
    def clearbit(self, via, key, i):
        s = self._string(key)
        old = s.setbit(i, 0)
        self._put(key, s.bytes())
        return bool(old)

    @command
    def getbit(self, via, key, i):
        return bool(self._string(key, True).getbit(i))

    @command
    def set_indexes(self, via, key, idx, value):
        s = self._string(key)
        s.set_indexes(np.asarray(idx, np.uint64), value)
        self._put(key, s.bytes())

    @command
    def get_indexes(self, via, key, idx):
        return self._string(key, True).get_indexes(np.asarray(idx, np.uint64)).astype(int).tolist()

    @command
    def set_range(self, via, key, frm, to):
        if frm >= to:
            return None  # an empty range sends no command: not even the key's type is looked at
        s = self._string(key)
        s.set_range(frm, to, 1)
        self._put(key, s.bytes())

    @command
    def clear_range(self, via, key, frm, to):
        if frm >= to:
            return None
        s = self._string(key)
        s.set_range(frm, to, 0)
        self._put(key, s.bytes())

    # ---- BITOP ---------------------------------------------------------------------------------------
    def _bitop_value(self, op, dest, srcs, values):
        return SM.bitop(op, values)

    @command
    def bitop(self, via, dest, op, srcs):
        """reply: the result's length (RBitSet's own and / or / xor return nothing)"""
        self._get(dest)  # every operand's type first
        values = [self._get(s) or b"" for s in srcs]
        res = self._bitop_value(op, dest, srcs, values)
        self._put(dest, res, "bitop")
        return None if via == "obj" else len(res)

    @command
    def bitop_not(self, via, dest, src):
        self._get(dest)
        res = self._bitop_value("not", dest, (src,), [self._get(src) or b""])
        self._put(dest, res, "bitop")
        return None if via == "obj" else len(res)

    # ---- typed fields (bitfield_model, bitfield_overflow_model) ----------------------------------------
    def _on_window(self, key, lo_bit, hi_bit, fn, padded=False):
        """fn(window, shift) -> (window after, replies) on the bytes that hold bits [lo_bit, hi_bit): the family
        models work on big integers, which a string of a megabyte makes slow.  The window ends where the
        string does if that is earlier, so the model grows it exactly as it would the whole string."""
        data = (self._padded(key) if padded else self._get(key)) or b""
        first, last = lo_bit >> 3, (hi_bit - 1) >> 3
        win = data[first: last + 1]
        after, replies = fn(win, 8 * first)
        if after != win:
            head = data[:first] + bytes(max(0, first - len(data)))
            self._put(key, head + after + data[last + 1:])
        return replies

    @staticmethod
    def _form(form, size):
        signed, fixed = FORMS[form]
        return signed, size if fixed is None else fixed

    def _field(self, key, op, form, size, offset, value):
        signed, size = self._form(form, size)
        FM.check(signed, size, offset)  # the arguments before the key's type
        return self._on_window(key, offset, offset + size,
                               lambda w, sh: FM.field(w, op, signed, size, offset - sh, value), padded=op == GET)

    @command
    def field_get(self, via, key, form, size, offset):
        return self._field(key, GET, form, size, offset, 0)

    @command
    def field_set(self, via, key, form, size, offset, value):
        return self._field(key, SET, form, size, offset, value)

    @command
    def field_incr(self, via, key, form, size, offset, value):
        return self._field(key, INCRBY, form, size, offset, value)

    def _fields_model(self, win, op, signed, size, mode, offsets, values):
        if mode == OM.WRAP:
            return FM.fields(win, op, signed, size, offsets, values)
        return OM.fields(win, op, signed, size, mode, offsets, values)

    def _fields(self, key, op, signed, size, mode, offsets, values, replies):
        for o in offsets:
            FM.check(signed, size, int(o))
        lo, hi = min(offsets), max(offsets) + size
        got = self._on_window(key, lo, hi, lambda w, sh: self._fields_model(
            w, op, signed, size, MODES[mode], [o - sh for o in offsets], values), padded=op == GET)
        nil = [r is None for r in got] if mode == "FAIL" and op != GET else None
        return (got if replies else None), nil

    @command
    def get_fields(self, via, key, size, signed, offsets):
        return self._fields(key, GET, signed, size, "WRAP", offsets, None, True)[0]

    @command
    def set_fields(self, via, key, size, signed, offsets, values, mode, replies):
        """reply: (the old values or None without replies, the nil mask under FAIL or None)"""
        return self._fields(key, SET, signed, size, mode, offsets, values, replies)

    @command
    def incr_fields(self, via, key, size, signed, offsets, values, mode, replies):
        return self._fields(key, INCRBY, signed, size, mode, offsets, values, replies)

    @command
    def bitfield(self, via, key, rows):
        """Spring Data's bitField: rows of (op, signed, size, offset, value, overflow or None)"""
        modes = resolve_modes(rows)
        for (_op, signed, size, offset, _v, _o) in rows:
            OM.check_type(signed, size)
            FM.check(signed, size, offset)
        lo = min(r[3] for r in rows)
        hi = max(r[3] + r[2] for r in rows)
        return self._on_window(key, lo, hi, lambda w, sh: OM.bitfield(
            w, [(op, signed, size, m, offset - sh, value) for (op, signed, size, offset, value, _o), m in zip(rows, modes)]))

    # ---- ranged BITCOUNT / BITPOS (bitrange_model) -----------------------------------------------------
    @command
    def bitcount(self, via, key, start, end, unit):
        data = self._get(key)
        if start is None:
            return SM.RedisString(data).bitcount()
        return RM.bitcount(data, start, end, UNITS[unit])

    @command
    def bitpos(self, via, key, bit, nargs, start, end, unit):
        return RM.bitpos_nargs(self._get(key), bit, nargs, start, end, UNITS[unit])

    @command
    def count_ranges(self, via, key, starts, ends, unit):
        return [int(x) for x in RM.count_ranges(self._get(key), starts, ends, UNITS[unit])]

    @command
    def pos_ranges(self, via, key, bit, starts, ends, unit):
        return [int(x) for x in RM.pos_ranges(self._get(key), bit, starts, ends, UNITS[unit])]

    # ---- the whole string ------------------------------------------------------------------------------
    @command
    def cardinality(self, via, key):
        return SM.RedisString(self._get(key)).bitcount()

    @command
    def size(self, via, key):
        return 8 * len(self._get(key) or b"")

    @command
    def length(self, via, key):
        n = SM.lua_length(self._get(key) or b"")
        if n is None:
            raise Failed(BIT_OFFSET)
        return n

    @command
    def to_bytes(self, via, key):
        return self._get(key) or b""

    @command
    def set_bytes(self, via, key, nbytes, seed):
        """SET key <nbytes random bytes of that seed> (nbytes >= 1)"""
        self._put(key, np.random.default_rng(seed).bytes(nbytes), "set")

    # ---- key level ---------------------------------------------------------------------------------------
    @command
    def exists(self, via, key):
        return key in self.data or key in self.hll

    @command
    def delete(self, via, key):
        had = key in self.data
        self._put(key, None)
        return had

    @command
    def clear(self, via, key):
        self._put(key, None)

    @command
    def rename(self, via, key, new):
        if key not in self.data:
            raise Failed(NO_SUCH_KEY)
        if new == key:
            return None
        value, timed = self.data[key], key in self.timeout
        self._put(key, None)
        self._put(new, value, "set")
        if timed:
            self.timeout.add(new)  # RENAME carries the timeout along
        return None

    @command
    def expire(self, via, key):
        if key not in self.data:
            return False
        self.timeout.add(key)
        return True

    @command
    def clear_expire(self, via, key):
        had = key in self.timeout
        self.timeout.discard(key)
        return had

    @command
    def ttl(self, via, key):
        """'missing', 'none' or 'set': a remaining time is only ever checked to be there or not"""
        return "missing" if key not in self.data else "set" if key in self.timeout else "none"

    # ---- the other type, and Bloom ---------------------------------------------------------------------------
    @command
    def hll_init(self, via, key):
        self.hll.add(key)

    @command
    def bloom_init(self, via, key, size, k):
        if key in self.cfg:
            return False
        self.cfg[key] = (size, k)
        return True

    def _bloom_indexes(self, key, ids):
        from oracle import oracle as O

        if key not in self.cfg:
            raise Failed(NOT_INIT)
        size, k = self.cfg[key]
        buf, offs = O.fixed_arena(POOL[np.asarray(ids, np.int64)])
        return O.bloom_hash_batch(buf, offs, k, size).astype(np.uint64), k

    @command
    def bloom_add(self, via, key, ids):
        """reply: (how many keys were new, the per-key flags); key i is new when it sets a bit that neither the
        string nor a key before it in the batch had set"""
        idx, k = self._bloom_indexes(key, ids)
        flat = idx.reshape(-1)
        seen = SM.RedisString(self._handle_view(key) if via == "handle" else self._get(key))
        was = seen.get_indexes(flat)
        _u, first = np.unique(flat, return_index=True)
        flags = np.zeros(len(ids), bool)
        flags[first[~was[first]] // k] = True
        s = self._string(key)
        s.set_indexes(flat, 1)
        self._put(key, s.bytes())
        return int(flags.sum()), flags.astype(int).tolist()

    @command
    def bloom_contains(self, via, key, ids):
        idx, k = self._bloom_indexes(key, ids)
        s = SM.RedisString(self._handle_view(key) if via == "handle" else self._padded(key))
        flags = s.get_indexes(idx.reshape(-1)).reshape(-1, k).all(axis=1)
        return int(flags.sum()), flags.astype(int).tolist()

    @command
    def bloom_count(self, via, key):
        from oracle import oracle as O

        if key not in self.cfg:
            raise Failed(NOT_INIT)
        size, k = self.cfg[key]
        return int(O.lib().orc_bloom_count_estimate(SM.RedisString(self._get(key)).bitcount(), size, k))
