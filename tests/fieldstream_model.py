"""A model of rbx_bitset_field_stream: a dict of bytearrays to which the commands are applied one at a time, in
array order, each as one BITFIELD with one sub-command through bitfield_overflow_model, under
bitstream_model's failure rule (a failing command fails alone and changes nothing; the first failure in
array order decides the return code).  Also the seeded batches the CPU and GPU tests share, and what each
batch must contain.  Shares no code with the engine."""
import random

import bitfield_model as F
import bitfield_overflow_model as B
from bitstream_model import E_ILLEGAL_ARGUMENT, E_REDIS, E_WRONGTYPE, OK  # noqa: F401

GET, SET, INCRBY = B.GET, B.SET, B.INCRBY
WRAP, SAT, FAIL = B.WRAP, B.SAT, B.FAIL
VALID, NIL, FAILED = 0, 1, 0xFF
OFFSET_LIMIT = 1 << 32


class FieldStreamModel:
    """strings: name -> bytearray of the keys that exist; wrong: the names that hold another type.  A command
    is (op, signed, size, mode, offset, value)."""

    def __init__(self, strings=None, wrong=()):
        self.strings = {bytes(k): bytearray(v) for k, v in (strings or {}).items()}
        self.wrong = {bytes(k) for k in wrong}
        self.events = []  # per command of the last run: None, or "type" / "offset" / "wrong" / "nil" / "sat_hi" / "sat_lo"
        self.first_failure = None

    def failure(self, name: bytes, cmd):
        """the kind a command fails with, in the single call's order: the type, the offset limit, the key's type"""
        _op, signed, size, _mode, offset, _value = cmd
        try:
            B.check_type(bool(signed), size)
        except F.RedisError:
            return "type"
        try:
            F.check(bool(signed), size, offset)
        except F.RedisError:
            return "offset"
        return "wrong" if name in self.wrong else None

    def _event(self, data: bytes, cmd):
        op, signed, size, mode, offset, value = cmd
        if op == GET or mode == WRAP:
            return None
        lo, hi = B.bounds(bool(signed), size)
        old = B._read(data, bool(signed), size, offset)
        t = (value if signed else value % (1 << 64)) if op == SET else old + value
        if lo <= t <= hi:
            return None
        return "nil" if mode == FAIL else ("sat_hi" if t > hi else "sat_lo")

    def run(self, names, cmd_key, cmds):
        """(return code, replies, status): the caller's errors first, with nothing changed; then each command."""
        names = [bytes(n) for n in names]
        self.events, self.first_failure = [], None
        for k, (op, signed, _size, mode, _offset, _value) in zip(cmd_key, cmds):
            if k >= len(names) or op not in (GET, SET, INCRBY) or mode not in (WRAP, SAT, FAIL) or signed not in (0, 1):
                return E_ILLEGAL_ARGUMENT, None, None
        rc, replies, status = OK, [], []
        for k, cmd in zip(cmd_key, cmds):
            name = names[k]
            kind = self.failure(name, cmd)
            if kind is not None:
                rc = rc or (E_WRONGTYPE if kind == "wrong" else E_REDIS)
                self.first_failure = self.first_failure or kind
                self.events.append(kind)
                replies.append(0)
                status.append(FAILED)
                continue
            op, signed, size, mode, offset, value = cmd
            data = bytes(self.strings.get(name, b""))
            self.events.append(self._event(B._grow(data, ((offset + size - 1) >> 3) + 1), cmd))
            after, (reply,) = B.bitfield(data, [(op, bool(signed), size, mode, offset, value)])
            if op != GET:  # a GET creates and grows nothing
                self.strings[name] = bytearray(after)
            replies.append(0 if reply is None else reply)
            status.append(NIL if reply is None else VALID)
        return rc, replies, status


# ---- the seeded batches -----------------------------------------------------------------------------------
# entries of `names`: four plain keys (the fourth missing at the start), a Bloom filter's bitmap (its
# {name}:config exists), an HLL (another type), a name that never exists (it is only read), and the first
# key's name again
KEYS = ("s0", "s1", "s2", "new", "bloom", "hll", "ghost", "s0")
HLL, GHOST = 5, 6
SEEDS = (11, 12)
NCMD = 600
CATEGORIES = ("repeated cell", "partly overlapping", "straddling", "nil", "sat_hi", "sat_lo", "type", "offset", "wrong",
              "equal names")


def random_batch(seed: int, contained: bool = False, n: int = NCMD):
    """(cmd_key, cmds) over the entries of KEYS.  contained: every field lies inside one aligned 64-bit word
    (the batch then has no straddling field, and nothing else is taken away)."""
    rng = random.Random(seed * 2 + int(contained))
    key, cmds = [], []
    while len(cmds) < n:
        k = rng.randrange(len(KEYS))
        signed = rng.randrange(2)
        size = rng.choice((1, 4, 5, 7, 8, 8, 13, 16, 16, 32, 33, 63, 64))
        if size == 64:
            signed = 1
        op = rng.choice((GET, SET, INCRBY, INCRBY))
        mode = rng.choice((WRAP, SAT, FAIL))
        shape = rng.randrange(4)
        if shape == 0:
            offset = size * rng.randrange(0, max(1, 512 // size))  # Redisson's own addressing: a multiple of the size
        elif shape == 1:
            offset = rng.randrange(0, 512)
        elif shape == 2:
            offset = rng.choice((0, 8, 60, 64, 100, 120, 127, 128))
        else:
            offset = rng.randrange(0, 5000)
        if contained and (offset >> 6) != ((offset + size - 1) >> 6):
            offset = (offset >> 6 << 6) + rng.randrange(0, 65 - size)
        lo, hi = B.bounds(bool(signed), size)
        value = rng.choice((0, 1, -1, 3, -7, hi, lo, hi + 1, lo - 1, rng.randrange(-300, 300), B.I64_MAX, B.I64_MIN))
        value = max(B.I64_MIN, min(B.I64_MAX, value))
        roll = rng.randrange(40)
        if roll == 0:
            size, signed = rng.choice(((0, 0), (0, 1), (64, 0), (65, 1)))
        elif roll == 1:
            offset = rng.choice((OFFSET_LIMIT, OFFSET_LIMIT - size + 1, (1 << 64) - 1))
        if k == GHOST and roll > 1:
            op = GET
        key.append(k)
        cmds.append((op, signed, size, mode, offset, value))
    return key, cmds


def coverage(cmd_key, cmds, model_events):
    """the CATEGORIES a batch holds, given the events of its model run"""
    names = list(KEYS)
    canon = [names.index(nm) for nm in names]
    have = {e for e in model_events if e is not None}
    cells, ranges, entries = set(), {}, set()
    for k, (op, _signed, size, _mode, offset, _value), e in zip(cmd_key, cmds, model_events):
        if e in ("type", "offset", "wrong"):
            continue
        if canon[k] == 0:
            entries.add(k)
        cell = (canon[k], offset, size)
        if cell in cells:
            have.add("repeated cell")
        cells.add(cell)
        if (offset >> 6) != ((offset + size - 1) >> 6):
            have.add("straddling")
        for lo, hi in ranges.setdefault(canon[k], set()):
            if lo < offset < hi < offset + size or offset < lo < offset + size < hi:  # neither holds the other
                have.add("partly overlapping")
        ranges[canon[k]].add((offset, offset + size))
    if len(entries) == 2:
        have.add("equal names")
    return have
