"""One keyspace model for the HyperLogLog commands, with exact headers.

A Keyspace holds HLL keys -- an oracle.RedisHll (registers, encoding, the sparse opcode string as Redis builds it,
element by element), the 64-bit cached cardinality of the header (bit 63 = invalid) and a TTL flag -- plus one bit-set
key and one Bloom key that answer WRONGTYPE.  Every command is a method (via, key, *args) -> (reply, error kind), as
in bitstring_model.py.  The rules are redis-7.2 hyperloglog.c's, as api_hll.cpp cites them and oracle/rbx_oracle.c
restates them; the engine-only calls (handles, register images, copies) follow include/rbx.h.

Elements travel as specs, small tuples that materialize() turns into the same bytes every time; register images for
unpack_max likewise (image()).  The hooks (_store_count, _invalidate, ...) are where hll_driver.FaultyModelEngine
injects its defects."""
import numpy as np

import hll_elements as E
from oracle import oracle as O

WRONGTYPE, ILLEGAL, REDIS, NO_SUCH_KEY = "WRONGTYPE", "illegal argument", "redis error", "no such key"
INVALID = 1 << 63
REGS = 16384
MAX_BYTES = O.HLL_SPARSE_MAX_BYTES
MAX_OPS = 16384  # opcodes of a sparse SET string the engine accepts (a valid string never has more)
BITS, BLOOM = "bits", "bloom"  # the keys of another type
COUNTS = (1, 2, 3, 32, 33, 50, 51)
LENGTHS = (8, 16, 32, 64, 9, 24)


# ---- elements and register images from specs ------------------------------------------------------------------
def window(rng):
    """(first register, width) of a cluster near 0, 16383 or a multiple of 64"""
    width = int(rng.choice((3, 6, 12, 70, 200)))
    at = int(rng.choice((0, REGS - width, 64 * int(rng.integers(1, 255)) - int(rng.integers(0, min(width, 8) + 1)))))
    return min(max(at, 0), REGS - width), width


def crafted(seed, n, counts=COUNTS):
    """n (register, count, length) triples in one clustered window, then the elements for them"""
    rng = np.random.default_rng([0xC4AF, seed])
    at, width = window(rng)
    low = [c for c in counts if c <= 3] or list(counts)
    out = []
    for _ in range(n):
        count = int(rng.choice(counts if rng.random() < 0.12 else low))
        out.append(E.element(at + int(rng.integers(0, width)), count, int(rng.choice(LENGTHS)), rng))
    return out


def materialize(spec):
    """spec -> a uint8[n, 16] matrix ("rows") or a list of bytes (every other kind)"""
    kind = spec[0]
    if kind == "rows":  # ("rows", seed, n): random 16-byte rows
        return np.random.default_rng([0x7035, spec[1]]).integers(0, 256, size=(spec[2], 16), dtype=np.uint8)
    if kind == "var":  # ("var", seed, n): lengths 0..120, the empty element first
        rng = np.random.default_rng([0x7A7, spec[1]])
        return [b""] + [rng.bytes(int(x)) for x in rng.integers(0, 121, size=spec[2] - 1)]
    if kind == "crafted":  # ("crafted", seed, n)
        return crafted(spec[1], spec[2])
    if kind == "low":  # ("low", seed, n): crafted with counts <= 3 only (stays sparse, runs form and merge)
        return crafted(spec[1], spec[2], (1, 2, 3))
    if kind == "at":  # ("at", seed, ((register, count, length), ...)): crafted one by one
        rng = np.random.default_rng([0xA7, spec[1]])
        return [E.element(i, c, n, rng) for i, c, n in spec[2]]
    if kind == "cat":  # ("cat", spec, spec, ...)
        parts = [materialize(s) for s in spec[1:]]
        return [bytes(r) for p in parts for r in p]
    if kind == "lit":  # ("lit", (element, ...)): the elements themselves
        return list(spec[1])
    if kind == "none":
        return []
    raise AssertionError(spec)


def count_of(spec) -> int:
    x = materialize(spec)
    return len(x)


def oracle_arena(x):
    return O.fixed_arena(x) if isinstance(x, np.ndarray) else O.arena(list(x))


def image(spec) -> np.ndarray:
    """a register image for unpack_max: ("few", seed) a few registers up to 3, ("value", seed) one register at 33 or
    more among them, ("bytes", seed) every other register of the first 3,200 (no sparse string within the limit)"""
    kind, seed = spec
    rng = np.random.default_rng([0x1A6E, seed])
    out = np.zeros(REGS, np.uint8)
    at, width = window(rng)
    n = int(rng.integers(1, 9))
    out[at + rng.integers(0, width, size=n)] = rng.integers(1, 4, size=n)
    if kind == "value":
        out[at + int(rng.integers(0, width))] = int(rng.choice((33, 40, 63)))
    elif kind == "bytes":
        out[0:3200:2] = 1
    else:
        assert kind == "few"
    return out


# ---- strings -----------------------------------------------------------------------------------------------------
def header(sparse: int, card: int) -> bytes:
    return b"HYLL" + bytes([sparse, 0, 0, 0]) + card.to_bytes(8, "little")


def parse(s: bytes):
    """An HLL string as SET accepts it -> (RedisHll, card), or None (isHLLObjectOrReply and the length checks)."""
    if len(s) < 16 or s[:4] != b"HYLL" or s[4] > 1:
        return None
    if s[4] == 0:
        if len(s) != 16 + 12288:
            return None
    else:
        i = p = nops = 0
        ops = s[16:]
        while p < len(ops):
            b = ops[p]
            if b & 0xC0 == 0x40:
                if p + 1 >= len(ops):
                    return None
                i, p = i + (((b & 0x3F) << 8) | ops[p + 1]) + 1, p + 2
            else:
                i, p = i + ((b & 0x3F) + 1 if b < 0x40 else (b & 3) + 1), p + 1
            nops += 1
            if i > REGS:
                return None
        if i != REGS or nops > MAX_OPS:
            return None
    return O.RedisHll.from_string(s), int.from_bytes(s[8:16], "little")


def normalized(ops: bytes) -> bool:
    """hll_kernels.hip sparse_normalized: zero runs maximal and canonical, no two adjacent VALs of one value"""
    prev, p = None, 0
    while p < len(ops):
        b = ops[p]
        if b & 0xC0 == 0x40:
            if (((b & 0x3F) << 8) | ops[p + 1]) + 1 <= 64:
                return False
            cur, p = "zero", p + 2
        else:
            cur, p = ("zero" if b < 0x40 else (b >> 2) & 31), p + 1
        if cur == prev:
            return False
        prev = cur
    return True


def normalized_bound(regs):
    """(no nonzero run longer than 4, B = zero-run bytes + one byte per nonzero register): the shortcut's bound"""
    r = np.asarray(regs)
    edges = np.flatnonzero(np.diff(r.astype(np.int16))) + 1
    starts, ends = np.concatenate([[0], edges]), np.concatenate([edges, [REGS]])
    lens, zero = ends - starts, r[starts] == 0
    return bool((lens[~zero] <= 4).all()), int(np.where(lens[zero] > 64, 2, 1).sum() + lens[~zero].sum())


def clone(h: O.RedisHll) -> O.RedisHll:
    out = O.RedisHll(h.max_bytes)
    out.ops[:] = h.ops
    out.len.value, out.dense.value, out.regs = h.len.value, h.dense.value, h.regs.copy()
    return out


class Hll:
    """one key: the Redis object, the header's cached cardinality, whether a TTL is set"""

    def __init__(self, h=None, card=0, ttl=False):
        self.h, self.card, self.ttl = h if h is not None else O.RedisHll(), card, ttl

    @property
    def dense(self) -> bool:
        return bool(self.h.dense.value)

    def string(self) -> bytes:
        return self.h.string(self.card.to_bytes(8, "little"))


class Keyspace:
    def __init__(self):
        self.keys = {}
        self.events = []  # what the last command did, for hll_driver.stats: ("promoted", why), ("recreated",), ...
        self.deleted = set()

    # ---- plumbing ---------------------------------------------------------------------------------------------
    def _wrong(self, *keys):
        return any(k in (BITS, BLOOM) for k in keys)

    def _create(self, key) -> Hll:
        """createHLLObject: sparse, one XZERO, cached cardinality 0 and valid"""
        k = self.keys[key] = self._new_key(key)
        if key in self.deleted:
            self.events.append(("recreated",))
            self.deleted.discard(key)
        return k

    def registers(self, key) -> np.ndarray:
        return self.keys[key].h.regs if key in self.keys else O.hll_new()

    # the hooks a faulty model overrides
    def _new_key(self, key) -> Hll:
        return Hll()

    def _invalidate(self, k: Hll, changed: bool) -> None:
        if changed:  # HLL_INVALIDATE_CACHE: only a register change; the low 63 bits stay
            k.card |= INVALID

    def _store_count(self, k: Hll, value: int) -> None:
        k.card = value

    def _after_merge(self, k: Hll) -> None:
        k.card |= INVALID  # pfmergeCommand invalidates always, also when no source exists

    def _use_dense(self, d: Hll, sources) -> bool:
        return d.dense or any(s.dense for s in sources)

    def _write_back(self, k: Hll, maxima: np.ndarray, use_dense: bool) -> None:
        k.h.merge_from(maxima, use_dense)  # ascending registers through hllSparseSet; may promote

    def _imported_card(self, card: int) -> int:
        return card

    def _elements(self, k: Hll, x):
        return x

    def _handle_target(self, key, create=True):
        """the key a handle call acts on: handles follow the name (hll_bind), a missing key is created"""
        if key not in self.keys and create:
            self._create(key)
        return self.keys.get(key)

    # ---- PFADD ------------------------------------------------------------------------------------------------
    def _add(self, k: Hll, spec) -> bool:
        """the elements of spec into k: whether a register changed"""
        x = self._elements(k, materialize(spec))
        if len(x) == 0:
            return False
        start_dense, start_ops, start_valid = k.dense, (None if k.dense else k.h.sparse_ops), not k.card >> 63
        changed = bool(k.h.pfadd(*oracle_arena(x)))
        if not start_dense:
            ok, b = normalized_bound(k.h.regs)
            shortcut = normalized(start_ops) and ok and 16 + b <= MAX_BYTES and int(k.h.regs.max()) <= 32
            self.events.append(("shortcut" if shortcut else "replay",))
            if k.dense:
                self.events.append(("promoted", "value in pfadd" if int(k.h.regs.max()) > 32 else "bytes in pfadd"))
        if not changed and start_valid:
            self.events.append(("unchanged on a valid cache",))
        return changed

    def _pfadd_one(self, key, spec) -> int:
        created = key not in self.keys
        k = self._create(key) if created else self.keys[key]
        changed = self._add(k, spec)
        self._invalidate(k, changed)
        return int(changed or created)

    def pfadd(self, via, key, spec):
        self.events = []
        if self._wrong(key):
            return None, WRONGTYPE
        return bool(self._pfadd_one(key, spec)), None

    def pfadd_multi(self, via, key, cmds):
        """cmds = ((key, spec), ...): a pipeline of PFADDs in one call, each reply sees the commands before it.  The
        call has one error code: a key of another type anywhere fails it, and nothing changes"""
        self.events = []
        if self._wrong(*[k for k, _ in cmds]):
            return None, WRONGTYPE
        return [self._pfadd_one(k, spec) for k, spec in cmds], None

    def pfadd_dev(self, via, key, spec):
        """rbx_hll_add_multi_dev through the key's open handle.  Registers and string follow PFADD, and the changed
        word is nonzero iff a register changed (a created key alone does not set it).  The header is the one
        deliberate deviation from Redis: rbx_hll_add_multi_dev, api_hll.cpp line 846 ("conservatively invalidate (the
        flags are device-side)"), sets the invalid bit on every PFADD through a handle, whether or not a register changes --
        that path's contract, stated here as such."""
        self.events = []
        k = self._handle_target(key)
        changed = self._add(k, spec)
        k.card |= INVALID
        return bool(changed), None

    # ---- PFCOUNT ----------------------------------------------------------------------------------------------
    def _count_one(self, k) -> int:
        if k is None:
            return 0
        if not k.card >> 63:  # a valid cache is returned as it stands, right or wrong
            self.events.append(("cache hit", k.card != O.hll_count(k.h.regs)))
            return k.card
        value = O.hll_count(k.h.regs)
        self.events.append(("recount",))
        self._store_count(k, value)
        return value

    def pfcount(self, via, key):
        self.events = []
        if self._wrong(key):
            return None, WRONGTYPE
        return self._count_one(self.keys.get(key)), None

    def pfcount_multi(self, via, key, others):
        """PFCOUNT key o1..on, n >= 1: the count of the register maxima; no header changes"""
        self.events = []
        if self._wrong(key, *others):
            return None, WRONGTYPE
        mx = O.hll_new()
        for k in (key,) + tuple(others):
            mx = np.maximum(mx, self.registers(k))
        return O.hll_count(mx), None

    def count_each(self, via, key, keys):
        """independent single-key PFCOUNTs in one call, by name or through the handles: the cache rule of PFCOUNT"""
        self.events = []
        if self._wrong(*keys):
            return None, WRONGTYPE
        if via == "handle":
            return [self._count_one(self._handle_target(k, create=False)) for k in keys], None
        return [self._count_one(self.keys.get(k)) for k in keys], None

    # ---- PFMERGE ----------------------------------------------------------------------------------------------
    def pfmerge(self, via, key, srcs):
        self.events = []
        if self._wrong(key, *srcs):
            return None, WRONGTYPE  # nothing changes
        d = self.keys[key] if key in self.keys else self._create(key)
        sources = [self.keys[s] for s in srcs if s in self.keys]
        was_dense = d.dense
        use_dense = self._use_dense(d, sources)
        mx = d.h.regs.copy()
        for s in sources:
            mx = np.maximum(mx, s.h.regs)
        self._write_back(d, mx, use_dense)
        if d.dense and not was_dense:
            self.events.append(("promoted", "dense source" if use_dense else "merge write-back"))
        self._after_merge(d)
        return None, None

    # ---- SET / GET ----------------------------------------------------------------------------------------------
    def set(self, via, key, s):
        self.events = []
        got = parse(s)
        if got is None:
            return None, WRONGTYPE  # "WRONGTYPE Key is not a valid HyperLogLog string value."; nothing changes
        h, card = got
        if key not in self.keys and key in self.deleted:
            self.deleted.discard(key)
        self.keys[key] = Hll(h, self._imported_card(card), False)  # the encoding and the 8 bytes as given; no TTL
        return None, None

    def get(self, via, key, encoding):
        self.events = []
        if self._wrong(key):
            return None, WRONGTYPE
        k = self.keys.get(key)
        if k is None:
            return b"", None
        if encoding == "dense":
            return header(0, k.card) + O.hll_dense_pack(k.h.regs), None
        if encoding == "sparse" and k.dense:
            ops = O.hll_sparse_pack(k.h.regs)
            if ops is None:
                return None, ILLEGAL
            return header(1, k.card) + ops, None
        return k.string(), None

    # ---- keys ----------------------------------------------------------------------------------------------------
    def delete(self, via, key):
        self.events = []
        gone = self.keys.pop(key, None)
        if gone is not None:
            self.deleted.add(key)
            self._deleted(key, gone)
        return gone is not None, None

    def _deleted(self, key, k: Hll) -> None:
        pass

    def exists(self, via, key):
        return key in self.keys, None

    def expire(self, via, key):
        if key in self.keys:
            self.keys[key].ttl = True
        return key in self.keys, None

    def persist(self, via, key):
        had = key in self.keys and self.keys[key].ttl
        if had:
            self.keys[key].ttl = False
        return had, None

    def ttl(self, via, key):
        return ("missing" if key not in self.keys else "set" if self.keys[key].ttl else "none"), None

    def copy(self, via, key, dst):
        """rbx_hll_copy_to inside one context: dst := the source's registers, encoding, string and card, no TTL"""
        self.events = []
        if self._wrong(key):
            return None, WRONGTYPE
        if key == dst:
            return None, None
        src = self.keys.get(key)
        if src is None:
            if self.keys.pop(dst, None) is not None:
                self.deleted.add(dst)
            return None, None
        self.deleted.discard(dst)
        self.keys[dst] = Hll(clone(src.h), src.card, self._copied_ttl(dst))
        return None, None

    def _copied_ttl(self, dst) -> bool:
        return False

    # ---- the handles' register exchange ---------------------------------------------------------------------------
    def open(self, via, key):
        """setup: the engine opens its long-lived handle on the (existing) key"""
        assert key in self.keys
        return None, None

    def pack(self, via, key):
        """rbx_hll_pack_registers: a read of the registers (the handle binds by name and creates a missing key)"""
        self.events = []
        return self._handle_target(key).h.regs.tobytes(), None

    def unpack_max(self, via, key, spec):
        """registers := max(registers, image); a sparse key takes the image as PFMERGE's write-back does"""
        self.events = []
        k = self._handle_target(key)
        was_dense = k.dense
        self._write_back(k, np.maximum(k.h.regs, image(spec)), False)
        if k.dense and not was_dense:
            self.events.append(("promoted", "unpack_max"))
        k.card |= INVALID
        return None, None
