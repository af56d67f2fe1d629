"""An independent model of Redis BITFIELD under OVERFLOW WRAP / SAT / FAIL and of one BITFIELD with mixed
sub-commands, as restated in DESIGN section 11.3 from redis 7.2 bitops.c bitfieldGeneric /
checkSignedBitfieldOverflow / checkUnsignedBitfieldOverflow.  Python big integers: every sum is exact.
It takes `check` / `extend` and the string layout from bitfield_model and shares no code with the engine."""
import bitfield_model as M
from bitfield_model import GET, INCRBY, SET  # noqa: F401

WRAP, SAT, FAIL = 0, 1, 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def bounds(signed: bool, size: int):
    return (-(1 << (size - 1)), (1 << (size - 1)) - 1) if signed else (0, (1 << size) - 1)


def rule(op: int, signed: bool, size: int, mode: int, old: int, value: int):
    """One sub-command on a field that holds `old` -> (the field after, the reply or None for nil)."""
    if op == GET:
        return old, old
    lo, hi = bounds(signed, size)
    if op == SET:
        t = value if signed else value % (1 << 64)  # an unsigned field takes the argument as a uint64_t
    else:
        t = old + value
    if lo <= t <= hi:
        now = t
    elif mode == WRAP:
        now = M.extend(t % (1 << size), signed, size)
    elif mode == SAT:
        now = hi if t > hi else lo
    else:
        return old, None
    return now, (old if op == SET else now)


def check_type(signed: bool, size: int) -> None:
    """Redis's own type check (the mixed list has no Redisson-side one)"""
    if size < 1 or size > (64 if signed else 63):
        raise M.RedisError("ERR Invalid bitfield type")


def _grow(data: bytes, need: int) -> bytes:
    return data + bytes(need - len(data)) if len(data) < need else data


def _read(data: bytes, signed: bool, size: int, offset: int) -> int:
    end = offset + size
    n = max(len(data), (end + 7) // 8)
    x = int.from_bytes(data + bytes(n - len(data)), "big")
    return M.extend((x >> (8 * n - end)) & ((1 << size) - 1), signed, size)


def _write(data: bytes, size: int, offset: int, now: int) -> bytes:
    n = len(data)
    shift = 8 * n - offset - size
    mask = (1 << size) - 1
    x = int.from_bytes(data, "big")
    return ((x & ~(mask << shift)) | ((now & mask) << shift)).to_bytes(n, "big")


def bitfield(data: bytes, cmds):
    """One BITFIELD on the string `data` (b"" = a missing key).  cmds: (op, signed, size, mode, offset, value).
    Every sub-command is checked first; the string is then sized for the SETs and INCRBYs (failing ones
    included); then they run in order -> (the string after, replies with None for nil)."""
    for op, signed, size, mode, offset, _v in cmds:
        if op not in (GET, SET, INCRBY) or mode not in (WRAP, SAT, FAIL):
            raise M.IllegalArgument("unknown operation or mode")
        check_type(signed, size)
        M.check(signed, size, offset)  # the offset limit (the size is legal here)
    need = max([((o + s - 1) >> 3) + 1 for op, _sg, s, _m, o, _v in cmds if op != GET], default=0)
    data = _grow(data, need)
    replies = []
    for op, signed, size, mode, offset, value in cmds:
        old = _read(data, signed, size, offset)
        now, reply = rule(op, signed, size, mode, old, int(value))
        if op != GET and reply is not None:
            data = _write(data, size, offset, now)
        replies.append(reply)
    return data, replies


def fields(data: bytes, op: int, signed: bool, size: int, mode: int, offsets, values=None):
    """A batch of one operation, type and mode -> (string, replies with None for nil).  The type check is
    bitfield_model's (Redisson's limits, then Redis's)."""
    offsets = [int(o) for o in offsets]
    for o in offsets:
        M.check(signed, size, o)
    if not offsets:
        return data, []
    return bitfield(data, [(op, signed, size, mode, o, 0 if values is None else int(values[i]))
                           for i, o in enumerate(offsets)])
