"""An independent model of Redis BITFIELD GET / SET / INCRBY (default OVERFLOW WRAP) on one string,
as restated in DESIGN section 11 from redis 7.2 bitops.c bitfieldGeneric.  The string is a Python
big integer (int.from_bytes(data, "big")): bit `offset` of the string is bit 8*len - 1 - offset of
the integer.  It shares no code with the engine."""

GET, SET, INCRBY = 0, 1, 2
MAX_OFFSET = 1 << 32


class IllegalArgument(Exception):
    pass


class RedisError(Exception):
    pass


def check(signed: bool, size: int, offset: int) -> None:
    if signed and size > 64:
        raise IllegalArgument("Size can't be greater than 64 bits")
    if not signed and size > 63:
        raise IllegalArgument("Size can't be greater than 63 bits")
    if size < 1:
        raise RedisError("ERR Invalid bitfield type")
    if offset < 0 or offset >= MAX_OFFSET or offset + size > MAX_OFFSET:
        raise RedisError("ERR bit offset is not an integer or out of range")


def extend(v: int, signed: bool, size: int) -> int:
    return v - (1 << size) if signed and v >> (size - 1) else v


def field(data: bytes, op: int, signed: bool, size: int, offset: int, value: int = 0):
    """One sub-command on the string `data` (b"" = a missing key) -> (the string after, the reply)."""
    check(signed, size, offset)
    end = offset + size
    if op == GET:
        n = max(len(data), (end + 7) // 8)  # read through zero padding; the string itself stays
        x = int.from_bytes(data + bytes(n - len(data)), "big")
        return data, extend((x >> (8 * n - end)) & ((1 << size) - 1), signed, size)
    if len(data) < ((end - 1) >> 3) + 1:
        data = data + bytes(((end - 1) >> 3) + 1 - len(data))
    n = len(data)
    x = int.from_bytes(data, "big")
    shift = 8 * n - end
    mask = (1 << size) - 1
    old = (x >> shift) & mask
    new = (value if op == SET else old + value) & mask
    x = (x & ~(mask << shift)) | (new << shift)
    return x.to_bytes(n, "big"), extend(old if op == SET else new, signed, size)


def fields(data: bytes, op: int, signed: bool, size: int, offsets, values=None):
    """A batch: every sub-command is checked first, then they run in order -> (string, replies)."""
    offsets = [int(o) for o in offsets]
    for o in offsets:
        check(signed, size, o)
    replies = []
    for i, o in enumerate(offsets):
        data, r = field(data, op, signed, size, o, 0 if values is None else int(values[i]))
        replies.append(r)
    return data, replies
