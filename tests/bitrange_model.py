"""A brute-force model of BITCOUNT key start end [BYTE|BIT] and BITPOS key bit [start [end [BYTE|BIT]]] over
np.unpackbits, written from the rules of DESIGN §11.2 (restated there from redis 7.2 bitops.c bitcountCommand /
bitposCommand) -- not from the kernels.  `data is None` = the key does not exist; b"" = an existing empty string.
The expected values of test_bitrange_cpu.py, test_bitrange_gpu.py and test_spring_data_bits_gpu.py come from
here."""
import numpy as np

BYTE, BIT = 0, 1


class RedisError(Exception):
    """an error reply"""


def bits_of(data: bytes) -> np.ndarray:
    """the string's bits in Redis order: bit i = byte i>>3, mask 0x80 >> (i&7)"""
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8))


def normalise(start: int, end: int, unit: int, nbytes: int):
    """Normalise(start, end): the inclusive bit interval (lo, hi), or None for the empty range"""
    t = 8 * nbytes if unit == BIT else nbytes
    if start < 0:
        start += t
    if end < 0:
        end += t
    start = max(start, 0)
    end = min(max(end, 0), t - 1)
    if start > end:
        return None
    return (start, end) if unit == BIT else (8 * start, 8 * end + 7)


def bitcount(data, start: int, end: int, unit: int = BYTE) -> int:
    if data is None:
        return 0
    if start < 0 and end < 0 and start > end:  # decided before normalising
        return 0
    iv = normalise(start, end, unit, len(data))
    if iv is None:
        return 0
    return int(bits_of(data)[iv[0]: iv[1] + 1].sum())


def bitpos(data, bit: int, start=None, end=None, unit=None) -> int:
    """start / end / unit None = not given"""
    if bit not in (0, 1):
        raise RedisError("ERR The bit argument must be 1 or 0.")
    if unit is not None and end is None:
        raise RedisError("ERR syntax error")
    if data is None:
        return -1 if bit else 0
    end_given = end is not None
    iv = normalise(0 if start is None else start, end if end_given else len(data) - 1, BYTE if unit is None else unit,
                   len(data))
    if iv is None:
        return -1
    lo, hi = iv
    hits = np.flatnonzero(bits_of(data)[lo: hi + 1] == bit)
    if hits.size:
        return lo + int(hits[0])
    if bit == 1 or end_given:
        return -1
    return hi + 1  # the string counts as zero-padded on the right


def bitpos_nargs(data, bit: int, nargs: int, start: int, end: int, unit: int) -> int:
    """the C ABI's calling form: nargs 0 = bit, 1 = + start, 2 = + start end unit"""
    if nargs < 2 and unit == BIT:
        if bit not in (0, 1):
            raise RedisError("ERR The bit argument must be 1 or 0.")
        raise RedisError("ERR syntax error")
    return bitpos(data, bit, start if nargs >= 1 else None, end if nargs == 2 else None, unit if nargs == 2 else None)


def count_ranges(data, starts, ends, unit: int = BYTE) -> np.ndarray:
    """the batch, with one cumulative sum shared by its queries (the same rules, not one slice per query)"""
    out = np.zeros(len(starts), np.uint64)
    if data is None or len(data) == 0:
        return out
    cum = np.concatenate([[0], np.cumsum(bits_of(data), dtype=np.int64)])
    for i, (s, e) in enumerate(zip(starts, ends)):
        s, e = int(s), int(e)
        if s < 0 and e < 0 and s > e:
            continue
        iv = normalise(s, e, unit, len(data))
        if iv is not None:
            out[i] = cum[iv[1] + 1] - cum[iv[0]]
    return out


def pos_ranges(data, bit: int, starts, ends=None, unit: int = BYTE) -> np.ndarray:
    """the batch, with the next position holding `bit` at or after each position computed once"""
    n = len(starts)
    if data is None:
        return np.full(n, -1 if bit else 0, np.int64)
    out = np.full(n, -1, np.int64)
    if len(data) == 0:
        return out
    bits = bits_of(data)
    nxt = np.full(bits.size + 1, bits.size, np.int64)  # nxt[p] = first q >= p with bits[q] == bit, else 8 * len
    idx = np.where(bits == bit, np.arange(bits.size), bits.size)
    nxt[:-1] = np.minimum.accumulate(idx[::-1])[::-1]
    for i in range(n):
        end_given = ends is not None
        iv = normalise(int(starts[i]), int(ends[i]) if end_given else len(data) - 1, unit, len(data))
        if iv is None:
            continue
        lo, hi = iv
        if nxt[lo] <= hi:
            out[i] = nxt[lo]
        elif bit == 0 and not end_given:
            out[i] = hi + 1
    return out
