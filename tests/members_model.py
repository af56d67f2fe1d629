"""A brute-force model of set-bit enumeration (rbx_bitset_members*) over np.unpackbits / np.flatnonzero, and of the
java.util.BitSet exchange as a line-by-line transcription of the two Java loops (M/RedissonBitSet.java:396-420
fromByteArrayReverse / toByteArrayReverse) over a Python-int BitSet.  Written from DESIGN §11.11; the interval comes
from bitrange_model's normalisation.  `data is None` = the key does not exist; b"" = an existing empty string.  It
shares no code with the engine."""
import numpy as np

from bitrange_model import BIT, BYTE, bits_of, normalise  # noqa: F401

ALL = (1 << 64) - 1  # limit: every member


def interval(data, nargs: int, start: int = 0, end: int = 0, unit: int = BYTE):
    """the inclusive bit interval (lo, hi) of a command, or None"""
    if data is None or len(data) == 0:
        return None
    if nargs == 0:
        return 0, 8 * len(data) - 1
    if start < 0 and end < 0 and start > end:  # BITCOUNT decides this before normalising
        return None
    return normalise(start, end, unit, len(data))


def all_members(data, nargs: int = 0, start: int = 0, end: int = 0, unit: int = BYTE) -> np.ndarray:
    iv = interval(data, nargs, start, end, unit)
    if iv is None:
        return np.zeros(0, np.uint64)
    return (iv[0] + np.flatnonzero(bits_of(data)[iv[0]: iv[1] + 1])).astype(np.uint64)


def members(data, nargs: int = 0, start: int = 0, end: int = 0, unit: int = BYTE, skip: int = 0, limit: int = ALL,
            cap: int = ALL):
    """(the page, total): the ones of rank skip .. skip + min(limit, cap) - 1, Python integers never wrap"""
    m = all_members(data, nargs, start, end, unit)
    return m[skip: skip + min(limit, cap)], int(m.size)


# ---- java.util.BitSet as a Python int: bit i of the int is BitSet bit i ----
def bitset_length(bs: int) -> int:
    """BitSet.length(): the highest set bit + 1, 0 for the empty set"""
    return bs.bit_length()


def from_byte_array_reverse(data) -> int:
    """fromByteArrayReverse(bytes)"""
    if data is None:
        return 0
    bits = 0
    for i in range(len(data) * 8):
        if (data[i // 8] & (1 << (7 - (i % 8)))) != 0:
            bits |= 1 << i
    return bits


def to_byte_array_reverse(bs: int) -> bytes:
    """toByteArrayReverse(bits); Java's int length() overflows at bit 2^31 - 1"""
    if bitset_length(bs) > 0x7FFFFFFF:
        raise OverflowError("BitSet.length() overflows")
    out = bytearray(bitset_length(bs) // 8 + 1)
    for i in range(bitset_length(bs)):
        if (bs >> i) & 1:
            out[i // 8] = out[i // 8] | (1 << (7 - (i % 8)))
    return bytes(out)


def to_long_array(bs: int) -> np.ndarray:
    """BitSet.toLongArray(): the words in use"""
    n = (bitset_length(bs) + 63) // 64
    return np.array([(bs >> (64 * w)) & ALL for w in range(n)], np.uint64)


def value_of(words) -> int:
    """BitSet.valueOf(long[]): trailing zero words are allowed"""
    bs = 0
    for w, x in enumerate(words):
        bs |= int(x) << (64 * w)
    return bs


# the same two conversions vectorised, for the large strings of the GPU tests (checked against the loops above in
# test_members_cpu.py)
def as_words_fast(data) -> np.ndarray:
    if not data:
        return np.zeros(0, np.uint64)
    b = np.frombuffer(bytes(data) + b"\0" * (-len(data) % 8), np.uint8)
    w = np.packbits(np.unpackbits(b), bitorder="little").view("<u8").astype(np.uint64)
    nz = np.flatnonzero(w)
    return w[: int(nz[-1]) + 1] if nz.size else w[:0]


def bytes_of_words_fast(words) -> bytes:
    w = np.ascontiguousarray(np.asarray(words, dtype="<u8"))
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    nz = np.flatnonzero(bits)
    if nz.size == 0:
        return b"\0"
    n = (int(nz[-1]) + 1) // 8 + 1
    full = np.packbits(bits).tobytes()
    return (full + b"\0")[:n]


# ---- many keys ----
WRONG = object()  # a key of another type: its commands fail alone


def stream(strings: dict, names, cmd_key, rows, cap=None):
    """rbx_bitset_members_stream: (off, out, status, any command failed).  strings: name -> bytes, None (missing; an
    absent name too) or WRONG; rows: (nargs, start, end, unit, skip, limit), limit None = all.  out holds the first
    min(total, cap) positions of the concatenation (cap None: all)."""
    off, parts, status = [0], [], []
    for k, (nargs, start, end, unit, skip, limit) in zip(cmd_key, rows):
        data = strings.get(names[int(k)])
        if data is WRONG:
            status.append(0xFF)
            off.append(off[-1])
            continue
        page, _total = members(data, nargs, start, end, unit, skip, ALL if limit is None else limit)
        parts.append(page)
        status.append(0)
        off.append(off[-1] + page.size)
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    return (np.array(off, np.uint64), out if cap is None else out[:cap], np.array(status, np.uint8),
            0xFF in status)
