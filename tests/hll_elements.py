"""HyperLogLog elements with a chosen hash.

MurmurHash64A (seed 0xADC83B19, as Redis' PFADD uses it and oracle.murmur64a restates it) is a bijection on each of
its 8-byte blocks: a block is mixed with odd multipliers and an xor-shift by 47 bits, both of which invert, and the
tail and the final avalanche invert as well.  So an element with any 64-bit hash is computed, not searched for:
every byte but the last full block is free, and that block is solved for the hash.  With it a PFADD reaches a
chosen register with a chosen count -- 33 (promotion by value), 50 and 51 (hllTau) included, which a search by
brute force never finds."""
import numpy as np

SEED = 0xADC83B19
M = 0xC6A4A7935BD1E995
R = 47
MASK = (1 << 64) - 1
M_INV = pow(M, -1, 1 << 64)
HLL_P, HLL_Q = 14, 50


def _unshift(x: int) -> int:
    """inverse of x ^= x >> 47 (the shift is past half the width: it is its own inverse)"""
    return x ^ (x >> R)


def _mix(k: int) -> int:
    k = (k * M) & MASK
    k ^= k >> R
    return (k * M) & MASK


def _unmix(k: int) -> int:
    k = (k * M_INV) & MASK
    k = _unshift(k)
    return (k * M_INV) & MASK


def preimage(h: int, length: int = 8, rng=None) -> bytes:
    """`length` >= 8 bytes whose MurmurHash64A is h: every block but the last full one, and the tail bytes when
    length % 8 != 0, come from rng; the last full block is solved for h."""
    assert length >= 8 and 0 <= h <= MASK
    rng = rng if rng is not None else np.random.default_rng()
    nblocks, ntail = length // 8, length % 8
    head = rng.bytes(8 * (nblocks - 1))
    tail = rng.bytes(ntail)
    state = SEED ^ ((length * M) & MASK)
    for i in range(nblocks - 1):  # forwards over the free blocks
        state = ((state ^ _mix(int.from_bytes(head[8 * i:8 * i + 8], "little"))) * M) & MASK
    # backwards from h: the avalanche, the tail, the last block's multiply
    x = _unshift(h)
    x = (x * M_INV) & MASK
    x = _unshift(x)
    if ntail:
        x = (x * M_INV) & MASK
        x ^= int.from_bytes(tail, "little")
    mixed = ((x * M_INV) & MASK) ^ state
    return head + _unmix(mixed).to_bytes(8, "little") + tail


def hash_for(index: int, count: int, rng) -> int:
    """a 64-bit hash that hllPatLen turns into (index, count): count - 1 zero bits above the 14 index bits, a one,
    random bits above it; count 51 = all 50 bits above the index zero"""
    assert 0 <= index < (1 << HLL_P) and 1 <= count <= HLL_Q + 1
    if count == HLL_Q + 1:
        return index
    top = HLL_P + count  # the first bit above the terminating one
    above = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62)
    return (index | (1 << (top - 1)) | (above << top)) & MASK


def element(index: int, count: int, length: int = 16, rng=None) -> bytes:
    """An element that PFADD puts into register `index` with hllPatLen == count (1..51)."""
    rng = rng if rng is not None else np.random.default_rng()
    return preimage(hash_for(index, count, rng), length, rng)
