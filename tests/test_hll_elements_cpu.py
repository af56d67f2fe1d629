"""hll_elements.py against the oracle: preimages of random hashes at every block / tail layout, and elements for
every count 1..51 at the registers at both ends and on both sides of a 64-register chunk boundary."""
import numpy as np
import pytest

import hll_elements as E
from oracle import oracle as O


@pytest.mark.parametrize("length", [8, 9, 15, 16, 24, 32, 64, 100])
def test_preimages_of_random_hashes(length):
    rng = np.random.default_rng(length)
    hashes = [0, E.MASK] + [int(x) for x in rng.integers(0, 1 << 64, size=998, dtype=np.uint64)]
    for h in hashes:
        e = E.preimage(h, length, rng)
        assert len(e) == length and O.murmur64a(e) == h


@pytest.mark.parametrize("length", [8, 9, 15, 16, 24, 32, 64, 100])
@pytest.mark.parametrize("index", [0, 63, 64, 16383])
def test_elements_for_every_count(index, length):
    rng = np.random.default_rng([index, length])
    for count in range(1, 52):
        assert O.hll_patlen(E.element(index, count, length, rng)) == (index, count)


def test_two_calls_give_different_elements():
    rng = np.random.default_rng(3)
    assert E.element(7, 33, 16, rng) != E.element(7, 33, 16, rng)
    assert O.hll_patlen(E.element(5, 51)) == (5, 51)  # without an rng of the caller's
