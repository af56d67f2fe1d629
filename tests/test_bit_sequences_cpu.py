"""The command sequences of bitstring_driver.py without a GPU: the generator, the model and the checker agree with
themselves; the sequences of the GPU test's seeds cover what they are there for; and each of eight defects, injected
into a copy of the model, is caught by them."""
import pytest

import bitstring_driver as D

SEEDS = range(8)   # test_bit_sequences_gpu.py runs the same
STEPS = 300
DEFECTS = {
    "a": "BITOP leaves the old destination's bytes behind a shorter result",
    "b": "growth keeps one stale nonzero byte between the old and the new length",
    "c": "a SETBIT of value 0 past the end does not lengthen the string",
    "d": "a shrinking setBytes keeps the old tail readable by GETBIT past the length",
    "e": "BITPOS ignores the end bound when bit = 0",
    "f": "SAT clamps signed fields to the unsigned bound",
    "g": "the long-lived Bloom handle keeps reading the bytes from before the last growth",
    "h": "BITOP with dest among the sources reads the source after it was overwritten",
}


@pytest.fixture(scope="module")
def stats():
    return [D.stats(seed, STEPS) for seed in SEEDS]


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_and_model_agree_with_themselves(seed):
    first = list(D.commands(seed, STEPS))
    assert len(first) == STEPS and first == list(D.commands(seed, STEPS))  # a pure function of the seed
    D.run(D.ModelEngine(), seed, STEPS)
    D.run(D.ModelEngine(), seed, STEPS, stop_at=40)  # a prefix replays


def test_every_kind_occurs_often(stats):
    kinds = {k + suffix for k in D.WEIGHTS for suffix in ("", "_dev") if suffix == "" or k in D.DEVICE}
    kinds |= {"bloom_add_dev", "bloom_contains_dev"}  # through the open handle
    total = {k: sum(s["kinds"].get(k, 0) for s in stats) for k in kinds}
    assert {k: n for k, n in total.items() if n < 10} == {}
    forms = {f: sum(s["forms"].get(f, 0) for s in stats) for f in D.FORMS}
    assert {f: n for f, n in forms.items() if n < 10} == {}
    assert sum(s["renames"]["existing"] for s in stats) >= 10 and sum(s["renames"]["missing"] for s in stats) >= 10


def test_every_kind_follows_another_family_on_the_same_key(stats):
    """directly after: the command before it in the stream was on the same key and of another family"""
    seen = set().union(*(s["after_other_family"] for s in stats))
    kinds = {k + suffix for k in D.WEIGHTS for suffix in ("", "_dev") if suffix == "" or k in D.DEVICE}
    kinds |= {"bloom_add_dev", "bloom_contains_dev"}
    assert kinds - seen == set()


def test_few_commands_end_in_an_error(stats):
    errors, n = sum(s["errors"] for s in stats), sum(s["n"] for s in stats)
    assert 0.02 * n <= errors <= 0.15 * n
    assert all(s["errors"] <= 0.15 * s["n"] for s in stats)


@pytest.mark.parametrize("seed", SEEDS)
def test_each_seed_grows_shrinks_and_overwrites_a_source(stats, seed):
    s = stats[seed]
    assert s["growths"] >= 6            # the length crosses a multiple of 256 bytes
    assert s["shrinks"] >= 3            # a setBytes or a BITOP result shorter than the string before
    assert s["self_growing_bitops"] >= 2  # dest among the sources, and the result outgrows dest's allocation


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_an_injected_defect_is_caught(defect):
    for seed in SEEDS:
        try:
            D.run(D.FaultyModelEngine(defect), seed, STEPS)
        except AssertionError as e:
            assert f"seed {seed}, step " in str(e) and "the last commands" in str(e)  # what a replay needs
            return
    pytest.fail("no seed notices that " + DEFECTS[defect])
