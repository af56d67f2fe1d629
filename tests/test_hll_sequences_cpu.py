"""The HyperLogLog command sequences of hll_driver.py without a GPU: the generator, the model and the checker agree
with themselves; the sequences of the GPU test's seeds cover what they are there for; and each of eleven defects,
injected into a copy of the model, is caught by them."""
import pytest

import hll_driver as D

SEEDS = range(8)   # test_hll_sequences_gpu.py runs the same
STEPS = 300
DEFECTS = {
    "a": "a single-key PFCOUNT does not store its result",
    "b": "a PFADD that changes nothing invalidates the cache",
    "c": "PFMERGE leaves the cache valid",
    "d": "a dense source leaves a sparse destination sparse",
    "e": "count 33 is stored as VAL 32 without a promotion",
    "f": "the merge write-back emits the fewest-bytes string instead of replaying in ascending order",
    "g": "a re-created key keeps the deleted key's opcode list",
    "h": "SET marks the given cache invalid",
    "i": "the second command on one key within a multi-key PFADD replies against the registers from before the call",
    "j": "the long-lived handle keeps writing the deleted key's registers",
    "k": "a copy keeps the destination's TTL",
}


@pytest.fixture(scope="module")
def stats():
    return [D.stats(seed, STEPS) for seed in SEEDS]


def all_labels():
    return {f"{kind}:{via}" for kind, vias in D.VIAS.items() for via in vias}


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_and_model_agree_with_themselves(seed):
    first = list(D.commands(seed, STEPS))
    assert len(first) == STEPS and first == list(D.commands(seed, STEPS))  # a pure function of the seed
    D.run(D.ModelEngine(), seed, STEPS)
    D.run(D.ModelEngine(), seed, STEPS, stop_at=40)  # a prefix replays


def test_every_kind_and_via_occurs_often(stats):
    total = {k: sum(s["kinds"].get(k, 0) for s in stats) for k in all_labels()}
    assert {k: n for k, n in total.items() if n < 10} == {}
    multi, repeated = sum(s["multi"] for s in stats), sum(s["repeated key in multi"] for s in stats)
    assert 3 * repeated >= multi  # a key is named again in at least a third of the multi-key PFADDs


def test_every_kind_follows_another_family_on_the_same_key(stats):
    """directly after: the command before it in the stream was on the same key and of another family"""
    seen = set().union(*(s["after_other_family"] for s in stats))
    assert set(D.WEIGHTS) - seen == set()


def test_few_commands_end_in_an_error(stats):
    errors, n = sum(s["errors"] for s in stats), sum(s["n"] for s in stats)
    assert 0.02 * n <= errors <= 0.15 * n
    assert all(s["errors"] <= 0.15 * s["n"] for s in stats)


@pytest.mark.parametrize("seed", SEEDS)
def test_each_seed_promotes_recreates_and_meets_both_cache_states(stats, seed):
    s = stats[seed]
    assert s["promoted"].get("bytes in pfadd", 0) >= 3
    assert s["promoted"].get("value in pfadd", 0) >= 1
    assert s["promoted"].get("merge write-back", 0) >= 1
    assert s["promoted"].get("dense source", 0) >= 1
    assert s["promoted"].get("unpack_max", 0) >= 1
    assert s["recreated"] >= 3
    assert s["cache hits"] >= 5 and s["recounts"] >= 5  # single-key PFCOUNTs
    assert s["wrong cache hits"] >= 1                   # a valid cache that disagrees with the registers
    assert s["unchanged on a valid cache"] >= 5         # PFADDs that change nothing: the header stays valid
    assert s["shortcut"] >= 5 and s["replay"] >= 5      # PFADDs on sparse keys: the shortcut's condition holds / fails


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_an_injected_defect_is_caught(defect):
    for seed in SEEDS:
        try:
            D.run(D.FaultyModelEngine(defect), seed, STEPS)
        except AssertionError as e:
            assert f"seed {seed}, step " in str(e) and "the last commands" in str(e)  # what a replay needs
            return
    pytest.fail("no seed notices that " + DEFECTS[defect])
