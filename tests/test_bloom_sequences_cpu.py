"""The Bloom filter command sequences of bloom_driver.py without a GPU: the generator, the model and the checker agree
with themselves; the sequences of the GPU test's seeds cover what they are there for; and each of thirteen defects,
injected into a copy of the model, is caught by them.

One case of the issue that set this suite up cannot occur and is replaced.  "An add whose keys are all already present
and which still lengthens the string": a bit past the string's end is zero, so the key that sets it is its first setter
and replies new.  What can go wrong in its place is asserted instead: per seed an add whose keys are all present (it
must change nothing), and an add that lengthens the string while its LAST key is not new (a duplicate of the key that
did); defect "e" drops the lengthening exactly there."""
import pytest

import bloom_driver as D

SEEDS = range(8)   # test_bloom_sequences_gpu.py runs the same
STEPS = 300
DEFECTS = D.DEFECTS


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


def test_every_kind_follows_another_family_on_the_same_filter(stats):
    """directly after: the command before it in the sequence was on the same filter and of another family"""
    seen = set().union(*(s["after_other_family"] for s in stats))
    assert set(D.WEIGHTS) - seen == set()


def test_few_commands_end_in_an_error(stats):
    errors, n = sum(s["errors"] for s in stats), sum(s["n"] for s in stats)
    assert 0.02 * n <= errors <= 0.15 * n
    assert all(s["errors"] <= 0.15 * s["n"] for s in stats)


@pytest.mark.parametrize("seed", SEEDS)
def test_each_seed_meets_the_turns_the_suite_is_there_for(stats, seed):
    s = stats[seed]
    assert s["all present"] >= 1                      # an add that must change nothing
    assert s["lengthens, last key not new"] >= 1      # the length comes from a key whose reply is 0 at the end
    assert s["duplicate"] >= 1
    assert s["shared zero bit"] >= 1                  # two different keys whose only zero bit is the same one
    assert s["repeated tenant"] >= 1
    assert s["missing read then written"] >= 1        # contains_multi on a missing string, then add_multi, same handles
    assert s["list again after a re-creation"] >= 1   # the same handle list after a tenant came back
    assert s["stream add then contains"] >= 1
    assert s["handle call after"] >= {"rename", "delete", "import", "re-init"}
    assert s["old handle refused"] >= 1               # re-init with another config, then a call on the old handle
    assert s["recreated"] >= 3


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_an_injected_defect_is_caught(defect):
    for seed in SEEDS:
        try:
            D.run(D.FaultyModelEngine(defect), seed, STEPS)
        except AssertionError as e:
            assert f"seed {seed}, step " in str(e) and "the last commands" in str(e)  # what a replay needs
            return
    pytest.fail("no seed notices that " + DEFECTS[defect])
