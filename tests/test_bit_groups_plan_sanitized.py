"""The host's planner for grouped BITOP / BITCOUNT calls (redisson_amd/csrc/bit_groups_plan.h: the phase rule and
forwarding) under ASan + UBSan, as a stand-alone host program (tests/c/bit_groups_plan_test.cpp): empty input, one
group, the read-after-write, write-after-read and write-after-write pairs, a destination among its own sources, a
group without a destination before and after a writer, forwarding taken and not taken (NOT, two entries, a failed
writer, an earlier phase), 1,000 pairs on distinct temporaries (one phase) and on one temporary (1,000 phases), a chain
of 1,000, key ids at nkeys - 1, a failed group between two dependent ones.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_bit_groups_plan_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/bit_groups_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "bit_groups_plan_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit_groups_plan_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
