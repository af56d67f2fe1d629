"""The host's planner for grouped PFCOUNT / PFMERGE calls (redisson_amd/csrc/hll_groups_plan.h: the argument check
and the phase rule) under ASan + UBSan, as a stand-alone host program (tests/c/hll_groups_plan_test.cpp): empty
input, one group, the read-after-write, write-after-read and write-after-write pairs, a destination among its own
sources, a failed group between two dependent ones, a chain of 1,000, 1,000 independent groups, key ids at
nkeys - 1.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_hll_groups_plan_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/hll_groups_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "hll_groups_plan_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hll_groups_plan_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
