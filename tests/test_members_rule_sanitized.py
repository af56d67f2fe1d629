"""The rules of set-bit enumeration and of the BitSet exchange (redisson_amd/csrc/members_rule.h) under ASan + UBSan, as
a stand-alone host program (tests/c/members_rule_test.cpp): the header compiles without HIP, and the interval, the page
(skip + limit and skip + cap past 2^64 do not wrap), the k-th one of a vector and the length() / 8 + 1 rule equal
restatements in 128-bit arithmetic at the boundary lengths with extreme arguments.  Nothing is preloaded.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_members_rule_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/members_rule_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "members_rule_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "members_rule_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
