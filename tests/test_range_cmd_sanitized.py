"""The read queries' command rule (redisson_amd/csrc/range_cmd.h) under ASan + UBSan, as a stand-alone host program
(tests/c/range_cmd_test.cpp): the header compiles without HIP, and the intervals, fixed replies and failure kinds
equal a bit-by-bit restatement at the boundary lengths with extreme starts and ends, without a signed overflow.
CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_range_cmd_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/range_cmd_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "range_cmd_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "range_cmd_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
