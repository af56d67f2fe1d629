"""The byte commands' rule (redisson_amd/csrc/byte_cmd.h) under ASan + UBSan, as a stand-alone host program
(tests/c/byte_cmd_test.cpp): the header compiles without HIP, and byte_run_step over every sequence of up to 4
commands from a small alphabet -- offsets and ranges around 0, the string's ends, the 2^29 limit and the ends of
int64_t -- equals a plain restatement on an array, without a signed overflow.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_byte_cmd_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/byte_cmd_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "byte_cmd_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "byte_cmd_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
