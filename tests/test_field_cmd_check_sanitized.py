"""The BITFIELD stream's per-command check (redisson_amd/csrc/field_rule.h field_cmd_check: the type, then the
offset limit) under ASan + UBSan, as a stand-alone host program (tests/c/field_cmd_check_test.cpp): u63 / u64 /
i64 / i65 / size 0, and the offsets 2^32 - size, 2^32 - size + 1 and 2^32 for every type.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_field_cmd_check_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/field_cmd_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "field_cmd_check_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "field_cmd_check_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
