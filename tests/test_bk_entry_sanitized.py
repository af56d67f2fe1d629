"""The partitioned contains' 5-byte entry format and geometry rules (redisson_amd/csrc/bk_entry.h) under ASan + UBSan,
as a stand-alone host program (tests/c/bk_entry_test.cpp): pack / unpack round trips on an exactly sized 64-byte line at
the corners (offset 0 and 2^21 - 1; thread 0 and 1023; tile iteration 0, 1, 2, 255, 256 and 511; block 0 and G - 1; G in
{1, 2, 255, 256}; every slot of the line), the key the probe rebuilds against the plain tile * 1024 + thread, the chunk
rule (no chunk at any grid 1-256 and any k 2-16 gives a block-local key index of 2^19 or more), and the segment capacity
(a multiple of 12 entries, segments at 64-byte aligned offsets) for filters of 2^21, 2^21 + 1, 2^27 and 2^32 - 3 bits.
CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redisson_amd", "csrc")


def test_bk_entry_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "../../tests/c/_build/bk_entry_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "_build", "bk_entry_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bk_entry_test: ok" in r.stdout
    assert "runtime error" not in r.stderr and "WARNING" not in r.stderr, r.stderr
