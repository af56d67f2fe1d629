"""The C-ABI library loads, exports every symbol include/*.h declares, and its
host-compiled device primitives agree with the oracle.  CPU only (no compute calls on a GPU)."""
import ctypes as C
import glob
import os
import re

import numpy as np

from oracle import oracle as O
from redisson_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        syms |= set(re.findall(r"\b(rbx_[a-z0-9_]+)\s*\(", txt))
    return syms


def test_library_loads_and_exports_all_declared_symbols():
    lib = L.lib()
    syms = declared_symbols()
    assert len(syms) > 40
    missing = [s for s in sorted(syms) if not hasattr(lib, s)]
    assert not missing, missing
    # and the Python binding covers the whole header
    assert syms <= set(L.SIGNATURES), sorted(syms - set(L.SIGNATURES))


def test_abi_version():
    assert L.lib().rbx_abi_version() == 1


def test_fastmod_host_compiled_matches_percent():
    assert L.lib().rbx_selftest_mod(200_000, 12345) == 0


def test_device_hash128_host_compiled_matches_oracle():
    rng = np.random.default_rng(9)
    out = (C.c_uint64 * 2)()
    for ln in list(range(0, 100)) + [127, 128, 129, 1000]:
        d = rng.bytes(ln)
        b = (C.c_uint8 * max(1, ln)).from_buffer_copy(d or b"\0")
        L.lib().rbx_selftest_hash128(b, ln, out)
        assert (out[0], out[1]) == O.redisson_hash128(d), ln


def test_bloom_index_sequence_host_compiled_matches_oracle():
    # the cursor every Bloom kernel walks (rbx_device.h BloomSeq) against RedissonBloomFilter.hash()
    rng = np.random.default_rng(11)
    m64 = (1 << 64) - 1
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 64, size=(300, 2), dtype=np.uint64)]
    pairs += [(m64, m64), (0, 0)]
    for k in (1, 2, 7, 8, 9, 16, 17, 32, 33, 40):
        out = (C.c_uint32 * k)()
        for size in (1, 2, 3, 1 << 19, 95_850_584, 4_294_967_293, 1 << 32):
            for h1, h2 in pairs:
                assert L.lib().rbx_selftest_bloom_indexes(h1, h2, k, size, out) == 0, (h1, h2, k, size)
                assert list(out) == O.bloom_indexes(h1, h2, k, size), (h1, h2, k, size)


def test_crc16_and_slot_exports():
    from redisson_amd import calc_slot, crc16, slot_to_gpu

    assert crc16(b"123456789") == 0x31C3
    for k in [b"foo{bar}baz", b"{}", b"a}b{c}", b"filter", b"{filter}:config", b""]:
        assert calc_slot(k) == O.calc_slot(k)
    assert [slot_to_gpu(s, 8) for s in (0, 2047, 2048, 16383)] == [0, 0, 1, 7]


def test_false_probability_plain_string():
    # BigDecimal.valueOf(p).toPlainString() stored in {name}:config (:288)
    buf = C.create_string_buffer(64)
    cases = {0.03: "0.03", 0.001: "0.001", 1e-4: "0.00010", 1e-10: "0.00000000010", 0.5: "0.5",
             1.0: "1.0", 0.0: "0.0", 0.01: "0.01", 1.5e-5: "0.000015", 0.123456789: "0.123456789"}
    for p, want in cases.items():
        L.lib().rbx_selftest_plain_string(p, buf, 64)
        assert buf.value.decode() == want, (p, buf.value)


def test_error_mapping_without_gpu():
    from redisson_amd.exceptions import IllegalArgumentException, raise_for

    s, k = C.c_int64(), C.c_uint32()
    rc = L.lib().rbx_bloom_optimal_config(1, 2.0, C.byref(s), C.byref(k))
    assert rc == L.RBX_E_ILLEGAL_ARGUMENT
    try:
        raise_for(rc, L.last_error())
    except IllegalArgumentException as e:
        assert "greater than 1" in str(e)
    rc = L.lib().rbx_bloom_optimal_config(100, 0.03, C.byref(s), C.byref(k))
    assert rc == 0 and (s.value, k.value) == (729, 5)


def test_ttl_symbols_declared():
    """The key-timeout entry points are exported and declared (RExpirable surface)."""
    import re

    hdr = open(os.path.join(ROOT, "include", "rbx.h")).read()
    for sym in ("rbx_pexpire", "rbx_persist", "rbx_pttl", "rbx_pexpiretime"):
        assert re.search(r"\b%s\(" % sym, hdr), sym


def test_negative_expected_insertions_like_the_reference():
    """tryInit(-n, p): optimalNumOfBits gives a negative size, which passes `size > getMaxSize()`
    (M/RedissonBloomFilter.java:270-276) -- the config is created, as in the oracle."""
    s, k = C.c_int64(), C.c_uint32()
    for n, p in [(-100, 0.03), (-1, 0.5), (-10_000_000, 0.01)]:
        assert L.lib().rbx_bloom_optimal_config(n, p, C.byref(s), C.byref(k)) == 0, (n, p)
        want = O.bloom_optimal(n, p)
        assert (s.value, k.value) == want, (n, p, s.value, k.value, want)
        assert s.value < 0


def test_product_library_has_no_wrong_answer_switches():
    """the timing diagnostics that make answers wrong exist only in the profiling build
    (librbx_diag.so, `make diag`); librbx.so rejects their keys, and the r02-r05 A/B variants removed in
    r06 are gone with their knobs.  The whitelist (include/rbx_bench.h) still answers."""
    lib = L.lib()
    for key in (b"stream_diag", b"contains_partition_flags", b"add_partition_diag"):
        assert lib.rbx_tune(key, 1 if key == b"stream_diag" else 4) == -1, key
        assert "profiling build" in L.last_error() or "librbx_diag" in L.last_error()
    for key in (b"stream_prefilter", b"stream_occupancy", b"stream_owner", b"stream_contains_slots",
                b"walk_reset_all", b"contains_qshape", b"contains_partials", b"add_rebucket_lines",
                b"add_region_kernel", b"add_multi_seg_lgs", b"stream_table_scale", b"contains_emit2_nt"):
        assert lib.rbx_tune(key, 1) == -1, key
    assert lib.rbx_tune(b"add_multi_table8", 1) == -1
    for key, val in ((b"add_multi_table8", 2), (b"contains_stage1", 4), (b"stream_table8", 1),
                     (b"add_multi_seg_grid", 8192), (b"host_small_bytes", 4 << 20), (b"host_tiny_keys", 16384),
                     (b"add_single_seg_keys", 256), (b"add_one_key", 1),
                     (b"host_tiny_spin", 1)):
        assert lib.rbx_tune(key, val) == 0, key
