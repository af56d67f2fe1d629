// api_staging.cpp -- key arenas and the host tiers of api_staging.h: validation and plain uploads, the
// small tier's one pinned transfer, the tiny tier's coherent block and its completion word.
#include "api_staging.h"

#include <chrono>

#include "tunables.h"

namespace rbx {

int fast_len(const KeysDev &k) {
    if (k.offsets) return 0;
    if (((uintptr_t)k.bytes & 15) != 0) return 0;
    if (k.stride == 16 || k.stride == 32 || k.stride == 64) return (int)k.stride;
    return 0;
}

int fast_len_hll(const KeysDev &k) {
    if (k.offsets) return 0;
    if (k.stride == 16 || k.stride == 32 || k.stride == 64) return ((uintptr_t)k.bytes & 15) ? 0 : (int)k.stride;
    if (k.stride == 8 && ((uintptr_t)k.bytes & 7) == 0) return 8;
    return 0;
}

int validate_keys(const rbx_keys *k) {
    if (!k) return fail(RBX_E_ILLEGAL_ARGUMENT, "keys is NULL");
    if (k->n && !k->bytes && !(k->offsets == nullptr && k->stride == 0))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "keys->bytes is NULL");
    return RBX_OK;
}

// Copies keys [i0, i1) of a host arena to device buffers; returns a device view with keys renumbered
// from 0 (the offsets as the caller's: KeysDev.off_base = offsets[i0]).
int upload_keys(rbx_ctx *c, const rbx_keys *k, uint64_t i0, uint64_t i1, KeysDev *out) {
    Staging &sg = c->dev->stage;
    uint64_t n = i1 - i0;
    if (k->offsets) {
        uint64_t b0 = k->offsets[i0], b1 = k->offsets[i1];
        RBX_TRY(sg.keys_bytes.reserve(b1 - b0 + 16));
        RBX_TRY(sg.keys_offs.reserve((n + 1) * 8));
        if (b1 > b0) HIP_TRY(hipMemcpyAsync(sg.keys_bytes.p, k->bytes + b0, b1 - b0, hipMemcpyHostToDevice, c->stream));
        // the caller's offsets as they are (the kernels subtract off_base): no rebased copy on the stack,
        // so no sync before returning (a pageable source is staged by the runtime before the call returns)
        HIP_TRY(hipMemcpyAsync(sg.keys_offs.p, k->offsets + i0, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        *out = KeysDev{sg.keys_bytes.as<uint8_t>(), sg.keys_offs.as<uint64_t>(), 0, n, b0};
    } else {
        uint64_t bytes = n * k->stride;
        RBX_TRY(sg.keys_bytes.reserve(bytes + 16));
        if (bytes) HIP_TRY(hipMemcpyAsync(sg.keys_bytes.p, k->bytes + i0 * k->stride, bytes, hipMemcpyHostToDevice, c->stream));
        *out = KeysDev{sg.keys_bytes.as<uint8_t>(), nullptr, k->stride, n};
    }
    return RBX_OK;
}

int out_flags_dev(rbx_ctx *c, const void *want, uint64_t n, uint8_t **d_out) {
    *d_out = nullptr;
    if (want) RBX_TRY(c->dev->stage.out_bytes.reserve(n));
    if (want) *d_out = c->dev->stage.out_bytes.as<uint8_t>();
    return RBX_OK;
}

// Small host batches -- the single-key add(T) / contains(T) Redisson sends most, and collections of up
// to host_small_bytes of key bytes (and a quarter as many keys): the keys are copied into pinned memory behind a zero
// count word and uploaded on the context stream in ONE transfer (no copy-stream hand-off, no sync before
// the launch: the slot's previous reader is waited for by its event), and the count and flags come back
// into the same pinned block with one sync.  (The pipelined path costs a fill, a sync, a copy-stream
// upload from pageable memory with two event hops, and a second sync: ~62 us for one key on the r05
// boxes, tools/microbench.py smallbatch.)
static size_t small_pin_bytes(uint64_t limit) { return kSmallHead + limit + limit / 4 + 64; }  // head | keys | tail

// the pinned block of the one-transfer path, laid out for host_small_bytes = limit (or a larger limit it
// already had); false (the caller takes the pipelined path) when pinned memory cannot be had
static bool small_pinned(rbx_ctx *c, uint64_t limit) {
    Staging &sg = c->dev->stage;
    if (sg.pin_small.p && sg.pin_small_limit >= limit) return true;
    sg.pin_small_limit = 0;
    if (sg.pin_small.alloc(small_pin_bytes(limit), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    sg.pin_small_limit = limit;
    return true;
}

// the process-wide limit is read ONCE here (rbx_tune may change it on another thread);
// the staging below uses the block's own layout (pin_small_limit >= the limit checked here)
bool bloom_small_fits(rbx_ctx *c, const rbx_keys *k) {
    const uint64_t limit = g_tune.small_bytes;
    if (!g_tune.small_host || k->n == 0 || k->n > limit / 4) return false;
    const uint64_t nb = arena_bytes(k);
    return nb + (k->offsets ? (k->n + 1) * 8 + 8 : 0) <= limit && small_pinned(c, limit);
}

// an error after small_stage queued the upload: the copy and any launches may still be reading the pinned
// block and slot 0, which the next small call overwrites -- drain the stream first
int small_fail(rbx_ctx *c, int rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// One-transfer staging of a small host arena (bloom_small_fits): pinned [0, head) zeroed, the key bytes
// from `head`, then the offsets (absolute: KeysDev.off_base), uploaded with one copy into staging slot 0
// on the context stream after slot 0's last reader (its event).  The caller records ev_done[0] after
// its launches, reads results back into hp / tail_h and syncs; the pinned block stays untouched until then.
int small_stage(rbx_ctx *c, const rbx_keys *keys, uint64_t head, SmallStage *s, const void *head_src,
                uint64_t head_src_at, uint64_t head_src_len) {
    Staging &sg = c->dev->stage;
    const size_t pin = sg.pin_small.cap;  // allocated by bloom_small_fits (small_pinned)
    head = (std::max<uint64_t>(head, 8) + 63) / 64 * 64;  // <= kSmallHead (callers bound it)
    uint8_t *hp = sg.pin_small.as<uint8_t>();
    const uint64_t n = keys->n, b0 = keys->offsets ? keys->offsets[0] : 0;
    const uint64_t nb = arena_bytes(keys);
    const uint64_t off_at = keys->offsets ? (head + nb + 7) / 8 * 8 : 0, end = off_at ? off_at + (n + 1) * 8 : head + nb;
    memset(hp, 0, head);
    if (head_src_len) memcpy(hp + head_src_at, head_src, head_src_len);  // e.g. segment offsets behind the counts
    if (nb) memcpy(hp + head, keys->bytes + b0, nb);
    if (off_at) memcpy(hp + off_at, keys->offsets, (n + 1) * 8);
    RBX_TRY(sg.slot_bytes[0].reserve(pin));
    uint8_t *dp = sg.slot_bytes[0].as<uint8_t>();
    HIP_TRY(hipStreamWaitEvent(c->stream, sg.ev_done[0], 0));  // slot 0's last reader (any stream)
    HIP_TRY(hipMemcpyAsync(dp, hp, end, hipMemcpyHostToDevice, c->stream));
    s->hp = hp;
    s->dp = dp;
    s->tail_h = hp + kSmallHead + sg.pin_small_limit;
    s->dk = KeysDev{dp + head, off_at ? (const uint64_t *)(dp + off_at) : nullptr, keys->stride, n, off_at ? b0 : 0};
    return RBX_OK;
}

// Tiny host batches -- add(T) / contains(T) and collections of up to host_tiny_keys keys and 64 KiB of key
// bytes: the keys are copied into coherent (uncached, device-mapped) pinned memory, the kernels read them
// from there over the host link and write their flags back into it, so the call is its launches and a wait
// for a completion word in the same block: no upload, no readback, no zeroed count word.  Counts are the flags' sums on the host
// (add(Collection) and contains(Collection) both count the keys whose reply is true,
// M/RedissonBloomFilter.java:104-137,208-236; per segment for the multi-tenant calls).
bool bloom_tiny_fits(rbx_ctx *c, const rbx_keys *keys) {
    const uint64_t lim = g_tune.tiny_keys;  // once per call
    if (!g_tune.small_host || keys->n == 0 || keys->n > lim || keys->n > kSegMaxKeys) return false;
    const uint64_t nb = arena_bytes(keys);
    if (nb > kTinyBytes) return false;
    Staging &sg = c->dev->stage;
    if (sg.pin_tiny.p) return true;
    void *d = nullptr;
    if (sg.pin_tiny.alloc(kTinyBlock, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(&d, sg.pin_tiny.p, 0) != hipSuccess) {
        (void)hipGetLastError();
        sg.pin_tiny.release();
        return false;
    }
    memset(sg.pin_tiny.p, 0, kTinyBlock);  // the completion word starts below every sequence number
    sg.pin_tiny_dev = (uint8_t *)d;
    sg.tiny_seq = 0;
    return true;
}

// the keys into the block (the previous call's kernels were done when it returned: tiny_wait); their device view
KeysDev tiny_stage(rbx_ctx *c, const rbx_keys *keys) {
    uint8_t *hp = c->dev->stage.tiny(), *dp = c->dev->stage.pin_tiny_dev;
    const uint64_t n = keys->n, b0 = keys->offsets ? keys->offsets[0] : 0;
    const uint64_t nb = arena_bytes(keys);
    if (nb) memcpy(hp + kTinyKeysAt, keys->bytes + b0, nb);
    if (keys->offsets) memcpy(hp + kTinyOffsAt, keys->offsets, (n + 1) * 8);
    return KeysDev{dp + kTinyKeysAt, keys->offsets ? (const uint64_t *)(dp + kTinyOffsAt) : nullptr, keys->stride, n,
                   keys->offsets ? b0 : 0};
}

// A tiny call learns that its kernels are done from a completion word in the block, not from the stream
// (`host_tiny_spin`, default 1): a one-key call's one-lane kernel stores a sequence number there last
// (system-scope release), other calls launch k_done_word behind their kernels, and the host spins on it --
// 7.2 / 9.6 us against 11.5 us for a one-wave kernel and a stream sync (tools/syncbench.hip).  After 2 ms
// without it (a queue still busy with earlier work, or a fault) the host waits for the stream, which also
// reports any error.
uint32_t tiny_next_seq(rbx_ctx *c) {
    uint32_t &last = c->dev->stage.tiny_seq;
    uint32_t seq = ++last;
    if (seq == 0) seq = last = 1;
    return seq;
}

// rc: the launches' result; word_launched: seq is on its way (else the call falls back to the stream)
int tiny_wait(rbx_ctx *c, int rc, uint32_t seq, bool word_launched) {
    const hipError_t e = hipGetLastError();
    if (rc != RBX_OK || e != hipSuccess || !word_launched) {
        const hipError_t es = hipStreamSynchronize(c->stream);
        RBX_TRY(rc);
        HIP_TRY(e);
        HIP_TRY(es);
        return RBX_OK;
    }
    const auto *h_done = (const uint32_t *)(c->dev->stage.tiny() + kTinyDoneAt);
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) != seq) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) != seq)
                return fail(RBX_E_DEVICE, "tiny call finished without its completion word");
            break;
        }
    }
    return RBX_OK;
}

// the launches' result -> the completion word behind them (or the stream when spinning is off) -> errors;
// spin: host_tiny_spin as the call read it
int tiny_done(rbx_ctx *c, int rc, bool spin) {
    spin = spin && rc == RBX_OK;
    const uint32_t seq = spin ? tiny_next_seq(c) : 0;
    if (spin) launch_done_word((uint32_t *)(c->dev->stage.pin_tiny_dev + kTinyDoneAt), seq, c->stream);
    return tiny_wait(c, rc, seq, spin);
}

}  // namespace rbx
