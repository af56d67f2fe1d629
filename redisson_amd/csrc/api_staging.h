// api_staging.h -- key arenas from host to device and the three tiers a host-buffer call picks from: tiny
// (coherent pinned block, no transfer), small (one pinned transfer), pipelined (copy-stream double buffer).
#pragma once
#include <cstring>

#include "rbx_ctx.h"

namespace rbx {

int fast_len(const KeysDev &k);
int fast_len_hll(const KeysDev &k);
int validate_keys(const rbx_keys *k);
// *d_out: the context's device bytes for n reply flags when the caller wants them (else null)
int out_flags_dev(rbx_ctx *c, const void *want, uint64_t n, uint8_t **d_out);
int upload_keys(rbx_ctx *c, const rbx_keys *k, uint64_t i0, uint64_t i1, KeysDev *out);

// key bytes of a host arena
inline uint64_t arena_bytes(const rbx_keys *k) { return k->offsets ? k->offsets[k->n] - k->offsets[0] : k->n * k->stride; }

// Runs fn(chunk view, chunk index range) over a host arena in chunks of ~staging_bytes:
// chunk j is uploaded on copy_stream into slot j%2 while chunk j-1 computes on `st`.
template <class Fn>
int pipelined_host_batches(rbx_ctx *c, const rbx_keys *k, hipStream_t st, Fn &&fn) {
    Staging &sg = c->dev->stage;
    uint64_t j = 0;
    for (uint64_t i0 = 0; i0 < k->n; ++j) {
        // chunk [i0, i1) of <= staging_bytes key bytes (at least one key)
        uint64_t i1;
        if (k->offsets) {
            uint64_t lo = i0 + 1, hi = k->n;
            const uint64_t b0 = k->offsets[i0];
            if (k->offsets[hi] - b0 <= sg.staging_bytes) {
                lo = hi;
            } else {
                while (hi - lo > 0) {  // largest i1 >= i0+1 with bytes <= staging
                    const uint64_t mid = (lo + hi + 1) / 2;
                    if (k->offsets[mid] - b0 <= sg.staging_bytes) lo = mid;
                    else hi = mid - 1;
                }
            }
            i1 = lo;
        } else {
            const uint64_t per = k->stride ? std::max<uint64_t>(1, sg.staging_bytes / k->stride) : k->n;
            i1 = std::min<uint64_t>(k->n, i0 + per);
        }
        const int s = (int)(j & 1);
        const uint64_t n = i1 - i0;
        const uint64_t b0 = k->offsets ? k->offsets[i0] : i0 * k->stride;
        const uint64_t nb = k->offsets ? k->offsets[i1] - b0 : n * k->stride;
        RBX_TRY(sg.slot_bytes[s].reserve(nb + 16));
        if (k->offsets) RBX_TRY(sg.slot_offs[s].reserve((n + 1) * 8));
        HIP_TRY(hipStreamWaitEvent(sg.copy_stream, sg.ev_done[s], 0));
        if (nb) HIP_TRY(hipMemcpyAsync(sg.slot_bytes[s].p, k->bytes + b0, nb, hipMemcpyHostToDevice, sg.copy_stream));
        if (k->offsets)
            HIP_TRY(hipMemcpyAsync(sg.slot_offs[s].p, k->offsets + i0, (n + 1) * 8, hipMemcpyHostToDevice, sg.copy_stream));
        HIP_TRY(hipEventRecord(sg.ev_copied[s], sg.copy_stream));
        HIP_TRY(hipStreamWaitEvent(st, sg.ev_copied[s], 0));
        KeysDev dk{sg.slot_bytes[s].as<uint8_t>(), k->offsets ? sg.slot_offs[s].as<uint64_t>() : nullptr, k->stride, n,
                   k->offsets ? b0 : 0};
        RBX_TRY(fn(dk, i0));
        HIP_TRY(hipEventRecord(sg.ev_done[s], st));
        i0 = i1;
    }
    return RBX_OK;
}

// ---- the small tier ---------------------------------------------------------------------------------
bool bloom_small_fits(rbx_ctx *c, const rbx_keys *k);
int small_fail(rbx_ctx *c, int rc);
struct SmallStage {
    uint8_t *hp = nullptr, *dp = nullptr, *tail_h = nullptr;  // pinned block, its device copy, readback area
    KeysDev dk{};
};
int small_stage(rbx_ctx *c, const rbx_keys *keys, uint64_t head, SmallStage *s, const void *head_src = nullptr,
                uint64_t head_src_at = 0, uint64_t head_src_len = 0);

// ---- the tiny tier ----------------------------------------------------------------------------------
// bump allocation in the block's arena region: the device view of a copy of src, nullptr when full (the
// caller then uploads as usual).  Every copy stays put until the call's final sync.
struct TinyArena {
    uint8_t *h, *d;
    size_t cap, used;
    const void *put(const void *src, size_t n) {
        const size_t at = (used + 63) / 64 * 64;
        if (at + n > cap) return nullptr;
        memcpy(h + at, src, n);
        used = at + n;
        return d + at;
    }
};
bool bloom_tiny_fits(rbx_ctx *c, const rbx_keys *keys);
KeysDev tiny_stage(rbx_ctx *c, const rbx_keys *keys);
uint32_t tiny_next_seq(rbx_ctx *c);
int tiny_wait(rbx_ctx *c, int rc, uint32_t seq, bool word_launched);
int tiny_done(rbx_ctx *c, int rc, bool spin);

}  // namespace rbx
