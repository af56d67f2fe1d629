// api_bench.cpp -- the measurement helpers of include/rbx_bench.h (tools/ and bench.py; not part of the
// Redisson surface).  rbx_tune, the other half of that header, is in rbx_api.cpp.
#include <cstring>

#include "rbx_ctx.h"

using namespace rbx;

extern "C" {

int rbx_bench_gather(rbx_ctx *c, const void *d_table, uint64_t table_bytes, uint64_t nkeys, uint32_t k,
                     void *d_sink, void *stream) {
    if (!c || !d_table || !d_sink || table_bytes < 4) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    launch_gather_probe((const uint32_t *)d_table, table_bytes / 4, nkeys, k, (uint32_t *)d_sink,
                        pick_stream(c, stream));
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_slice_probe(rbx_ctx *c, const void *d_entries, uint64_t per_bucket, uint32_t nbuckets,
                          const void *d_bitmap, uint64_t slice_bytes, unsigned grid, void *d_sink, void *stream) {
    if (!c || !d_entries || !d_bitmap || !d_sink || grid < 8 || slice_bytes < 4 || (slice_bytes & (slice_bytes - 1)))
        return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    uint32_t lg = 0;
    while ((4ULL << lg) < slice_bytes) ++lg;
    launch_bench_slice_probe(d_entries, per_bucket, nbuckets, (const uint32_t *)d_bitmap, lg, grid & ~7u,
                             (uint32_t *)d_sink, pick_stream(c, stream));
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_add_stamps(rbx_ctx *c, unsigned long long *out, uint32_t n) {
    if (!c || !out || n > 16) return fail(RBX_E_ILLEGAL_ARGUMENT, "rbx_bench_add_stamps: n <= 16");
    // the context's lock and device, and only this context's work drained
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    RBX_TRY(set_device(c));  // fails on a shut context (the stamps freed)
    DevBuf &stamps = c->dev->pa.stamps;
    if (stamps.cap == 0) {
        memset(out, 0, n * 8);
        return RBX_OK;
    }
    RBX_TRY(quiesce(c));
    HIP_TRY(hipMemcpyAsync(out, stamps.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(stamps.p, 0, 16 * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RBX_OK;
}

int rbx_bench_stream_read(rbx_ctx *c, const void *d_buf, uint64_t bytes, void *d_sink, void *stream) {
    if (!c || !d_buf || !d_sink || ((uintptr_t)d_buf & 15)) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    launch_stream_read(d_buf, bytes, (uint32_t *)d_sink, pick_stream(c, stream));
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_stream_write(rbx_ctx *c, void *d_buf, uint64_t bytes, void *stream) {
    if (!c || !d_buf || ((uintptr_t)d_buf & 15)) return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    launch_stream_write(d_buf, bytes, pick_stream(c, stream));
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_gather_segments(rbx_ctx *c, const void *d_table, uint64_t table_bytes, uint64_t segment_bytes,
                              uint64_t keys_per_segment, uint64_t nkeys, void *d_sink, void *stream) {
    if (!c || !d_table || !d_sink || segment_bytes < 4 || table_bytes < segment_bytes || !keys_per_segment)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    launch_gather_segments((const uint32_t *)d_table, table_bytes / 4, segment_bytes / 4, keys_per_segment, nkeys,
                           (uint32_t *)d_sink, pick_stream(c, stream));
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_gather_regions(rbx_ctx *c, const void *d_table, uint64_t table_bytes, uint64_t region_bytes,
                             uint64_t nlanes, unsigned grid, void *d_sink, void *stream) {
    if (!c || !d_table || !d_sink || region_bytes < 4 || table_bytes < region_bytes || grid < 8)
        return fail(RBX_E_ILLEGAL_ARGUMENT, "bad argument");
    RBX_TRY(set_device(c));
    launch_gather_regions((const uint32_t *)d_table, table_bytes / 4, region_bytes / 4, nlanes, (uint32_t *)d_sink,
                          pick_stream(c, stream), grid & ~7u);
    HIP_TRY(hipGetLastError());
    return RBX_OK;
}

int rbx_bench_stream_geometry(rbx_ctx *c, uint64_t *out) {
    if (!c || !out) return fail(RBX_E_ILLEGAL_ARGUMENT, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(c->ks.mu);
    if (c->shut) return fail(RBX_E_ILLEGAL_STATE, "the context has been shut down");
    for (int i = 0; i < 4; ++i) out[i] = c->dev->strm.geom[i];
    return RBX_OK;
}

}  // extern "C"
