// bytestream_kernels.hip -- GETRANGE / SETRANGE / APPEND / GET on device strings: the single calls
// (rbx_string_getrange / _setrange / _append) and the ordered stream over many keys (rbx_string_stream, DESIGN
// §11.12).  Command i is (key[i], cmds[i]); byte_cmd.h has its rules, the strings are reached through the BitKey
// table of the bit streams (rbx_kernels.h), and bitrange_device.h has the two tiers' list.
//
//  1. Plan (writes nothing to any string): k_by_pairs emits (canonical key, position), cell_sort lists each key's
//     commands in array order, and in k_by_plan ONE lane walks each key's run with byte_key_step from the key's
//     running state (ByteKeyState: the length word's value at first, then what the chunks before produced).  Per
//     command: where its bytes lie, how many, read or write, long or not (plan word), its reply and status, its
//     yield for the scan that makes `off`.  k_by_plan_serial does the same in array order for a tiny batch.
//  2. Rounds, after the host created or grew every written string to its final length: k_by_walk<G> gives each run
//     with commands left one group of G lanes, which executes the run's short commands in order from the run's
//     cursor and stops at its next long command, listing it (rs_list_claim); k_by_tiles then sweeps the listed
//     commands in tiles over the whole device.  One long command per key and round: the tiles of one launch never
//     touch the same string bytes, and the next round is the next launch.
//  3. k_by_lengths stores each written key's planned final length.
//
// Order inside one launch: a run is executed by ONE lane group and no other group touches its string in that launch.
// The lanes of the group store different bytes of a write and load different bytes of a later read, so behind every
// command that writes the group fences at workgroup scope (the wait for its stores that the fence implies) before
// the next command's loads.  The string pointers are neither const nor __restrict__ and every address depends on
// the lane, so the loads stay on the vector path: a scalar load could answer from the scalar cache, which the
// vector stores do not update.
// The zero-padding invariant: a write lies inside [at, at + cnt) with at + cnt <= the planned final length, and what
// lay between the old length and `at` was zero before.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitrange_device.h"
#include "bloom_common.h"
#include "rbx_kernels.h"

#include "byte_cmd.h"  // after rbx_device.h's RBX_HD

namespace rbx {

typedef unsigned long long u64;

// ---- the plan word of one command: at | cnt << 30 | kind << 60 | long << 62 (at, cnt <= 2^29) ----
constexpr int kByCntShift = 30, kByKindShift = 60;
constexpr u64 kByFieldMask = (1ULL << 30) - 1, kByLong = 1ULL << 62;
constexpr u64 kByRead = 1, kByWrite = 2;  // kind; 0 = nothing to move
__device__ __forceinline__ u64 plan_at(u64 w) { return w & kByFieldMask; }
__device__ __forceinline__ u64 plan_cnt(u64 w) { return (w >> kByCntShift) & kByFieldMask; }
__device__ __forceinline__ u64 plan_kind(u64 w) { return (w >> kByKindShift) & 3; }

// ---------------------------------------------------------------------------------
// Moving cnt bytes with `width` lanes (lane `l` of them): 16-byte vectors over the middle where source and
// destination are aligned alike, byte accesses over the misaligned head and tail -- and over everything where
// they are not.  Source and destination never overlap (a string against the value buffer or the output).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void lanes_copy(uint8_t *dst, const uint8_t *src, u64 cnt, uint32_t l, uint32_t width) {
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0 && cnt >= 32) {
        const u64 head = (16 - ((uintptr_t)dst & 15)) & 15;
        for (u64 b = l; b < head; b += width) dst[b] = src[b];
        const u64 nvec = (cnt - head) >> 4;
        uint4 *d = (uint4 *)(dst + head);
        const uint4 *s = (const uint4 *)(src + head);
        for (u64 v = l; v < nvec; v += width) d[v] = s[v];
        for (u64 b = head + (nvec << 4) + l; b < cnt; b += width) dst[b] = src[b];
    } else {
        for (u64 b = l; b < cnt; b += width) dst[b] = src[b];
    }
}

// where command p's bytes come from and go to
struct ByteMove { uint8_t *dst; const uint8_t *src; };
__device__ __forceinline__ ByteMove move_of(const BitKey &bk, u64 w, u64 p, const rbx_string_cmd *cmds, const uint8_t *vals,
                                            const u64 *off, uint8_t *out) {
    uint8_t *s = (uint8_t *)bk.words;
    if (plan_kind(w) == kByRead) return ByteMove{out + off[p], s + plan_at(w)};
    return ByteMove{s + plan_at(w), vals + cmds[p].val_off};
}

// ---------------------------------------------------------------------------------
// 1. Plan
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_by_state_init(const BitKey *__restrict__ tab, uint32_t nkeys,
                                                       ByteKeyState *__restrict__ state) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nkeys; i += stride) {
        const BitKey k = tab[i];
        bool missing;
        const u64 len = rs_len(k, &missing);
        state[i] = ByteKeyState{len, missing ? 0u : kByExists, 0u};
    }
}

// cell = the canonical key; a command that is the caller's error goes behind every key (cell nkeys) and flags the call
__global__ __launch_bounds__(256) void k_by_pairs(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                  const rbx_string_cmd *__restrict__ cmds, uint32_t m, uint32_t nkeys,
                                                  u64 vals_len, uint32_t *__restrict__ cell, uint32_t *__restrict__ pos,
                                                  u64 *sum) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const uint32_t k = key[i];
        const bool bad = k >= nkeys || byte_cmd_illegal(cmds[i], vals_len);
        if (bad) atomicOr(sum + kByFlags, (u64)kRsIllegal);
        cell[i] = bad ? nkeys : tab[k].canon;
        pos[i] = i;
    }
}

// what a lane gathers over the commands it plans
struct PlanAcc {
    u64 first[kByteKinds] = {~0ULL, ~0ULL, ~0ULL};
    u64 nlong = 0, tiles = 0;
};

// one command on its key's running state; gpos = its position in the call
__device__ __forceinline__ void plan_one(const rbx_string_cmd &c, bool wrong, ByteKeyState &ks, u64 gpos, uint32_t short_max,
                                         uint32_t tile_lg, u64 *plan, u64 *yield, int64_t *reply, uint8_t *status,
                                         PlanAcc &acc) {
    const ByteStep s = byte_key_step(ks.len, !(ks.flags & kByExists), wrong, c);
    u64 w = 0;
    if (s.fails) {
        acc.first[s.fails - 1] = min(acc.first[s.fails - 1], gpos);
    } else {
        ks.len = s.len;
        if (s.exists) ks.flags |= kByExists;
        if (s.writes) ks.flags |= kByWritten;
        if (s.cnt) {
            w = s.at | (s.cnt << kByCntShift) | ((s.writes ? kByWrite : kByRead) << kByKindShift);
            if (s.cnt > short_max) {
                w |= kByLong;
                ++acc.nlong;
                acc.tiles += ((s.cnt - 1) >> tile_lg) + 1;
            }
        }
    }
    *plan = w;
    *yield = s.writes || s.fails ? 0 : s.cnt;
    if (reply) *reply = s.reply;
    if (status) *status = byte_step_status(s);
}

__device__ __forceinline__ void plan_publish(const PlanAcc &acc, u64 *sum) {
    for (int k = 0; k < kByteKinds; ++k)
        if (acc.first[k] != ~0ULL) rs_first_min(sum + k, acc.first[k]);
    if (acc.nlong) {
        atomicAdd(sum + kByLongCmds, acc.nlong);
        atomicAdd(sum + kByTiles, acc.tiles);
    }
}

// One lane per run of the sorted chunk (the lane at the run's head); i0 = the chunk's first position in the call.
// plan / yield / replies / status are the chunk's slices.
__global__ __launch_bounds__(256) void k_by_plan(const BitKey *__restrict__ tab, const rbx_string_cmd *__restrict__ cmds,
                                                 const uint32_t *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                 uint32_t m, uint32_t nkeys, u64 i0, uint32_t short_max, uint32_t tile_lg,
                                                 ByteKeyState *state, u64 *__restrict__ plan, u64 *__restrict__ yield,
                                                 int64_t *__restrict__ replies, uint8_t *__restrict__ status, u64 *sum) {
    const uint32_t stride = gridDim.x * blockDim.x;
    PlanAcc acc;
    u64 most = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const uint32_t c = cell[i];
        if (c >= nkeys) {  // the caller's error: the call is refused, the scan still reads a yield
            plan[pos[i]] = 0;
            yield[pos[i]] = 0;
            continue;
        }
        if (i > 0 && cell[i - 1] == c) continue;  // not a run's head
        const bool wrong = tab[c].flags & kBitKeyWrong;
        ByteKeyState ks = state[c];
        const u64 before = acc.nlong;
        for (uint32_t j = i; j < m && cell[j] == c; ++j) {
            const uint32_t p = pos[j];
            plan_one(cmds[p], wrong, ks, i0 + p, short_max, tile_lg, plan + p, yield + p, replies ? replies + p : nullptr,
                     status ? status + p : nullptr, acc);
        }
        most = max(most, acc.nlong - before);
        state[c] = ks;
    }
    plan_publish(acc, sum);
    if (most) atomicMax(sum + kByMostLong, most);
}

// A tiny batch in array order, one lane, no sort: the keys' states are read and written in place, and a key's
// long commands are counted in its state.
__global__ void k_by_plan_serial(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                 const rbx_string_cmd *__restrict__ cmds, uint32_t m, uint32_t nkeys, u64 vals_len,
                                 uint32_t short_max, uint32_t tile_lg, ByteKeyState *state, u64 *__restrict__ plan,
                                 u64 *__restrict__ yield, int64_t *__restrict__ replies, uint8_t *__restrict__ status,
                                 u64 *sum) {
    PlanAcc acc;
    u64 most = 0;
    for (uint32_t p = 0; p < m; ++p) {
        const uint32_t k = key[p];
        if (k >= nkeys || byte_cmd_illegal(cmds[p], vals_len)) {
            sum[kByFlags] |= kRsIllegal;
            plan[p] = yield[p] = 0;
            continue;
        }
        const BitKey bk = tab[k];
        ByteKeyState ks = state[bk.canon];
        const u64 before = acc.nlong;
        plan_one(cmds[p], bk.flags & kBitKeyWrong, ks, p, short_max, tile_lg, plan + p, yield + p,
                 replies ? replies + p : nullptr, status ? status + p : nullptr, acc);
        ks.nlong += (uint32_t)(acc.nlong - before);
        most = max(most, (u64)ks.nlong);
        state[bk.canon] = ks;
    }
    plan_publish(acc, sum);
    if (most) atomicMax(sum + kByMostLong, most);
}

// ---------------------------------------------------------------------------------
// 2. Rounds
// ---------------------------------------------------------------------------------
// the runs of the sorted chunk: each head's cursor starts at the head, and the heads are listed (in any order)
__global__ __launch_bounds__(256) void k_by_heads(const uint32_t *__restrict__ cell, uint32_t m, uint32_t nkeys,
                                                  uint32_t *__restrict__ cur, uint32_t *__restrict__ heads, u64 *nheads) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const uint32_t c = cell[i];
        if (c >= nkeys || (i > 0 && cell[i - 1] == c)) continue;
        cur[i] = i;
        heads[atomicAdd(nheads, 1ULL)] = i;
    }
}

// One group of G lanes per run; the grid strides over the listed heads.  The group executes the run's commands from
// the cursor: a short one itself, the next long one goes on the round's list and ends the group's round.
template <int G>
__global__ __launch_bounds__(256) void k_by_walk(const BitKey *tab, const rbx_string_cmd *cmds, const uint8_t *vals,
                                                 const u64 *plan, const u64 *off, uint8_t *out, const uint32_t *cell,
                                                 const uint32_t *pos, uint32_t m, uint32_t *cur, const uint32_t *heads,
                                                 const u64 *nheads, uint32_t tile_lg, u64 *list, u64 *longs) {
    constexpr uint32_t kGroups = 256 / G;
    const uint32_t gl = threadIdx.x & (G - 1);
    const u64 nh = *nheads;
    for (u64 h = blockIdx.x * kGroups + threadIdx.x / G; h < nh; h += (u64)gridDim.x * kGroups) {
        const uint32_t i = heads[h], c = cell[i];
        const BitKey bk = tab[c];
        uint32_t j = cur[i];
        bool listed = false;
        for (; j < m && cell[j] == c && !listed; ++j) {
            const uint32_t p = pos[j];
            const u64 w = plan[p];
            if (w & kByLong) {
                if (gl == 0) rs_list_claim(list, longs, p, 0, (plan_cnt(w) - 1) << 3, tile_lg);
                listed = true;
            } else if (w) {
                const ByteMove mv = move_of(bk, w, p, cmds, vals, off, out);
                lanes_copy(mv.dst, mv.src, plan_cnt(w), gl, G);
                // the group's stores reach memory before the loads of the run's next command
                if (plan_kind(w) == kByWrite) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
        }
        if (gl == 0) cur[i] = j;  // (every lane of the group read the cursor before this store: one wave, in step)
    }
}

// a tiny batch without a long command: one group of G lanes runs it in array order
template <int G>
__global__ void k_by_walk_serial(const BitKey *tab, const uint32_t *key, const rbx_string_cmd *cmds, const uint8_t *vals,
                                 const u64 *plan, const u64 *off, uint8_t *out, uint32_t m) {
    for (uint32_t p = 0; p < m; ++p) {
        const u64 w = plan[p];
        if (!w) continue;
        const ByteMove mv = move_of(tab[key[p]], w, p, cmds, vals, off, out);
        lanes_copy(mv.dst, mv.src, plan_cnt(w), threadIdx.x, G);
        if (plan_kind(w) == kByWrite) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

// The tiles of the round's listed commands, numbered across the list (*list = long commands << kRsTileBits | tiles,
// as the walk left it).  Workgroup w takes tiles w, w + grid, ...
__global__ __launch_bounds__(256) void k_by_tiles(const BitKey *tab, const uint32_t *key, const rbx_string_cmd *cmds,
                                                  const uint8_t *vals, const u64 *plan, const u64 *off, uint8_t *out,
                                                  uint32_t tile_lg, const u64 *list, const u64 *longs) {
    const u64 lw = *list;
    const uint32_t nlong = (uint32_t)(lw >> kRsTileBits);
    const u64 ntiles = lw & ((1ULL << kRsTileBits) - 1);
    if (nlong == 0) return;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RsTile rt = rs_tile_of(longs, nlong, t);
        const u64 p = rt.i, w = plan[p], cnt = plan_cnt(w);
        const ByteMove mv = move_of(tab[key[p]], w, p, cmds, vals, off, out);
        const u64 b0 = rt.own << tile_lg;  // b0 < cnt: the tile is one of the command's (the list's invariant)
        lanes_copy(mv.dst + b0, mv.src + b0, min((u64)1 << tile_lg, cnt - b0), threadIdx.x, 256);
    }
}

// ---------------------------------------------------------------------------------
// 3. Lengths
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_by_lengths(const BitKey *__restrict__ tab, const ByteKeyState *__restrict__ state,
                                                    uint32_t nkeys) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nkeys; i += stride) {
        const BitKey k = tab[i];
        if (k.canon == i && (state[i].flags & kByWritten) && k.len) *k.len = state[i].len;
    }
}

// ---------------------------------------------------------------------------------
// The single calls: one command's bytes in tiles over the grid, and the string's new length
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_by_copy_one(uint8_t *dst, const uint8_t *src, u64 cnt, uint32_t tile_lg, u64 *len,
                                                     u64 new_len) {
    const u64 ntiles = cnt ? ((cnt - 1) >> tile_lg) + 1 : 0;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 b0 = t << tile_lg;
        lanes_copy(dst + b0, src + b0, min((u64)1 << tile_lg, cnt - b0), threadIdx.x, 256);
    }
    if (len && blockIdx.x == 0 && threadIdx.x == 0) *len = new_len;
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_bytes_copy(uint8_t *dst, const uint8_t *src, uint64_t cnt, uint32_t tile_bytes, unsigned long long *d_len,
                       uint64_t new_len, hipStream_t st) {
    const uint32_t lg = log2_of(tile_bytes);
    const uint64_t ntiles = cnt ? ((cnt - 1) >> lg) + 1 : 1;
    hipLaunchKernelGGL(k_by_copy_one, dim3((unsigned)std::min<uint64_t>(ntiles, kMaxGrid)), dim3(256), 0, st, dst, src,
                       (u64)cnt, lg, d_len, (u64)new_len);
}

void launch_bytestream_state_init(const BitKey *d_tab, uint32_t nkeys, ByteKeyState *d_state, hipStream_t st) {
    hipLaunchKernelGGL(k_by_state_init, dim3(grid_for(nkeys, kMaxGrid)), dim3(256), 0, st, d_tab, nkeys, d_state);
}

int launch_bytestream_sort(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, uint32_t m,
                           uint32_t nkeys, uint64_t vals_len, int key_bits, unsigned long long *d_sum, void *d_scratch,
                           size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<uint32_t> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, m, &b);
    if (e) return e;
    hipLaunchKernelGGL(k_by_pairs, dim3(grid_for(m, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, m, nkeys,
                       (u64)vals_len, b.cell_in, b.pos_in, d_sum);
    return cell_sort(b, m, 0, key_bits, st);
}

int launch_bytestream_plan(const BitKey *d_tab, const rbx_string_cmd *d_cmds, uint32_t m, uint32_t nkeys, uint64_t i0,
                           uint32_t short_max, uint32_t tile_bytes, ByteKeyState *d_state, unsigned long long *d_plan,
                           unsigned long long *d_yield, int64_t *d_replies, uint8_t *d_status, unsigned long long *d_sum,
                           void *d_scratch, size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<uint32_t> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, m, &b);
    if (e) return e;
    hipLaunchKernelGGL(k_by_plan, dim3(grid_for(m, kMaxGrid)), dim3(256), 0, st, d_tab, d_cmds, b.cell_out, b.pos_out, m,
                       nkeys, (u64)i0, short_max, log2_of(tile_bytes), d_state, d_plan, d_yield, d_replies, d_status, d_sum);
    return 0;
}

void launch_bytestream_plan_serial(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, uint32_t m,
                                   uint32_t nkeys, uint64_t vals_len, uint32_t short_max, uint32_t tile_bytes,
                                   ByteKeyState *d_state, unsigned long long *d_plan, unsigned long long *d_yield,
                                   int64_t *d_replies, uint8_t *d_status, unsigned long long *d_sum, hipStream_t st) {
    hipLaunchKernelGGL(k_by_plan_serial, dim3(1), dim3(1), 0, st, d_tab, d_key, d_cmds, m, nkeys, (u64)vals_len, short_max,
                       log2_of(tile_bytes), d_state, d_plan, d_yield, d_replies, d_status, d_sum);
}

int launch_bytestream_heads(uint32_t m, uint32_t nkeys, uint32_t *d_cur, uint32_t *d_heads, unsigned long long *d_nheads,
                            void *d_scratch, size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<uint32_t> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, m, &b);
    if (e) return e;
    hipLaunchKernelGGL(k_by_heads, dim3(grid_for(m, kMaxGrid)), dim3(256), 0, st, b.cell_out, m, nkeys, d_cur, d_heads,
                       d_nheads);
    return 0;
}

int launch_bytestream_walk(int lanes, const BitKey *d_tab, const rbx_string_cmd *d_cmds, const uint8_t *d_vals,
                           const unsigned long long *d_plan, const unsigned long long *d_off, uint8_t *d_out, uint32_t m,
                           uint32_t *d_cur, const uint32_t *d_heads, const unsigned long long *d_nheads,
                           uint32_t tile_bytes, unsigned long long *d_list, unsigned long long *d_long, void *d_scratch,
                           size_t scratch_bytes, hipStream_t st) {
    CellSortBufs<uint32_t> b;
    int e = cell_sort_carve(d_scratch, scratch_bytes, m, &b);
    if (e) return e;
    const uint32_t lg = log2_of(tile_bytes);
#define BY_WALK(G)                                                                                                       \
    hipLaunchKernelGGL(k_by_walk<G>, dim3(grid_for((uint64_t)m * G, kMaxGrid)), dim3(256), 0, st, d_tab, d_cmds, d_vals,  \
                       d_plan, d_off, d_out, b.cell_out, b.pos_out, m, d_cur, d_heads, d_nheads, lg, d_list, d_long)
    RBX_FOR_LANES(lanes, BY_WALK);
#undef BY_WALK
    return 0;
}

void launch_bytestream_walk_serial(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds,
                                   const uint8_t *d_vals, const unsigned long long *d_plan, const unsigned long long *d_off,
                                   uint8_t *d_out, uint32_t m, hipStream_t st) {
#define BY_SERIAL(G) \
    hipLaunchKernelGGL(k_by_walk_serial<G>, dim3(1), dim3(G), 0, st, d_tab, d_key, d_cmds, d_vals, d_plan, d_off, d_out, m)
    RBX_FOR_LANES(lanes, BY_SERIAL);
#undef BY_SERIAL
}

void launch_bytestream_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_string_cmd *d_cmds, const uint8_t *d_vals,
                             const unsigned long long *d_plan, const unsigned long long *d_off, uint8_t *d_out,
                             uint32_t tile_bytes, const unsigned long long *d_list, const unsigned long long *d_long,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_by_tiles, dim3(kMaxGrid), dim3(256), 0, st, d_tab, d_key, d_cmds, d_vals, d_plan, d_off, d_out,
                       log2_of(tile_bytes), d_list, d_long);
}

void launch_bytestream_lengths(const BitKey *d_tab, const ByteKeyState *d_state, uint32_t nkeys, hipStream_t st) {
    hipLaunchKernelGGL(k_by_lengths, dim3(grid_for(nkeys, kMaxGrid)), dim3(256), 0, st, d_tab, d_state, nkeys);
}

}  // namespace rbx
