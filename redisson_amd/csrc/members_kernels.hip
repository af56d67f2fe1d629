// members_kernels.hip -- set-bit enumeration (rbx_bitset_members) and the java.util.BitSet exchange
// (rbx_bitset_as_words / rbx_bitset_set_words) over the engine's bitmap strings; DESIGN §11.11, rules:
// members_rule.h.  Like bitrange_kernels.hip, the enumeration works on a normalised bit interval [lo, hi]
// (lo <= hi < 8 * length), reads aligned 16-byte vectors -- the last one may reach into the zero padding behind the
// length, never past the allocation -- masks them with bitrange_device.h's vec_wanted and stores nothing to the
// bitmap.  A position is (vector index << 7) + offset in 64-bit arithmetic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bitrange_device.h"
#include "bloom_common.h"
#include "members_rule.h"
#include "rbx_kernels.h"

namespace rbx {

// ---------------------------------------------------------------------------------
// 1. The page.  P is the block directory of the whole string (launch_bits_directory).  One wave corrects the
// interval's first and last block by a masked count: state = {the ones below lo, the page's first rank, its end
// rank}, ranks counted from the interval's first one; counts = {written, total}.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_members_head(const uint4 *__restrict__ vecs, uint64_t len, uint64_t lo, uint64_t hi,
                                                     uint64_t skip, uint64_t cap, const unsigned long long *__restrict__ P,
                                                     unsigned long long *__restrict__ state,
                                                     unsigned long long *__restrict__ counts) {
    const uint32_t lane = threadIdx.x;
    const uint64_t b0 = lo >> kBlockLog2, bh = hi >> kBlockLog2;
    uint64_t below = P[b0], upto = P[bh + 1];
    if (lo > (b0 << kBlockLog2)) below += wave_count(vecs, b0 << kBlockLog2, lo - 1, lane);
    const uint64_t last = min((bh + 1) << kBlockLog2, len * 8) - 1;  // block bh's last bit inside the string
    if (hi < last) upto -= wave_count(vecs, hi + 1, last, lane);
    uint64_t first, count;
    members_page(upto - below, skip, ~0ULL, cap, &first, &count);
    if (lane == 0) {
        state[0] = below;
        state[1] = first;
        state[2] = first + count;
        counts[0] = count;
        counts[1] = upto - below;
    }
}

// ---------------------------------------------------------------------------------
// 2. Expand: one workgroup per 4 KiB block of the interval, one vector per thread.  Block b holds the ranks
// [P[b] - below, P[b + 1] - below) (its part inside [lo, hi]: the first block starts at rank 0, the last one may end
// earlier than the directory says, which the bound below only overestimates); a block without a rank of the page
// [first, end) is not read.  The workgroup scans its threads' masked counts, then CONSECUTIVE THREADS TAKE
// CONSECUTIVE RANKS: a thread finds the vector of its rank by a search over the 256 inclusive counts in LDS and
// selects the k-th one of that vector, so that a wave stores 512 contiguous bytes whatever the block's fill.  (The
// owner-stores alternative issues, on a full block, 128 stores per lane that lie 1 KiB apart within the wave.)
// ---------------------------------------------------------------------------------
// One workgroup, one masked vector per thread: x = the wanted ones of vector v0 + tid.  rs = the rank of the block's
// first one; the ones whose rank lies in [first, end) go to out[obase + rank - first], as far as that index is below
// cap.  Returns the block's ones.  Every thread of the workgroup calls it (it holds barriers).
__device__ __forceinline__ uint32_t block_expand(const uint4 x, uint64_t v0, uint64_t rs, uint64_t first, uint64_t end,
                                                 unsigned long long *__restrict__ out, uint64_t obase, uint64_t cap) {
    __shared__ uint32_t s_incl[256];
    __shared__ uint4 s_vec[256];
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t incl = popc4(x);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
    const uint32_t nb = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_incl[tid] = before + incl;
    s_vec[tid] = x;
    __syncthreads();
    // the block's own ranks [l0, l1) of the page
    const uint64_t l0 = first > rs ? first - rs : 0, l1 = end > rs ? min((uint64_t)nb, end - rs) : 0;
    for (uint64_t k = l0 + tid; k < l1; k += 256) {
        uint32_t a = 0, z = 255;  // the first vector whose inclusive count exceeds k
        while (a < z) {
            const uint32_t m = (a + z) >> 1;
            if (s_incl[m] > (uint32_t)k) z = m;
            else a = m + 1;
        }
        const uint4 y = s_vec[a];
        const uint32_t kk = (uint32_t)k - (a ? s_incl[a - 1] : 0u);
        const uint64_t idx = obase + (rs + k - first);
        if (idx < cap) out[idx] = ((v0 + a) << 7) + vec_select(y.x, y.y, y.z, y.w, kk);
    }
    __syncthreads();  // the next block rewrites the LDS
    return nb;
}

__global__ __launch_bounds__(256) void k_members_expand(const uint4 *__restrict__ vecs, uint64_t nvec, uint64_t lo,
                                                        uint64_t hi, const unsigned long long *__restrict__ P,
                                                        const unsigned long long *__restrict__ state,
                                                        unsigned long long *__restrict__ out) {
    const uint64_t below = state[0], first = state[1], end = state[2];
    if (first >= end) return;
    const uint64_t b0 = lo >> kBlockLog2, bh = hi >> kBlockLog2;
    for (uint64_t b = b0 + blockIdx.x; b <= bh; b += gridDim.x) {  // every condition here is uniform in the workgroup
        const uint64_t pb = P[b], pb1 = P[b + 1];
        const uint64_t rs = b == b0 ? 0 : pb - below, re = pb1 - below;
        if (pb1 == pb || re <= first || rs >= end) continue;
        const uint64_t v = b * 256 + threadIdx.x;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (v < nvec) x = vec_wanted<false>(ld_nt16(vecs + v), v, lo, hi);
        block_expand(x, b * 256, rs, first, end, out, 0, ~0ULL);
    }
}

// ---------------------------------------------------------------------------------
// 3. asBitSet(): *nwords = 1 + the index of the string's last non-zero 64-bit word (the caller zeroes it; the
// length comes from the device length word, and what a vector holds past it is zero), then min(cap_words, *nwords)
// words, each half a 32-bit load with the bits of its bytes reversed.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_words_last(const uint4 *__restrict__ vecs, const unsigned long long *__restrict__ d_len,
                                                    uint64_t cap_bytes, unsigned long long *nwords) {
    // (the length clamped to the allocation, as rs_len does: the host keeps the allocation at or above it)
    const uint64_t nvec = (min((uint64_t)*d_len, cap_bytes) + 15) >> 4, stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
        const uint4 x = ld_nt16(vecs + v);
        if (x.x | x.y) mx = 2 * v + 1;
        if (x.z | x.w) mx = 2 * v + 2;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned long long)__shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(nwords, mx);
}

__global__ __launch_bounds__(256) void k_words_export(const uint4 *__restrict__ vecs, const unsigned long long *__restrict__ nwords,
                                                      uint64_t cap_words, unsigned long long *__restrict__ out) {
    const uint64_t m = min((uint64_t)*nwords, cap_words), stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * v < m; v += stride) {
        const uint4 x = ld_nt16(vecs + v);  // word 2 v < *nwords: the vector lies inside the string's vectors
        out[2 * v] = (uint64_t)rev_bytes(x.x) | (uint64_t)rev_bytes(x.y) << 32;
        if (2 * v + 1 < m) out[2 * v + 1] = (uint64_t)rev_bytes(x.z) | (uint64_t)rev_bytes(x.w) << 32;
    }
}

// ---------------------------------------------------------------------------------
// 4. set(BitSet): *highest1 = 1 + the highest set bit of the words (the caller zeroes it: 0 = none), and, into a
// zeroed allocation, the string of `bytes` bytes (members_rule.h words_string_len; every bit past the highest is
// clear, so whole vectors are stored and the padding stays zero) with its length word.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_words_highest(const unsigned long long *__restrict__ words, uint64_t n,
                                                       unsigned long long *highest1) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned long long w = words[i];
        if (w) mx = words_highest(i, w) + 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned long long)__shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(highest1, mx);
}

__global__ __launch_bounds__(256) void k_words_import(const unsigned long long *__restrict__ words, uint64_t n, uint64_t bytes,
                                                      uint4 *__restrict__ vecs, unsigned long long *d_len) {
    const uint64_t nvec = (bytes + 15) >> 4, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
        const unsigned long long w0 = 2 * v < n ? words[2 * v] : 0, w1 = 2 * v + 1 < n ? words[2 * v + 1] : 0;
        vecs[v] = make_uint4(rev_bytes((uint32_t)w0), rev_bytes((uint32_t)(w0 >> 32)), rev_bytes((uint32_t)w1),
                             rev_bytes((uint32_t)(w1 >> 32)));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_len = bytes;
}

// ---------------------------------------------------------------------------------
// 5. Many keys (rbx_bitset_members_stream): command i is (key[i], cmds[i]) over the BitKey table of the bit streams,
// in the two tiers of the range stream (their list and summary: bitrange_device.h), and in two passes around one scan:
//   count   k_ms_count<G>: a group of G lanes per command counts an interval of at most short_max bytes and stores
//           the command's yield (the page's size: members_page with the command's skip and limit); a longer interval
//           is listed with its tile numbers (rs_list_claim), its tiles are counted by the whole grid
//           (k_ms_tile_count) and one lane per listed command turns the tile counts into the ranks of the tiles'
//           first ones and the command's yield (k_ms_long_yield);
//   scan    the yields' exclusive prefix sums, in place (k_bits_block_scan), plus the carry of the chunks before;
//   expand  k_ms_expand_short<G>: the lane that owns a vector stores its ones (a short interval is a few vectors,
//           and the group's lanes write neighbouring ranks); k_ms_expand_tiles: a workgroup per tile walks its
//           4 KiB blocks through block_expand, the coalesced pattern of the single key.
// off[i] = the index in `out` of command i's first position; a position whose index is not below cap is dropped.
// ---------------------------------------------------------------------------------
constexpr int kMsFlags = rs_flags_at(kMsFirsts), kMsLong = rs_long_at(kMsFirsts);

// the interval of a legal command on a key of the right type, from the table entry
__device__ __forceinline__ bool ms_interval(const BitKey &bk, const rbx_members_cmd &c, uint64_t *lo, uint64_t *hi) {
    bool missing;
    const uint64_t len = rs_len(bk, &missing);
    return members_interval(c.nargs, c.start, c.end, c.unit, len, lo, hi);
}

template <int G>
__global__ __launch_bounds__(256) void k_ms_count(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                  const rbx_members_cmd *__restrict__ cmds, uint32_t n, uint32_t nkeys,
                                                  uint32_t short_max, uint32_t tile_lg, unsigned long long *__restrict__ off,
                                                  uint8_t *__restrict__ status, unsigned long long *sum,
                                                  unsigned long long *__restrict__ longs) {
    constexpr uint32_t kGroups = 256 / G;
    const uint32_t gl = threadIdx.x & (G - 1);
    const uint32_t ngroups = gridDim.x * kGroups;
    const uint32_t g0 = blockIdx.x * kGroups + threadIdx.x / G;
    for (uint32_t base = 0; base < n; base += ngroups) {  // the same trip count in every lane of the grid
        const uint64_t i = (uint64_t)base + g0;
        bool store = false, walk = false;
        uint64_t lo = 0, hi = 0;
        uint8_t st = 0;
        rbx_members_cmd c = {};
        const uint4 *vecs = nullptr;
        if (i < n) {
            c = cmds[i];
            const uint32_t k = key[i];
            if (k >= nkeys || members_cmd_illegal(c.nargs, c.unit)) {
                if (gl == 0) atomicOr(sum + kMsFlags, (unsigned long long)kRsIllegal);
            } else {
                const BitKey bk = tab[k];
                store = true;
                if (bk.flags & kBitKeyWrong) {
                    st = kRsFailedStatus;
                    if (gl == 0) rs_first_min(sum, i);  // (the one "first" word: the first command on a wrong key)
                } else if (ms_interval(bk, c, &lo, &hi)) {
                    vecs = (const uint4 *)bk.words;
                    if ((hi >> 3) - (lo >> 3) + 1 > short_max) {
                        if (gl == 0) rs_list_claim(sum + kMsLong, longs, i, lo, hi, tile_lg);
                    } else {
                        walk = true;
                    }
                }
            }
        }
        uint64_t acc = 0;
        if (walk)
            for (uint64_t v = (lo >> 7) + gl, v1 = hi >> 7; v <= v1; v += G) acc += popc4(vec_wanted<false>(vecs[v], v, lo, hi));
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor((unsigned long long)acc, o, G);
        if (store && gl == 0) {
            uint64_t first, count;
            members_page(acc, c.skip, c.limit, ~0ULL, &first, &count);  // (a listed command: 0 until k_ms_long_yield)
            off[i] = count;
            if (status) status[i] = st;
        }
    }
}

__global__ __launch_bounds__(256) void k_ms_tile_count(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                       const rbx_members_cmd *__restrict__ cmds, uint32_t tile_lg,
                                                       const unsigned long long *__restrict__ longs, uint32_t nlong,
                                                       uint64_t ntiles, unsigned long long *__restrict__ tilecnt) {
    __shared__ unsigned long long s_part[4];
    const uint64_t tile_vecs = 1ULL << (tile_lg - 4);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RsTile mt = rs_tile_of(longs, nlong, t);
        const BitKey bk = tab[key[mt.i]];
        uint64_t lo, hi, n1 = 0;
        if (ms_interval(bk, cmds[mt.i], &lo, &hi)) {  // (always: listed commands have an interval)
            const uint4 *vecs = (const uint4 *)bk.words;
            const uint64_t v1 = hi >> 7, cb = (lo >> 7) + mt.own * tile_vecs, ce = min(cb + tile_vecs - 1, v1);
            for (uint64_t v = cb + threadIdx.x; v <= ce; v += 256) n1 += popc4(vec_wanted<false>(ld_nt16(vecs + v), v, lo, hi));
        }
        block_sum4(n1, s_part, [&](unsigned long long sum) { tilecnt[t] = sum; });
    }
}

// one lane per listed command: tilecnt[t] := the ones of the command before its tile t, off[i] := its yield
__global__ __launch_bounds__(256) void k_ms_long_yield(const rbx_members_cmd *__restrict__ cmds,
                                                       const unsigned long long *__restrict__ longs, uint32_t nlong,
                                                       uint64_t ntiles, unsigned long long *__restrict__ tilecnt,
                                                       unsigned long long *__restrict__ off) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nlong; j += stride) {
        const uint64_t i = rs_entry_pos(longs[j]), t0 = rs_entry_tile(longs[j]);
        const uint64_t t1 = j + 1 < nlong ? rs_entry_tile(longs[j + 1]) : ntiles;
        unsigned long long run = 0;
        for (uint64_t t = t0; t < t1; ++t) {
            const unsigned long long c = tilecnt[t];
            tilecnt[t] = run;
            run += c;
        }
        uint64_t first, count;
        members_page(run, cmds[i].skip, cmds[i].limit, ~0ULL, &first, &count);
        off[i] = count;
    }
}

// off[0 .. m] += *carry: the chunk's exclusive sums and its total become the call's
__global__ __launch_bounds__(256) void k_ms_carry(unsigned long long *__restrict__ off, uint64_t m1,
                                                  const unsigned long long *__restrict__ carry) {
    const unsigned long long c = *carry;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m1; i += stride) off[i] += c;
}

template <int G>
__global__ __launch_bounds__(256) void k_ms_expand_short(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                         const rbx_members_cmd *__restrict__ cmds, uint32_t n,
                                                         uint32_t short_max, const unsigned long long *__restrict__ off,
                                                         unsigned long long *__restrict__ out, uint64_t cap) {
    constexpr uint32_t kGroups = 256 / G;
    const uint32_t gl = threadIdx.x & (G - 1);
    const uint32_t ngroups = gridDim.x * kGroups;
    for (uint64_t i = blockIdx.x * kGroups + threadIdx.x / G; i < n; i += ngroups) {  // uniform inside a group
        const unsigned long long o = off[i], y = off[i + 1] - o;
        if (y == 0 || o >= cap) continue;  // nothing to write: an empty page, a failed command, or past the output
        const rbx_members_cmd c = cmds[i];
        const BitKey bk = tab[key[i]];
        uint64_t lo, hi;
        if (!ms_interval(bk, c, &lo, &hi) || (hi >> 3) - (lo >> 3) + 1 > short_max) continue;  // (a tile's command)
        const uint4 *vecs = (const uint4 *)bk.words;
        const uint64_t first = c.skip, end = c.skip + y, v1 = hi >> 7;  // y > 0: skip < total, and end <= total
        uint64_t run = 0;  // the ones before this step, the same in every lane of the group
        for (uint64_t vb = lo >> 7; vb <= v1 && run < end; vb += G) {
            const uint64_t v = vb + gl;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (v <= v1) x = vec_wanted<false>(vecs[v], v, lo, hi);
            const uint32_t cnt = popc4(x);
            uint32_t incl = cnt;
#pragma unroll
            for (int s = 1; s < G; s <<= 1) {
                const uint32_t z = __shfl_up(incl, s, G);
                if (gl >= (uint32_t)s) incl += z;
            }
            uint64_t r = run + incl - cnt;
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t q = w[j];
                while (q) {  // position p of the word at bit 31 - p: the leading one is the next in string order
                    const uint32_t p = (uint32_t)__builtin_clz(q);
                    q &= ~(0x80000000u >> p);
                    const uint64_t idx = o + (r - first);
                    if (r >= first && r < end && idx < cap) out[idx] = (v << 7) + 32u * j + p;
                    ++r;
                }
            }
            run += __shfl(incl, G - 1, G);
        }
    }
}

__global__ __launch_bounds__(256) void k_ms_expand_tiles(const BitKey *__restrict__ tab, const uint32_t *__restrict__ key,
                                                         const rbx_members_cmd *__restrict__ cmds, uint32_t tile_lg,
                                                         const unsigned long long *__restrict__ longs, uint32_t nlong,
                                                         uint64_t ntiles, const unsigned long long *__restrict__ tilepre,
                                                         const unsigned long long *__restrict__ off,
                                                         unsigned long long *__restrict__ out, uint64_t cap) {
    const uint64_t tile_vecs = 1ULL << (tile_lg - 4);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // every condition here is uniform in the workgroup
        const RsTile mt = rs_tile_of(longs, nlong, t);
        const unsigned long long o = off[mt.i], y = off[mt.i + 1] - o;
        if (y == 0 || o >= cap) continue;
        const rbx_members_cmd c = cmds[mt.i];
        const BitKey bk = tab[key[mt.i]];
        uint64_t lo, hi;
        if (!ms_interval(bk, c, &lo, &hi)) continue;  // (never)
        const uint64_t first = c.skip, end = c.skip + y;
        uint64_t rs = tilepre[t];  // the rank of the tile's first one
        if (rs >= end) continue;
        const bool last = mt.own + 1 >= rs_tiles(lo, hi, tile_lg);
        if (!last && tilepre[t + 1] <= first) continue;  // the whole tile lies before the page
        const uint4 *vecs = (const uint4 *)bk.words;
        const uint64_t v1 = hi >> 7, cb = (lo >> 7) + mt.own * tile_vecs, ce = min(cb + tile_vecs - 1, v1);
        for (uint64_t vb = cb; vb <= ce && rs < end; vb += 256) {
            const uint64_t v = vb + threadIdx.x;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (v <= ce) x = vec_wanted<false>(ld_nt16(vecs + v), v, lo, hi);
            rs += block_expand(x, vb, rs, first, end, out, o, cap);
        }
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
void launch_members_count(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds, uint32_t n,
                          uint32_t nkeys, uint32_t short_max, uint32_t tile_bytes, unsigned long long *d_off,
                          uint8_t *d_status, unsigned long long *d_sum, unsigned long long *d_long, hipStream_t st) {
    const uint32_t lg = log2_of(tile_bytes);
#define MS_COUNT(G)                                                                                                        \
    hipLaunchKernelGGL(k_ms_count<G>, dim3(grid_for((uint64_t)n * G, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n, nkeys, short_max, lg, \
                       d_off, d_status, d_sum, d_long)
    RBX_FOR_LANES(lanes, MS_COUNT);
#undef MS_COUNT
}

void launch_members_tiles_count(const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds, uint32_t tile_bytes,
                                const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                                unsigned long long *d_tiles, unsigned long long *d_off, hipStream_t st) {
    hipLaunchKernelGGL(k_ms_tile_count, dim3((unsigned)std::min<uint64_t>(ntiles, kMaxGrid)), dim3(256), 0, st, d_tab, d_key,
                       d_cmds, log2_of(tile_bytes), d_long, nlong, ntiles, d_tiles);
    hipLaunchKernelGGL(k_ms_long_yield, dim3(grid_for(nlong, kMaxGrid)), dim3(256), 0, st, d_cmds, d_long, nlong, ntiles,
                       d_tiles, d_off);
}

void launch_members_carry(unsigned long long *d_off, uint64_t m1, const unsigned long long *d_carry, hipStream_t st) {
    hipLaunchKernelGGL(k_ms_carry, dim3(grid_for(m1, kMaxGrid)), dim3(256), 0, st, d_off, m1, d_carry);
}

void launch_members_expand_short(int lanes, const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds,
                                 uint32_t n, uint32_t short_max, const unsigned long long *d_off, uint64_t *d_out,
                                 uint64_t cap, hipStream_t st) {
#define MS_EXPAND(G)                                                                                                   \
    hipLaunchKernelGGL(k_ms_expand_short<G>, dim3(grid_for((uint64_t)n * G, kMaxGrid)), dim3(256), 0, st, d_tab, d_key, d_cmds, n, short_max, \
                       d_off, (unsigned long long *)d_out, cap)
    RBX_FOR_LANES(lanes, MS_EXPAND);
#undef MS_EXPAND
}

void launch_members_expand_tiles(const BitKey *d_tab, const uint32_t *d_key, const rbx_members_cmd *d_cmds,
                                 uint32_t tile_bytes, const unsigned long long *d_long, uint32_t nlong, uint64_t ntiles,
                                 const unsigned long long *d_tiles, const unsigned long long *d_off, uint64_t *d_out,
                                 uint64_t cap, hipStream_t st) {
    hipLaunchKernelGGL(k_ms_expand_tiles, dim3((unsigned)std::min<uint64_t>(ntiles, kMaxGrid)), dim3(256), 0, st, d_tab, d_key,
                       d_cmds, log2_of(tile_bytes), d_long, nlong, ntiles, d_tiles, d_off, (unsigned long long *)d_out, cap);
}

void launch_members_head(const uint32_t *words, uint64_t len, uint64_t lo, uint64_t hi, uint64_t skip, uint64_t cap,
                         const unsigned long long *d_dir, unsigned long long *d_state, unsigned long long *d_counts,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_members_head, dim3(1), dim3(64), 0, st, (const uint4 *)words, len, lo, hi, skip, cap, d_dir, d_state,
                       d_counts);
}

void launch_members_expand(const uint32_t *words, uint64_t len, uint64_t lo, uint64_t hi, const unsigned long long *d_dir,
                           const unsigned long long *d_state, uint64_t *d_out, hipStream_t st) {
    const uint64_t blocks = (hi >> kBlockLog2) - (lo >> kBlockLog2) + 1;
    hipLaunchKernelGGL(k_members_expand, dim3((unsigned)std::min<uint64_t>(blocks, kMembersMaxGrid)), dim3(256), 0, st,
                       (const uint4 *)words, (len + 15) >> 4, lo, hi, d_dir, d_state, (unsigned long long *)d_out);
}

void launch_words_last(const uint32_t *words, uint64_t cap_bytes, const unsigned long long *d_len,
                       unsigned long long *d_nwords, hipStream_t st) {
    hipLaunchKernelGGL(k_words_last, dim3(grid_for(cap_bytes >> 4, kMaxGrid)), dim3(256), 0, st, (const uint4 *)words, d_len,
                       cap_bytes, d_nwords);
}

void launch_words_export(const uint32_t *words, uint64_t cap_bytes, const unsigned long long *d_nwords, uint64_t cap_words,
                         uint64_t *d_out, hipStream_t st) {
    const uint64_t m = std::min(cap_words, cap_bytes >> 3);  // what the grid is sized for: the kernel stops at *d_nwords
    if (m == 0) return;
    hipLaunchKernelGGL(k_words_export, dim3(grid_for((m + 1) >> 1, kMaxGrid)), dim3(256), 0, st, (const uint4 *)words,
                       d_nwords, cap_words, (unsigned long long *)d_out);
}

void launch_words_highest(const uint64_t *d_words, uint64_t n, unsigned long long *d_highest1, hipStream_t st) {
    hipLaunchKernelGGL(k_words_highest, dim3(grid_for(n, kMaxGrid)), dim3(256), 0, st, (const unsigned long long *)d_words, n,
                       d_highest1);
}

void launch_words_import(const uint64_t *d_words, uint64_t n, uint64_t bytes, uint32_t *words, unsigned long long *d_len,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_words_import, dim3(grid_for((bytes + 15) >> 4, kMaxGrid)), dim3(256), 0, st,
                       (const unsigned long long *)d_words, n, bytes, (uint4 *)words, d_len);
}

}  // namespace rbx
