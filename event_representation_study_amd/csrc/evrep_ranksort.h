// evrep_ranksort.h -- the workgroup pair sort behind the dense ranks of evrep_dist.hip (k_dense_rank) and evrep_sort.hip
// (k_sort_image): one workgroup of sixteen waves sorts the n (key, index) pairs of its segment, stably, by a 32-bit key.
//
// A stable LSD radix sort through global scratch, four passes of eight bits: per pass a digit histogram (wave_match: one LDS
// atomic per wave and distinct digit), then chunks of 4 096 pairs in order -- every wave ranks its 256 pairs against its own row
// of per-digit counters, the rows are scanned over the sixteen waves on top of the running digit bases, and the pairs are
// scattered.  The first pass takes its keys from the caller's functor (index = position), the last one lands in the second pair
// of buffers.
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kDistThreads = 1024;                    // one workgroup of sixteen waves per segment
constexpr int kDistWaves = kDistThreads / 64;
constexpr int kRankBits = 8, kRankRadix = 1 << kRankBits, kRankPasses = 32 / kRankBits;
constexpr int kRankItems = 4;                         // pairs per lane and chunk
constexpr int kRankWaveSpan = 64 * kRankItems;        // consecutive pairs one wave owns in a chunk
constexpr int kRankChunk = kDistThreads * kRankItems;
static_assert(kRankRadix <= kDistThreads && kRankPasses % 2 == 0, "the last pass lands in the second pair of buffers");

// float bits -> unsigned key of the same order; -0.0 is +0.0
__device__ inline uint32_t rank_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

__host__ __device__ inline size_t rank_array_bytes(int64_t total) { return ((size_t)total * sizeof(uint32_t) + 255) & ~(size_t)255; }

struct RankSortLds {
    uint32_t hist[kRankRadix];                 // a pass's digit histogram, then the running digit bases
    uint32_t wave_cnt[kDistWaves][kRankRadix];
    uint32_t scan_tmp[kDistWaves];
};

// key_at(i) -> the uint32 key of pair i in [0, n) (called twice per pair, in the first pass only).  ka / ia / kb / ib: the
// segment's own n-entry slices of the four scratch arrays.  Every thread of the workgroup calls it with the same arguments; on
// return the sorted keys are in kb, the positions they came from in ib, visible to the whole workgroup.
template <class KeyAt>
__device__ inline void rank_pair_sort(KeyAt key_at, int64_t n, uint32_t *ka, uint32_t *ia, uint32_t *kb, uint32_t *ib, RankSortLds &s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int pass = 0; pass < kRankPasses; ++pass) {
        const int shift = pass * kRankBits;
        const bool to_b = (pass & 1) != 0;                // a, b, a, b: pass 0 reads the caller's keys, the last pass lands in b
        const uint32_t *ksrc = to_b ? ka : kb, *isrc = to_b ? ia : ib;
        uint32_t *kdst = to_b ? kb : ka, *idst = to_b ? ib : ia;
        if (tid < kRankRadix) s.hist[tid] = 0;
        __syncthreads();
        for (int64_t i0 = 0; i0 < n; i0 += kDistThreads) {
            const int64_t i = i0 + tid;
            const bool valid = i < n;
            const uint32_t k = valid ? (pass == 0 ? key_at(i) : ksrc[i]) : 0u;
            const uint32_t d = (k >> shift) & (uint32_t)(kRankRadix - 1);
            uint32_t r;
            bool last;
            wave_match(d, kRankBits, valid, lane, r, last);
            if (valid && last) atomicAdd(&s.hist[d], r + 1u);
        }
        __syncthreads();
        uint32_t tot;
        const uint32_t hv = tid < kRankRadix ? s.hist[tid] : 0u;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(hv, s.scan_tmp, &tot);
        if (tid < kRankRadix) s.hist[tid] = ex;           // (block_exclusive_scan ends in a barrier: every hv is read)
        __syncthreads();
        for (int64_t c0 = 0; c0 < n; c0 += kRankChunk) {
            for (int j = lane; j < kRankRadix; j += 64) s.wave_cnt[wave][j] = 0;     // this wave's row: nobody else reads it now
            uint32_t k[kRankItems], ix[kRankItems], off[kRankItems];
#pragma unroll
            for (int it = 0; it < kRankItems; ++it) {
                const int64_t i = c0 + (int64_t)wave * kRankWaveSpan + it * 64 + lane;
                const bool valid = i < n;
                k[it] = valid ? (pass == 0 ? key_at(i) : ksrc[i]) : 0u;
                ix[it] = valid ? (pass == 0 ? (uint32_t)i : isrc[i]) : 0u;
                const uint32_t d = (k[it] >> shift) & (uint32_t)(kRankRadix - 1);
                uint32_t r;
                bool last;
                wave_match(d, kRankBits, valid, lane, r, last);
                __builtin_amdgcn_wave_barrier();
                const uint32_t before = valid ? s.wave_cnt[wave][d] : 0u;
                off[it] = before + r;
                __builtin_amdgcn_wave_barrier();
                if (valid && last) s.wave_cnt[wave][d] = before + r + 1u;
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
            if (tid < kRankRadix) {                       // the rows become each wave's first destination per digit
                uint32_t run = s.hist[tid];
#pragma unroll
                for (int w = 0; w < kDistWaves; ++w) {
                    const uint32_t t = s.wave_cnt[w][tid];
                    s.wave_cnt[w][tid] = run;
                    run += t;
                }
                s.hist[tid] = run;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < kRankItems; ++it) {
                const int64_t i = c0 + (int64_t)wave * kRankWaveSpan + it * 64 + lane;
                if (i < n) {
                    const uint32_t d = (k[it] >> shift) & (uint32_t)(kRankRadix - 1);
                    const uint32_t dst = s.wave_cnt[wave][d] + off[it];     // < n: the digit bases partition [0, n)
                    kdst[dst] = k[it];
                    idst[dst] = ix[it];
                }
            }
        }
        __syncthreads();                                  // the pairs are in place for every wave of this workgroup
    }
}

}  // namespace evrep
