// evrep_wave_search.h -- the 64-ary search a wavefront makes through an ascending int64 array in global memory, shared by
// the windows of a device-resident recording (evrep_windows.hip) and the seek of a decoded DAT file (evrep_decode.hip).
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kWinThreads = 256;                                            // four waves: four queries per workgroup

__device__ inline int64_t wave_uniform(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The first index i in [0, n] with a[i] > q (n if there is none) of the ascending a[0, n): np.searchsorted(a, q, "right").
// Called by all 64 lanes of a wave with the same arguments; every lane returns the result.  Invariant: a[i] <= q below lo,
// a[hi] > q or hi == n.  A round cuts [lo, hi) into 64 pieces of `step` entries; lane l probes the LAST entry of piece l
// (pieces past the end hold nothing and vote "not greater"); the first lane that sees a greater entry names the piece that
// holds the answer, and its probe becomes the new hi.  No lane voting means the last entry, hi - 1, is <= q: the answer is hi.
// With 64 entries or fewer the pieces are single entries: the round reads them side by side and ends the search.
__device__ inline int64_t wave_upper_bound(const int64_t *__restrict__ a, int64_t n, int64_t q) {
    const int lane = threadIdx.x & (kWave - 1);
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t step = (hi - lo + kWave - 1) / kWave;
        const int64_t first = lo + (int64_t)lane * step;            // the lane's piece: [first, min(first + step, hi))
        bool greater = false;
        if (first < hi) {
            const int64_t last = (first + step < hi ? first + step : hi) - 1;
            greater = a[last] > q;
        }
        const unsigned long long votes = __ballot(greater);
        if (votes == 0) return hi;
        const int64_t k = __builtin_amdgcn_readfirstlane(__ffsll((long long)votes) - 1);
        const int64_t nlo = lo + k * step;
        hi = (nlo + step < hi ? nlo + step : hi) - 1;
        lo = nlo;
    }
    return lo;
}

}  // namespace evrep
