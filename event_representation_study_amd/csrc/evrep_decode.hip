// evrep_decode.hip -- raw event files decoded on the device into the structure-of-arrays columns of a recording (x u16,
// y u16, t i64, p i8: ev-licious io/utils/events.py:7-8): Prophesee DAT records (io/utils/prophesee_utils.py:8-61: a uint32
// timestamp and a uint32 word, x in bits 0-13, y in bits 14-27, p in bit 28; 8 bytes for event types 0 and 12, 28 for type 40)
// and the 5-byte records of N-Caltech / N-MNIST (io/bin_event_handle.py:37-51), and EventBaseReader.seek_time
// (prophesee_utils.py:367-418) on the decoded t column.
//
// A call decodes ONE CHUNK of a file and ACCUMULATES into a 64-byte evrep_decode_state that stays on the device: the chunks
// of a file follow one another on a stream with no host wait between them.  The columns are written at the state's n_out; a
// descent across a chunk joint is seen because the state holds the previous chunk's last timestamp.  Kernels of one call:
//   STRICT    k_decode_pass<F, kPassStrict> (decode + checks)                                    -> k_decode_finish
//   DROP_OOB  k_decode_pass<F, kPassCount> (kept records per slice + checks) -> k_decode_scan (one workgroup)
//             -> k_decode_pass<F, kPassWrite> (compaction; the strict body where nothing is dropped) -> k_decode_finish
// Only k_decode_finish (one thread, after the passes) writes the fields the passes read (n_in, n_out, t_last), so no
// workgroup of a pass can see a half-updated state.
//
// The strict body.  A lane owns a GROUP of 16 consecutive records whose first OUTPUT index is a multiple of 16: it stores
// whole 16-byte pieces of every column (x and y two each, t eight, p one) and loads whole pieces of the payload -- eight for
// DAT (sixteen 8-byte loads where the chunk starts at an odd output index: the group is then only 8-byte aligned in the
// payload), five or six for the 80 bytes of 16 BIN records, which lie at the same offset inside their 16-byte pieces for
// every group of a call (80 is a multiple of 16), so one byte shift, uniform over the call, lines them up in registers.
// The fewer than 16 records in front of the first and behind the last whole group, and every record of a DAT stride other
// than 8, take the one-record path with narrow loads and stores.
//
// Checks.  Every lane keeps the count and the first file index of its out-of-frame records (x >= W or y >= H) and of its
// descents (t smaller than the predecessor's, over the RAW record order in both modes); a wave reduces them once, at the end
// of the kernel, and one lane adds them to the state: integer atomics, atomicMin for the first indices (-1, "none", is the
// largest unsigned value).
#pragma once
#include "evrep_common.h"
#include "evrep_wave_search.h"

namespace evrep {

constexpr int kDecThreads = 256;
constexpr int kDecGrid = 1024;                        // workgroups of a pass = slices of the DROP_OOB compaction
constexpr int kDecGroup = 16;                         // records of a lane's group
constexpr int kFmtDat = 0, kFmtBin5 = 1;
constexpr int kPassStrict = 0, kPassCount = 1, kPassWrite = 2;
constexpr int64_t kDecOverrun = (int64_t)EVREP_DECODE_N_IN_OVERRUN;

// scratch of a DROP_OOB call: this header, then kDecGrid uint32 kept counts and kDecGrid uint32 exclusive offsets
struct DecodeScratch {
    int64_t total;          // kept records of the call
    int64_t declined;       // 1: the call writes nothing (capacity, or an earlier overrun)
    int64_t pad[30];
};
static_assert(sizeof(DecodeScratch) == 256, "the counts start on a 256-byte boundary");

struct DecodeArgs {
    const uint8_t *raw;     // 16-byte aligned payload, readable up to the next multiple of 16 bytes behind the last record
    int64_t n;              // records of this call
    int64_t first_index;    // the file index of record 0
    int32_t stride;         // DAT: bytes per record
    int32_t H, W;
    uint16_t *x, *y;
    int64_t *t;
    int8_t *p;
    int64_t capacity;
    evrep_decode_state *state;
};

struct DecodeChecks {
    uint32_t oob = 0, desc = 0;
    int64_t oob_first = INT64_MAX, desc_first = INT64_MAX;
    __device__ inline void see(bool out_of_frame, bool descent, int64_t index) {
        if (out_of_frame) { ++oob; oob_first = index < oob_first ? index : oob_first; }
        if (descent) { ++desc; desc_first = index < desc_first ? index : desc_first; }
    }
};

struct DecodedRecord { uint32_t x, y, t; bool pos; };

// one record with narrow loads (the edges of a call, general strides, the compaction)
template <int F>
__device__ inline DecodedRecord fetch_record(const uint8_t *__restrict__ raw, int32_t stride, int64_t i) {
    DecodedRecord r;
    if (F == kFmtDat) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(raw + i * stride);   // two 4-byte loads: right for every stride
        const uint32_t v = w[1];
        r.t = w[0]; r.x = v & 0x3FFFu; r.y = (v >> 14) & 0x3FFFu; r.pos = (v >> 28) & 1u;
    } else {
        const uint8_t *b = raw + i * 5;
        r.x = b[0]; r.y = b[1]; r.pos = (b[2] & 128u) != 0;
        r.t = ((uint32_t)(b[2] & 127u) << 16) | ((uint32_t)b[3] << 8) | b[4];
    }
    return r;
}

template <int F>
__device__ inline uint32_t fetch_t(const uint8_t *__restrict__ raw, int32_t stride, int64_t i) {
    if (F == kFmtDat) return *reinterpret_cast<const uint32_t *>(raw + i * stride);
    const uint8_t *b = raw + i * 5;
    return ((uint32_t)(b[2] & 127u) << 16) | ((uint32_t)b[3] << 8) | b[4];
}

// the timestamp in front of record i of the call: the previous chunk's last one for i == 0 (-1 at the start of a file)
template <int F>
__device__ inline int64_t predecessor_t(const DecodeArgs &a, int64_t i, int64_t t_last) {
    return i == 0 ? t_last : (int64_t)fetch_t<F>(a.raw, a.stride, i - 1);
}

template <int F, bool CHECK>
__device__ inline void decode_one(const DecodeArgs &a, int64_t i, int64_t out0, int64_t t_last, DecodeChecks &c) {
    const DecodedRecord r = fetch_record<F>(a.raw, a.stride, i);
    if (CHECK) c.see(r.x >= (uint32_t)a.W || r.y >= (uint32_t)a.H, (int64_t)r.t < predecessor_t<F>(a, i, t_last), a.first_index + i);
    const int64_t o = out0 + i;
    a.x[o] = (uint16_t)r.x; a.y[o] = (uint16_t)r.y; a.t[o] = (int64_t)r.t; a.p[o] = r.pos ? 1 : -1;
}

// the 16 decoded records of a group -> 13 stores of 16 bytes at output index o (a multiple of 16)
template <bool CHECK>
__device__ inline void emit_group(const DecodeArgs &a, const uint32_t (&xs)[kDecGroup], const uint32_t (&ys)[kDecGroup],
                                  const uint32_t (&ts)[kDecGroup], const uint32_t (&ps)[kDecGroup], int64_t o, int64_t index0,
                                  int64_t prev, DecodeChecks &c) {
    if (CHECK) {
#pragma unroll
        for (int k = 0; k < kDecGroup; ++k) {
            c.see(xs[k] >= (uint32_t)a.W || ys[k] >= (uint32_t)a.H, (int64_t)ts[k] < prev, index0 + k);
            prev = (int64_t)ts[k];
        }
    }
    uint32_t px[8], py[8], pp[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        px[k] = xs[2 * k] | (xs[2 * k + 1] << 16);
        py[k] = ys[2 * k] | (ys[2 * k + 1] << 16);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pp[k] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) pp[k] |= (ps[4 * k + j] ? 0x01u : 0xFFu) << (8 * j);
    }
    gstore16(a.x + o, make_uint4(px[0], px[1], px[2], px[3]));
    gstore16(a.x + o + 8, make_uint4(px[4], px[5], px[6], px[7]));
    gstore16(a.y + o, make_uint4(py[0], py[1], py[2], py[3]));
    gstore16(a.y + o + 8, make_uint4(py[4], py[5], py[6], py[7]));
#pragma unroll
    for (int k = 0; k < 8; ++k) gstore16(a.t + o + 2 * k, make_uint4(ts[2 * k], 0u, ts[2 * k + 1], 0u));   // uint32 zero-extended
    gstore16(a.p + o, make_uint4(pp[0], pp[1], pp[2], pp[3]));
}

// DAT, 8-byte records: the group of records [i0, i0 + 16), 16-byte aligned in the payload where `aligned`
template <bool CHECK>
__device__ inline void dat_group(const DecodeArgs &a, int64_t i0, bool aligned, int64_t o, int64_t t_last, DecodeChecks &c) {
    const uint8_t *d = a.raw + i0 * 8;
    uint32_t xs[kDecGroup], ys[kDecGroup], ts[kDecGroup], ps[kDecGroup], ws[kDecGroup];
    if (aligned) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 v = gload16(d + 16 * k);
            ts[2 * k] = v.x; ws[2 * k] = v.y; ts[2 * k + 1] = v.z; ws[2 * k + 1] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kDecGroup; ++k) {
            const uint2 v = *reinterpret_cast<const uint2 *>(d + 8 * k);
            ts[k] = v.x; ws[k] = v.y;
        }
    }
#pragma unroll
    for (int k = 0; k < kDecGroup; ++k) {
        xs[k] = ws[k] & 0x3FFFu; ys[k] = (ws[k] >> 14) & 0x3FFFu; ps[k] = (ws[k] >> 28) & 1u;    // bits 29-31 are ignored
    }
    emit_group<CHECK>(a, xs, ys, ts, ps, o, a.first_index + i0, CHECK ? predecessor_t<kFmtDat>(a, i0, t_last) : 0, c);
}

// BIN: the 80 bytes of the group start `shift` bytes (0..15, the same for every group of the call) into the 16-byte piece at
// `piece`; DW = shift / 4 picks the dwords, the byte alignment does the rest.  The sixth piece is read only where the
// group reaches into it (shift > 0): behind the last group it may not exist otherwise.
template <int DW>
__device__ inline void bin5_line_up(const uint32_t (&w)[24], uint32_t bytes, uint32_t (&v)[20]) {
#pragma unroll
    for (int j = 0; j < 20; ++j) v[j] = __builtin_amdgcn_alignbyte(w[j + DW + 1], w[j + DW], bytes);
}
__device__ inline uint32_t byte_of(const uint32_t (&v)[20], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xFFu; }

template <bool CHECK>
__device__ inline void bin5_group(const DecodeArgs &a, int64_t i0, uint32_t shift, int64_t o, int64_t t_last, DecodeChecks &c) {
    const uint8_t *piece = a.raw + (i0 * 5 - shift);
    uint32_t w[24], v[20];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint4 q = gload16(piece + 16 * k);
        w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
    }
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (shift) q = gload16(piece + 80);
    w[20] = q.x; w[21] = q.y; w[22] = q.z; w[23] = q.w;
    switch (shift >> 2) {                                            // (uniform over the call)
        case 0: bin5_line_up<0>(w, shift & 3u, v); break;
        case 1: bin5_line_up<1>(w, shift & 3u, v); break;
        case 2: bin5_line_up<2>(w, shift & 3u, v); break;
        default: bin5_line_up<3>(w, shift & 3u, v); break;
    }
    uint32_t xs[kDecGroup], ys[kDecGroup], ts[kDecGroup], ps[kDecGroup];
#pragma unroll
    for (int k = 0; k < kDecGroup; ++k) {
        const uint32_t b2 = byte_of(v, 5 * k + 2);
        xs[k] = byte_of(v, 5 * k); ys[k] = byte_of(v, 5 * k + 1); ps[k] = b2 >> 7;
        ts[k] = ((b2 & 127u) << 16) | (byte_of(v, 5 * k + 3) << 8) | byte_of(v, 5 * k + 4);
    }
    emit_group<CHECK>(a, xs, ys, ts, ps, o, a.first_index + i0, CHECK ? predecessor_t<kFmtBin5>(a, i0, t_last) : 0, c);
}

// every record of the call written at out0 + its index, the grid striding over the groups
template <int F, bool CHECK>
__device__ inline void strict_body(const DecodeArgs &a, int64_t out0, int64_t t_last, DecodeChecks &c) {
    const int64_t tid = (int64_t)blockIdx.x * kDecThreads + threadIdx.x, nthreads = (int64_t)gridDim.x * kDecThreads;
    if (F == kFmtDat && a.stride != 8) {
        for (int64_t i = tid; i < a.n; i += nthreads) decode_one<F, CHECK>(a, i, out0, t_last, c);
        return;
    }
    int64_t head = (kDecGroup - (out0 & (kDecGroup - 1))) & (kDecGroup - 1);       // records in front of the first whole group
    head = head < a.n ? head : a.n;
    const int64_t groups = (a.n - head) / kDecGroup, tail0 = head + groups * kDecGroup;
    if (tid < head) decode_one<F, CHECK>(a, tid, out0, t_last, c);
    if (tail0 + tid < a.n) decode_one<F, CHECK>(a, tail0 + tid, out0, t_last, c);
    const bool aligned = (head & 1) == 0;                            // DAT: groups start on a 16-byte boundary of the payload
    const uint32_t shift = (uint32_t)((head * 5) & 15);              // BIN: 80 g + 5 head, modulo 16
    for (int64_t g = tid; g < groups; g += nthreads) {
        const int64_t i0 = head + g * kDecGroup;
        if (F == kFmtDat) dat_group<CHECK>(a, i0, aligned, out0 + i0, t_last, c);
        else bin5_group<CHECK>(a, i0, shift, out0 + i0, t_last, c);
    }
}

__device__ inline void wave_add_checks(const DecodeChecks &c, evrep_decode_state *state) {
    uint32_t oob = c.oob, desc = c.desc;
    int64_t of = c.oob_first, df = c.desc_first;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        oob += __shfl_xor(oob, d, kWave);
        desc += __shfl_xor(desc, d, kWave);
        const int64_t o2 = __shfl_xor((long long)of, d, kWave), d2 = __shfl_xor((long long)df, d, kWave);
        of = o2 < of ? o2 : of;
        df = d2 < df ? d2 : df;
    }
    if ((threadIdx.x & (kWave - 1)) != 0) return;
    if (oob) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&state->oob_count), (unsigned long long)oob);
        atomicMin(reinterpret_cast<unsigned long long *>(&state->oob_first), (unsigned long long)of);
    }
    if (desc) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&state->desc_count), (unsigned long long)desc);
        atomicMin(reinterpret_cast<unsigned long long *>(&state->desc_first), (unsigned long long)df);
    }
}

// the records of slice s of the compaction: [s * per, min(n, (s + 1) * per)), per a multiple of the workgroup
__device__ inline int64_t slice_records(int64_t n) {
    const int64_t per = (n + kDecGrid - 1) / kDecGrid;
    return (per + kDecThreads - 1) / kDecThreads * kDecThreads;
}

__global__ void k_decode_init(evrep_decode_state *state) {
    state->n_in = 0; state->n_out = 0; state->oob_count = 0; state->oob_first = -1;
    state->desc_count = 0; state->desc_first = -1; state->t_first = -1; state->t_last = -1;
}

// grid kDecGrid, 256 threads
template <int F, int PASS>
__global__ __launch_bounds__(kDecThreads) void k_decode_pass(DecodeArgs a, DecodeScratch *__restrict__ scratch) {
    __shared__ uint32_t tmp[kDecThreads / kWave];
    const int64_t n_in = a.state->n_in, out0 = a.state->n_out, t_last = a.state->t_last;
    DecodeChecks c;
    if (PASS == kPassStrict) {
        // the checks run even where the call declines to write: the counts of a file do not depend on the capacity
        if ((n_in & kDecOverrun) || out0 + a.n > a.capacity) {
            for (int64_t i = (int64_t)blockIdx.x * kDecThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kDecThreads) {
                const DecodedRecord r = fetch_record<F>(a.raw, a.stride, i);
                c.see(r.x >= (uint32_t)a.W || r.y >= (uint32_t)a.H, (int64_t)r.t < predecessor_t<F>(a, i, t_last), a.first_index + i);
            }
        } else {
            strict_body<F, true>(a, out0, t_last, c);
        }
        wave_add_checks(c, a.state);
        return;
    }
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch + 1), *off = cnt + kDecGrid;
    if (PASS == kPassWrite) {
        if (scratch->declined) return;
        if (scratch->total == a.n) {                                 // nothing is dropped: the strict columns, bit for bit
            strict_body<F, false>(a, out0, t_last, c);
            return;
        }
    }
    const int64_t per = slice_records(a.n), begin = (int64_t)blockIdx.x * per;
    const int64_t end = begin + per < a.n ? begin + per : a.n;
    int64_t kept = 0;
    for (int64_t i0 = begin; i0 < end; i0 += kDecThreads) {
        const int64_t i = i0 + threadIdx.x;
        DecodedRecord r = {};
        bool keep = false;
        if (i < end) {
            r = fetch_record<F>(a.raw, a.stride, i);
            keep = r.x < (uint32_t)a.W && r.y < (uint32_t)a.H;
            if (PASS == kPassCount) c.see(!keep, (int64_t)r.t < predecessor_t<F>(a, i, t_last), a.first_index + i);
        }
        uint32_t total;
        const uint32_t rank = block_exclusive_scan<kDecThreads / kWave>(keep ? 1u : 0u, tmp, &total);
        if (PASS == kPassWrite && keep) {
            const int64_t o = out0 + off[blockIdx.x] + kept + rank;
            a.x[o] = (uint16_t)r.x; a.y[o] = (uint16_t)r.y; a.t[o] = (int64_t)r.t; a.p[o] = r.pos ? 1 : -1;
        }
        kept += total;
    }
    if (PASS == kPassCount) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = (uint32_t)kept;
        wave_add_checks(c, a.state);
    }
}

// one workgroup of kDecGrid threads: the slices' exclusive offsets, the total, and whether the call may write
__global__ __launch_bounds__(kDecGrid) void k_decode_scan(DecodeArgs a, DecodeScratch *__restrict__ scratch) {
    __shared__ uint32_t tmp[kDecGrid / kWave];
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch + 1), *off = cnt + kDecGrid;
    uint32_t total;
    off[threadIdx.x] = block_exclusive_scan<kDecGrid / kWave>(cnt[threadIdx.x], tmp, &total);
    if (threadIdx.x == 0) {
        scratch->total = total;
        scratch->declined = ((a.state->n_in & kDecOverrun) || a.state->n_out + (int64_t)total > a.capacity) ? 1 : 0;
    }
}

// one thread, behind the passes of a call: the fields the next call reads
template <int F>
__global__ void k_decode_finish(DecodeArgs a, const DecodeScratch *__restrict__ scratch) {
    evrep_decode_state *s = a.state;
    const int64_t added = scratch ? scratch->total : a.n;
    const bool declined = (s->n_in & kDecOverrun) || s->n_out + added > a.capacity;
    if ((s->n_in & ~kDecOverrun) == 0) s->t_first = (int64_t)fetch_t<F>(a.raw, a.stride, 0);
    s->t_last = (int64_t)fetch_t<F>(a.raw, a.stride, a.n - 1);
    s->n_in = (s->n_in + a.n) | (declined ? kDecOverrun : 0);
    if (!declined) s->n_out += added;
}

// EventBaseReader.seek_time(q, term) on the ascending t[0, n): grid ceil(nq / 4), 256 threads, wave w answers query w.
// The bisection probes t[middle] while more than `term` records remain -- a chain of wave-uniform loads, at most
// log2(n / term) -- and a probe EQUAL to q ends the search at middle + 1: the reader has consumed the probed record, which
// need not be the first with that timestamp.  What remains is searched for the first t >= q, i.e. the first t > q - 1.
__global__ __launch_bounds__(kWinThreads) void k_dat_seek_time(const int64_t *__restrict__ t, int64_t n,
                                                               const int64_t *__restrict__ queries, int64_t nq, int64_t term,
                                                               int64_t *__restrict__ out_idx) {
    const int64_t w = ((int64_t)blockIdx.x * kWinThreads + threadIdx.x) / kWave;
    if (w >= nq) return;                                             // (wave-uniform)
    const int64_t q = wave_uniform(queries[w]);
    int64_t res = -1;
    if (n == 0 || q <= 0) res = 0;
    else if (q > wave_uniform(t[n - 1])) res = n;
    int64_t low = 0, high = n;
    while (res < 0 && high - low > term) {
        const int64_t middle = (low + high) / 2;
        const int64_t m = wave_uniform(t[middle]);
        if (m > q) high = middle;
        else if (m < q) low = middle + 1;
        else res = middle + 1;
    }
    if (res < 0) res = low + wave_upper_bound(t + low, high - low, q - 1);
    if ((threadIdx.x & (kWave - 1)) == 0) out_idx[w] = res;
}

}  // namespace evrep
