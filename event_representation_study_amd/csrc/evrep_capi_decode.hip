// evrep_capi_decode.hip -- the extern "C" surface, part 14: raw event files decoded on the device (evrep_decode.hip):
// argument checks and launches.  No plan, no workspace: the calls work on the caller's arrays, state and scratch.
#include "evrep_capi_shared.h"
#include "evrep_decode.hip"

using namespace evrep;
using evrep_host::hip_check;


template <int F>
static int decode_call(const void *raw, int64_t n, int32_t stride, int64_t first_index, int32_t H, int32_t W, uint32_t flags,
                       uint16_t *x, uint16_t *y, int64_t *t, int8_t *p, int64_t capacity, evrep_decode_state *state,
                       void *scratch_, void *stream_) {
    if (n < 0 || n > EVREP_DECODE_MAX_N || first_index < 0 || capacity < 0 || H < 1 || W < 1) return EVREP_EINVAL;
    if (flags != EVREP_DECODE_STRICT && flags != EVREP_DECODE_DROP_OOB) return EVREP_EINVAL;
    if (stride < 8 || (stride & 3)) return EVREP_EINVAL;
    if (bad_ptr(state, 8) || misaligned(raw, 16) || misaligned(scratch_, 256)) return EVREP_EINVAL;
    if (misaligned(x, 16) || misaligned(y, 16) || misaligned(t, 16) || misaligned(p, 16)) return EVREP_EINVAL;
    if (n > 0 && (!raw || !x || !y || !t || !p || (flags == EVREP_DECODE_DROP_OOB && !scratch_))) return EVREP_EINVAL;
    if (n == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    const DecodeArgs a = {static_cast<const uint8_t *>(raw), n, first_index, stride, H, W, x, y, t, p, capacity, state};
    if (flags == EVREP_DECODE_STRICT) {
        k_decode_pass<F, kPassStrict><<<kDecGrid, kDecThreads, 0, stream>>>(a, nullptr);
        LAUNCH_CHECK("k_decode_pass(strict)");
        k_decode_finish<F><<<1, 1, 0, stream>>>(a, nullptr);
        LAUNCH_CHECK("k_decode_finish");
        return EVREP_OK;
    }
    DecodeScratch *scratch = static_cast<DecodeScratch *>(scratch_);
    k_decode_pass<F, kPassCount><<<kDecGrid, kDecThreads, 0, stream>>>(a, scratch);
    LAUNCH_CHECK("k_decode_pass(count)");
    k_decode_scan<<<1, kDecGrid, 0, stream>>>(a, scratch);
    LAUNCH_CHECK("k_decode_scan");
    k_decode_pass<F, kPassWrite><<<kDecGrid, kDecThreads, 0, stream>>>(a, scratch);
    LAUNCH_CHECK("k_decode_pass(write)");
    k_decode_finish<F><<<1, 1, 0, stream>>>(a, scratch);
    LAUNCH_CHECK("k_decode_finish");
    return EVREP_OK;
}

extern "C" {

size_t evrep_decode_scratch_bytes(int64_t n) {
    (void)n;                                                        // one count and one offset per slice, whatever n
    return up256(sizeof(DecodeScratch) + 2 * (size_t)kDecGrid * sizeof(uint32_t));
}

int evrep_decode_state_init(evrep_decode_state *state, void *stream_) {
    if (bad_ptr(state, 8)) return EVREP_EINVAL;
    k_decode_init<<<1, 1, 0, as_stream(stream_)>>>(state);
    LAUNCH_CHECK("k_decode_init");
    return EVREP_OK;
}

int evrep_decode_dat(const void *raw, int64_t n, int32_t stride, int64_t first_index, int32_t H, int32_t W, uint32_t flags,
                     uint16_t *x, uint16_t *y, int64_t *t, int8_t *p, int64_t capacity, evrep_decode_state *state, void *scratch,
                     void *stream) {
    return decode_call<kFmtDat>(raw, n, stride, first_index, H, W, flags, x, y, t, p, capacity, state, scratch, stream);
}

int evrep_decode_bin5(const void *raw, int64_t n, int64_t first_index, int32_t H, int32_t W, uint32_t flags, uint16_t *x,
                      uint16_t *y, int64_t *t, int8_t *p, int64_t capacity, evrep_decode_state *state, void *scratch, void *stream) {
    return decode_call<kFmtBin5>(raw, n, 8, first_index, H, W, flags, x, y, t, p, capacity, state, scratch, stream);
}

int evrep_dat_seek_time(const int64_t *t, int64_t n, const int64_t *queries, int64_t nq, int64_t term, int64_t *out_idx,
                        void *stream_) {
    if (n < 0 || nq < 0 || nq > EVREP_WINDOWS_MAX_QUERIES || term < 1) return EVREP_EINVAL;
    if (misaligned(t, 8) || (n > 0 && !t)) return EVREP_EINVAL;
    if (misaligned(queries, 8) || misaligned(out_idx, 8) || (nq > 0 && (!queries || !out_idx))) return EVREP_EINVAL;
    if (nq == 0) return EVREP_OK;
    const unsigned grid = (unsigned)((nq + kWinThreads / kWave - 1) / (kWinThreads / kWave));
    k_dat_seek_time<<<grid, kWinThreads, 0, as_stream(stream_)>>>(t, n, queries, nq, term, out_idx);
    LAUNCH_CHECK("k_dat_seek_time");
    return EVREP_OK;
}

}  // extern "C"
