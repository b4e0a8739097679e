// evrep_capi_shared.h -- what the translation units of the extern "C" surface share on the host side: the status plumbing,
// the argument checks every entry point is written with, and the carver every scratch layout is written with.  The library is
// built from fifteen translation units compiled in parallel (build.SOURCES; each says in its first line what it holds).
// No allocation, no global state besides the thread-local last HIP error string, no environment variable read.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "evrep_common.h"

#define EVREP_HIDDEN __attribute__((visibility("hidden")))

namespace evrep_host {
EVREP_HIDDEN char *last_error_buf();       // the calling thread's 256-byte error string (evrep_capi.hip)
EVREP_HIDDEN int hip_check(hipError_t e, const char *what);
// the pixel-sorted stream + chunk offsets + WindowMeta from the runs of k_block_keysort (evrep_capi.hip)
EVREP_HIDDEN int column_sort_keys(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, hipStream_t stream);
}  // namespace evrep_host

#define LAUNCH_CHECK(what)                                              \
    do {                                                                \
        int rc_ = evrep_host::hip_check(hipGetLastError(), what);       \
        if (rc_ != EVREP_OK) return rc_;                                \
    } while (0)

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The argument checks of the entry points.  a: the alignment in bytes, a power of two.  An OPTIONAL pointer (NULL allowed) is
// held to its alignment with misaligned(): NULL passes; a required one with bad_ptr().
static inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
static inline bool bad_ptr(const void *p, uintptr_t a) { return !p || misaligned(p, a); }
static inline bool is_float_dtype(int32_t dtype) { return dtype == EVREP_F64 || dtype == EVREP_F32; }
static inline hipStream_t as_stream(void *stream) { return static_cast<hipStream_t>(stream); }

static inline int check_common(const evrep_plan *plan, const void *events, const void *offsets, const void *ws) {
    if (!plan || plan->abi_version != EVREP_ABI_VERSION || !offsets || !ws) return EVREP_EINVAL;
    if (plan->total_events > 0 && !events) return EVREP_EINVAL;
    if (misaligned(events, 16) || misaligned(ws, 256)) return EVREP_EINVAL;
    return EVREP_OK;
}

// One description per scratch region: a layout function walks the region with a Carver, part by part, each part starting on a
// 256-byte boundary.  The *_scratch_bytes function runs it over a null base and reads `off`; the entry point runs it over the
// caller's scratch and reads the pointers.  (Regions a kernel carves too keep __host__ __device__ *_off_* functions instead.)
struct Carver {
    char *base;        // may be null: sizes only
    size_t off = 0;    // bytes taken so far
    explicit Carver(void *scratch) : base(static_cast<char *>(scratch)) {}
    template <typename T>
    T *take(size_t bytes) {
        T *part = reinterpret_cast<T *>(base ? base + off : nullptr);
        off += up256(bytes);
        return part;
    }
};

#define WS(type, field) reinterpret_cast<type *>(static_cast<char *>(workspace) + plan->field)
#define CWS(type, field) reinterpret_cast<const type *>(static_cast<const char *>(workspace) + plan->field)

constexpr double kKeySortedMaxPerUnit = 220.0;   // average records per builder unit up to which the key-sorted pass is chosen (r04: 110 -> 220, the warm path of the builders beats the per-key column sort for a single builder per binning pass up to 500 000 events on 640x480: bin + build 159 vs 163 us for ERGO-12, 91 vs 115 us for EventStack)
constexpr double kDeepStageMinPerUnit = 110.0;   // classic passes: windows denser than this stage 256 records per unit (stage_classic)
