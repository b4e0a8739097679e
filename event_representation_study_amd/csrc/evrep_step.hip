// evrep_step.hip -- what is left of ev-YOLOv6's training step behind loss.backward() (yolov6/core/engine.py:547-552):
// scaler.step(optimizer) with torch's Nesterov SGD behind it, scaler.update() and ModelEMA.update(model)
// (yolov6/utils/ema.py:30-41), for ALL tensors of the model in three launches and with nothing read on the host.
// include/evrep.h states the statements with evrep_train_step.
//
//   k_step_check    grid (chunks): a workgroup reads the gradient of its chunk; a wave that saw a value that is not finite
//                   sets found_inf to 1 with one integer atomic.  What _amp_foreach_non_finite_check_and_unscale_ tests.
//   k_step_apply    grid (chunks): unscale, weight decay, momentum, the Nesterov step, the EMA of the value just written and
//                   the zero of the gradient, an element at a time in registers: read g, p, buf, e, write p, buf, e, g.
//   k_step_finish   one thread: _amp_update_scale_'s automaton, applied_steps, found_inf back to 0.
//
// THE TABLES.  One launch serves every tensor: workgroup c reads chunk c of the chunk table -- (tensor, first element,
// count <= EVREP_STEP_CHUNK) -- and that tensor's row of the tensor table.  Both are device memory the host side built; a chunk
// that does not fit its tensor, a tensor that names no group of the hyper row: the workgroup returns and touches nothing.
//
// ALIGNMENT.  A chunk's first element may lie 0, 4, 8 or 12 bytes past a 16-byte boundary and the four arrays of a tensor
// need not share that offset.  The chunk is cut by p's address: `head` scalar elements up to p's next 16-byte boundary, then
// groups of four elements, a lane per group, then 0..3 scalar elements.  An array whose address at the first group is a
// multiple of 16 moves its groups as 16-byte loads and stores; another one as four 4-byte ones per group.  No access, of
// either width, lies outside [first, first + count) of its array.
//
// ROUNDING.  float32, every statement ONE operation (__fmul_rn / __fadd_rn); the library is compiled with -ffp-contract=off
// and this file repeats it as a pragma.  No floating-point atomic, no scratch, no grid-wide barrier: the launches are ordered
// by the stream, can be captured into a graph, and two calls give equal bits.
#pragma once
#include "evrep_common.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kStepChunk = EVREP_STEP_CHUNK;
static_assert(kStepChunk % (4 * kThreads) == 0, "a chunk is whole rounds of four elements per lane");

struct StepArgs {
    const evrep_step_tensor *tensors;   // DEVICE [n_tensors]
    const evrep_step_chunk *chunks;     // DEVICE [n_chunks]
    const float *hyper;                 // DEVICE [EVREP_STEP_HYPER_EMA + 3 * n_groups]: ema_d, ema_1md, then lr, momentum, wd per group
    int32_t *amp;                       // DEVICE [EVREP_STEP_AMP_WORDS]: found_inf, scale (float bits), growth_tracker; null: no scaler
    int32_t *applied;                   // DEVICE [1]: applied_steps; null in evrep_ema_update
    double growth, backoff;
    int32_t interval, n_tensors, n_groups;
    uint32_t flags;                     // EVREP_STEP_* of the call
    int32_t ema_only;                   // evrep_ema_update: every tensor is taken as EVREP_STEP_EMA_ONLY
};

// chunk blockIdx.x and its tensor; false (the workgroup returns) if the two do not fit each other
__device__ inline bool step_chunk(const StepArgs &a, evrep_step_chunk &c, evrep_step_tensor &t) {
    c = a.chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= a.n_tensors || c.count < 1 || c.count > kStepChunk || c.first < 0) return false;
    t = a.tensors[c.tensor];
    return c.first <= t.n - (int64_t)c.count;
}

__device__ inline float gload_f32(const float *p) {
    return *reinterpret_cast<const float __attribute__((address_space(1))) *>(reinterpret_cast<uintptr_t>(p));
}

// four consecutive floats at q: one 16-byte access if `vec` (q is then a multiple of 16), else four 4-byte ones
__device__ inline float4 step_load4(const float *q, bool vec) {
    if (vec) return gload16f(q);
    return make_float4(gload_f32(q), gload_f32(q + 1), gload_f32(q + 2), gload_f32(q + 3));
}
__device__ inline void step_store4(float *q, bool vec, float4 v) {
    if (vec) {
        gstore16(q, make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)));
    } else {
        gstore_f32(q, v.x); gstore_f32(q + 1, v.y); gstore_f32(q + 2, v.z); gstore_f32(q + 3, v.w);
    }
}

// scalar elements up to the next 16-byte boundary of q, at most n
__device__ inline int step_head(const float *q, int n) {
    const int head = (4 - (int)((reinterpret_cast<uintptr_t>(q) >> 2) & 3u)) & 3;
    return head < n ? head : n;
}
__device__ inline bool step_aligned(const float *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

__device__ inline bool step_bad(float v) { return !(__fsub_rn(v, v) == 0.0f); }   // NaN, +inf, -inf

__global__ __launch_bounds__(kThreads) void k_step_check(const StepArgs a) {
    evrep_step_chunk c;
    evrep_step_tensor t;
    if (!step_chunk(a, c, t)) return;
    if (!(t.flags & EVREP_STEP_HAS_GRAD) || (t.flags & EVREP_STEP_EMA_ONLY) || !t.g) return;
    const float *g = t.g + c.first;
    const int n = c.count, head = step_head(g, n), nb = (n - head) >> 2, tid = (int)threadIdx.x;
    bool bad = false;
    if (tid < head) bad = step_bad(gload_f32(g + tid));
    for (int j = tid; j < nb; j += kThreads) {
        const float4 v = gload16f(g + head + 4 * j);
        bad = bad || step_bad(v.x) || step_bad(v.y) || step_bad(v.z) || step_bad(v.w);
    }
    const int tail0 = head + 4 * nb;
    if (tid < n - tail0) bad = bad || step_bad(gload_f32(g + tail0 + tid));
    if (__any(bad ? 1 : 0) && (tid & (kWave - 1)) == 0) atomicOr(a.amp, 1);
}

// what a workgroup's elements share
struct StepRule {
    float inv, wd, mom, neg_lr, ema_d, ema_1md;
    bool step, first, has_ema, zero;
};

__device__ inline void step_elem(const StepRule &r, float &p, float g, float &buf, float &e) {
    if (r.step) {
        const float gu = __fmul_rn(g, r.inv);
        const float d = r.wd != 0.0f ? __fadd_rn(gu, __fmul_rn(r.wd, p)) : gu;
        float d2 = d;
        if (r.mom != 0.0f) {
            buf = r.first ? d : __fadd_rn(__fmul_rn(buf, r.mom), d);
            d2 = __fadd_rn(d, __fmul_rn(r.mom, buf));
        }
        p = __fadd_rn(p, __fmul_rn(r.neg_lr, d2));
    }
    if (r.has_ema) {
        e = __fmul_rn(e, r.ema_d);
        e = __fadd_rn(e, __fmul_rn(r.ema_1md, p));
    }
}

__global__ __launch_bounds__(kThreads) void k_step_apply(const StepArgs a) {
    evrep_step_chunk c;
    evrep_step_tensor t;
    if (!step_chunk(a, c, t)) return;
    const bool ema_only = a.ema_only || (t.flags & EVREP_STEP_EMA_ONLY);
    const bool has_grad = !ema_only && (t.flags & EVREP_STEP_HAS_GRAD) && t.g;
    StepRule r;
    r.has_ema = (t.flags & EVREP_STEP_HAS_EMA) && t.ema;
    r.zero = has_grad && (a.flags & EVREP_STEP_ZERO_GRAD);
    r.step = has_grad && !(a.amp && a.amp[0] != 0);
    if (!t.p || (!r.has_ema && !has_grad)) return;
    r.ema_d = a.hyper[0];
    r.ema_1md = a.hyper[1];
    r.inv = 1.0f; r.wd = 0.0f; r.mom = 0.0f; r.neg_lr = 0.0f; r.first = false;
    if (r.step) {
        if (t.group < 0 || t.group >= a.n_groups) return;
        const float *h = a.hyper + EVREP_STEP_HYPER_EMA + 3 * t.group;
        r.neg_lr = -h[0]; r.mom = h[1]; r.wd = h[2];
        if (a.amp) r.inv = (float)(1.0 / (double)__int_as_float(a.amp[1]));
        r.first = *a.applied == 0;
        if (r.mom != 0.0f && !t.buf) return;                            // a group with momentum and a tensor without a buffer
    }
    const bool ld_g = r.step, ld_buf = r.step && r.mom != 0.0f && !r.first, st_buf = r.step && r.mom != 0.0f;
    float *p = t.p + c.first, *g = has_grad ? t.g + c.first : nullptr, *buf = (has_grad && t.buf) ? t.buf + c.first : nullptr;
    float *e = r.has_ema ? t.ema + c.first : nullptr;
    const int n = c.count, head = step_head(p, n), nb = (n - head) >> 2, tail0 = head + 4 * nb, tid = (int)threadIdx.x;

    // the 0..3 elements in front of p's boundary and the 0..3 behind the last group: lanes 0..2 and 64..66
    int s = -1;
    if (tid < head) s = tid;
    else if (tid >= kWave && tid - kWave < n - tail0) s = tail0 + tid - kWave;
    if (s >= 0) {
        float pv = gload_f32(p + s), gv = ld_g ? gload_f32(g + s) : 0.0f, bv = ld_buf ? gload_f32(buf + s) : 0.0f;
        float ev = r.has_ema ? gload_f32(e + s) : 0.0f;
        step_elem(r, pv, gv, bv, ev);
        if (r.step) gstore_f32(p + s, pv);
        if (st_buf) gstore_f32(buf + s, bv);
        if (r.has_ema) gstore_f32(e + s, ev);
        if (r.zero) gstore_f32(g + s, 0.0f);
    }
    if (nb == 0) return;
    const bool vg = g && step_aligned(g + head), vb = buf && step_aligned(buf + head), ve = e && step_aligned(e + head);
    for (int j = tid; j < nb; j += kThreads) {
        const int i = head + 4 * j;
        float4 pv = step_load4(p + i, true);
        float4 gv = ld_g ? step_load4(g + i, vg) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 bv = ld_buf ? step_load4(buf + i, vb) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 ev = r.has_ema ? step_load4(e + i, ve) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        step_elem(r, pv.x, gv.x, bv.x, ev.x);
        step_elem(r, pv.y, gv.y, bv.y, ev.y);
        step_elem(r, pv.z, gv.z, bv.z, ev.z);
        step_elem(r, pv.w, gv.w, bv.w, ev.w);
        if (r.step) step_store4(p + i, true, pv);
        if (st_buf) step_store4(buf + i, vb, bv);
        if (r.has_ema) step_store4(e + i, ve, ev);
        if (r.zero) step_store4(g + i, vg, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    }
}

__global__ __launch_bounds__(kWave) void k_step_finish(const StepArgs a) {
    if (threadIdx.x != 0) return;
    int found = 0;
    if (a.amp) {
        found = a.amp[0] != 0;
        if (!(a.flags & EVREP_STEP_KEEP_SCALE)) {
            const float scale = __int_as_float(a.amp[1]);
            if (found) {
                a.amp[1] = __float_as_int((float)((double)scale * a.backoff));
                a.amp[2] = 0;
            } else {
                const int ok = a.amp[2] + 1;
                if (ok == a.interval) {
                    const float grown = (float)((double)scale * a.growth);
                    if (!step_bad(grown)) a.amp[1] = __float_as_int(grown);
                    a.amp[2] = 0;
                } else {
                    a.amp[2] = ok;
                }
            }
        }
        a.amp[0] = 0;
    }
    *a.applied = *a.applied + (found ? 0 : 1);
}

}  // namespace evrep
