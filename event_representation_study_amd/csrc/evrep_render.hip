// evrep_render.hip -- ev-licious' Events.render (io/utils/render.py:9-141) for a batch of windows: the per-pixel STATE every
// rendering type is a function of (k_render_state, a stream builder over the binned records) and the streaming launch that
// turns it into frames (k_render_compose).  Included by evrep_capi_builders.hip behind evrep_builders.hip.
//
// With integer coordinates every type reads, per pixel,
//   bit 0  some event with p > 0        bit 1  some event with p <= 0        bit 2  the LAST event in array order has p > 0
//   bit 3  (every pixel of the window)  the window holds <= 2 rows: _render_timesurface returns zeros for it
//   net      #positive - #negative                                                           (EVENT_FRAME)
//   surface  the ordered sum  img = fl32(double(img) + exp(-(t[-1] - t_i) / tau)), array order  (TIME_SURFACE, np.add.at)
// and cast=False (_jitter_events: every event also drawn at (x, y+1), (x+1, y), (x+1, y+1), the four copies concatenated) is a
// 2 x 2 stencil over the state: the sources of output pixel (y, x) are, latest copy first, (y-1, x-1), (y, x-1), (y-1, x), (y, x).
namespace evrep {

constexpr uint32_t kRsPos = 1u, kRsNeg = 2u, kRsLastPos = 4u, kRsFew = 8u;

// --------------------------------------------------------------------------------------------
// k_render_state: one wave per 128-pixel unit, the skeleton of k_event_stack_stream.  The unit's records arrive 64 at a time in
// array order (stream_unit_records after the key-sorted pass, whatever the unit holds; the pixel-sorted stream's segment of the
// unit after the other passes: sorted by (pixel, rank), so a pixel's records keep their order there too).  Per pixel of the tile:
//   flg   atomicOr of the two polarity flags
//   last  atomicMax of ((rank + 1) << 1 | positive): 64 bits, a window of the classic passes may hold 2^31 - 1 rows
//   net   atomicAdd of +1 / -1
//   acc   the ordered float32 sum: a leader election per pixel and batch (ds_min of the lane on a tag word, as k_voxel_stream's
//         float64 sums: the lowest pending lane of a pixel adds first), never a floating-point atomic
// The tile leaves as one burst; every pixel of every output is written exactly once, 0 where no event fell.  Nothing depends on
// ascending timestamps.  The wave of a window's first unit leaves the window's merged WindowMeta in the workspace after the
// key-sorted pass (the other passes publish it themselves): the status words are then on the device for a caller that may not wait.
// LDS: last [npixa] u64 | flg [npixa] | net [npixa] | acc [npixa] f32 | tag [npixa] | head [64 * RB] | srcs [128] | sb [npixa] bytes
__host__ __device__ inline size_t render_state_lds_bytes(int npixa, int rb) {
    return (size_t)npixa * 8 + (size_t)4 * npixa * 4 + (size_t)(64 * rb + 128) * 4 + align16((size_t)npixa);
}
template <int RB>
__global__ __launch_bounds__(kWave, 6) void k_render_state(BinView bv, const int64_t *__restrict__ off, int H, int W, int nchunk, UnitCfg uc,
                                                       double tau, WindowMeta *__restrict__ meta_out, unsigned char *__restrict__ state,
                                                       int32_t *__restrict__ net, float *__restrict__ surface) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x;
    const int uid = chunk_unit((int)(gridDim.x * gridDim.y * gridDim.z));
    int chunk, nch;
    const ChunkGeom g = unit_geom(H, W, nchunk, uc, chunk, nch, uid);
    const int b = g.b;
    const int64_t beg = off[b];
    const int64_t n_win = off[b + 1] - beg;
    const int npixa = (uc.span + uc.merge) * kChunkPx;
    unsigned long long *last = reinterpret_cast<unsigned long long *>(smem);
    uint32_t *flg = reinterpret_cast<uint32_t *>(last + npixa);
    int *netl = reinterpret_cast<int *>(flg + npixa);
    float *acc = reinterpret_cast<float *>(netl + npixa);
    uint32_t *tag = reinterpret_cast<uint32_t *>(acc + npixa);
    uint32_t *head = tag + npixa;
    uint32_t *srcs = head + 64 * RB;
    unsigned char *sb = reinterpret_cast<unsigned char *>(srcs + 128);
    {   // last, flg, net, acc: zero; tags: free
        uint4 *z = reinterpret_cast<uint4 *>(smem);
        for (int v = lane; v * 16 < npixa * 20; v += kWave) z[v] = make_uint4(0u, 0u, 0u, 0u);
        uint4 *t4 = reinterpret_cast<uint4 *>(tag);
        for (int v = lane; v * 4 < npixa; v += kWave) t4[v] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    const int4 *evw = bv.ev + beg;
    int t_last = 0;   // t[-1]: the window's last ROW (render.py:132), in frame or not
    if (surface && n_win > 0) t_last = evw[n_win - 1].z;
    const int c0 = g.c0;
    wave_phase();
    // one batch: lane holds one record (lanes in array order inside a pixel)
    auto batch = [&](bool have, uint32_t px, uint32_t rank, int t, int p) {
        have = have && px < (uint32_t)g.npix;   // (a record of the unit's keys lies in the unit: the tile is never written outside)
        if (have) {
            const bool pos = p > 0;
            atomicMax(&last[px], ((unsigned long long)(rank + 1u) << 1) | (pos ? 1ull : 0ull));
            atomicOr(&flg[px], pos ? kRsPos : kRsNeg);
            if (net) atomicAdd(&netl[px], pos ? 1 : -1);
        }
        if (surface) {   // wave-uniform
            double v = 0.0;
            if (have) v = exp_neg_range((double)((int64_t)t - (int64_t)t_last) / tau);   // -(t[-1] - t) / float(tau): a float64 division
            bool pend = have;
            while (__any(pend)) {
                if (pend) atomicMin(&tag[px], (uint32_t)lane);
                wave_phase();
                const bool win = pend && tag[px] == (uint32_t)lane;
                wave_phase();
                if (win) {
                    acc[px] = (float)((double)acc[px] + v);
                    tag[px] = ~0u;
                    pend = false;
                }
                wave_phase();
            }
        }
    };
    if (bv.fused) {
        stream_unit_records<RB>(bv, b, beg, n_win, H * nchunk, g.row * nchunk + chunk, g.row * nchunk + chunk + nch, head, srcs, StreamNoPre(),
            [&](bool have, const Rec8 &q, const uint2 &) {
                const uint32_t rank = q.y >> 11, p2 = (q.y >> 9) & 3u;
                int p = (int)p2 - 1;
                if (have && p2 == 3u) p = evw[rank].w;
                batch(have, ((q.y & 511u) - (uint32_t)c0) & 511u, rank, (int)q.x, p);
            });
    } else if (n_win > 0) {
        const uint32_t *co = bv.chunk_off + ((size_t)b * H + g.row) * (nchunk + 1);
        uint32_t cs = co[chunk], ce = co[chunk + nch];
        if ((int64_t)cs < beg || (int64_t)ce > beg + n_win) ce = cs;   // (the unit's segment lies inside its window's records)
        const int key0 = g.row * W + c0;
        for (uint32_t j = cs; j < ce; j += kWave) {   // (cs, ce: wave-uniform)
            const bool have = j + (uint32_t)lane < ce;
            Rec r = make_int4(key0, 0, 0, 0);
            if (have) r = bv.sorted[j + lane];
            batch(have, (uint32_t)(r.x - key0), (uint32_t)r.y, r.z, r.w);
        }
    }
    wave_phase();
    const uint32_t few = n_win <= 2 ? kRsFew : 0u;
    for (int px = lane; px < g.npix; px += kWave)
        sb[px] = (unsigned char)(flg[px] | (((uint32_t)last[px] & 1u) << 2) | few);
    wave_phase();
    const size_t o = ((size_t)b * H + g.row) * (size_t)W + (size_t)c0;   // the unit's first pixel in (B, H, W)
    {   // the state bytes: a lead up to the next 4-byte boundary, whole dwords, a tail
        const int lead = min(g.npix, (int)((4u - (uint32_t)(o & 3u)) & 3u));
        const int nd = (g.npix - lead) >> 2, tail0 = lead + 4 * nd;
        unsigned char *dst = state + o;
        if (lane < lead) dst[lane] = sb[lane];
        if (lane < nd) {
            const unsigned char *s4 = sb + lead + 4 * lane;
            *reinterpret_cast<uint32_t *>(dst + lead + 4 * lane) = (uint32_t)s4[0] | ((uint32_t)s4[1] << 8) | ((uint32_t)s4[2] << 16) | ((uint32_t)s4[3] << 24);
        }
        if (tail0 + lane < g.npix) dst[tail0 + lane] = sb[tail0 + lane];
    }
    if (net) for (int px = lane; px < g.npix; px += kWave) net[o + px] = netl[px];
    if (surface) for (int px = lane; px < g.npix; px += kWave) surface[o + px] = acc[px];
    if (bv.fused && g.row == 0 && chunk == 0) {   // wave-uniform: what k_window_meta leaves for the read-backs
        WindowMeta m = window_meta(bv, off, b);
        if (lane == 0) {
            m.status &= 0xffffu;
            if (n_win <= 0) m.status |= EVREP_ST_EMPTY;
            else if (m.tmin == m.tmax) m.status |= EVREP_ST_FLAT_TIME;
            for (int i = 0; i < 6; ++i) m.pad[i] = 0;
            meta_out[b] = m;
        }
    }
}

// --------------------------------------------------------------------------------------------
// k_render_compose: state (+ net / surface + canvas) -> frames.  No plan, no workspace.  The batch's output is one flat array: a
// lane produces the 4 consecutive pixels 4 q .. 4 q + 3 of (B, H, W) -- 12 bytes, three dword stores at a 4-byte boundary whatever
// H * W is (a quad may straddle two windows: the window and the pixel inside it are stepped per pixel); only the batch's last
// quad, when B * H * W is no multiple of 4, leaves as bytes.  Window blockIdx.y owns the quads whose first pixel is its own.
// (y, x) is decoded only for the cast=False stencil, whose three neighbour states are plain byte loads (1 byte per pixel: cache).
// TIME_SURFACE: the 256 x 4 float64 table sits in LDS; a pixel leaves as two 16-byte stores.
// grid (ceil((ceil(H * W / 4) + 1) / 256), B), 256 threads; TYPE: RenderingType's value, JIT: cast=False.
constexpr int kRcThreads = 256;
template <int TYPE, bool JIT>
__global__ __launch_bounds__(kRcThreads) void k_render_compose(const unsigned char *__restrict__ state, const int32_t *__restrict__ net,
                                                          const float *__restrict__ surface, const double *__restrict__ lut,
                                                          const unsigned char *__restrict__ canvas, int canvas_batched, int B, int H, int W,
                                                          void *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *slut = reinterpret_cast<double *>(smem);
    if (TYPE == EVREP_RENDER_TIME_SURFACE) {
        for (int i = threadIdx.x; i < 1024; i += kRcThreads) slut[i] = lut[i];
        __syncthreads();
    }
    const int b = blockIdx.y;
    const uint32_t npx = (uint32_t)H * (uint32_t)W;
    const uint64_t wb = (uint64_t)b * npx, total = (uint64_t)B * npx;
    const uint64_t q = ((wb + 3u) >> 2) + (uint64_t)blockIdx.x * kRcThreads + threadIdx.x;
    const uint64_t g0 = q << 2;
    if (g0 >= wb + npx) return;   // a later window's quad (or none)
    const int nv = (int)min((uint64_t)4, total - g0);
    uint32_t sw = 0u;
    if (nv == 4) sw = *reinterpret_cast<const uint32_t *>(state + g0);
    else for (int k = 0; k < nv; ++k) sw |= (uint32_t)state[g0 + k] << (8 * k);
    uint32_t l = (uint32_t)(g0 - wb);
    int bb = b;
    uint32_t w3[3] = {0u, 0u, 0u};   // the quad's 12 bytes
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < nv) {
            const uint64_t gp = g0 + (uint64_t)k;
            uint32_t s = (sw >> (8 * k)) & 255u;
            if (TYPE == EVREP_RENDER_TIME_SURFACE) {
                double4 c = make_double4(0.0, 0.0, 0.0, 0.0);
                const float f = surface[gp] * 256.0f;   // cm(img): lut[min(int(img * N), N - 1)], the product in float32
                if (!(s & kRsFew) && f == f) {
                    const int idx = f >= 255.0f ? 255 : (f < 0.0f ? 0 : (int)f);
                    c = make_double4(slut[4 * idx], slut[4 * idx + 1], slut[4 * idx + 2], slut[4 * idx + 3]);
                }
                double2 *o2 = reinterpret_cast<double2 *>(out) + gp * 2u;
                o2[0] = make_double2(c.x, c.y);
                o2[1] = make_double2(c.z, c.w);
            } else {
                uint32_t r, gch, bl;
                if (TYPE == EVREP_RENDER_EVENT_FRAME) {
                    const int n = min(max(net[gp], -7), 7);   // uint8(clip(20 * net + 128, 0, 255)): 0 from -7 down, 255 from 7 up
                    r = gch = bl = (uint32_t)min(max(20 * n + 128, 0), 255);
                } else {
                    if (JIT) {
                        const uint32_t y = l / (uint32_t)W, x = l - y * (uint32_t)W;
                        const unsigned char *sp = state + gp;
                        const uint32_t a = (y > 0u && x > 0u) ? sp[-(W + 1)] : 0u, c = x > 0u ? sp[-1] : 0u, d = y > 0u ? sp[-W] : 0u;
                        if (TYPE == EVREP_RENDER_RED_BLUE_OVERLAP) s |= a | c | d;
                        else s = (a & 3u) ? a : ((c & 3u) ? c : ((d & 3u) ? d : s));
                    }
                    if (!(s & 3u)) {
                        r = gch = bl = 255u;
                        if (canvas) {
                            const unsigned char *cp = canvas + ((canvas_batched ? (uint64_t)bb * npx : 0u) + l) * 3u;
                            r = cp[0]; gch = cp[1]; bl = cp[2];
                        }
                    } else if (TYPE == EVREP_RENDER_RED_BLUE_OVERLAP) {
                        r = (s & kRsNeg) ? 255u : 0u; gch = 0u; bl = (s & kRsPos) ? 255u : 0u;
                    } else if (TYPE == EVREP_RENDER_RED_BLUE_NO_OVERLAP) {
                        r = (s & kRsLastPos) ? 0u : 255u; gch = 0u; bl = (s & kRsLastPos) ? 255u : 0u;
                    } else {
                        r = gch = bl = (s & kRsLastPos) ? 255u : 0u;
                    }
                }
                const uint32_t vals[3] = {r, gch, bl};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int byte = 3 * k + ch;
                    w3[byte >> 2] |= vals[ch] << (8 * (byte & 3));
                }
            }
            if (++l == npx) { l = 0u; ++bb; }
        }
    }
    if (TYPE != EVREP_RENDER_TIME_SURFACE) {
        unsigned char *o1 = reinterpret_cast<unsigned char *>(out) + g0 * 3u;
        if (nv == 4) {
            uint32_t *o4 = reinterpret_cast<uint32_t *>(o1);
            o4[0] = w3[0]; o4[1] = w3[1]; o4[2] = w3[2];
        } else {
            for (int i = 0; i < 3 * nv; ++i) o1[i] = (unsigned char)(w3[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace evrep
