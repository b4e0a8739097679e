/*
 * evrep.h -- C ABI of libevrep.so, the MI355X (gfx950) event-representation engine.
 *
 * The reference (uzh-rpg/event_representation_study) has no FFI: its boundary is a set of
 * importable Python names.  Each entry point below replaces the hot
 * loop behind one of those names; the Python host mirror under
 * event_representation_study_amd/representations/ binds them with ctypes (INTEGRATION.md shows
 * the stub a reference maintainer would add).  Citations are relative to the reference tree.
 *
 * Conventions
 *   - plain C types only; every pointer marked DEVICE is a HIP device pointer, `stream` is a
 *     hipStream_t passed as void* (NULL = the null stream);
 *   - no global state (nothing is remembered between calls, no environment variable is read, any number of host
 *     threads may drive any number of devices and streams), no allocation: the caller owns a workspace of
 *     evrep_workspace_bytes();
 *   - every call is asynchronous on `stream` and returns an EVREP_* status (launch errors
 *     included); data-dependent failures the reference reports as Python exceptions are
 *     recorded per window in the workspace and read back with evrep_read_status();
 *   - events are int32 rows [x, y, t, p] (the '<i4' structured array the reference adapters
 *     build, ev-YOLOv6/yolov6/data/gen1_2yolo.py:567-571), time-sorted, B windows concatenated,
 *     window b = rows [offsets[b], offsets[b+1]);
 *   - outputs are dense, channel-last (B, H, W, C), written exactly once (zero fill fused).
 */
#ifndef EVREP_H_
#define EVREP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVREP_ABI_VERSION 3

/* return codes */
#define EVREP_OK 0
#define EVREP_EINVAL 1      /* bad argument (sizes, NULL pointers, unsupported C / k / bins) */
#define EVREP_EWORKSPACE 2  /* workspace too small */
#define EVREP_EHIP 3        /* a HIP launch failed; see evrep_last_hip_error() */
#define EVREP_ENOTBINNED 4  /* builder called on a plan that has not been binned */

/* per-window status bits (evrep_read_status) */
#define EVREP_ST_EMPTY 1u      /* window has no events (reference: ValueError on t.min()) */
#define EVREP_ST_OOB 2u        /* some x + y*W outside [0, H*W) (reference: IndexError in put / zero channel in MDES) */
#define EVREP_ST_UNSORTED 4u   /* timestamps not ascending: evrep_mdes / evrep_optimized, evrep_event_stack, evrep_time_surface (premap bit 1) and evrep_tore work in array order as the reference does; the other builders' tensors are undefined */
#define EVREP_ST_FLAT_TIME 8u  /* t[-1] == t[0] (reference divides by zero) */
#define EVREP_ST_HOT_OVERFLOW 16u /* a builder could not queue a unit of a clustered window (the workspace's hot list was full): pixels of the window are unwritten */

/* MDES function / aggregation codes (representation_search/operations.py:42-87, :16-34) */
enum evrep_func { EVREP_F_TIMESTAMP = 0, EVREP_F_POLARITY, EVREP_F_COUNT, EVREP_F_TIMESTAMP_POS,
                  EVREP_F_TIMESTAMP_NEG, EVREP_F_COUNT_POS, EVREP_F_COUNT_NEG };
enum evrep_agg { EVREP_A_SUM = 0, EVREP_A_MEAN, EVREP_A_MAX, EVREP_A_VARIANCE };
enum evrep_dtype { EVREP_F64 = 0, EVREP_F32 = 1 };

#define EVREP_MAX_CHANNELS 16  /* MDES channels per launch (larger stacks: several launches) */
#define EVREP_MAX_DIM 4096     /* H, W */

/* Host-side description of one batch; filled by evrep_plan_init, read-only afterwards. */
typedef struct evrep_plan {
    int32_t abi_version;
    int32_t B, H, W;
    int64_t total_events;          /* offsets[B] */
    int64_t max_events_per_window; /* upper bound used to size grids; no host sync needed */
    int32_t chunk, nblk;           /* row-partition geometry (derived) */
    int32_t nchunk, reserved;      /* 128-pixel column chunks per row (derived); reserved = the binning pass chosen:
                                      2 = key-sorted (k_block_keysort alone; the builder waves finish the order by pixel),
                                      3 = k_block_keysort + the column sort per (row, chunk) key (dense windows),
                                      1 = k_block_rowsort + the column sort per row, 0 = the three-kernel pass */
    int32_t flags;                 /* EVREP_PLAN_* bits the plan was made with */
    int32_t pacing;                /* store pacing of the wide float64 builders (evrep_plan_set_pacing): -1 = automatic,
                                      0 = off, > 0 = every builder wave starts its stores no earlier than this many
                                      10 ns ticks after it started */
    size_t off_meta, off_table, off_stats, off_rowoff, off_chunkoff, off_sorted1, off_sorted2, off_cuts, off_scratch;
    size_t workspace_bytes;
} evrep_plan;

/* evrep_plan_init_ex flags: which binning passes the plan may choose from (A/B timing and the cross-pass parity
 * tests; every pass produces the same tensors bit for bit -- but for the time surface, whose stream builder (after the
 * key-sorted pass, dense windows) takes one exponential per event where the ordered builder takes one per slice: the two
 * forms agree to 1e-13 relative), and tuning / A/B knobs. */
#define EVREP_PLAN_NO_KEY_PASS 1u       /* keep passes 2 and 3 (k_block_keysort) out of the choice */
#define EVREP_PLAN_THREE_KERNEL 2u      /* the round-1 three-kernel pass (0) only */
#define EVREP_PLAN_FORCE_KEY_SORTED 4u  /* pass 2 also for windows denser than it is chosen for */
#define EVREP_PLAN_BIG_BLOCKS 8u        /* key-sorted pass: 8192-event blocks also for short windows */
#define EVREP_PLAN_NO_FUSED_SCATTER 16u /* three-kernel pass: separate scan and scatter kernels */
#define EVREP_PLAN_X_SPAN2 64u          /* experiment: float64 MDES units of two 128-pixel chunks (NOTES.md 8) */
#define EVREP_PLAN_X_STAGE128 128u      /* experiment: a 128-record stage also for one-chunk units of sparse windows */
#define EVREP_PLAN_X_TAIL_MERGE 256u    /* experiment: a row's last unit also takes a short tail chunk (NOTES.md r04: slower) */
#define EVREP_PLAN_X_STAGE64 512u       /* experiment: key-sorted one-chunk units stage 64 records: units of > 64 records leave the two-batch path */
#define EVREP_PLAN_X_HANDOVER2 1024u    /* experiment: two-chunk units beyond the record stage also go to the hot launch whole */
#define EVREP_PLAN_X_HANDOVER_DENSE 2048u /* experiment: one-chunk units are handed over whole on dense windows as well */
#define EVREP_PLAN_X_NO_SWEEP_MAIN 4096u  /* experiment: TORE and the accumulators keep the ordered main launch on dense windows */
#define EVREP_PLAN_X_NO_MONSTER_HANDOVER 8192u /* experiment: two-chunk units hand nothing over, not even their monster units */
#define EVREP_PLAN_X_POLSTATS_ORDERED 65536u /* A/B: the n_imagenet accumulators by k_polstats also where r06 streams them (k_polstats_stream) */
#define EVREP_PLAN_X_ESTACK_ORDERED 131072u /* A/B: EventStack by k_event_stack also where r06 streams it (k_event_stack_stream) */
#define EVREP_PLAN_X_MDES_NO_COOP 4194304u /* A/B: the ordered float32 ERGO-12's big hot units by time slices of one-wave workgroups (r05) instead of k_mdes_coop */
#define EVREP_PLAN_X_TS_STREAM 1048576u   /* tests / A/B: the time surface by k_time_surface_stream at every density */
#define EVREP_PLAN_X_TS_ORDERED 2097152u  /* A/B: the time surface by k_time_surface also where r06 streams it */
#define EVREP_PLAN_X_MDES_STREAM 524288u  /* tests / A/B: ERGO-12 by k_mdes_stream at every density (default: where it is measured faster) */
#define EVREP_PLAN_X_MDES_ORDERED 262144u /* A/B: ERGO-12 by k_mdes also where r06 streams it (k_mdes_stream) */
#define EVREP_PLAN_X_TORE_ORDERED 32768u  /* A/B: TORE by the ordered / handed-over paths (k_tore) also where r06 streams it (k_tore_stream) */
#define EVREP_PLAN_X_VOXEL_ORDERED 16384u /* A/B: the voxel grid by the ordered paths (k_voxel) also after the key-sorted pass,
                                             where r06 streams it (k_voxel_stream); same tensors bit for bit */

int evrep_abi_version(void);
const char *evrep_last_hip_error(void);

/* Fill `plan` for B windows of an H x W sensor holding total_events events, at most
 * max_events_per_window in any one window. */
int evrep_plan_init(evrep_plan *plan, int32_t B, int32_t H, int32_t W, int64_t total_events,
                    int64_t max_events_per_window);
/* The same with EVREP_PLAN_* flags (evrep_plan_init = flags 0).  The library itself reads no environment variable:
 * the Python binding translates EVREP_BIN_CLASSIC / EVREP_BIN_THREE_KERNEL / EVREP_BIN_KEY_SORTED / ... into flags. */
int evrep_plan_init_ex(evrep_plan *plan, int32_t B, int32_t H, int32_t W, int64_t total_events,
                       int64_t max_events_per_window, uint32_t flags);
/* Store pacing of the builders whose launch is bound by HBM writes (NOTES.md 3.2, Store pacing): ticks = -1 automatic (what
 * evrep_plan_init sets), 0 off, > 0 explicit hold in 10 ns ticks.  Results never depend on it. */
int evrep_plan_set_pacing(evrep_plan *plan, int32_t ticks);
size_t evrep_workspace_bytes(const evrep_plan *plan);

/* The (y,x) binning pass every builder consumes: a stable two-level partition of each window's
 * events by pixel id x + y*W (row partition across workgroups, then column partition inside one
 * workgroup per row), plus per-window statistics (t range, bounding box, MDES polarity flags).
 * Replaces the per-builder `index = y*W + x` scatter of event_stack.py:123-125,
 * operations.py:40, time_surface.py:67, tore.py:23-47.
 * events DEVICE int32 [total,4]; offsets DEVICE int64 [B+1]; workspace DEVICE. */
int evrep_bin_events(const evrep_plan *plan, const int32_t *events, const int64_t *offsets,
                     void *workspace, void *stream);

/* MixedDensityEventStack.stack (representation_search/mixed_density_event_stack.py:25-151) with
 * Operations.exec/run (operations.py:15-89) for C <= EVREP_MAX_CHANNELS channels:
 * window[c] in 0..6 (anything else = the reference's failed channel -> zeros), func[c], agg[c].
 * out DEVICE (B,H,W,C) of out_dtype, each value multiplied by `scale` (1.0, or 255.0 as
 * gen1_transforms.py:31 does). */
int evrep_mdes(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
               int32_t C, const int32_t *window, const int32_t *func, const int32_t *agg, double scale,
               int32_t out_dtype, void *out, void *stream);

/* The "SBT" stacking of MixedDensityEventStack (mixed_density_event_stack.py:76-107): EIGHT windows cut by the normalised
 * time t_s instead of by event count -- w0 all, w1..w3 i/3 <= t_s <= (i+1)/3 (inclusive both ends), w4..w7 t_s <= 1/2, 1/4,
 * 1/8, 1/16.  evrep_mdes_sbt_windows forms them for B windows (timestamps ascending, as every builder requires) as rank
 * ranges: bounds DEVICE int32 [B][8][2] {lo, hi}, flags DEVICE uint32 [B][2] (which windows hold p == -1 / out-of-frame
 * events).  evrep_mdes_ex = evrep_mdes with window[c] in 0..7 over those windows; bounds == flags == NULL: evrep_mdes. */
int evrep_mdes_sbt_windows(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t *bounds,
                           uint32_t *flags, void *stream);
int evrep_mdes_ex(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t C,
                  const int32_t *window, const int32_t *func, const int32_t *agg, double scale, int32_t out_dtype,
                  void *out, const int32_t *bounds, const uint32_t *flags, void *stream);

/* get_optimized_representation (optimized_representation.py:86-134): the ERGO-12 triples. */
int evrep_optimized(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                    double scale, int32_t out_dtype, void *out, void *stream);

/* EventStack.make_stack + post_stack (event_stack.py:45-131) of one half (past, or the reversed future) per
 * window: level k = polarity of the last event at each pixel among events[off_k:].
 * out DEVICE (B,H,W,S) float32; premap 1 applies p -> (p+1)//2 first (gen1_transforms.py:34) and the value is
 * int8(2p - 1) (event_stack.py:18); premap 0: p is {0,1}; premap 2: the p column already holds the int8 value
 * (EventStack.pre_stack builds both halves on the host side: past as is, future reversed and negated, :21-41).
 * `scale`: the int8 value as float32 times `scale`, one float32 multiply; pixels without an event stay +0. */
int evrep_event_stack(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                      int32_t stack_size, int32_t premap, float scale, float *out, void *stream);

/* ToTimesurface.__call__ (time_surface.py:25-74): S <= 8 surfaces sampled at event indices.
 * indices == NULL: the cuts gen1_transforms.py:79-81 computes, searchsorted(t_norm, 1..S);
 * otherwise DEVICE int32 [B,S], the `indices` argument of ToTimesurface.__call__.
 * premap bit 0 applies p -> int8((p+1)/2) first (gen1_transforms.py:70-72); bit 1 (premap 2 / 3): the timestamps are NOT
 * ascending -- the scan of time_surface.py:66-74 runs in ARRAY order whatever the timestamps, and so do the kernels; the bit
 * only keeps them from factorising the exponentials around a reference time (a memory timestamp may then lie far BEHIND a
 * cut's).  The caller must hand `indices` itself for such a window: searchsorted on an unsorted array is the caller's numpy's.
 * out DEVICE (B,H,W,2S) float64/float32, channel c = 2s+p.
 * Precision (float64): within 1e-12 relative of numpy's exp((mem - t_i) / tau) wherever that is a normal float64; subnormal
 * values (exp's argument between -745.13 and -708.4) within 4 * 2^-1074 absolute, 0 exactly where numpy gives 0, inf where it
 * overflows.  Two forms compute it: exp((t - tref) / tau) * exp((tref - t_cut) / tau) around the last cut tref (one
 * exponential per event), and exp((t - t_cut) / tau) per slice.  The factorised form is taken only while every factor is a
 * normal float64: no live cut more than 600 tau from tref and no event of the window (binning statistics: t.min(), t.max())
 * more than 700 tau before or after it.  float32: the float64 value rounded once.
 * `scale`: every surface value, untouched pixels included, is exp(.) * scale in float64 before that rounding (the factorised form
 * carries scale in its per-slice factor); slices the scan never reaches stay exactly 0. */
int evrep_time_surface(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                       int32_t slices, const int32_t *indices, double tau, int32_t premap, double scale,
                       int32_t out_dtype, void *out, void *stream);

/* The same with float64 timestamps (time_surface.py:66-74 is dtype-agnostic): tf DEVICE double [total_events], one time per
 * event, indexed like `events` (whose own t column then only orders them); `indices` must be given.  tf == NULL:
 * evrep_time_surface. */
int evrep_time_surface_ftime(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                             int32_t slices, const int32_t *indices, const double *tf, double tau, int32_t premap,
                             double scale, int32_t out_dtype, void *out, void *stream);

/* events2ToreFeature (tore.py:6-83) for one sample time per window, k <= 8.
 * sample_times == NULL: T = t[-1] (gen1_transforms.py:63); otherwise DEVICE int32 [B].
 * frame_mode 0: the events' bounding box, origin-shifted (gen1_transforms.py:61-64); the window's
 *               output is a compact (Hbb,Wbb,2k) array at out + b*H*W*2k, bbox via evrep_read_bbox; a window whose
 *               out-of-frame events (EVREP_ST_OOB) stretch the box beyond H x W has no such array: nothing is written for it;
 * frame_mode 1: full (H,W) frame, origin-shifted by (xmin,ymin) (n_imagenet .../imagenet.py:1095-1103);
 * frame_mode 2: full (H,W) frame, no shift (x, y used as 0-based pixel coordinates).
 * Timestamps that are not ascending (EVREP_ST_UNSORTED): array order, each event replacing the (pixel, polarity) k-vector v by the
 * sorted [dt] + v[:k-1] -- what np.partition yields there on numpy >= 2.0 / AVX2+ hosts (tore.py:22-25).
 * `scale`: the finished float32 value max(log(v + 1) - log(151), 0) times `scale`, one float32 multiply, empty FIFOs included; a
 * negative scale is taken (the values then descend along a FIFO).
 * out DEVICE float32. */
int evrep_tore(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
               int32_t k, int32_t frame_mode, const int32_t *sample_times, float scale, float *out, void *stream);

/* The same with FLOAT64 timestamps (n_imagenet hands seconds as '<f8', imagenet.py:1002-1006,1093-1103; tore.py itself
 * computes currentSampleTime - ts in whatever dtype it is given): tf DEVICE double [total_events] = every event's
 * time, indexed like `events` (their t column is then only used for the sortedness check); sample_times_f DEVICE
 * double [B] or NULL (= tf of the window's last event).  tf == NULL: exactly evrep_tore. */
int evrep_tore_ftime(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t k,
                     int32_t frame_mode, const int32_t *sample_times, const double *tf, const double *sample_times_f,
                     float scale, float *out, void *stream);

/* compute_repr (representation_search/gromov_wasserstein.py:72-82) with t normalised as :96;
 * mode 0.  mode 1 = tonic.transforms.ToVoxelGrid as gen1_transforms.py:22-25 consumes it
 * (restated from tonic's published algorithm; parity unpinned).  mode 2 = ev-licious
 * events_to_voxel_grid, integer-pixel path (ev-licious/src/evlicious/tools/utils.py:52-108), before
 * its optional normalisation (evrep_voxel_normalize applies it to the whole batch).  out DEVICE (B,H,W,bins) float64.
 * `scale` (here and in evrep_voxel_range / evrep_voxel_tnorm): the finished float64 sum of a (pixel, bin) cell times `scale`,
 * once, at the pixels that hold an event; a pixel without events stays +0 whatever the sign of scale. */
int evrep_voxel(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                int32_t bins, int32_t mode, double scale, double *out, void *stream);
/* The same with an explicit time range per window (mode 2 only): t_range DEVICE int64 [B,2] = the t0_us, t1_us
 * arguments of events_to_voxel_grid (utils.py:52,60-63), in the units of the events' t column; NULL = t[0], t[-1].
 * Events outside the range fall outside the bins and are dropped, except that the bin index is truncated toward
 * zero as the reference's astype("int32") does (:67), so up to one bin before t0_us still counts into bin 0. */
int evrep_voxel_range(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                      int32_t bins, int32_t mode, double scale, const int64_t *t_range, double *out, void *stream);

/* ev-licious events_to_voxel_grid for SUB-PIXEL event coordinates (Events.divider > 1; utils.py:86-102): the
 * bilinear-in-x/y draw of every event into its four surrounding pixels, float32 accumulation in the reference's
 * order.  `events` carries the TRUNCATED coordinates (x.astype("int32"), :92-93), xy DEVICE double [total,2] the
 * original (x, y) of every event (indexed like `events`); t_range as evrep_voxel_range.
 * out DEVICE float32 (B,H,W,bins), before the optional normalisation (evrep_voxel_normalize). */
/* compute_repr(x, y, t, p, width, height, bins) itself (representation_search/gromov_wasserstein.py:72-82): the caller hands
 * its own normalised time per event -- tnorm DEVICE double [total_events], indexed like `events`, used exactly as the
 * reference uses `t`: b = (bins - 1) * t, blim in {int(b), int(b) + 1}, grid[y, x, blim] += (1 - |blim - b|) * p, lower
 * bin for every event, then the upper bin.  The events' own t column only orders them.  out DEVICE double (B,H,W,bins). */
int evrep_voxel_tnorm(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                      const double *tnorm, int32_t bins, double scale, double *out, void *stream);

int evrep_voxel_subpixel(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                         const double *xy, int32_t bins, const int64_t *t_range, float *out, void *stream);

/* The rest of ev-licious events_to_voxel_grid for a whole batch (utils.py:56,77-83, the numpy variant): the channel-last grids
 * that evrep_voxel_range (mode 2, float64) or evrep_voxel_subpixel (float32) wrote become the channel-first float32 tensor
 * the reference returns, standardised over each window's non-zero entries.
 * grid DEVICE (B,H,W,bins) float64 / float32 (grid_dtype); out DEVICE float (B,bins,H,W), every element written exactly once.
 * Without EVREP_VOXNORM_NORMALIZE: out[b,c,y,x] = (float)grid[b,y,x,c], bit for bit, in one launch; scratch is not used and
 * stats_out must be NULL.  With it, per window and with v = (float)grid value, every sum, mean, std and the quotient in float64
 * and no multiply fused with an add:
 *     n = #{v != 0};  mean = (sum over v != 0 of v) / n;  std = sqrt((sum over v != 0 of (v - mean)^2) / n)   (two passes)
 *     n > 0 and std > 0:  out = (float)(((double)v - mean) / (1e-5 + std)) where v != 0, +0 elsewhere;
 *     otherwise the window is written un-normalised, as without the flag.
 * stats_out DEVICE double [B][4] = { n, mean, std, applied (1 or 0) } or NULL; mean = std = 0 for n = 0.
 * Reproducible bit for bit: nothing is added atomically, a window is summed in slices that depend on (H, W, bins, grid_dtype)
 * alone and the partial sums are combined in slice order, so two calls agree, and a window gives the same bits alone and at
 * any place of any batch.  Three launches; does not allocate, reads nothing back, does not wait for the device.
 * 1 <= B <= 65535, H, W >= 1, 1 <= bins <= EVREP_MAX_CHANNELS, H * W * bins < 2^31; grid, out, scratch (DEVICE,
 * evrep_voxel_normalize_scratch_bytes(B, H, W, bins) bytes; 0 for sizes the call refuses) and stats_out 16-byte aligned.
 * Anything else, a NULL pointer, an unknown dtype or flag bit is EVREP_EINVAL before any launch. */
#define EVREP_VOXNORM_NORMALIZE 1u
size_t evrep_voxel_normalize_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t bins);
int evrep_voxel_normalize(const void *grid, int32_t grid_dtype, int32_t B, int32_t H, int32_t W, int32_t bins, uint32_t flags,
                          float *out, double *stats_out, void *scratch, void *stream);

/* n_imagenet's per-polarity accumulators (n_imagenet/real_cnn_model/data/imagenet.py:169-511,841-871:
 * reshape_then_acc, _acc_time, _acc_count, _acc_count_pol, _acc_count_only, _acc_all, _flat, _flat_pol,
 * _acc_exp, _acc_time_pol, _acc_intensity) as ONE builder: channel c = stat[c] of the events of polarity
 * class pol[c] at each pixel.  pol: EVREP_PS_ANY (every event), EVREP_PS_POS (p > 0), EVREP_PS_NEG (p < 0).
 * stat: COUNT = torch.bincount (:187-189); TMAX / TMIN = torch_scatter.scatter_max / scatter_min of the
 * normalised time, 0 where empty (:203-206,236-239); FLAG = 1 where any event (:405-406); EXP =
 * exp(-(1 - TMAX)/tau) over the WHOLE frame, empty pixels included (:461-465); SIGNED = count(p>0) -
 * count(p<0) (:866).  tnorm DEVICE double [total_events] = (t - t[0]) / (t[-1] - t[0]) per window in
 * float64 (:180-181,198-199), indexed like `events`; the events' own t column is not used.
 * The window-level normalisations (count / count.max() :190-191, min-max of the intensity :867) are
 * the caller's.  out DEVICE (B,H,W,C) float32, C <= 16. */
#define EVREP_PS_ANY 0
#define EVREP_PS_POS 1
#define EVREP_PS_NEG 2
#define EVREP_PS_COUNT 0
#define EVREP_PS_TMAX 1
#define EVREP_PS_TMIN 2
#define EVREP_PS_FLAG 3
#define EVREP_PS_EXP 4
#define EVREP_PS_SIGNED 5
int evrep_polstats(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                   const double *tnorm, int32_t C, const int32_t *pol, const int32_t *stat, double tau, float *out,
                   void *stream);

/* EST quantisation layer, forward (ev-YOLOv6/yolov6/models/learned_repr.py:143-179): channel p*C + i of a
 * pixel = sum over its events of t_n * f(t_n - i/(C-1)), float32, events of a pixel added in time order (what
 * vox.put_(idx, values, accumulate=True) does on the CPU, :173).  f = the layer's value MLP (:9-43), a scalar
 * function of a scalar with LeakyReLU activations, i.e. EXACTLY piecewise linear: the caller passes it as
 * nseg segments {u_next, a, c} (f(u) = a*u + c for u below u_next, ascending, DEVICE double [nseg][3]) plus a
 * uniform bucket index over [lo, hi] (DEVICE uint32 [nbucket]: first segment that can contain the bucket's left
 * edge) -- built on the host from the MLP weights (event_representation_study_amd/est.py).
 * tnorm DEVICE float [total_events] = t / t.max() per window (:159-160), indexed like `events`; p > 0 selects
 * the second half of the channels (the layer expects p in {0, 1}).  out DEVICE (B,H,W,2C) float32, C <= 8. */
int evrep_est_voxel(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                    const float *tnorm, int32_t C, const double *segments, int32_t nseg, const uint32_t *buckets,
                    int32_t nbucket, double lo, double hi, float *out, void *stream);

/* The EST layer's backward with respect to its value MLP.  f(u) = a_k u + c_k on piece k, so for an upstream gradient
 * grad_out = dL/d out of evrep_est_voxel (DEVICE float (B,H,W,2C), contiguous)
 *   dL/da_k = sum over (event n, bin i) with piece(u_ni) = k of grad_out[b_n, y_n, x_n, p_n*C + i] * tn_n * u_ni
 *   dL/dc_k = the same sum of                                    grad_out[b_n, y_n, x_n, p_n*C + i] * tn_n
 * with u_ni = float32(tn_n - float32(i/(C-1))) and the piece chosen by the same walk as the forward.  Each term is formed
 * in float64 (G * tn exactly, then one rounding for * u) and summed in float64 in an order fixed by the library's source:
 * two calls on the same inputs give the same bits, and no floating-point atomic is used.  grad_seg DEVICE double [nseg][2]
 * {d/da, d/dc}, overwritten (pieces no event falls into hold 0).  The events are read in array order (x, y, p of the int32
 * rows; tnorm as for evrep_est_voxel; the stream is offsets[0] .. offsets[B]): no plan, no binning pass, no workspace.
 * Events outside the frame or with p not in {0, 1} contribute nothing; the events themselves get no gradient (t is data).
 * nseg <= EVREP_EST_BWD_MAX_SEG (the per-workgroup table of 2 * nseg doubles lives in LDS), 2 <= C <= 8.
 * scratch DEVICE, 16-byte aligned, evrep_est_backward_scratch_bytes(total_events, nseg) bytes with total_events >=
 * offsets[B] - offsets[0] (0 for arguments out of range); its contents need not be kept or cleared between calls.
 * Does not allocate, does not wait for the device, reads no size on the host. */
#define EVREP_EST_BWD_MAX_SEG 8192
size_t evrep_est_backward_scratch_bytes(int64_t total_events, int32_t nseg);
int evrep_est_voxel_backward(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W,
                             const float *tnorm, int32_t C, const double *segments, int32_t nseg,
                             const uint32_t *buckets, int32_t nbucket, double lo, double hi,
                             const float *grad_out, double *grad_seg, void *scratch, void *stream);

/* The EST layer's event preparation (learned_repr.py:145,159-160,164,170) for a stream that is already on the device.
 * events5 DEVICE float [n][5] rows [x, y, t, p, b], contiguous, 4-byte aligned, grouped by ascending batch index b.  Writes
 *   rows    DEVICE int32 [n][4] {trunc(x), trunc(y), 0, trunc(p)} (truncated toward zero as .long() does), 16-byte aligned:
 *           the `events` of evrep_est_voxel / evrep_est_voxel_backward;
 *   offsets DEVICE int64 [B+1], fully overwritten: offsets[k] = the number of events with b < k, so a batch index that never
 *           occurs and every index beyond the last event's come out as empty items;
 *   tnorm   DEVICE float [n]: t / (the maximum of t over the event's item), one correctly rounded float32 division.  A NaN
 *           time makes the whole item NaN (torch.max propagates it), an all-zero item is 0/0 = NaN as in the reference.  An
 *           item whose maximum is a zero while it also holds negative times takes +0 if both zeros occur;
 *   status  DEVICE uint32 [1], overwritten: an OR of the EVREP_EST_PREP_* bits over all events.  An event that sets a bit
 *           still gets its row and its tnorm, and nothing is written outside offsets[0..B] whatever b holds; with a bit set
 *           the other outputs are not meaningful.  The cost of the offsets is the sum of the upward jumps of b: B for a
 *           grouped stream.
 * The maxima are integer atomicMax operations on an order-preserving image of the float32 times: two calls on the same
 * input give the same bits, and no floating-point atomic is used.  n > 0, 1 <= B <= 65535 (what evrep_plan_init accepts),
 * H, W in 1..EVREP_MAX_DIM; anything else, a NULL pointer or a misaligned one is EVREP_EINVAL before any launch.  scratch
 * DEVICE, 4-byte aligned, evrep_est_prepare_scratch_bytes(n, B) bytes (0 for arguments out of range); it is cleared by the
 * call itself and need not be kept.  No plan, no workspace.  Does not allocate, does not wait for the device, reads no size
 * on the host. */
#define EVREP_EST_PREP_DESCENDING 1u    /* some b[i] < b[i-1]: the stream is not grouped by batch index */
#define EVREP_EST_PREP_BAD_INDEX 2u     /* some b negative, non-integral, non-finite or >= B */
#define EVREP_EST_PREP_BAD_POLARITY 4u  /* some p not exactly 0 or 1 */
#define EVREP_EST_PREP_OUT_OF_FRAME 8u  /* some trunc(x) outside [0, W) or trunc(y) outside [0, H), or x / y not finite */
size_t evrep_est_prepare_scratch_bytes(int64_t n, int32_t B);
int evrep_est_prepare(const float *events5, int64_t n, int32_t B, int32_t H, int32_t W, int32_t *rows, int64_t *offsets,
                      float *tnorm, uint32_t *status, void *scratch, void *stream);

/* Synchronous read-backs (they synchronise `stream`). status: HOST uint32 [B];
 * bbox: HOST int32 [B,4] = xmin, ymin, xmax, ymax of each window's in-frame events. */
int evrep_read_status(const evrep_plan *plan, const void *workspace, uint32_t *status, void *stream);
/* The same statistics WITHOUT a synchronisation: B records of 64 bytes {int32 tmin, tmax, xmin, xmax, ymin, ymax; uint32
 * neg_flags, oob_flags, status; int32 n_valid; 24 bytes reserved} are copied to meta_out (HOST, ideally pinned) behind the
 * work queued on `stream`; they are valid once the caller has synchronised the stream -- so a per-sample wrapper needs ONE
 * synchronisation for the status and the result together. */
int evrep_copy_window_meta_async(const evrep_plan *plan, const void *workspace, void *meta_out, void *stream);
int evrep_read_bbox(const evrep_plan *plan, const void *workspace, int32_t *bbox, void *stream);

/* Placement probe (no reference counterpart): writes zeros over `bytes` of `out` with the write footprint of the float64
 * 12-channel builder and nothing else.  On MI355X the physical placement of a ~1 GB output tensor decides up to 25 % of a
 * builder launch (NOTES.md section 8); a producer that allocates its output ring once can time this call into a few
 * candidate allocations and keep the fastest (engine.probe_output_placement does).  out DEVICE, 16-byte aligned. */
int evrep_probe_store(void *out, size_t bytes, void *stream);

/* OTMI(Xs, Xt, h).solve()[1] (representation_search/compute_otmi.py:61-93) in closed form for
 * POT's max_iter=0 path: mean over the LxL zero-padded grid of |Ks - Kt|.
 * Xs DEVICE double [n,ds], Xt DEVICE double [m,dt] (ds, dt <= 32); scratch DEVICE of
 * evrep_gwd_scratch_bytes(n, m), 256-byte aligned; cost DEVICE double [1].
 * Arithmetic: float64 statistics (mean and variance per dimension from the sums of x - row 0 and its square, so the score
 * does not depend on where a cloud sits: timestamps in microseconds need no rebasing; a cloud of one point or of equal points has
 * sigma = 0 and costs NaN, as in the reference); the pairwise exponents in float32 accuracy on the matrix cores -- clouds of <= 15
 * dimensions (both) as exact three-way bfloat16 splits of the float32 operands (v_mfma_f32_32x32x16_bf16), wider ones as
 * float32 MFMA chains; exponentials in float32; sums in float64.  Measured against the float64 value: 5e-9 relative on
 * uniform clouds of 1e4 points at h = 0.7; up to 9e-7 on clouds of two or three points; 6.8e-6 at worst (the split form at
 * h = 0.2 on a cloud a quarter of whose points agree in 12 of 14 columns; tests/test_gpu_gwd_edges.py, NOTES.md).  The
 * reference's budget is 1e-5. */
size_t evrep_gwd_scratch_bytes(int64_t n, int64_t m);
int evrep_gwd_padded_l1(const double *Xs, int64_t n, int32_t ds, const double *Xt, int64_t m, int32_t dt,
                        double h, void *scratch, double *cost, void *stream);

/* P solves at once: costs[p] = evrep_gwd_padded_l1 of the pair p, bit for bit, in six launches for ALL pairs (a single
 * solve is five launches, four of them tiny).  The clouds' sizes are read on the DEVICE, so pairs produced by
 * evrep_otmi_event_clouds / evrep_otmi_rep_clouds are scored without a host read-back.
 * Xs DEVICE double: pair p's source cloud = rows [xs_row[p], xs_row[p] + n[p]) of ds columns (xs_row NULL: p * n_cap);
 * likewise Xt / xt_row / m / dt.  xs_row, n, xt_row, m DEVICE int64 [P].  n_cap, m_cap: upper bounds of n[p], m[p]
 * (they size the scratch slots; a pair beyond them, or with an empty cloud, costs NaN).  All pairs share ds, dt, h.
 * scratch DEVICE of evrep_gwd_batch_scratch_bytes; costs DEVICE double [P]. */
size_t evrep_gwd_batch_scratch_bytes(int32_t P, int32_t ds, int32_t dt, int64_t n_cap, int64_t m_cap);
int evrep_gwd_padded_l1_batch(int32_t P, const double *Xs, const int64_t *xs_row, const int64_t *n, int32_t ds,
                              const double *Xt, const int64_t *xt_row, const int64_t *m, int32_t dt, int64_t n_cap,
                              int64_t m_cap, double h, void *scratch, double *costs, void *stream);

/* The point clouds of the harness otmi(events, rep, height, width, rep_size)
 * (representation_search/compute_otmi.py:96-211), built on the device in the reference's own order.
 * evrep_otmi_event_clouds: events DEVICE int32 [total,4] + offsets DEVICE int64 [B+1] (B windows) -> for window b the
 *   three scored sensor quadrants (the most populated one is skipped, :134-135; quadrants 2-4 re-origined, :140-147;
 *   float32 x / ((W-1)//2), y / ((H-1)//2), (t - t0) / (t1 - t0), (p - pmin) / (pmax - pmin), rows with
 *   x < (W-1)//2 and y < (H-1)//2 kept, :164-173): Xs DEVICE double [B][3][cap][4], n_out DEVICE int64 [B][3],
 *   quad_out DEVICE int32 [B][3] (which quadrant each slot holds).  cap >= the longest window.
 *   Held to the reference's arithmetic at its edges (tests/test_gpu_otmi_edges.py):
 *   - an event outside the frame (x < 0, x >= W, y < 0, y >= H, any int32) belongs to no quadrant; the column x = W/2 - 1
 *     is the last one on the left, so with an odd W the middle column is on the right (likewise rows);
 *   - among equally populated quadrants the FIRST one is skipped (all four of an empty window: quadrant 0);
 *   - a scored quadrant without an event gives n_out = 0 and the rows of its slot are not written (the reference raises
 *     there; a cost formed from such a slot is NaN);
 *   - t0 and t1 are the quadrant's first and last member in ARRAY order and the differences are taken in int64 before
 *     the float32 rounding, so any int32 timestamps and polarities, descending or unsorted ones included, divide as in
 *     the reference: a quadrant of one timestamp (or one event) has NaN in the t column, one of a single polarity NaN in
 *     the p column (0 / 0), and with t0 == t1 among other timestamps the column holds +inf, -inf and NaN;
 *   - H = 2 or W = 2 keeps no row ((W-1)//2 = 0): n_out = 0 in all three slots.
 * evrep_otmi_rep_clouds: rep DEVICE (items, S, S, C) letterboxed representations, item i belongs to window i % B ->
 *   for slot k the cut of quadrant quad[i % B][k] (:150-155,177-179), two positional channels (:181-198), rows with
 *   sum |feat| > 0 (:200-202): Xt DEVICE double [items][3][m_cap][C+2], m_out DEVICE int64 [items][3];
 *   m_cap >= (S - S/2 + 1)^2.
 * Both cut their input into slices, one workgroup each, that meet through `scratch`: DEVICE, 16-byte aligned, of
 * evrep_otmi_scratch_bytes(B) / evrep_otmi_scratch_bytes(items) bytes (no initialisation needed). */
size_t evrep_otmi_scratch_bytes(int32_t windows_or_items);
int evrep_otmi_event_clouds(const int32_t *events, const int64_t *offsets, int32_t B, int32_t height, int32_t width,
                            int64_t cap, double *Xs, int64_t *n_out, int32_t *quad_out, void *scratch, void *stream);
int evrep_otmi_rep_clouds(const void *rep, int32_t rep_dtype, int32_t items, int32_t B, int32_t S, int32_t C,
                          const int32_t *quad, int64_t m_cap, double *Xt, int64_t *m_out, void *scratch, void *stream);

/* One step of the representation search (representation_search/optimization.py:116-304): the clouds of n_cand candidate
 * stacks that differ in ONE channel, without materialising them.
 * base DEVICE (B, S, S, C): the letterboxed stack of the channels chosen so far (the others as the reference leaves them:
 *   zeros inside the image, 114 in the letterbox rows); bank DEVICE (B, S, S, R): R letterboxed candidate channels,
 *   channel-last; both of `dtype` (EVREP_F64 / EVREP_F32).  cand HOST int32 [n_cand], each in [0, R) (repeats allowed;
 *   read before the call returns).
 * Item i = j * B + b is candidate cand[j] on window b: base[b, y, x, :] with channel `slot` replaced by
 *   bank[b, y, x, cand[j]].  Xt DEVICE double [items][3][m_cap][C+2] and m_out DEVICE int64 [items][3] receive exactly
 *   what evrep_otmi_rep_clouds writes for these items = n_cand * B representations (quadrant cuts by quad, positional
 *   channels, rows with sum |feat| > 0 and no NaN, STABLE order; rows from m_out on are left untouched).
 * scratch DEVICE, 16-byte aligned, of evrep_otmi_scratch_bytes(items).  EVREP_EINVAL before any launch for a null
 *   pointer, slot outside [0, C), a cand[j] outside [0, R), items > 65535, C + 2 > 32, S < 4, a misaligned scratch. */
int evrep_otmi_rep_clouds_bank(const void *base, const void *bank, int32_t dtype, int32_t B, int32_t S, int32_t C, int32_t R,
                               int32_t slot, const int32_t *cand, int32_t n_cand, const int32_t *quad, int64_t m_cap,
                               double *Xt, int64_t *m_out, void *scratch, void *stream);

/* Per-channel resize of a channel-last representation (B,H,W,C) -> (B,Ho,Wo,C), what resize_image /
 * resize_image_process do with cv2.resize per channel before a representation is stored or scored
 * (ev-YOLOv6/yolov6/data/gen4/precompute_reps.py:179-260,424; gen1_2yolo.py:230-265).  The interpolation is given as
 * separable tap tables: output row oy = sum_{t < ycount[oy]} ywt[oy*T + t] * (source row ystart[oy] + t), likewise
 * for columns -- built on the host from OpenCV's published INTER_AREA / INTER_LINEAR table construction
 * (event_representation_study_amd/gwd_pipeline.py; parity unpinned against cv2, which is absent).
 * in DEVICE float64/float32 (in_dtype); tap tables DEVICE; out DEVICE float64/float32 (out_dtype: the reference stores
 * float32, precompute_reps.py:434), every value times `scale`. */
int evrep_resize_taps(const void *in, int32_t in_dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                      int32_t T, const int32_t *ystart, const int32_t *ycount, const double *ywt, const int32_t *xstart,
                      const int32_t *xcount, const double *xwt, double scale, int32_t out_dtype, void *out, void *stream);

/* EXTENSION (no live call of the reference computes this): entropic Gromov-Wasserstein by
 * projected gradient, restated from POT's published ot.gromov.entropic_gromov_wasserstein (init_matrix,
 * tensor_product, gwggrad, gwloss, sinkhorn_knopp) with FIXED iteration counts instead of its tolerance tests --
 * the solver family of the reference's dead-code call ot.gromov.gromov_wasserstein(Ks, Kt, p, q, "kl_loss")
 * (representation_search/gromov_wasserstein.py:62-69).  PARITY UNPINNED against POT (absent); checked against
 * oracle/gw_oracle.py.
 * C1 DEVICE double [n,n], C2 DEVICE double [m,m], p DEVICE double [n], q DEVICE double [m];
 * loss 0 = "square_loss", 1 = "kl_loss"; precision EVREP_F64 (v_mfma_f64_16x16x4_f64) or EVREP_F32
 * (v_mfma_f32_16x16x4_f32; plan and Gibbs kernel in float32, Sinkhorn scalings in float64);
 * scratch DEVICE of evrep_gw_scratch_bytes(n, m, precision); T_out DEVICE double [n,m] or NULL; gw_out DEVICE double [1].
 * C1 and C2 need not be symmetric: C1[i][k] and C2[j][l] are read row-major as given, and T_out[i][j] couples point i of the
 * first space with point j of the second.  A point of zero mass (p[i] == 0 or q[j] == 0) gives a row or column of T_out that
 * is exactly 0 and does not influence gw or the rest of the plan: both equal those of the problem without the point.  With
 * zeros in BOTH marginals POT's published recurrence yields NaN (it forms (1 / p) * K, a row of inf, and multiplies it by the
 * zero scaling of a zero-mass column); this solver computes u = p / (K v) and stays finite, with the same zero rows and columns.
 * outer_iters == 0 is accepted: T_out is then p q^T and gw the loss of that product plan. */
size_t evrep_gw_scratch_bytes(int64_t n, int64_t m, int32_t precision);
int evrep_entropic_gw(const double *C1, int64_t n, const double *C2, int64_t m, const double *p, const double *q,
                      int32_t loss, double epsilon, int32_t outer_iters, int32_t sinkhorn_iters, int32_t precision,
                      void *scratch, double *T_out, double *gw_out, void *stream);

/* The ev-licious event filters (ev-licious/src/evlicious/tools/filters.py:23-109, tools/utils.py:110-200) on the device.
 * Every filter writes keep DEVICE uint8 [total_events]: one byte per event in ARRAY order, 1 = the event passes; an event
 * outside the frame (the reference raises IndexError) is dropped and touches no state.  `state` DEVICE [B,H,W] is the
 * reference's per-pixel state array: read as the incoming state, overwritten with the outgoing one, so successive windows of
 * one recording chain calls; the windows of one batch are independent.  t_base HOST int64 [B]: the absolute time of t == 0
 * of each window's int32 t column (NULL: 0); it is copied with hipMemcpyAsync into the workspace (the slot evrep_time_surface
 * keeps its cuts in during a call): a PAGEABLE array is staged by the HIP runtime before the call returns and may be released
 * then (the call may wait for that staging); a PINNED array must stay unchanged until `stream` has reached the copy.  All of
 * them need a plan whose binning pass has run on this workspace.  The library cannot tell (a plan is read-only host data, so
 * EVREP_ENOTBINNED is not returned): on an unbinned or foreign workspace the result is UNDEFINED -- where the kernels find
 * the stream's offsets inconsistent with the window they leave every event dropped and the state untouched.  They give the
 * same mask under every binning pass; after the key-sorted pass (reserved == 2) they run the per-key column sort first.
 *
 * evrep_filter_pixel_fsm: the sequential per-pixel filters, `kind`:
 *   EVREP_FILTER_REFRACTORY  RefractoryPeriod (utils.py:193-200): an event passes iff t - last >= param (the period), and only
 *                            a passing event sets last = t.  state float64, absolute time, -inf at rest.
 *   EVREP_FILTER_CONTRAST    ContrastThresholdIncrease (utils.py:184-191): activity += p; passes iff |activity| >= param (the
 *                            factor), then activity = 0.  state int32.  The reference's Events hold p in {-1, +1}.
 *   EVREP_FILTER_CHANGE_MAP  resize_to_resolution's change map (utils.py:143-158) over a batch of CELL coordinates
 *                            (evrep_filter_cell_map): change += p * 1.0 / param (param = fx * fy; float64 sum rounded to float32),
 *                            passes iff |change| >= 1, then change -= p.  state float32.
 *   param must be > 0.  t_base is only read by EVREP_FILTER_REFRACTORY.
 * evrep_filter_background: BackgroundActivity (utils.py:170-179): event i is dropped iff t_last > 0 and t - t_last > depth with
 *   t_last = timestamps[y, x] before the update; every event then writes t into rows [max(y - r, 0), y + r), columns
 *   [max(x - r, 0), x + r).  Evaluated in closed form: t_last = t of the latest earlier event j (array order) with
 *   x - r + 1 <= x_j <= x + r and y - r + 1 <= y_j <= y + r, else the incoming state.  1 <= radius <= EVREP_FILTER_MAX_RADIUS,
 *   depth > 0.  state float64 [B,H,W] in / out = the reference's `timestamps`, absolute time, -inf at rest.
 * evrep_filter_mask_gather: HotPixel.insert (filters.py:53): keep[i] = mask[b, y, x] != 0; mask DEVICE uint8 [B,H,W].
 * evrep_filter_cell_map: events_out[i] = (x // fx, y // fy, t, p), the cells of resize_to_resolution (utils.py:150-151);
 *   out-of-frame events get (-1, -1).  events_out DEVICE int32 [total,4].
 * evrep_filter_compact: STABLE compaction of the kept rows of all B windows: events_out DEVICE int32 [>= kept,4] (total rows
 *   always suffice), offsets_out DEVICE int64 [B+1]; the sizes are read on the device, nothing returns to the host.  scratch
 *   DEVICE of evrep_filter_compact_scratch_bytes(B, total) bytes, 16-byte aligned, no initialisation needed. */
#define EVREP_FILTER_REFRACTORY 0
#define EVREP_FILTER_CONTRAST 1
#define EVREP_FILTER_CHANGE_MAP 2
#define EVREP_FILTER_MAX_RADIUS 4
int evrep_filter_pixel_fsm(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t kind,
                           double param, const int64_t *t_base, void *state, uint8_t *keep, void *stream);
int evrep_filter_background(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, double depth,
                            int32_t radius, const int64_t *t_base, double *state, uint8_t *keep, void *stream);
int evrep_filter_mask_gather(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W,
                             int64_t max_events_per_window, const uint8_t *mask, uint8_t *keep, void *stream);
int evrep_filter_cell_map(const int32_t *events, int64_t total, int32_t H, int32_t W, int32_t fy, int32_t fx, int32_t *events_out,
                          void *stream);
size_t evrep_filter_compact_scratch_bytes(int32_t B, int64_t total);
int evrep_filter_compact(const int32_t *events, const int64_t *offsets, int32_t B, const uint8_t *keep, int32_t *events_out,
                         int64_t *offsets_out, void *scratch, void *stream);

/* Windows cut from a DEVICE-RESIDENT recording (ev-licious/src/evlicious/io/h5_event_handle.py:10-11,52-103,
 * io/utils/event_handle.py:51-58; ev-YOLOv6/yolov6/data/gen1_2yolo.py:186-198).  The recording is uploaded once as the
 * structure-of-arrays columns ev-licious' Events hold (io/utils/events.py:7-8): x, y uint16, t int64 ascending, p int8, n
 * events.  Neither call takes a plan or a workspace, allocates, or waits for the device.
 *
 * evrep_time_to_index: out_idx[k] = the first index i with t[i] > queries[k], n if there is none -- numpy's
 *   searchsorted(t, q, side="right"); with q = ceil(q' + 1e-3) - 1 this is the reference's searchsorted(t, q' + 1e-3) on
 *   integral microsecond times, ties included.  t DEVICE int64 [n], queries DEVICE int64 [nq], out_idx DEVICE int64 [nq].
 *   One wavefront per query, a 64-ary search of ceil(log64 n) rounds.  nq <= EVREP_WINDOWS_MAX_QUERIES.
 * evrep_windows_gather: B source ranges [i0[b], i1[b]) -- they may overlap, repeat or be empty -- into packed int32 rows:
 *   events_out[dst_offsets[b] + k] = (x[i0[b] + k], y[..], t[..] - base[b], p[..]), rows [dst_offsets[0], dst_offsets[B]).
 *   i0, i1 DEVICE int64 [B]; dst_offsets DEVICE int64 [B+1], ascending, dst_offsets[b+1] - dst_offsets[b] = i1[b] - i0[b];
 *   events_out DEVICE int32 [>= dst_offsets[B], 4], 16-byte aligned.  rebase_mode: EVREP_REBASE_NONE base = 0;
 *   EVREP_REBASE_FIRST base[b] = t[i0[b]] (Gen1's _load_events; 0 for an empty window); EVREP_REBASE_GIVEN base[b] =
 *   base_in[b], DEVICE int64 [B] (NULL otherwise).  base_out DEVICE int64 [B] receives base[b]; status_out DEVICE uint32 [B]
 *   receives EVREP_WST_* bits (cleared by the call).  p is copied as stored.  B <= EVREP_WINDOWS_MAX_B.
 *   EVREP_WST_BAD_RANGE: i0 < 0, i0 > i1 or i1 > n -- nothing of that window is read or written.
 *   EVREP_WST_T_OVERFLOW: some t - base[b] is outside int32; those rows are written SATURATED (INT32_MAX / INT32_MIN).
 *   EVREP_WST_BAD_OFFSETS: dst_offsets gives the window more rows than its range holds; the surplus rows are not written. */
#define EVREP_REBASE_NONE 0
#define EVREP_REBASE_FIRST 1
#define EVREP_REBASE_GIVEN 2
#define EVREP_WST_BAD_RANGE 1u
#define EVREP_WST_T_OVERFLOW 2u
#define EVREP_WST_BAD_OFFSETS 4u
#define EVREP_WINDOWS_MAX_QUERIES (1 << 30)
#define EVREP_WINDOWS_MAX_B (1 << 24)
int evrep_time_to_index(const int64_t *t, int64_t n, const int64_t *queries, int64_t nq, int64_t *out_idx, void *stream);
int evrep_windows_gather(const uint16_t *x, const uint16_t *y, const int64_t *t, const int8_t *p, int64_t n, const int64_t *i0,
                         const int64_t *i1, const int64_t *dst_offsets, int32_t B, int32_t rebase_mode, const int64_t *base_in,
                         int32_t *events_out, int64_t *base_out, uint32_t *status_out, void *stream);

/* Raw event files decoded on the device into the columns of a recording (x, y uint16, t int64, p int8): Prophesee DAT
 * records (ev-licious/src/evlicious/io/utils/prophesee_utils.py:8-61: a uint32 timestamp and a uint32 word holding x in bits
 * 0-13, y in bits 14-27, p in bit 28, bits 29-31 ignored; 8 bytes for event types 0 and 12, 28 for type 40, whose further
 * fields are skipped) and the 5-byte records of N-Caltech / N-MNIST (io/bin_event_handle.py:37-51: x = b0, y = b1, p = bit 7
 * of b2, t = (b2 & 127) << 16 | b3 << 8 | b4).  p is +1 where the bit is set and -1 otherwise; t is zero-extended, never
 * negative.  No call allocates or waits for the device; every result of the checks stays on the device.
 *
 * evrep_decode_state: eight int64 fields a FILE accumulates over the calls that decode its chunks, one behind the other on
 *   one stream.  n_in: records seen (bit EVREP_DECODE_N_IN_OVERRUN: some call found n_out + its records > capacity; that
 *   call and every later one write nothing and leave n_out as it is, the checks still run).  n_out: records written; a call
 *   writes its columns at [n_out, ...).  oob_count / oob_first: records with x >= W or y >= H, and the file index of the
 *   first (-1: none).  desc_count / desc_first: records whose t is smaller than their predecessor's in the RAW record order,
 *   across chunk joints too, and the file index of the first (-1: none).  t_first, t_last: t of the first and of the last
 *   RAW record (-1: no record yet).  evrep_decode_state_init starts a file (one launch).
 * evrep_decode_dat: n records of `stride` bytes (a multiple of 4, >= 8) at raw, DEVICE, 16-byte aligned.  first_index: the
 *   index record 0 has in the file (oob_first and desc_first are file indices).  x, y, t, p DEVICE, 16-byte aligned,
 *   `capacity` entries each.  flags: EVREP_DECODE_STRICT -- every record is written, out-of-frame ones are counted only;
 *   EVREP_DECODE_DROP_OOB -- out-of-frame records are left out, the others keep their order (a count launch, one scan
 *   workgroup, a write launch; with nothing dropped the columns equal the strict ones).  scratch DEVICE, 256-byte aligned,
 *   evrep_decode_scratch_bytes(n) bytes, needed by DROP_OOB only (NULL otherwise); it is free again when the call's
 *   launches have run.  n <= EVREP_DECODE_MAX_N.  With stride 8 a lane decodes 16 records whose output index starts at a
 *   multiple of 16: 16-byte loads (8-byte where n_out is odd) and 16-byte stores of every column.
 * evrep_decode_bin5: the same for 5-byte records.  raw must be readable up to the next multiple of 16 bytes behind the last
 *   record: the payload is read in whole aligned 16-byte pieces.
 * evrep_dat_seek_time: EventBaseReader.seek_time(queries[k], term) (prophesee_utils.py:367-418) on the ascending t DEVICE
 *   int64 [n] -> out_idx[k], the reader's record position: n for a query above t[n-1], 0 for a query <= 0; otherwise bisect
 *   [0, n) while more than `term` records remain -- a probe t[middle] EQUAL to the query ends at middle + 1, which need not be
 *   the first record with that timestamp -- and then take the first record of the remaining range with t >= query.  One
 *   wavefront per query.  term >= 1, nq <= EVREP_WINDOWS_MAX_QUERIES. */
typedef struct evrep_decode_state {
    int64_t n_in, n_out, oob_count, oob_first, desc_count, desc_first, t_first, t_last;
} evrep_decode_state;
#define EVREP_DECODE_STRICT 0u
#define EVREP_DECODE_DROP_OOB 1u
#define EVREP_DECODE_N_IN_OVERRUN (1ll << 62)
#define EVREP_DECODE_MAX_N (1ll << 30)
size_t evrep_decode_scratch_bytes(int64_t n);
int evrep_decode_state_init(evrep_decode_state *state, void *stream);
int evrep_decode_dat(const void *raw, int64_t n, int32_t stride, int64_t first_index, int32_t H, int32_t W, uint32_t flags,
                     uint16_t *x, uint16_t *y, int64_t *t, int8_t *p, int64_t capacity, evrep_decode_state *state, void *scratch,
                     void *stream);
int evrep_decode_bin5(const void *raw, int64_t n, int64_t first_index, int32_t H, int32_t W, uint32_t flags, uint16_t *x,
                      uint16_t *y, int64_t *t, int8_t *p, int64_t capacity, evrep_decode_state *state, void *scratch, void *stream);
int evrep_dat_seek_time(const int64_t *t, int64_t n, const int64_t *queries, int64_t nq, int64_t term, int64_t *out_idx,
                        void *stream);

/* N-ImageNet's event front end and base_augment on the device (n_imagenet/real_cnn_model/data/imagenet.py: load_event :30-57,
 * reshape_event_no_sample :104-108, slice_event :60-84, base_augment("train") :1140-1187), for the B windows of a batch in one
 * call: a count launch, one scan workgroup, a write launch.  The call takes no plan and no workspace, neither allocates nor
 * waits for the device, and reads every size on the device.
 *
 * evrep_nimg_prepare: events DEVICE int32 [total,4] rows (x, y, t - base, p as stored), 16-byte aligned -- what
 *   evrep_windows_gather writes --; offsets DEVICE int64 [B+1], ascending; t_base DEVICE int64 [B], the absolute time of t == 0
 *   per window (NULL: 0); params DEVICE evrep_nimg_params [B].  Per row of window b, every step the reference's float64
 *   operation as one IEEE operation:
 *     time      t_s = (double)(t_base[b] + t) / 1e6                                                       (:51)
 *     polarity  EVREP_NIMG_P_UINT8: p is first read as load_event reads it, through uint8 (p & 0xFF)        (:36)
 *               if the minimum of p over the WHOLE window (before any slice) is >= -0.5: every p <= 0.5 becomes -1   (:54-55)
 *     reshape   x_f = (double)x * sx, y_f = (double)y * sy (sx = new_w / orig_w, sy = new_h / orig_h; 1.0 without)  (:105-106)
 *     slice     rows [s0, s1) of the window AND the strict t_s > t_lo && t_s < t_hi (-inf / +inf when unused)  (:65,69,82)
 *     time flip EVREP_AUG_TIME_FLIP: the sliced rows leave in reverse order, t' = T - t_s with T the t_s of the last sliced
 *               row (taken before the crop), p' = -p                                                       (:1168-1172)
 *     x flip    EVREP_AUG_X_FLIP: x' = (img_w - 1) - x_f                                                   (:1161)
 *     shift     EVREP_NIMG_TRAIN only: x'' = x' + x_shift, y'' = y_f + y_shift; the row is kept iff 0 <= x'' < img_w and
 *               0 <= y'' < img_h.  Without EVREP_NIMG_TRAIN (augment=None) nothing is shifted or cropped.  (:1143-1152)
 *   Per kept row, in output order: events_out DEVICE int32 [>= total,4] = (trunc x'', trunc y'', 0, sign p'); t_out DEVICE
 *   double [>= total] = t'; tnorm_out DEVICE double [>= total] = (t' - t'_first) / (t'_last - t'_first) over the window's first
 *   and last output rows (:198-199); xy_out DEVICE double [>= total,2] or NULL = (x'', y'') untruncated, 16-byte aligned.
 *   Per window: offsets_out DEVICE int64 [B+1]; status_out DEVICE uint32 [B], EVREP_AUG_* bits:
 *     EVREP_AUG_EMPTY      no row kept;
 *     EVREP_AUG_FLAT_TIME  t'_last == t'_first: tnorm is NaN there, as the reference's is;
 *     EVREP_AUG_BAD_SLICE  s0 < 0, s0 > s1 or s1 > the window's rows: nothing of the window is read, no row is kept.
 *   scratch DEVICE of evrep_nimg_prepare_scratch_bytes(B, total) bytes, 16-byte aligned, no initialisation needed.
 *   A window holds fewer than 2^31 rows, the batch fewer than 2^32; B <= EVREP_NIMG_MAX_B. */
typedef struct evrep_nimg_params {
    int64_t s0, s1;          /* index slice [s0, s1) of the window's rows */
    double t_lo, t_hi;       /* strict time slice in seconds */
    int32_t x_shift, y_shift;
    uint32_t flags;          /* EVREP_AUG_TIME_FLIP | EVREP_AUG_X_FLIP */
    uint32_t reserved;
} evrep_nimg_params;
#define EVREP_NIMG_TRAIN 1u
#define EVREP_NIMG_P_UINT8 2u
#define EVREP_AUG_TIME_FLIP 1u
#define EVREP_AUG_X_FLIP 2u
#define EVREP_AUG_EMPTY 1u
#define EVREP_AUG_FLAT_TIME 2u
#define EVREP_AUG_BAD_SLICE 4u
#define EVREP_NIMG_MAX_B (1 << 24)
size_t evrep_nimg_prepare_scratch_bytes(int32_t B, int64_t total);
int evrep_nimg_prepare(const int32_t *events, const int64_t *offsets, int32_t B, const int64_t *t_base, const evrep_nimg_params *params,
                       double sx, double sy, int32_t img_h, int32_t img_w, uint32_t mode, int32_t *events_out, double *t_out,
                       double *tnorm_out, double *xy_out, int64_t *offsets_out, uint32_t *status_out, void *scratch, void *stream);

/* N-ImageNet's DiST image (n_imagenet/real_cnn_model/data/imagenet.py:873-999, reshape_then_acc_adj_sort) for B windows in one
 * call of three launches, and the dense rank it ends in.  Neither call takes a plan or a workspace, allocates, waits for the
 * device or reads a size on the host: both may be captured into a graph.
 *
 * evrep_dist: prim DEVICE float [B,H,W,6], what evrep_polstats writes for pol = {POS, POS, POS, NEG, NEG, NEG}, stat = {COUNT,
 *   TMAX, TMIN, COUNT, TMAX, TMIN}; out DEVICE float [B,2,H,W], channel 0 positive, channel 1 negative.  Per (window, polarity)
 *   image, every step the reference's float32 statement as one IEEE operation (divisions correctly rounded, no FMA):
 *     clip     th = #{ j : S_j < H*W*clip_rate }, S_j the running number of pixels over the DISTINCT count values in ascending
 *              order; the float64 product and S_j are compared in float32, as torch compares an int64 tensor with a Python
 *              float; count = min(count, th).  Exact for any counts.                                           (:897-906)
 *     stencil  earliest = 1 where count == 0; s = 5x5 sum of count, zero padding; nb = 25 * (s / 25);
 *              disc = (max5x5(latest) + max5x5(-earliest)) / nb, -inf padding; where count > 0: latest -= alpha * disc;
 *              latest < 0 -> 0; nb == 1 -> 0.                                                                    (:926-968)
 *     rank     out = #{distinct values < latest} / #{distinct values} over the image, +0.0 and -0.0 one value.   (:970-990)
 *   clip_rate >= 0 (the reference: 0.99), alpha (the reference: 3.0).  scratch DEVICE of evrep_dist_scratch_bytes(B, H, W) bytes,
 *   16-byte aligned, no initialisation needed.  B <= EVREP_DIST_MAX_B; H, W <= EVREP_MAX_DIM.  A NaN in prim (a window whose
 *   events share one timestamp) is ranked as its bit pattern orders it, which is not what the reference's sort does.
 * evrep_dense_rank_f32: S segments of float32 keys, segment s = keys [seg_offsets[s], seg_offsets[s+1]); out[i] =
 *   #{distinct keys of i's segment < keys[i]} / #{distinct keys of the segment}, one correctly rounded float32 division.
 *   seg_offsets DEVICE int64 [S+1], ascending from seg_offsets[0] >= 0 (a segment may be empty; one whose offsets descend or
 *   pass seg_offsets[S] is left alone); keys, out DEVICE float [>= seg_offsets[S]]; n_distinct_out DEVICE int32 [S] or NULL;
 *   scratch DEVICE of evrep_dense_rank_scratch_bytes(S, total) bytes with total >= seg_offsets[S], 16-byte aligned.  One
 *   workgroup per segment (a stable radix sort of (key, index) pairs through the scratch), so it is meant for many segments of
 *   up to a few hundred thousand keys; a segment holds fewer than 2^32 keys.  S <= EVREP_RANK_MAX_SEGMENTS.
 * The *_scratch_bytes functions return 0 for arguments the calls refuse. */
#define EVREP_DIST_MAX_B (1 << 20)
#define EVREP_RANK_MAX_SEGMENTS (1 << 24)
#define EVREP_RANK_MAX_TOTAL ((int64_t)1 << 40)
size_t evrep_dist_scratch_bytes(int32_t B, int32_t H, int32_t W);
int evrep_dist(const float *prim, int32_t B, int32_t H, int32_t W, double clip_rate, float alpha, float *out, void *scratch,
               void *stream);
size_t evrep_dense_rank_scratch_bytes(int32_t S, int64_t total);
int evrep_dense_rank_f32(const float *keys, const int64_t *seg_offsets, int32_t S, float *out, int32_t *n_distinct_out,
                         void *scratch, void *stream);

/* N-ImageNet's sorted timestamp image (n_imagenet/real_cnn_model/data/imagenet.py:513-838, reshape_then_acc_sort) for B windows:
 * the time index per event in front of evrep_polstats, and the image statements behind it.  Neither call takes a plan or a
 * workspace, allocates, waits for the device or reads a size on the host: both may be captured into a graph.
 *
 * evrep_time_index: t DEVICE double [>= offsets[B]], the events' times in seconds, indexed like the batch's events; offsets DEVICE
 *   int64 [B+1], ascending.  Per event idx = (int64)(t * 1e6): one IEEE float64 multiply and a truncation, as
 *   (event_tensor[:, 2] * TIME_SCALE).long() does (:522,528).  out DEVICE double [>= offsets[B]] receives
 *     EVREP_TIME_INDEX_RAW   (double)idx;
 *     EVREP_TIME_INDEX_RANK  the consecutive dense rank of idx inside its window, torch.unique_consecutive +
 *                            repeat_interleave(arange) (:523-524): the number of positions j <= i of the window, its first
 *                            excepted, with idx[j] != idx[j-1].  The count restarts at every window.
 *   status_out DEVICE uint32 [B] is overwritten with EVREP_SORT_EMPTY (the window has no event) and EVREP_SORT_DECREASING (idx
 *   falls somewhere inside the window: the consecutive rank is a dense rank only where it never does).  Three launches (count,
 *   one scan workgroup, write) with several workgroups per window; scratch DEVICE of evrep_time_index_scratch_bytes(B, total)
 *   bytes, total >= offsets[B] - offsets[0], 16-byte aligned, no initialisation needed.  The batch holds fewer than 2^32 events;
 *   B <= EVREP_SORT_MAX_B.
 * evrep_sort_image: prim DEVICE float [B,H,W,2K], what evrep_polstats writes for K = 1: pol {ANY, ANY} or K = 2: pol {POS, POS,
 *   NEG, NEG}, stat {FLAG, TMAX} per class, with the output of evrep_time_index as its per-event value.  out DEVICE float
 *   [B,C,H,W] in the reference's channel order: per class [FLAG if EVREP_SORT_USE_IMAGE] + the sort channel, nq > 0: once per
 *   quantize[c] (HOST int32 [nq], every value > 0, nq <= EVREP_SORT_MAX_Q); C = K * (use_image + max(nq, 1)).  One workgroup per
 *   (window, class).
 *     without EVREP_SORT_STRICT  sort = TMAX as it is, in every quantised copy too (the reference's float64 round(v * q) / q of
 *                 an integer v returns v).  A class without a pixel whose TMAX is > 0 ORs EVREP_SORT_NO_INDEX << class into
 *                 status[window]: the reference's hot_event_sort.max() raises there (:597-599).
 *     with EVREP_SORT_STRICT     hot = pixels with FLAG; U = distinct TMAX among them; rank = distinct TMAX below the pixel's own;
 *                 sort = (float)rank / (float)(U - 1), one correctly rounded division, at hot pixels, 0 elsewhere and everywhere
 *                 when U == 1 (:571-592); per q: round_half_even(sort * (float)q) / (float)q as separate float32 operations.  A
 *                 class without events is the reference's one event at pixel (0, 0) (:650-655): FLAG set there, sort zero, no
 *                 status bit.  TMAX must be exact in float32: pass the RANK form of evrep_time_index, windows below 2^24 events.
 *   status DEVICE uint32 [B] is OR-ed into (zero it, or pass what evrep_time_index wrote).  scratch DEVICE of
 *   evrep_sort_image_scratch_bytes(B, H, W, K) bytes, 16-byte aligned, no initialisation needed.
 * The *_scratch_bytes functions return 0 for arguments the calls refuse. */
#define EVREP_TIME_INDEX_RAW 0
#define EVREP_TIME_INDEX_RANK 1
#define EVREP_SORT_EMPTY 1u
#define EVREP_SORT_DECREASING 2u
#define EVREP_SORT_NO_INDEX 4u /* << class: 4 the first (ANY or POS), 8 the second (NEG) */
#define EVREP_SORT_STRICT 1u
#define EVREP_SORT_USE_IMAGE 2u
#define EVREP_SORT_MAX_B (1 << 20)
#define EVREP_SORT_MAX_Q 16
size_t evrep_time_index_scratch_bytes(int32_t B, int64_t total);
int evrep_time_index(const double *t, const int64_t *offsets, int32_t B, int32_t mode, double *out, uint32_t *status_out,
                     void *scratch, void *stream);
size_t evrep_sort_image_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t K);
int evrep_sort_image(const float *prim, int32_t B, int32_t H, int32_t W, int32_t K, uint32_t flags, const int32_t *quantize,
                     int32_t nq, float *out, uint32_t *status, void *scratch, void *stream);

/* The rows the study's own representations are built from, out of what evrep_nimg_prepare leaves: the host step of n_imagenet's
 * reshape_then_optimized / reshape_then_event_stack / reshape_then_tore (imagenet.py:1025-1107) in front of evrep_optimized,
 * evrep_event_stack and evrep_tore_ftime, for the B windows of a batch.  One memset and two launches (a reduction per window over
 * several workgroups, a write pass); no plan, no workspace, no allocation, nothing waits for the device or reads a size on the
 * host: the call may be captured into a graph.
 *
 * evrep_nimg_study_rows: rows DEVICE int32 [>= offsets[B],4] = (trunc x, trunc y, 0, sign p), 16-byte aligned; t DEVICE double
 *   [>= offsets[B]], seconds; xy DEVICE double [>= offsets[B],2], the untruncated coordinates, 16-byte aligned (read for
 *   EVREP_STUDY_TORE only, else it may be NULL); offsets DEVICE int64 [B+1], ascending.  want: which row sets are written
 *   (EVREP_STUDY_MDES | _STACK | _TORE, not 0); the output of a set that is not wanted is not touched and may be NULL.  With
 *   ti = (int64)trunc(t) of a row, tmin the minimum of ti over its window, t_last the t of the window's last row and k the row's
 *   index inside its window, every set DEVICE int32 [>= offsets[B],4], 16-byte aligned, indexed like rows:
 *     rows_mdes   (x, y, (int32)(ti - tmin), p): astype(np.int64) and t - t.min() of MixedDensityEventStack.stack
 *                 (mixed_density_event_stack.py:26-33); the difference wraps to 32 bits where it does not fit (EVREP_STUDY_T_RANGE)
 *     rows_stack  (x, y, 0, p > 0 ? 1 : -1): p' = (p + 1) // 2 (imagenet.py:1051), then 2 p' - 1 (event_stack.py:18), for
 *                 evrep_event_stack's premap 2.  They are the window's past half, ti <= t_last (event_stack.py:34), only where no
 *                 row has EVREP_STUDY_FUTURE; the future half of such a window is not formed here
 *     rows_tore   ((int32)trunc((x - xmin) + 1.0) - 1, (int32)trunc((y - ymin) + 1.0) - 1, m, p) from the float64 xy and their
 *                 minima over the window, every operation one IEEE float64 operation (imagenet.py:1098-1099, tore.py:29-33);
 *                 m = k, or -k in a window with EVREP_STUDY_UNORDERED: the order marker events2ToreFeature's float-time form
 *                 hands evrep_tore_ftime beside times_f64 = t.  sample_times DEVICE double [B] = t_last (imagenet.py:1100), 0 for
 *                 an empty window; wanted with this set
 *   status DEVICE uint32 [B] is overwritten with
 *     EVREP_STUDY_EMPTY      the window has no row (no other bit is set then)
 *     EVREP_STUDY_FUTURE     a row with (double)ti > t_last, or a t_last that is NaN: times that descend or are negative
 *     EVREP_STUDY_T_RANGE    a t that is NaN or not below 2^63 in magnitude (tested before the cast; such a row's time column is 0
 *                            and it takes no part in tmin), or max ti - tmin above INT32_MAX
 *     EVREP_STUDY_FLAT       every ti of the window is equal (informational: the builders define what they do then)
 *     EVREP_STUDY_UNORDERED  t[k + 1] - t[k] >= 0 fails somewhere in the window (informational: it chooses TORE's order marker)
 *   xy must be finite.  scratch DEVICE of evrep_nimg_study_rows_scratch_bytes(B, total) bytes, total >= offsets[B] - offsets[0],
 *   16-byte aligned, no initialisation needed; its size depends on B alone.  1 <= H, W <= EVREP_MAX_DIM (the frame the rows lie
 *   on; coordinates are not checked against it), 0 <= B <= EVREP_NIMG_MAX_B, a window holds fewer than 2^31 rows; anything
 *   else, a NULL or misaligned pointer that is needed, want == 0 or an unknown want bit is EVREP_EINVAL before anything is
 *   launched.  evrep_nimg_study_rows_scratch_bytes returns 0 for arguments the call refuses. */
#define EVREP_STUDY_MDES 1u
#define EVREP_STUDY_STACK 2u
#define EVREP_STUDY_TORE 4u
#define EVREP_STUDY_EMPTY 1u
#define EVREP_STUDY_FUTURE 2u
#define EVREP_STUDY_T_RANGE 4u
#define EVREP_STUDY_FLAT 8u
#define EVREP_STUDY_UNORDERED 16u
size_t evrep_nimg_study_rows_scratch_bytes(int32_t B, int64_t total);
int evrep_nimg_study_rows(const int32_t *rows, const double *t, const double *xy, const int64_t *offsets, int32_t B, int32_t H,
                          int32_t W, uint32_t want, int32_t *rows_mdes, int32_t *rows_stack, int32_t *rows_tore,
                          double *sample_times, uint32_t *status, void *scratch, void *stream);

/* The detector's input batch in ONE launch: what Gen1H5.__getitem__ does after get_item_transform, plus collate_fn and
 * Trainer.prepro_data (ev-YOLOv6/yolov6/data/gen1_2yolo.py:230-265,320-398,427-447; data_augment.py:31-85,110-184;
 * yolov6/core/engine.py:629-635).  A channel-last representation becomes the channel-first float32 tensor of the detector; per
 * output element, with T the dtype of rep and no multiply fused with an add:
 *     R  R(b, y, x, c) = what evrep_resize_taps writes with scale 1 and out_dtype T through the given tap tables (x taps, then y
 *        taps, both sums in float64 in tap order, one cast to T); one tap of weight 1 per row and column copies the source.
 *     L  I(b, y, x, c) = R(b, y - top, x - left, c) inside the nh x nw rectangle of the S x S square, pad[c] elsewhere.
 *     W  where flags[b] has EVREP_DETIN_WARP: cv2.warpAffine(I, M[:2], dsize=(S, S), borderValue=pad) with its defaults
 *        (INTER_LINEAR, BORDER_CONSTANT), restated from OpenCV's published algorithm -- parity unpinned (cv2 absent).  The inverse
 *        map comes as integer tables in 10-bit fixed point, warp[b] = { adelta[S], bdelta[S], X0[S], Y0[S] } (X0, Y0 per output
 *        row, rounding offset 16 included):  X = (X0[y] + adelta[x]) >> 5, Y = (Y0[y] + bdelta[x]) >> 5 (arithmetic shifts);
 *        sx = clamp(X >> 5, -32768, 32767), sy likewise; ax = (X & 31) / 32, ay = (Y & 31) / 32;  the value, in T, is
 *        ((v00 w00 + v01 w01) + v10 w10) + v11 w11, w00 = (1-ay)(1-ax), w01 = (1-ay) ax, w10 = ay (1-ax), w11 = ay ax, v00 at
 *        (sy, sx), v01 at (sy, sx+1), v10 at (sy+1, sx), v11 at (sy+1, sx+1), a tap outside [0, S) being pad[c].  The sums
 *        X0 + adelta and Y0 + bdelta are the caller's to keep inside int32 (event_representation_study_amd/detector_input.py
 *        refuses a matrix whose tables leave it); the kernel adds them in 64 bits.
 *     F  F(b, y, x, c) = W(b, S-1-y if EVREP_DETIN_FLIPUD, S-1-x if EVREP_DETIN_FLIPLR, c)
 *        out[b, c, y, x] = (float)F(b, y, x, C-1-c) * scale        (scale = (float)(1.0 / 255): torch's `.float() / 255`; 1: as is)
 * rep DEVICE float64/float32 (rep_dtype) [B,H,W,C]; tap tables DEVICE as for evrep_resize_taps, for nh rows and nw columns of
 * T weights each; pad DEVICE double [C]; flags DEVICE uint32 [B] with warp DEVICE int32 [B,4,S] (entries of samples without
 * EVREP_DETIN_WARP are not read), or both NULL: no sample warps or flips; out DEVICE float [B,C,S,S], every element written
 * exactly once.  1 <= B <= 65535, 1 <= C <= EVREP_MAX_CHANNELS, H, W, S, T in 1..EVREP_MAX_DIM, the rectangle inside the
 * square; anything else, a NULL or misaligned pointer or a NaN scale is EVREP_EINVAL before any launch.  Every index is
 * brought into range before a load, whatever the tables hold.  Does not allocate, does not wait for the device. */
#define EVREP_DETIN_WARP 1u
#define EVREP_DETIN_FLIPUD 2u
#define EVREP_DETIN_FLIPLR 4u
int evrep_detector_input(const void *rep, int32_t rep_dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t nh, int32_t nw,
                         int32_t T, const int32_t *ystart, const int32_t *ycount, const double *ywt, const int32_t *xstart,
                         const int32_t *xcount, const double *xwt, int32_t S, int32_t top, int32_t left, const double *pad,
                         const uint32_t *flags, const int32_t *warp, float scale, float *out, void *stream);

/* The same batch from frames of DIFFERENT sizes (TORE's per-window bounding boxes; representations/gen1_transforms.py:51-67),
 * in one launch, with the resize tap tables made on the device.
 * evrep_resize_tap_tables: ONE launch fills the tap tables of n_axes axes.  axes DEVICE int32 [n_axes][6] = { src, dst,
 *   interpolation (EVREP_TAPS_*), T, row offset, weight offset }: for every output index d < dst of the axis it writes
 *   start[row offset + d], count[row offset + d] and the T float64 weights at weights[weight offset + d * T], zeros after the
 *   first count.  The tables equal, bit for bit, the non-zero run of every row of OpenCV's published INTER_AREA / INTER_LINEAR
 *   weight matrix in float64 as event_representation_study_amd/gwd_pipeline.py resize_taps builds it on the host (count 0 and
 *   start 0 for a row without an entry); EVREP_TAPS_IDENTITY (src == dst) is one tap of weight 1 at d.  T is the caller's upper
 *   bound on count (2 for LINEAR, ceil(src / dst) + 1 for AREA, 1 for IDENTITY; a larger T only pads).  start, count DEVICE int32
 *   [n_rows], weights DEVICE double [n_wt]; max_dst >= every dst.  An axis with src, dst or T < 1 or an unknown interpolation,
 *   and a run that would leave [0, n_rows) or [0, n_wt), is not written.  1 <= n_axes, 1 <= max_dst <= EVREP_MAX_DIM,
 *   1 <= n_rows, n_wt < 2^31; anything else, a NULL or misaligned pointer is EVREP_EINVAL before the launch.
 * evrep_detector_input_frames: what evrep_detector_input computes, sample b reading its own frame through its own tables.  frames
 *   HOST [B]; per sample, with T the dtype of the frames:
 *     R1 R1(y, x, c) = what evrep_resize_taps writes for the H x W frame at src with scale 1 and out_dtype T through the stage-1
 *        tables (rows: rh entries from row1 with T1 weights each from wrow1; columns: rw entries from col1 / wcol1).
 *     R  T2 == 0: R = R1 and nh x nw == rh x rw.  T2 > 0 (letterbox needs a resize of its own): R(y, x, c) = (T) sum over the y
 *        taps of (sum over the x taps of (double)R1 * xw2) * yw2 through the stage-2 tables (nh entries from row2 / wrow2,
 *        nw from col2 / wcol2, T2 weights each), tap rows and columns clamped to the rh x rw rectangle: what two passes of
 *        evrep_resize_taps compute through an rh x rw image in memory; here no intermediate image exists.
 *     L, W, F and the conversion as for evrep_detector_input with this sample's nh, nw, top, left and flags (EVREP_DETIN_*).
 *   The entry point checks the whole table on the host -- rep_dtype; 1 <= B <= 65535; 1 <= C <= EVREP_MAX_CHANNELS; S, every H,
 *   W, rh, rw, nh, nw, T1 in 1..EVREP_MAX_DIM, T2 in 0..EVREP_MAX_DIM; the nh x nw rectangle at top, left inside the square; every
 *   offset >= 0 and offset + length inside n_rows / n_wt; src non-NULL and aligned to the element; no unknown flag bit; warp
 *   DEVICE int32 [B,4,S] given exactly when some sample has EVREP_DETIN_WARP; a non-NaN scale; every other pointer non-NULL and
 *   aligned -- and returns EVREP_EINVAL before any launch otherwise.  It then copies the table with one asynchronous copy on
 *   `stream` into frames_dev (DEVICE, evrep_detector_input_frames_scratch_bytes(B) bytes, 8-byte aligned; the kernel reads that
 *   copy, so `frames` may be reused when the call returns) and launches once.  start, count, weights DEVICE as
 *   evrep_resize_tap_tables wrote them (ordered before this call on `stream`); pad DEVICE double [C]; out DEVICE float
 *   [B,C,S,S], every element written exactly once.  Every index taken from a device table is brought into range before a
 *   load.  Neither call allocates; neither waits for the device beyond what the runtime's copy from pageable host memory does
 *   (pinned `frames` avoid that). */
#define EVREP_TAPS_LINEAR 0
#define EVREP_TAPS_AREA 1
#define EVREP_TAPS_IDENTITY 2
typedef struct evrep_detin_frame {
    const void *src;              /* DEVICE [H,W,C], channel last */
    int32_t H, W;
    int32_t rh, rw, T1;           /* stage 1: H x W -> rh x rw */
    int32_t row1, col1;           /* table rows of its rh row entries / rw column entries */
    int32_t wrow1, wcol1;         /* where their weights start */
    int32_t nh, nw, T2;           /* stage 2: rh x rw -> nh x nw, bilinear; T2 == 0: none */
    int32_t row2, col2, wrow2, wcol2;
    int32_t top, left;            /* the nh x nw rectangle in the S x S square */
    uint32_t flags;               /* EVREP_DETIN_* */
    int32_t reserved;             /* 0 */
} evrep_detin_frame;              /* 88 bytes */
int evrep_resize_tap_tables(const int32_t *axes, int32_t n_axes, int32_t max_dst, int32_t *start, int32_t *count, double *weights,
                            int64_t n_rows, int64_t n_wt, void *stream);
size_t evrep_detector_input_frames_scratch_bytes(int32_t B);
int evrep_detector_input_frames(const evrep_detin_frame *frames, int32_t B, int32_t rep_dtype, int32_t C, int32_t S,
                                const int32_t *start, const int32_t *count, const double *weights, int64_t n_rows, int64_t n_wt,
                                const double *pad, const int32_t *warp, float scale, void *frames_dev, float *out, void *stream);

/* The detector's output in ONE launch: ev-YOLOv6's non_max_suppression (yolov6/utils/nms.py:59-129) with the CPU kernel of
 * torchvision.ops.nms behind it, for the B images of a batch, one workgroup per image.  pred[b] is (N, 5 + C) float32, a row
 * [cx, cy, w, h, obj, cls_0 .. cls_{C-1}]; every statement below is one float32 operation, none fused with another:
 *   candidates  ct = conf_thres (a float: torch compares a float32 tensor with a Python scalar in float32).  A box is a
 *               candidate iff obj > ct and max_c cls_c > ct; a NaN obj or a NaN among the classes fails.
 *   rows        conf_c = cls_c * obj; corners x1 = cx - w / 2, x2 = cx + w / 2, y likewise.  EVREP_NMS_MULTI_LABEL and C > 1: one
 *               row per (box i, class c) with conf_c > ct; otherwise one row per candidate with c the FIRST maximum of conf_c,
 *               kept iff conf_c > ct.  A row's number is i * C + c.  n_classes >= 0: a row survives iff its class is among
 *               classes_host[0 .. n_classes) (HOST int32; values outside [0, C) match nothing; n_classes = 0 drops every row);
 *               n_classes = -1: no filter, classes_host is not read.
 *   order       conf descending, equal conf by row number ascending (torchvision's stable sort).  More than max_nms rows: the
 *               first max_nms of that order (the reference's unstable argsort leaves ties at the cut open: here the lower
 *               row number goes first).
 *   greedy      o = cls * 4096, or cls * 0 with EVREP_NMS_AGNOSTIC; every corner is c' = c + o (this addition rounds: at 8192
 *               an ulp is 2^-10); area = (x2' - x1') * (y2' - y1').  A row is kept iff no EARLIER KEPT row i suppresses it:
 *               w = max(0, min(x2'_i, x2'_j) - max(x1'_i, x1'_j)), h likewise, inter = w * h,
 *               ovr = inter / ((area_i + area_j) - inter), suppressed iff (double)ovr > iou_thres.  NaN suppresses nothing.
 *   output      det[b]: the first max_det kept rows as the UN-offset [x1, y1, x2, y2, conf, (float)c], zeros behind them;
 *               count[b]: how many.  Every byte of det and count is written on every call.
 * Not mirrored: the reference's 10 s time limit, half-precision input.
 * pred DEVICE float [B,N,5+C]; det DEVICE float [B,max_det,6]; count DEVICE int32 [B]; all 4-byte aligned.
 * scratch DEVICE, 16-byte aligned: five arrays of B * R uint32 (the four of the pair sort and the row numbers), R the rows an
 *   image can have at the worst, every row of every image a candidate: R = N * C with EVREP_NMS_MULTI_LABEL and C > 1, R = N
 *   otherwise.  Its size is evrep_dense_rank_scratch_bytes(B, 5 * ceil(B * R / 4)) -- four arrays of that total are the five
 *   of B * R.  Needs no initialisation.
 * 1 <= B <= 65535, N >= 1, 1 <= C <= EVREP_NMS_MAX_CLASSES, N * C <= EVREP_NMS_MAX_ROWS, 1 <= max_det <= EVREP_NMS_MAX_DET,
 * max_nms >= 1, conf_thres and iou_thres in [0, 1], -1 <= n_classes <= EVREP_NMS_MAX_ROWS, the total above at most
 * EVREP_RANK_MAX_TOTAL; anything else, an unknown flag, a
 * NULL or misaligned pointer is EVREP_EINVAL before any launch.  Does not allocate, does not wait for the device, reads nothing
 * back: the call may be captured into a graph. */
#define EVREP_NMS_MULTI_LABEL 1u
#define EVREP_NMS_AGNOSTIC 2u
#define EVREP_NMS_MAX_DET 1024
#define EVREP_NMS_MAX_CLASSES 4096
#define EVREP_NMS_MAX_ROWS (1 << 24)
int evrep_nms(const float *pred, int32_t B, int32_t N, int32_t C, float conf_thres, double iou_thres, uint32_t flags,
              const int32_t *classes_host, int32_t n_classes, int32_t max_nms, int32_t max_det, float *det, int32_t *count,
              void *scratch, void *stream);

/* Scoring the detections in ONE launch: the statistics step of ev-YOLOv6's validation loop (yolov6/core/evaler.py:206-258) with
 * yolov6/utils/metrics.py's process_batch and ConfusionMatrix.process_batch behind it, for the B images of a batch, one
 * workgroup per image.  Per image b the detections are rows j = 0 .. count[b]-1 of det[b], [x1, y1, x2, y2, conf, cls] in NMS
 * order (what evrep_nms wrote); the labels are the rows of `targets` whose column 0 equals b (float equality), in array order
 * k = 0 .. M-1, [image, cls, cx, cy, w, h].  Every statement below is one float32 operation, none fused with another (the library
 * is built with -ffp-contract=off and the kernel file repeats it as a pragma):
 *   geometry    (normalised mode, evaler.py:228-249)  detections: scale_coords with ratio_pad given and scale_exact false, with
 *               geom[b] = [pad_x, pad_y, gain, w0, h0] the float32 pad, gain[0] and source frame: x = (x - pad_x) / gain clamped
 *               to [0, w0], y = (y - pad_y) / gain clamped to [0, h0] (clamp: v < 0 ? 0 : v > hi ? hi : v, a NaN stays).
 *               labels, in this order: xywh2xyxy (x1 = cx - w / 2, x2 = cx + w / 2, y likewise), x *= img_w, y *= img_h of the
 *               letterboxed image, then the same scale_coords.
 *   native      EVREP_DETEVAL_NATIVE: labels are [image, cls, x1, y1, x2, y2] and both sides are taken as they are (what
 *               process_batch(detections, labels, iouv) receives); geom, img_h and img_w are not read.
 *   iou         general.box_iou(labels, detections): area = (x2 - x1) * (y2 - y1) for each side,
 *               w = clamp(min(x2l, x2d) - max(x1l, x1d), 0), h likewise, inter = w * h, iou = inter / ((area_l + area_d) - inter).
 *               0 / 0 is NaN, and a NaN matches nothing.
 *   correct     (process_batch) for detection j let k*(j) be the label with cls_k == cls_j (float equality) of greatest
 *               iou(k, j) and iou*(j) that value.  correct[j, i] iff iou*(j) >= iouv[i] (float32, not strict) and no j' < j has
 *               k*(j') == k*(j) and iou*(j') >= iouv[i].  This equals the reference's sort / unique / unique for every threshold.
 *               TIE: among labels of equal greatest IoU the LOWEST label index wins.  The reference's argsort()[::-1] is numpy's
 *               unstable sort and leaves this open: its outcome depends on numpy's build and the CPU (as the ties at evrep_nms's
 *               max_nms cut are).
 *   confusion   (ConfusionMatrix.process_batch; only with matrix != NULL)  only detections with conf > `conf` take part.  For
 *               detection j the best label over ALL classes with iou > iou_thres (strict); for label k the detection of greatest
 *               IoU among those whose best label is k.  Ties: lowest label index, then lowest detection index (open in the
 *               reference for the same reason).  A matched label adds 1 at [int(cls_det), int(cls_label)]; an unmatched label
 *               adds 1 at [nc, int(cls_label)]; detections that won no label add 1 at [int(cls_det), nc], but only if the image
 *               has at least one match.  matrix is DEVICE int64 [(nc+1) * (nc+1)], row-major, accumulated with integer atomics
 *               across images and calls; the caller zeroes it once.  A class outside [0, nc) sets EVREP_DETEVAL_ST_BAD_CLASS and
 *               that update is skipped (the reference raises or wraps).  EVREP_DETEVAL_SKIP_EMPTY is the evaler's guard
 *               (evaler.py:215-225): an image with count[b] == 0 contributes nothing to the matrix.
 *   limits      an image with more than EVREP_DETEVAL_MAX_LABELS labels sets EVREP_DETEVAL_ST_LABEL_OVERFLOW, gets all-false
 *               rows and adds nothing to the matrix (the cap lets the label boxes and the (label, threshold) table of one image
 *               live in LDS); a count[b] outside [0, max_det] is clamped and sets EVREP_DETEVAL_ST_BAD_COUNT.
 *   outputs     correct DEVICE uint8 [B,max_det,T], rows at or beyond count[b] are 0, every byte written on every call;
 *               detn (or NULL) DEVICE float [B,max_det,6]: the native-space detections, zeros beyond count[b], every byte
 *               written; tbox (or NULL) DEVICE float [n_t,4]: the native-space box of every target row, zeros for a row whose
 *               column 0 is no integer in [0, B), every byte written; n_labels DEVICE int32 [B]: the labels of each image (the
 *               true number, also above the cap); status DEVICE uint32 [B]: the bits above, 0 when all is well.
 * det DEVICE float [B,max_det,6]; count DEVICE int32 [B]; targets DEVICE float [n_t,6] (NULL allowed when n_t == 0); geom DEVICE
 * float [B,5] (NULL allowed in native mode); iouv_host HOST float [T], read during the call; pointers 4-byte aligned, matrix
 * 8-byte aligned.  1 <= B <= 65535, 1 <= max_det <= EVREP_NMS_MAX_DET, 0 <= n_t <= EVREP_DETEVAL_MAX_TARGETS,
 * 1 <= T <= EVREP_DETEVAL_MAX_T and no threshold NaN, img_h and img_w in 1..EVREP_MAX_DIM in normalised mode, with a matrix
 * 1 <= nc <= EVREP_NMS_MAX_CLASSES and conf, iou_thres not NaN; anything else, an unknown flag, a NULL or misaligned pointer is
 * EVREP_EINVAL before any launch.  Needs no scratch.  Does not allocate, does not wait for the device, reads nothing back: the
 * call may be captured into a graph. */
#define EVREP_DETEVAL_NATIVE 1u
#define EVREP_DETEVAL_SKIP_EMPTY 2u
#define EVREP_DETEVAL_MAX_LABELS 1024
#define EVREP_DETEVAL_MAX_T 16
#define EVREP_DETEVAL_MAX_TARGETS (1 << 24)
#define EVREP_DETEVAL_ST_LABEL_OVERFLOW 1u
#define EVREP_DETEVAL_ST_BAD_CLASS 2u
#define EVREP_DETEVAL_ST_BAD_COUNT 4u
int evrep_det_match(const float *det, const int32_t *count, int32_t B, int32_t max_det, const float *targets, int64_t n_t,
                    const float *geom, int32_t img_h, int32_t img_w, const float *iouv_host, int32_t T, uint32_t flags,
                    int64_t *matrix, int32_t nc, float conf, float iou_thres, uint8_t *correct, float *detn, float *tbox,
                    int32_t *n_labels, uint32_t *status, void *stream);

/* Average precision on the device: yolov6/utils/metrics.py's ap_per_class and compute_ap (without the plots) for the rows a
 * validation run left resident, with no host sort and no host loop.  tp DEVICE uint8 [n,T] (non-zero: true); conf DEVICE float
 * [n]; pred_cls DEVICE float [n]; target_cls DEVICE float [m]; nc classes.  Every float64 statement below is ONE IEEE operation
 * rounded on its own: nothing is contracted into a fused multiply-add (-ffp-contract=off, and the kernel file repeats it as a
 * pragma), no float atomic, no reassociation; the result is the same bits from run to run.
 *   A1 order    rows are ordered by DESCENDING conf; rows of equal conf keep array order (stable), and -0.0 equals +0.0.  Array
 *               order is (batch, image, detection), the layout the evaluator builds.  This is the declared TIE rule: the
 *               reference's argsort(-conf) is numpy's unstable sort and leaves the outcome open among equal confidences.
 *   A2 classes  class c in [0, nc) owns the rows with pred_cls == c (float equality) and n_l[c] = the number of targets with
 *               target_cls == c.  A prediction or target class outside [0, nc) or not integral (a NaN too) sets
 *               EVREP_AP_ST_BAD_CLASS and takes part in nothing.  A NaN conf sets EVREP_AP_ST_NAN_CONF; what the rows of its
 *               class hold is then unspecified.
 *   A3 counts   for a class with n_p > 0 rows and n_l > 0 labels, at its k-th row (1-based, in A1's order): tpc[k,j] = the integer
 *               count of true tp[.,j] among its first k rows (fpc = k - tpc), recall[k,j] = double(tpc) / double(n_l) (the
 *               reference's n_l + 1e-16 IS n_l in float64), precision[k,j] = double(tpc) / double(k).  A class with n_p == 0 or
 *               n_l == 0 has all-zero rows in every output.
 *   A4 curves   px = numpy's linspace(0, 1, 1000), UPLOADED (tables), not recomputed.  r[c] = interp(-px, -conf_c, recall[:,0],
 *               left = 0); p[c] = interp(-px, -conf_c, precision[:,0], left = 1); conf_c the class's confidences widened to
 *               float64.
 *   A5 interp   interp(x, xp, fp, left, right = fp[last]) is numpy's: x < xp[0] gives left; x > xp[last] gives right; otherwise
 *               j is the LARGEST index with xp[j] <= x; j last gives fp[last]; xp[j] == x gives fp[j]; otherwise
 *               ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j].  "Largest" is what makes repeated abscissae (tied
 *               confidences, the flat runs of mrec) well defined.
 *   A6 ap       per (class, threshold j): mrec = [0, recall[:,j], recall[last,j] + 0.01]; mpre = [1, precision[:,j], 0] replaced
 *               by its running maximum taken from the right; y = interp(x, mrec, mpre) over x = linspace(0, 1, 101);
 *               ap = sum over i = 0..99 of (d[i] * (y[i] + y[i+1])) / 2.0 with d = numpy's diff(x), added in ascending i, one
 *               addition at a time (numpy's trapz adds the same terms pairwise: the two differ by rounding only).
 *   A7 f1       f1 = ((2 * p) * r) / ((p + r) + 1e-16), elementwise.
 * tables DEVICE double [1201]: px[1000], x[101], d[100].  counts_dev: NULL, or DEVICE int64 [2] = {n, m} as they are known on
 * the device only (what evrep_det_ap_gather's cursor holds); then the arguments n and m are CAPACITIES: the arrays and the
 * workspace are sized by them, each device number is clamped to [0, capacity], and nothing is read back.
 * Outputs, all DEVICE, every byte written on every call: p, r, f1 double [nc,1000]; ap double [nc,T]; n_labels, n_pred int64
 * [nc] (the targets and the rows of each class); any_correct uint32 [1] (1 iff any tp byte of the n rows is non-zero, rows of
 * a bad class included: the reference's stats[0].any()); status uint32 [1].
 * The launches: keys and class counts; one workgroup that scans the class counts; a stable LSD radix sort of (class, conf key)
 * carrying the row index, eight bits a pass (count per tile of EVREP_AP_SORT_TILE rows, one workgroup's scan, scatter); the
 * integer scan of tp over the sorted rows, the T thresholds of a row together (sums per tile of EVREP_AP_SCAN_TILE rows, one
 * wave's scan, write); the running maximum from the right, segmented by class (heads, one wave's walk, write); the curves; the
 * areas.  Every dependency between workgroups is a launch boundary: no workgroup waits for another inside a launch.
 * PRACTICAL RANGE: the two one-wave steps (the scan of the tiles' tp sums, the walk of the tiles' maxima) visit the
 * n / EVREP_AP_SCAN_TILE scan tiles one after the other, a dependent read and write each: about 2 000 steps at 10^6 rows (part
 * of the 0.8 ms measured for scans, curves and areas), 4 M steps -- seconds -- at the formal limit below.  The limit is what
 * the 32-bit positions allow; the step is built for validation runs of up to some 10^7 rows.
 * 0 <= n, m < 2^31 (n == 0 or m == 0 is legal: zero curves, and no launch that indexes an empty array), 1 <= T <=
 * EVREP_DETEVAL_MAX_T, 1 <= nc <= EVREP_NMS_MAX_CLASSES; pointers aligned to their element, workspace to 256 bytes, tp / conf /
 * pred_cls may be NULL when n == 0 and target_cls when m == 0; anything else is EVREP_EINVAL before any launch.
 * evrep_det_ap_workspace_bytes(n, T, nc) is the workspace (0 for a refused shape); a smaller workspace_bytes is EVREP_EWORKSPACE.
 * The call writes nothing outside its outputs and the first evrep_det_ap_workspace_bytes bytes of workspace, does not allocate,
 * does not wait for the device, reads nothing back.
 *
 * evrep_det_ap_gather compacts ONE scored batch into those rows: correct DEVICE uint8 [B,max_det,T] and count DEVICE int32 [B]
 * as evrep_det_match wrote and read them, conf_cls DEVICE float [B,max_det,2] (columns 4 and 5 of det), targets DEVICE float
 * [n_t,2] (image, class).  cursor DEVICE int64 [2], zeroed by the caller before the first batch.  The rows 0 .. clamp(count[b],
 * 0, max_det) - 1 of image b go to tp / conf / pred_cls at cursor[0] + the clamped counts of the images in front of it: (batch,
 * image, detection) order.  The class of every target row whose image is an integer in [0, B) (the rows the evaluator counts)
 * goes to target_cls from cursor[1] on, in array order.  Then cursor moves by the two numbers.  Two launches (the cursor is
 * moved by the second: a launch boundary behind every workgroup that read it), no scratch.  cap_n >= B * max_det rows must
 * be free behind the cursor (the caller sizes the rows for every batch; a row that would not fit is not written); cap_n, cap_m
 * < 2^31; 1 <= B <= 65535, 1 <= max_det <= EVREP_NMS_MAX_DET, 0 <= n_t <= EVREP_DETEVAL_MAX_TARGETS. */
#define EVREP_AP_SORT_TILE 2048
#define EVREP_AP_SCAN_TILE 512
#define EVREP_AP_GATHER_CHUNK 1024  /* evrep_det_ap_gather's second launch: target rows, and images, per round of its one workgroup */
#define EVREP_AP_GATHER_IMAGES 256  /* its first launch: the images in front of its own that a workgroup sums per round */
#define EVREP_AP_ST_BAD_CLASS 1u
#define EVREP_AP_ST_NAN_CONF 2u
size_t evrep_det_ap_workspace_bytes(int64_t n, int32_t T, int32_t nc);
int evrep_det_ap(const uint8_t *tp, const float *conf, const float *pred_cls, const float *target_cls, int64_t n, int64_t m,
                 int32_t T, int32_t nc, const int64_t *counts_dev, const double *tables, double *p, double *r, double *f1,
                 double *ap, int64_t *n_labels, int64_t *n_pred, uint32_t *any_correct, uint32_t *status, void *workspace,
                 size_t workspace_bytes, void *stream);
int evrep_det_ap_gather(const uint8_t *correct, const float *conf_cls, const int32_t *count, int32_t B, int32_t max_det, int32_t T,
                        const float *targets, int64_t n_t, uint8_t *tp, float *conf, float *pred_cls, int64_t cap_n,
                        float *target_cls, int64_t cap_m, int64_t *cursor, void *stream);

/* The training targets: what ev-YOLOv6's ComputeLoss.__call__ does between the head's output and the loss terms
 * (yolov6/models/losses/loss.py:73-111) for the B images of a batch, with no (B, M, A) array in memory.
 *
 * evrep_det_targets_pad is ComputeLoss.preprocess (loss.py:219-236).  The labels of image b are the rows of `targets` whose
 *   column 0 equals b (float equality), in array order, [image, cls, cx, cy, w, h] float32.  Every value is widened exactly to
 *   float64, as are width and height; then, one float64 operation per statement, bx = cx * width, by = cy * height,
 *   bw = w * width, bh = h * height, x1 = bx - bw * 0.5, y1 = by - bh * 0.5, x2 = x1 + bw, y2 = y1 + bh (the updated x1, y1: the
 *   in-place xywh2xyxy of yolov6/utils/general.py:58-64).  gt[b, m] = [cls, x1, y1, x2, y2] for the image's m-th label, m < M;
 *   the rows behind the last label are [-1, 0, 0, 0, 0].  An image with more than M labels keeps its first M and sets
 *   EVREP_TAL_ST_LABEL_OVERFLOW.  n_labels[b] is the true number.  Every byte of gt, n_labels and status is written.
 *   targets DEVICE float [n_t,6] (NULL allowed when n_t == 0); gt DEVICE double [B,M,5] (NULL allowed when M == 0); n_labels
 *   DEVICE int32 [B]; status DEVICE uint32 [B].  1 <= B <= 65535, 0 <= M <= EVREP_TAL_MAX_LABELS, 0 <= n_t <=
 *   EVREP_DETEVAL_MAX_TARGETS, width and height finite.  One launch, no scratch.
 *
 * evrep_tal_assign is TaskAlignedAssigner.forward (yolov6/assigners/tal_assigner.py, assigner_utils.py) on such a gt.  The
 *   reference's route is float64 (preprocess builds its tensor from Python floats) but for ONE float32 quantity, the predicted
 *   box's own area; each statement below is one operation of the stated type, none fused with another (-ffp-contract=off, and the
 *   kernel file repeats it as a pragma).  max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b.  pd_scores, pd_bboxes and
 *   anc_points are float32 and widened where they meet a float64 value.
 *   row         row m of image b is VALID iff ((x1 + y1) + x2) + y2 > 0 (mask_gt), its class lies in [0, nc) and the image is
 *               finite (below).  A valid-box row whose class lies outside [0, nc) sets EVREP_TAL_ST_BAD_CLASS and is treated as
 *               padding (the reference raises or wraps).
 *   in-gt       d = min(min(ax - x1, ay - y1), min(x2 - ax, y2 - ay)); in_gt = d > 1e-9: a centre on an edge is outside.
 *   iou         ix1 = max(x1, px1), ix2 = min(x2, px2), y likewise; ov = max(ix2 - ix1, 0) * max(iy2 - iy1, 0);
 *               a1 = max(x2 - x1, 0) * max(y2 - y1, 0); a2 = max(px2 - px1, 0f) * max(py2 - py1, 0f) in FLOAT32, then widened;
 *               iou = ov / (((a1 + a2) - ov) + 1e-9).
 *   metric      al = score^alpha * iou^beta, score = pd_scores[b, a, long(cls)]; x^0 = 1, x^1 = x, x^n is n - 1 successive
 *               multiplications by x, left to right.  The reference uses alpha = 1, beta = 6.
 *   key         al if in_gt and al > 0, else +0.
 *   top-k       per valid row the first `topk` anchors of the TOTAL order (key descending, anchor index ascending) over all A
 *               anchors (all of them when topk > A); a selected anchor is a CANDIDATE of the row iff it is in_gt.  Zero keys are
 *               therefore chosen by lowest index, inside the box or not: one of the outcomes the reference's torch.topk may
 *               produce, made definite (as evrep_nms settles its max_nms ties).  Rows that are not valid have no candidates.
 *   anchor      c = the rows it is a candidate of.  c == 0: background, row 0.  c == 1: that row.  c > 1: the FIRST row of greatest
 *               iou over ALL M rows -- padding and rows it is no candidate of included (select_highest_overlaps, reproduced).
 *               fg = c > 0; target_labels = long(cls) of the row when that lies in [0, nc), else 0; target_bboxes = the row's
 *               box.  Background anchors carry row 0's label and box, as the reference returns them.
 *   scores      pos_al[m] / pos_ov[m] = the greatest al / iou over the anchors assigned to row m, 0 when there is none (al is the
 *               metric, not the key; only values > 0 take part; a row whose class lies outside [0, nc) has al = 0).
 *               target_scores[b, a, :] is zero but at a foreground anchor's label, where it is (al * pos_ov) / (pos_al + 1e-9).
 *   shapes      M == 0 is the reference's early return: labels nc, everything else zero, status 0.
 *   status      EVREP_TAL_ST_BAD_CLASS as above; EVREP_TAL_ST_NONFINITE: an inf or NaN among pd_scores[b], pd_bboxes[b] or gt[b] --
 *               the whole image is written as if it had no valid row.  (anc_points must be finite; products of finite inputs that
 *               overflow are outside the contract.)
 *   outputs     target_labels DEVICE int64 [B,A]; target_bboxes [B,A,4] and target_scores [B,A,nc] DEVICE double -- the
 *               reference's dtype -- or, with EVREP_TAL_F32_OUT, float: the same float64 values rounded once at the store;
 *               fg DEVICE uint8 [B,A]; status DEVICE uint32 [B].  Every byte of each is written on every call.
 *   scratch     DEVICE, 256-byte aligned, evrep_tal_workspace_bytes(B, M, A) bytes (0 for a refused shape): per (image, anchor)
 *               three 32-bit words and one double, per (image, row) two 64-bit words, each array rounded up to 256 bytes.  Needs
 *               no initialisation: the call clears what it reads.
 * pd_scores DEVICE float [B,A,nc]; pd_bboxes DEVICE float [B,A,4] xyxy; anc_points DEVICE float [A,2]; gt DEVICE double [B,M,5]
 * (NULL allowed when M == 0).  1 <= B <= 65535, 0 <= M <= EVREP_TAL_MAX_LABELS, 1 <= A <= EVREP_TAL_MAX_ANCHORS,
 * 1 <= nc <= EVREP_TAL_MAX_CLASSES, A * nc < 2^31, 1 <= topk <= EVREP_TAL_MAX_TOPK, alpha and beta in 0..EVREP_TAL_MAX_POWER;
 * anything else, an unknown flag, a NULL or misaligned pointer is EVREP_EINVAL before any launch.  Integer atomics only: two
 * calls give equal bits.  One async memset of status and up to four launches; does not allocate, does not wait for the
 * device, reads nothing back: the call may be captured into a graph. */
#define EVREP_TAL_F32_OUT 1u
#define EVREP_TAL_MAX_TOPK 64
#define EVREP_TAL_MAX_LABELS 1024
#define EVREP_TAL_MAX_CLASSES 4096
#define EVREP_TAL_MAX_ANCHORS (1 << 24)
#define EVREP_TAL_MAX_POWER 16
#define EVREP_TAL_ST_LABEL_OVERFLOW 1u
#define EVREP_TAL_ST_BAD_CLASS 2u
#define EVREP_TAL_ST_NONFINITE 4u
int evrep_det_targets_pad(const float *targets, int64_t n_t, int32_t B, int32_t M, float width, float height, double *gt,
                          int32_t *n_labels, uint32_t *status, void *stream);
size_t evrep_tal_workspace_bytes(int32_t B, int32_t M, int32_t A);
int evrep_tal_assign(const float *pd_scores, const float *pd_bboxes, const float *anc_points, const double *gt, int32_t B,
                     int32_t M, int32_t A, int32_t nc, int32_t topk, int32_t alpha, int32_t beta, uint32_t flags,
                     int64_t *target_labels, void *target_bboxes, void *target_scores, uint8_t *fg, uint32_t *status,
                     void *scratch, void *stream);

/* evrep_atss_assign is ATSSAssigner.forward (yolov6/assigners/atss_assigner.py with iou2d_calculator.py and assigner_utils.py),
 * what ComputeLoss.__call__ assigns with while epoch_num < warmup_epoch (loss.py:84-97), on the gt evrep_det_targets_pad writes,
 * with no (B, M, A) array in memory.  Every statement below is ONE float64 operation unless a type is named, none fused with
 * another; float32 inputs are widened exactly; max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b.
 *   anchor      the box is float32 (ax1, ay1, ax2, ay2).  area_a = fl32(fl32(ax2 - ax1) * fl32(ay2 - ay1)), unclamped;
 *               acx = fl32(fl32(ax1 + ax2) / 2f), acy likewise; all three are then widened.  The centre comes from the box.
 *   row         VALID as for evrep_tal_assign: ((x1 + y1) + x2) + y2 > 0, the class in [0, nc) (else EVREP_TAL_ST_BAD_CLASS and
 *               the row counts as padding), the image finite.
 *   overlap     o(m, a) of bbox_overlaps, mode iou: w = max(min(x2, ax2) - max(x1, ax1), 0), h likewise; ov = w * h;
 *               area_g = (x2 - x1) * (y2 - y1), unclamped; u = max((area_g + area_a) - ov, 1e-6) -- the double 1e-6 --; o = ov / u.
 *   distance    dx = (x1 + x2) / 2.0 - acx, dy likewise; d = sqrt(dx * dx + dy * dy), correctly rounded.
 *   candidates  level l holds the anchors [s_l, s_l + level_counts[l]), s_l the sum of the counts before it.  For every valid row
 *               each level contributes the first `topk` of its anchors in the TOTAL order (d ascending, anchor index ascending):
 *               equal distances, which the reference's torch.topk leaves open, go to the lower index.
 *   threshold   over the n = n_levels * topk values v_i = o(m, c_i) in the order (level, place in the level's order):
 *               mean = (...((v_0 + v_1) + v_2)...) / n; ss = the (v_i - mean) * (v_i - mean) added in the same order;
 *               thr = mean + sqrt(ss / (n - 1)).  n == 1 gives the reference's NaN: no positives.  (torch adds in another order:
 *               thr may differ from torch's in its last bits.)
 *   positive    a candidate with o > thr whose centre (acx, acy) is in-gt, as for evrep_tal_assign (d > 1e-9).
 *   anchor      c = the rows it is a positive of.  c == 0: background -- target_labels nc, row 0's box, scores zero.  c == 1: that
 *               row.  c > 1: the FIRST row of greatest o over ALL M rows (select_highest_overlaps, reproduced).  fg = c > 0;
 *               target_labels of a foreground anchor = long(cls) of the row when that lies in [0, nc), else 0.
 *   scores      target_scores[b, a, :] is zero but at a foreground anchor's label: fl32(iou) with iou of evrep_tal_assign (the
 *               row against pd_bboxes[b, a]), or 1 when pd_bboxes is NULL.  The reference holds target_scores in float32.
 *   shapes      M == 0 is the reference's early return: labels nc, everything else zero, status 0.
 *   status      EVREP_TAL_ST_BAD_CLASS as above; EVREP_TAL_ST_NONFINITE: an inf or NaN among gt[b] or pd_bboxes[b] -- the whole
 *               image is written as if it had no valid row.  (anchors must be finite.)
 *   outputs     target_labels DEVICE int64 [B,A]; target_bboxes [B,A,4] DEVICE double, or float with EVREP_ATSS_F32_BOXES;
 *               target_scores [B,A,nc] DEVICE double, or float with EVREP_ATSS_F32_SCORES: the same values, rounded once at the
 *               store (fl32(iou) is stored exactly in either); fg DEVICE uint8 [B,A]; status DEVICE uint32 [B].  Every byte of
 *               each is written on every call.
 *   scratch     DEVICE, 256-byte aligned, evrep_atss_workspace_bytes(B, M, A) bytes (0 for a refused shape): per (image, anchor)
 *               three 32-bit words and one double, each array rounded up to 256 bytes.  Needs no initialisation.
 * anchors DEVICE float [A,4] xyxy; level_counts HOST int32 [n_levels], read before the call returns; gt DEVICE double [B,M,5]
 * (NULL allowed when M == 0); pd_bboxes DEVICE float [B,A,4] xyxy or NULL.  1 <= B <= 65535, 0 <= M <= EVREP_TAL_MAX_LABELS,
 * 1 <= A <= EVREP_TAL_MAX_ANCHORS, 1 <= nc <= EVREP_TAL_MAX_CLASSES, A * nc < 2^31, 1 <= n_levels <= EVREP_ATSS_MAX_LEVELS,
 * 1 <= topk <= EVREP_ATSS_MAX_TOPK, n_levels * topk <= EVREP_ATSS_MAX_CANDIDATES, topk <= level_counts[l] for every level (the reference itself fails
 * on a smaller level), the counts add up to A; anything else, an unknown flag, a NULL or misaligned pointer is EVREP_EINVAL
 * before any launch.  Integer atomics only: two calls give equal bits.  One async memset of status and up to four launches;
 * does not allocate, does not wait for the device, reads nothing back: the call may be captured into a graph. */
#define EVREP_ATSS_F32_BOXES 1u
#define EVREP_ATSS_F32_SCORES 2u
#define EVREP_ATSS_MAX_TOPK 32
#define EVREP_ATSS_MAX_LEVELS 8
#define EVREP_ATSS_MAX_CANDIDATES 256
size_t evrep_atss_workspace_bytes(int32_t B, int32_t M, int32_t A);
int evrep_atss_assign(const float *anchors, const int32_t *level_counts, int32_t n_levels, const double *gt, const float *pd_bboxes,
                      int32_t B, int32_t M, int32_t A, int32_t nc, int32_t topk, uint32_t flags, int64_t *target_labels,
                      void *target_bboxes, void *target_scores, uint8_t *fg, uint32_t *status, void *scratch, void *stream);

/* The loss terms of ComputeLoss.__call__ (loss.py:176-217: VarifocalLoss, BboxLoss with IOUloss(xyxy, giou, eps = 1e-10) of
 * yolov6/utils/figure_iou.py and _df_loss) and bbox_decode (loss.py:238-244), values AND gradients, for the targets
 * evrep_tal_assign wrote.  Every statement below is ONE float64 operation unless a type is named; float32 inputs are widened
 * exactly; nothing is fused; exp / log are the double library functions; max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b.
 * R = reg_max, K = R + 1 with EVREP_DETLOSS_USE_DFL, else K = 1 (pred_distri holds the four distances themselves and R is not
 * read).  z = pred_distri, p = pred_scores (after the sigmoid).
 *   decode     aps = fl32(anc / stride) per coordinate, widened.  Per side s of (l, t, r, b), with DFL: m = max_k z[s,k];
 *              e_k = exp(z[s,k] - m); Z = the e_k added left to right; pr_k = e_k / Z; d_s = the products pr_k * k added left to
 *              right.  Without: d_s = z[s].  box = [ax - d_l, ay - d_t, ax + d_r, ay + d_b] in stride units.
 *   sums       w[b,a] = target_scores[b,a,:] added left to right; tss = all w in a fixed order that depends on (B, A) only;
 *              norm = tss > 1 ? tss : 1, decided on the device.
 *   class      q = target_scores; lab = fg[b,a] && target_labels[b,a] == c; wt = lab ? q : (0.75 * p) * p;
 *              bce = -(q * max(log(p), -100) + (1 - q) * max(log(1 - p), -100)); loss_cls = (sum of bce * wt) / norm.
 *   box        per foreground anchor, tb = target_bboxes / stride: inter = max(min(x2, tx2) - max(x1, tx1), 0) * (y likewise);
 *              w1 = x2 - x1; h1 = (y2 - y1) + eps; w2, h2 likewise; union = ((w1 * h1 + w2 * h2) - inter) + eps;
 *              iou = inter / union; cw = max(x2, tx2) - min(x1, tx1), ch likewise; c_area = cw * ch + eps;
 *              giou = iou - (c_area - union) / c_area; loss_iou = (sum of (1 - giou) * w) / norm.
 *   DFL        per foreground anchor and side: t = min(max(distance of tb from aps, 0), R - 0.01); tl = (long)t;
 *              wl = (tl + 1) - t; wr = 1 - wl; lse = m + log(Z); ce(k) = lse - z[s,k]; side = ce(tl) * wl + ce(tl + 1) * wr;
 *              dfl = (((side_l + side_t) + side_r) + side_b) / 4; loss_dfl = (sum of dfl * w) / norm.  Without DFL loss_dfl = 0;
 *              with no foreground anchor loss_iou = loss_dfl = 0 and grad_distri is all zeros.
 *   gradients  of L = w_class * loss_cls + w_iou * loss_iou + w_dfl * loss_dfl with respect to p and z, what torch's autograd
 *              gives for the reference's statements: BCE's backward is (p - q) / max((1 - p) * p, (double)1e-12f) -- torch holds
 *              that constant as a float, 9.999999960041972e-13 --, also where the log was clamped; wt is not detached (a non-label element adds bce * (1.5 * p)); the clamp at 0 passes the gradient at
 *              x >= 0; min / max of equal arguments split it in halves; d d_s / d z[s,k] = pr_k * (k - d_s); the DFL part is
 *              ((w_dfl * w) / norm / 4) * ((pr_k - wl [k == tl]) - wr [k == tl + 1]).  Formed in float64, rounded ONCE at the
 *              store.  Every byte of both arrays is written; the rows of background anchors in grad_distri are zeros.
 *   status     EVREP_DETLOSS_ST_BAD_LABEL: a foreground anchor whose label lies outside [0, nc): background for the class term
 *              (the reference's one_hot raises), a foreground anchor for the box terms.  Non-finite inputs propagate as in torch.
 * evrep_detloss_decode: boxes_s DEVICE float [B,A,4] = the float64 box rounded once; boxes_px DEVICE float [B,A,4] =
 *   fl32(box * stride), what evrep_tal_assign takes as pd_bboxes.  One launch, no scratch.  flags: EVREP_DETLOSS_USE_DFL.
 * evrep_detloss: pred_scores DEVICE float [B,A,nc]; pred_distri DEVICE float [B,A,4K]; anc_points DEVICE float [A,2] (pixels);
 *   stride DEVICE float [A]; target_labels DEVICE int64 [B,A]; target_bboxes [B,A,4] (pixels) and target_scores [B,A,nc] DEVICE
 *   double, or float with EVREP_DETLOSS_F32_TARGETS; fg DEVICE uint8 [B,A].  losses DEVICE double [5] = loss_cls, loss_iou,
 *   loss_dfl (normalised, unweighted), tss, the number of foreground anchors.  grad_scores DEVICE float [B,A,nc], grad_distri
 *   DEVICE float [B,A,4K]: with EVREP_DETLOSS_NO_GRAD they may be NULL and nothing of them is computed.  status DEVICE uint32
 *   [B].  scratch DEVICE, 256-byte aligned, evrep_detloss_workspace_bytes(B, A, nc) bytes (0 for a refused shape): B * A
 *   doubles, then min(ceil(B * A / 256), 256) doubles, then B * min(ceil(A * nc / 256), ceil(2048 / B)) doubles, then three
 *   times B * ceil(A / 256) doubles, each array rounded up to 256 bytes.  Needs no initialisation.
 * 1 <= B <= 65535, 1 <= A <= EVREP_TAL_MAX_ANCHORS, 1 <= nc <= EVREP_TAL_MAX_CLASSES, A * nc < 2^31, 0 <= R <=
 * EVREP_DETLOSS_MAX_REG (1 <= R with EVREP_DETLOSS_USE_DFL); anything else, an unknown flag, a NULL or misaligned pointer is
 * EVREP_EINVAL before any launch.  One async memset of status and four launches; no floating-point atomics: two calls give
 * equal bits.  Does not allocate, does not wait for the device, reads nothing back: the call may be captured into a graph. */
#define EVREP_DETLOSS_USE_DFL 1u
#define EVREP_DETLOSS_NO_GRAD 2u
#define EVREP_DETLOSS_F32_TARGETS 4u
#define EVREP_DETLOSS_MAX_REG 32
#define EVREP_DETLOSS_ST_BAD_LABEL 1u
int evrep_detloss_decode(const float *pred_distri, const float *anc_points, const float *stride, int32_t B, int32_t A, int32_t R,
                         uint32_t flags, float *boxes_s, float *boxes_px, void *stream);
size_t evrep_detloss_workspace_bytes(int32_t B, int32_t A, int32_t nc);
int evrep_detloss(const float *pred_scores, const float *pred_distri, const float *anc_points, const float *stride,
                  const int64_t *target_labels, const void *target_bboxes, const void *target_scores, const uint8_t *fg, int32_t B,
                  int32_t A, int32_t nc, int32_t R, double w_class, double w_iou, double w_dfl, uint32_t flags, double *losses,
                  float *grad_scores, float *grad_distri, uint32_t *status, void *scratch, void *stream);

/* The distillation losses of loss_distill.py (ComputeLoss.__call__ :62-279, distill_loss_cls :281-292, BboxLoss.forward
 * :395-464 with distill_loss_dfl :489-500, distill_loss_cw :294-340), values AND gradients with respect to the student's
 * tensors.  Every statement is ONE float64 operation as above; x / T is a float64 division; exp / log are the double library
 * functions.  p, z = the student's pred_scores, pred_distri; tp, tz = the teacher's; T = temperature.
 *   terms      loss_cls, loss_iou, loss_dfl, w, tss, status: the statements of evrep_detloss, by the same device code, but
 *              norm = tss > 0 ? tss : 1 (loss_distill.py divides loss_cls where tss > 0 and the box terms unless tss == 0).
 *   softmax    of n logits x at T: m = max_k (x_k / T); e_k = exp(x_k / T - m); Z = the e_k added left to right; pr_k = e_k / Z.
 *   KL row     ps = softmax of the student's row, pt = of the teacher's: the terms pt_k * log(pt_k) - pt_k * log(ps_k), the first
 *              product being 0 where pt_k == 0 (torch's xlogy); spt = the pt_k added left to right.
 *   class      over ALL B * A rows of nc scores: d_loss_cls = (T * T) * (the rows' KL sums in a fixed order that depends on the
 *              shape only, as every sum of KL terms here).  Not normalised.  With nc == 1 it is exactly 0, and so is its part of every gradient.
 *   DFL        with EVREP_DETLOSS_USE_DFL, over the 4 * n_fg rows of K bins of the foreground anchors' sides (n_fg = their
 *              number): sum = their KL sums in a fixed order; W = the w[b,a] of the FOREGROUND anchors in a fixed order;
 *              d_loss_dfl = (((T * T) * (sum / (4 * n_fg))) * W) / norm -- the reference multiplies the mean over the rows by
 *              every anchor's bbox_weight and adds.  0 without DFL and with n_fg == 0.  The teacher's boxes are not decoded.
 *   gradients  of L = w_class * (loss_cls + k_class * d_loss_cls) + w_iou * loss_iou + w_dfl * (loss_dfl + k_dfl * d_loss_dfl):
 *              grad_scores = (w_class / norm) * g_vfl + ((w_class * k_class) * T) * (ps_c * spt - pt_c), g_vfl the class
 *              gradient of evrep_detloss; a foreground side's grad_distri[k] = (the value of evrep_detloss's rule with this norm)
 *              + cdd * (ps_k * spt - pt_k), cdd = ((((w_dfl * k_dfl) * T) * W) / norm) / (4 * n_fg).  Each sum is formed in
 *              float64 and rounded ONCE at the store; every element is written once; background rows of grad_distri are zeros.
 *              The teacher's tensors get no gradient.
 * evrep_detloss_distill: the arguments of evrep_detloss, plus t_pred_scores DEVICE float [B,A,nc], t_pred_distri DEVICE float
 *   [B,A,4K], temperature (finite, > 0, else EVREP_EINVAL), k_class = decay * distill_weight["class"], k_dfl = decay *
 *   distill_weight["dfl"] (the caller forms decay = ((1 - cos(epoch * pi / max_epoch)) / 2) * (0.01 - 1) + 1).  losses DEVICE
 *   double [8] = loss_cls, loss_iou, loss_dfl (normalised), d_loss_cls, d_loss_dfl (before k_*), tss, n_fg, W.  flags, limits
 *   and refusals as evrep_detloss, but nc <= EVREP_DISTILL_MAX_CLASSES (a whole row of scores lies in LDS).  scratch DEVICE, 256-byte aligned, evrep_detloss_distill_workspace_bytes(B, A, nc) bytes (0
 *   for a refused shape): B * A doubles; three times min(ceil(B * A / 256), 256) doubles; two times B * min(ceil(A / rt),
 *   ceil(2048 / B)) doubles with rt = min(256, 2048 / nc), the whole rows of a staged tile; four times B * ceil(A / 256)
 *   doubles; each array rounded up to 256 bytes.  Needs no initialisation.  One async memset of status and FOUR launches: rows
 *   (w, tss, and W and n_fg, which every foreground gradient needs, in a fixed order), class (p and tp held in LDS, each
 *   read from memory once), box, fold.  No floating-point atomics: two calls give equal bits.  Does not allocate, does not
 *   wait for the device, reads nothing back: the call may be captured into a graph.  What a NaN tss gives is not pinned.
 * evrep_detloss_cwd: distill_loss_cw over L <= EVREP_CWD_MAX_LEVELS levels of maps s, t DEVICE float [n,c,h,w].  Per (n, c)
 *   row of h * w values, x = s / tau, y = t / tau: ms = max x, Zs = sum exp(x - ms), ls_i = (x_i - ms) - log(Zs); lt_i likewise;
 *   pt_i = exp(lt_i); row = sum pt_i * (lt_i - ls_i); spt = sum pt_i; grad_s_i = (tau / (n * c)) * (exp(ls_i) * spt - pt_i),
 *   rounded once at the store.  The three sums of a row are taken in an order that depends on h * w only.  A level's loss =
 *   (its rows in index order) * ((tau * tau) / (n * c)).  out DEVICE double [4] = the levels added left to right, then each
 *   level (0 beyond L).  A row of at most EVREP_CWD_STAGE values is held in LDS between the passes, a longer one is re-read.
 *   levels_host HOST [L], read before the call returns; grad_s may be NULL with EVREP_DETLOSS_NO_GRAD (the only flag).
 *   n, c, h, w >= 1; n * c, h * w and the rows of all levels <= EVREP_TAL_MAX_ANCHORS; tau finite and > 0; anything else, a NULL
 *   or misaligned pointer is EVREP_EINVAL before any launch.  scratch DEVICE, 256-byte aligned,
 *   evrep_detloss_cwd_workspace_bytes(levels_host, L) bytes (0 for a refused table): one double per row, rounded up to 256
 *   bytes; needs no initialisation.  Two launches, no atomics, no allocation, no wait, nothing read back.
 *
 * 16-BIT MAPS (training under autocast, evaluation with model.half()).  The entries that take the network's own maps have a
 * typed twin beside them -- evrep_detloss_cwd_typed here, evrep_dethead_predict_typed, _train_typed and _train_backward_typed
 * below -- whose level structs hold void pointers and which take a dtype code EVREP_DT_F32, EVREP_DT_F16 (IEEE binary16) or
 * EVREP_DT_BF16 (bfloat16): one per call for the head, one for the student's maps and one for the teacher's here.
 *   W1 widen   a 16-bit map element is widened EXACTLY to float32 at its load: float16 by IEEE conversion, bfloat16 by placing
 *              its 16 bits on top of 16 zero bits.  Subnormals and -0.0 keep value and sign; nothing is flushed.  From there
 *              every rule stated for float32 maps applies unchanged, so a typed entry gives the bits the float32 entry gives on
 *              the widened maps; all forward outputs stay float32 (out here stays float64).
 *   W2 round   the head's backward forms its float32 value as stated below and rounds it ONCE, to nearest even, to the maps'
 *              dtype at the store: overflow gives +-inf, a NaN stays a NaN, and what is too small gives +-0 (float16: every
 *              |x| <= 2^-25, so every float32 subnormal; bfloat16 has float32's exponent range and keeps float32 subnormals as
 *              its own).  The result is torch's float32_tensor.to(dtype) bit for bit wherever it is no NaN.
 *   W3 cwd     evrep_detloss_cwd_typed writes grad_s in FLOAT32 whatever the maps' dtype: an element is tau / (n * c) times a
 *              difference of probabilities, about 1e-8 at the reference's shapes, below float16's smallest subnormal before
 *              the loss scale multiplies it.  The caller multiplies by the incoming gradient first and rounds once after.
 * With EVREP_DT_F32 a typed entry is the float32 entry.  Limits and refusals are those of the float32 entries; a map pointer
 * must be aligned to ITS element size (2 bytes for the 16-bit codes); an unknown dtype code is EVREP_EINVAL before any launch.
 * evrep_cast16_host(src, dst, n, dtype, dir): W1 (dir 0: src HOST 16-bit [n] -> dst HOST float [n]) and W2 (dir 1: float ->
 * 16-bit) on the HOST, by the very functions the kernels use (csrc/evrep_f16.h); dtype EVREP_DT_F16 or EVREP_DT_BF16. */
#define EVREP_DT_F32 0
#define EVREP_DT_F16 1
#define EVREP_DT_BF16 2
int evrep_cast16_host(const void *src, void *dst, int64_t n, int32_t dtype, int32_t dir);
typedef struct { const float *s; const float *t; float *grad_s; int32_t n, c, h, w; } evrep_cwd_level;
typedef struct { const void *s; const void *t; float *grad_s; int32_t n, c, h, w; } evrep_cwd_level_typed;
#define EVREP_DISTILL_MAX_CLASSES 2048
#define EVREP_CWD_MAX_LEVELS 3
#define EVREP_CWD_STAGE 4096
size_t evrep_detloss_distill_workspace_bytes(int32_t B, int32_t A, int32_t nc);
int evrep_detloss_distill(const float *pred_scores, const float *pred_distri, const float *t_pred_scores, const float *t_pred_distri,
                          const float *anc_points, const float *stride, const int64_t *target_labels, const void *target_bboxes,
                          const void *target_scores, const uint8_t *fg, int32_t B, int32_t A, int32_t nc, int32_t R, double w_class,
                          double w_iou, double w_dfl, double temperature, double k_class, double k_dfl, uint32_t flags, double *losses,
                          float *grad_scores, float *grad_distri, uint32_t *status, void *scratch, void *stream);
size_t evrep_detloss_cwd_workspace_bytes(const evrep_cwd_level *levels_host, int32_t L);
int evrep_detloss_cwd(const evrep_cwd_level *levels_host, int32_t L, double tau, uint32_t flags, double *out, void *scratch,
                      void *stream);
size_t evrep_detloss_cwd_typed_workspace_bytes(const evrep_cwd_level_typed *levels_host, int32_t L);
int evrep_detloss_cwd_typed(const evrep_cwd_level_typed *levels_host, int32_t L, double tau, uint32_t flags, int32_t s_dtype,
                            int32_t t_dtype, double *out, void *scratch, void *stream);

/* What Detect.forward does behind its last convolutions (ev-YOLOv6/yolov6/models/effidehead.py:89-173, with
 * generate_anchors(is_eval = True) and dist2bbox(xywh) behind it): the per-level maps of cls_preds / reg_preds, NCHW as the
 * convolutions leave them, -> the prediction tensor of evaluation, the two tensors of training, and the maps' gradients.
 *   levels     L levels l = 0 .. L-1, 1 <= L <= EVREP_DETHEAD_MAX_LEVELS.  Level l has a map of h_l x w_l, n_l = h_l * w_l anchors,
 *              offset off_l (the sum of the earlier n) and stride s_l (float32).  N = A = sum n_l.
 *   anchors    anchor a = off_l + i * w_l + j, row-major as flatten(2) orders it; its point is ax = j + 0.5, ay = i + 0.5 (the
 *              reference's grid_cell_offset, fixed at 0.5), formed in the kernel: no anchor tensor is read.
 *   inputs     K = R + 1 with EVREP_DETHEAD_USE_DFL, else K = 1.  cls_l float32 [B, nc, h_l, w_l]: the raw logits of cls_preds[l];
 *              reg_l float32 [B, 4K, h_l, w_l], channel side * K + k -- what reshape([-1, 4, K, n_l]) means, and the last axis of
 *              pred_distri.
 * Evaluation (evrep_dethead_predict).  Every statement is ONE float64 operation; inputs are widened exactly; nothing is fused.
 *   E1         the side distance d_side is the decode rule of evrep_detloss above (m, e_k, Z, pr_k, d added left to right), by
 *              the same device function (csrc/evrep_dfl.h); without DFL d = z.
 *   E2         x1 = ax - d_0; y1 = ay - d_1; x2 = ax + d_2; y2 = ay + d_3; cx = (x1 + x2) / 2, cy likewise; w = x2 - x1;
 *              h = y2 - y1; each of the four is multiplied by s_l, then rounded once to float32 into pred[b, a, 0:4].
 *   E3         pred[b, a, 4] = 1.0f.
 *   E4         pred[b, a, 5 + c] = fl32(1 / (1 + exp(-x))) with x = cls_l[b, c, i, j].
 * Training (evrep_dethead_train).
 *   T1         pred_scores[b, a, c] is the value of E4.
 *   T2         pred_distri[b, a, ch] = reg_l[b, ch, i, j], a bit copy.
 * Backward (evrep_dethead_train_backward): torch's sigmoid_backward on the stored output, in float32, one operation per
 * statement.
 *              gcls_l[b, c, i, j] = (g * (1 - p)) * p with g = grad_scores[b, a, c] and p the stored pred_scores[b, a, c];
 *              greg_l[b, ch, i, j] = grad_distri[b, a, ch], a bit copy.
 *              grad_scores with all gcls, or grad_distri with all greg, may be NULL together: that half is skipped
 *              (pred_scores may then be NULL too); both halves NULL is EVREP_EINVAL.
 * Inputs must be finite: NaN and infinities do not fault, their results are unspecified.  Large finite logits are inside
 * the contract.
 * levels_host HOST [L], read before the call returns and passed to the kernel by value; its cls / reg / gcls / greg DEVICE,
 * 4-byte aligned.  pred DEVICE float [B,N,5+nc]; pred_scores DEVICE float [B,A,nc]; pred_distri DEVICE float [B,A,4K];
 * grad_scores, grad_distri DEVICE float of the same shapes.  Every element of every output is written on every call.
 * 1 <= B <= 65535, 1 <= nc <= EVREP_TAL_MAX_CLASSES, 0 <= R <= EVREP_DETLOSS_MAX_REG (1 <= R with EVREP_DETHEAD_USE_DFL),
 * h, w >= 1, N <= EVREP_TAL_MAX_ANCHORS, stride finite and > 0; anything else, an unknown flag, a NULL required pointer or a
 * pointer not aligned to 4 bytes is EVREP_EINVAL before any launch.  One launch each: a workgroup stages a tile of
 * EVREP_DETHEAD_TILE consecutive anchors of one (image, level) in LDS and moves its rows as one contiguous span, 16 bytes per
 * lane between the span's 16-byte boundaries.  No scratch, no atomics, no allocation, no wait for the device, nothing read
 * back: the calls may be captured into a graph, and two calls give equal bits.
 * The *_typed entries (16-BIT MAPS above): the maps cls_l / reg_l / gcls_l / greg_l of a call share ONE dtype, given by its
 * code; W1 stands in front of E1-E4 and T1, T2 becomes "the exact widening" instead of "a bit copy", and W2 stands behind both
 * backward rules (greg_l is grad_distri rounded once).  pred, pred_scores, pred_distri, grad_scores, grad_distri stay float32. */
typedef struct { const float *cls; const float *reg; int32_t h, w; float stride; } evrep_dethead_level;
typedef struct { float *gcls; float *greg; int32_t h, w; } evrep_dethead_grad_level;
typedef struct { const void *cls; const void *reg; int32_t h, w; float stride; } evrep_dethead_level_typed;
typedef struct { void *gcls; void *greg; int32_t h, w; } evrep_dethead_grad_level_typed;
#define EVREP_DETHEAD_USE_DFL 1u
#define EVREP_DETHEAD_MAX_LEVELS 8
#define EVREP_DETHEAD_TILE 64
int evrep_dethead_predict(const evrep_dethead_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags,
                          float *pred, void *stream);
int evrep_dethead_train(const evrep_dethead_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags,
                        float *pred_scores, float *pred_distri, void *stream);
int evrep_dethead_train_backward(const evrep_dethead_grad_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                                 uint32_t flags, const float *pred_scores, const float *grad_scores, const float *grad_distri,
                                 void *stream);
int evrep_dethead_predict_typed(const evrep_dethead_level_typed *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                                uint32_t flags, int32_t dtype, float *pred, void *stream);
int evrep_dethead_train_typed(const evrep_dethead_level_typed *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                              uint32_t flags, int32_t dtype, float *pred_scores, float *pred_distri, void *stream);
int evrep_dethead_train_backward_typed(const evrep_dethead_grad_level_typed *levels_host, int32_t L, int32_t B, int32_t nc,
                                       int32_t R, uint32_t flags, int32_t dtype, const float *pred_scores,
                                       const float *grad_scores, const float *grad_distri, void *stream);

/* What is left of the training step behind loss.backward() (ev-YOLOv6/yolov6/core/engine.py:547-552): scaler.step(optimizer)
 * with torch's Nesterov SGD behind it (solver/build.py), scaler.update() and ModelEMA.update(model) (yolov6/utils/ema.py:30-41),
 * for all tensors of a model at once.  float32 parameters and gradients only.
 *   tensors    DEVICE [n_tensors] evrep_step_tensor, 8-byte aligned: p the parameter (or, with EVREP_STEP_EMA_ONLY, the model's
 *              entry of a buffer such as BN running statistics, which is only read), g its gradient, buf its momentum buffer, ema
 *              the EMA model's entry, all DEVICE float [n], 4-byte aligned; n >= 0, and a tensor of 0 elements has no chunk;
 *              group its row of the hyper row; flags: EVREP_STEP_HAS_GRAD (g is given and the tensor is stepped; buf is given
 *              too unless the group's momentum is 0 on every call that uses the table), EVREP_STEP_HAS_EMA (ema is given),
 *              EVREP_STEP_EMA_ONLY (p is read, only ema is written; g and buf are ignored).  A pointer its flags do not ask
 *              for may be NULL.  The arrays of different tensors, and the four of one tensor, do not overlap.
 *   chunks     DEVICE [n_chunks] evrep_step_chunk, 8-byte aligned: elements [first, first + count) of tensor `tensor`,
 *              1 <= count <= EVREP_STEP_CHUNK; every element of every tensor lies in exactly one chunk.  One workgroup per chunk.
 *   hyper      DEVICE float [EVREP_STEP_HYPER_EMA + 3 * n_groups]: ema_d = fl32(decay), ema_1md = fl32(1 - decay) with the
 *              subtraction in double, then per group lr, momentum, weight_decay, each rounded to float32 once.
 *   amp        DEVICE int32 [EVREP_STEP_AMP_WORDS] or NULL (no scaler): found_inf (0 between calls), scale (the bits of a
 *              float32), growth_tracker.
 *   applied    DEVICE int32 [1]: applied_steps, the steps that were not skipped.
 * evrep_train_step is three launches, ordered by the stream:
 *   check      (with amp, without EVREP_STEP_NO_CHECK) found_inf = 1 if any element of any g with HAS_GRAD is NaN or an infinity:
 *              the scaled gradient as stored, what _amp_foreach_non_finite_check_and_unscale_ tests.  An integer atomic.
 *   apply      per element, every statement ONE float32 operation, rounded on its own, in this order:
 *                inv = fl32(1 / double(scale)); 1 without amp
 *                if found_inf == 0 and HAS_GRAD:
 *                  g' = g * inv
 *                  d  = weight_decay != 0 ? g' + weight_decay * p : g'
 *                  momentum != 0:  buf = applied_steps == 0 ? d : buf * momentum + d;   d2 = d + momentum * buf
 *                  momentum == 0:  d2 = d, buf is neither read nor written
 *                  p  = p + (-lr) * d2
 *                if HAS_EMA:  e = e * ema_d;  e = e + ema_1md * p      (p the value just written; also when the step was skipped)
 *                with EVREP_STEP_ZERO_GRAD and HAS_GRAD:  g = +0.0     (also when the step was skipped)
 *              On the first applied step buf is not read: it may be uninitialised, as torch leaves it absent.  A first step that
 *              was skipped leaves it so.  (A buffer of -0.0 is the same as an absent one: -0.0 * momentum + d == d bit for bit.)
 *   finish     one thread.  With amp and without EVREP_STEP_KEEP_SCALE, _amp_update_scale_'s automaton: found_inf != 0:
 *              scale = fl32(double(scale) * backoff), tracker = 0; else s = tracker + 1; s == growth_interval:
 *              scale = fl32(double(scale) * growth) if that is finite, tracker = 0; else tracker = s.
 *              Then applied_steps += (found_inf == 0) and found_inf = 0.
 *   EVREP_STEP_NO_CHECK with EVREP_STEP_KEEP_SCALE is the route of a foreign scaler that has made its own check: the caller
 *   writes found_inf and scale into amp before the call and keeps updating the scale itself.
 * evrep_ema_update is the apply launch with every tensor taken as EVREP_STEP_EMA_ONLY: only hyper[0], hyper[1], p and ema are
 * read and only ema is written.
 * The aligned body of a chunk moves 16 bytes per lane, with 4-byte accesses for the 0..3 elements in front of p's 16-byte
 * boundary and behind the last whole group; an array that does not share p's offset from a 16-byte boundary moves in 4-byte
 * accesses.  No access lies outside [first, first + count) of any array.  The tables are the caller's statement: a chunk that
 * does not fit its tensor, a group >= n_groups, or a momentum != 0 for a tensor without buf is skipped whole and nothing else
 * is checked on the device.
 * 0 <= n_tensors, 0 <= n_chunks < 2^31 (0: no apply launch), 1 <= n_groups <= EVREP_STEP_MAX_GROUPS; with amp and without
 * EVREP_STEP_KEEP_SCALE growth and backoff finite and > 0 and growth_interval >= 1; anything else, an unknown flag, a NULL
 * required pointer or a misaligned one is EVREP_EINVAL before any launch.  No scratch, no floating-point atomic, no grid-wide
 * barrier, no allocation, no wait for the device, nothing read back: the calls may be captured into a graph, and two calls
 * give equal bits. */
typedef struct { float *p; float *g; float *buf; float *ema; int64_t n; int32_t group; uint32_t flags; } evrep_step_tensor;
typedef struct { int64_t first; int32_t tensor; int32_t count; } evrep_step_chunk;
#define EVREP_STEP_HAS_GRAD 1u
#define EVREP_STEP_HAS_EMA 2u
#define EVREP_STEP_EMA_ONLY 4u
#define EVREP_STEP_ZERO_GRAD 1u
#define EVREP_STEP_NO_CHECK 2u
#define EVREP_STEP_KEEP_SCALE 4u
#define EVREP_STEP_CHUNK 4096
#define EVREP_STEP_MAX_GROUPS 16
#define EVREP_STEP_HYPER_EMA 2
#define EVREP_STEP_AMP_WORDS 3
int evrep_train_step(const evrep_step_tensor *tensors, int32_t n_tensors, const evrep_step_chunk *chunks, int64_t n_chunks,
                     const float *hyper, int32_t n_groups, int32_t *amp, int32_t *applied_steps, double growth, double backoff,
                     int32_t growth_interval, uint32_t flags, void *stream);
int evrep_ema_update(const evrep_step_tensor *tensors, int32_t n_tensors, const evrep_step_chunk *chunks, int64_t n_chunks,
                     const float *hyper, void *stream);

/* ev-licious' Events.render (ev-licious/src/evlicious/io/utils/render.py:9-141) for B windows of integer coordinates: two calls,
 * one stream builder over the binned records and one streaming launch.  Neither allocates, waits for the device or reads a
 * size on the host: both may be captured into a graph.  Limits: B <= 65535, H * W * 4 < 2^31.
 *
 * evrep_render_state: requires evrep_bin_events on the same plan and workspace, as every builder.  `state` is a caller-owned
 *   tensor with this meaning (as `prim` is between evrep_polstats and evrep_dist), one byte per pixel:
 *     bit 0  some event of the pixel has p > 0          bit 1  some event has p <= 0
 *     bit 2  the pixel's LAST event in array order has p > 0 (the reversed first-visit loop of _render_no_overlap_numba)
 *     bit 3  set on every pixel of a window of <= 2 rows: _render_timesurface returns zeros for such a window
 *   net (or NULL): #positive - #negative events of the pixel (_render_event_frame's np.add.at of p in {-1, +1}).
 *   surface (or NULL): the image of _render_timesurface before the colour map: per event in array order
 *     img = fl32(double(img) + v),  v = exp(-(t[-1] - t) / tau) in float64 (a division, an exponential, nothing fused), t[-1]
 *     the t of the window's last ROW; tau > 0 (3e4 in the reference), only read with surface.  One lane per pixel adds at a
 *     time, elected in array order: no floating-point atomic.
 *   Every element of every given tensor is written exactly once, 0 where no event fell.  Only array order matters: timestamps
 *   need not ascend.  A window with out-of-frame rows (x + y * W outside [0, H * W), as for every builder) keeps EVREP_ST_OOB in
 *   its status word and contributes its in-frame events.
 *   After the call the window statistics of the workspace (what evrep_read_status copies) are merged on the device under every
 *   binning pass.  state, net, surface DEVICE [B,H,W], 4-byte aligned.
 * evrep_render_compose: state (+ net / surface + canvas) -> frames, `type` one of EVREP_RENDER_*  (RenderingType's values).
 *     RED_BLUE_OVERLAP         a pixel with events: (255 if bit 1, 0, 255 if bit 0)
 *     RED_BLUE_NO_OVERLAP      a pixel with events: (0, 0, 255) if bit 2 else (255, 0, 0)
 *     BLACK_WHITE_NO_OVERLAP   a pixel with events: 255 x 3 if bit 2 else 0 x 3
 *       a pixel without events: the canvas' pixel; canvas DEVICE uint8 [B,H,W,3] (canvas_is_batched 1) or [H,W,3] for every
 *       window (0), or NULL = white.  out never aliases canvas.
 *       flags EVREP_RENDER_JITTER (cast=False, _jitter_events: every event also at (x, y+1), (x+1, y), (x+1, y+1), clipped to the
 *       frame, the four copies concatenated): a 2 x 2 stencil over the state; for output pixel (y, x) the sources are, latest
 *       copy first, (y-1, x-1), (y, x-1), (y-1, x), (y, x): OVERLAP takes the union of their bits 0 and 1, the NO_OVERLAP types
 *       bit 2 of the first source that has an event.
 *     EVENT_FRAME              needs net: uint8(clip(20 * net + 128, 0, 255)) on three channels; canvas is ignored
 *     TIME_SURFACE             needs surface and lut (DEVICE double [256][4], 8-byte aligned): out = lut[min(int(img * 256), 255)],
 *       the product in float32 (matplotlib's Colormap.__call__ on a float image); a window of <= 2 rows (bit 3): zeros, alpha
 *       included; canvas is ignored
 *   out DEVICE, 16-byte aligned: uint8 [B,H,W,3], colours in the reference's channel order as stored; TIME_SURFACE: double
 *   [B,H,W,4].  EVREP_RENDER_JITTER with EVENT_FRAME or TIME_SURFACE is EVREP_EINVAL (the reference ignores cast there: pass
 *   0).  Every violation of the above is EVREP_EINVAL before any launch. */
#define EVREP_RENDER_RED_BLUE_OVERLAP 1
#define EVREP_RENDER_RED_BLUE_NO_OVERLAP 2
#define EVREP_RENDER_BLACK_WHITE_NO_OVERLAP 3
#define EVREP_RENDER_TIME_SURFACE 4
#define EVREP_RENDER_EVENT_FRAME 5
#define EVREP_RENDER_JITTER 1u
int evrep_render_state(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                       uint8_t *state, int32_t *net, float *surface, double tau, void *stream);
int evrep_render_compose(const uint8_t *state, const int32_t *net, const float *surface, const double *lut,
                         const uint8_t *canvas, int32_t canvas_is_batched, int32_t B, int32_t H, int32_t W, int32_t type,
                         uint32_t flags, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EVREP_H_ */
