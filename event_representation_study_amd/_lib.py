"""ctypes binding of libevrep.so (the C ABI declared in include/evrep.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing
a builder raises.  (The library is built in-tree by ``event_representation_study_amd.build``.)
"""
import ctypes
import os
import types

# torch bundles its own libamdhip64.so.7; it must be the process's HIP runtime (same SONAME as /opt/rocm's) before
# libevrep.so is loaded, otherwise device pointers / streams from torch are foreign to our launches.
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EVREP_LIB_PATH") or os.path.join(_PKG, "libevrep.so")  # env override: A/B builds

EVREP_OK, EVREP_EINVAL, EVREP_EWORKSPACE, EVREP_EHIP, EVREP_ENOTBINNED = 0, 1, 2, 3, 4
ST_EMPTY, ST_OOB, ST_UNSORTED, ST_FLAT_TIME, ST_HOT_OVERFLOW = 1, 2, 4, 8, 16
F64, F32 = 0, 1
MAX_CHANNELS = 16
MAX_DIM = 4096
ABI_VERSION = 3

FUNCS = ["timestamp", "polarity", "count", "timestamp_pos", "timestamp_neg", "count_pos", "count_neg"]
AGGS = ["sum", "mean", "max", "variance"]


class Plan(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("total_events", ctypes.c_int64),
        ("max_events_per_window", ctypes.c_int64),
        ("chunk", ctypes.c_int32), ("nblk", ctypes.c_int32),
        ("nchunk", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("pacing", ctypes.c_int32),
        ("off_meta", ctypes.c_size_t), ("off_table", ctypes.c_size_t), ("off_stats", ctypes.c_size_t),
        ("off_rowoff", ctypes.c_size_t),
        ("off_chunkoff", ctypes.c_size_t),
        ("off_sorted1", ctypes.c_size_t), ("off_sorted2", ctypes.c_size_t), ("off_cuts", ctypes.c_size_t),
        ("off_scratch", ctypes.c_size_t),
        ("workspace_bytes", ctypes.c_size_t),
    ]


class Status(tuple):
    """A SYMBOLS entry (c_int, argtypes) whose int is an EVREP_* status code: api() gives the function an errcheck."""


def _st(argtypes):
    return Status((ctypes.c_int, argtypes))


# every symbol include/evrep.h declares: name -> (restype, argtypes); _st(argtypes) for the entry points that return a status
_vp, _i32, _i64, _f64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_float
_PP = ctypes.POINTER(Plan)
_I32P = ctypes.POINTER(ctypes.c_int32)
SYMBOLS = {
    "evrep_abi_version": (ctypes.c_int, []),
    "evrep_last_hip_error": (ctypes.c_char_p, []),
    "evrep_plan_init": _st([_PP, _i32, _i32, _i32, _i64, _i64]),
    "evrep_plan_init_ex": _st([_PP, _i32, _i32, _i32, _i64, _i64, ctypes.c_uint32]),
    "evrep_plan_set_pacing": _st([_PP, _i32]),
    "evrep_workspace_bytes": (ctypes.c_size_t, [_PP]),
    "evrep_bin_events": _st([_PP, _vp, _vp, _vp, _vp]),
    "evrep_probe_store": _st([_vp, ctypes.c_size_t, _vp]),
    "evrep_mdes": _st([_PP, _vp, _vp, _vp, _i32, _I32P, _I32P, _I32P, _f64, _i32, _vp, _vp]),
    "evrep_mdes_sbt_windows": _st([_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "evrep_mdes_ex": _st([_PP, _vp, _vp, _vp, _i32, _I32P, _I32P, _I32P, _f64, _i32, _vp, _vp, _vp, _vp]),
    "evrep_optimized": _st([_PP, _vp, _vp, _vp, _f64, _i32, _vp, _vp]),
    "evrep_event_stack": _st([_PP, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp]),
    "evrep_time_surface": _st([_PP, _vp, _vp, _vp, _i32, _vp, _f64, _i32, _f64, _i32, _vp, _vp]),
    "evrep_time_surface_ftime": _st([_PP, _vp, _vp, _vp, _i32, _vp, _vp, _f64, _i32, _f64, _i32, _vp, _vp]),
    "evrep_tore": _st([_PP, _vp, _vp, _vp, _i32, _i32, _vp, _f32, _vp, _vp]),
    "evrep_tore_ftime": _st([_PP, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _f32, _vp, _vp]),
    "evrep_voxel": _st([_PP, _vp, _vp, _vp, _i32, _i32, _f64, _vp, _vp]),
    "evrep_voxel_range": _st([_PP, _vp, _vp, _vp, _i32, _i32, _f64, _vp, _vp, _vp]),
    "evrep_voxel_tnorm": _st([_PP, _vp, _vp, _vp, _vp, _i32, _f64, _vp, _vp]),
    "evrep_voxel_subpixel": _st([_PP, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "evrep_polstats": _st([_PP, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _f64, _vp, _vp]),
    "evrep_est_voxel": _st([_PP, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _f64, _f64, _vp, _vp]),
    "evrep_est_backward_scratch_bytes": (ctypes.c_size_t, [_i64, _i32]),
    "evrep_est_voxel_backward": _st([_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _f64, _f64, _vp, _vp, _vp, _vp]),
    "evrep_est_prepare_scratch_bytes": (ctypes.c_size_t, [_i64, _i32]),
    "evrep_est_prepare": _st([_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evrep_read_status": _st([_PP, _vp, _vp, _vp]),
    "evrep_read_bbox": _st([_PP, _vp, _vp, _vp]),
    "evrep_copy_window_meta_async": _st([_PP, _vp, _vp, _vp]),
    "evrep_gwd_scratch_bytes": (ctypes.c_size_t, [_i64, _i64]),
    "evrep_resize_taps": _st([_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _i32, _vp, _vp]),
    "evrep_gw_scratch_bytes": (ctypes.c_size_t, [_i64, _i64, _i32]),
    "evrep_entropic_gw": _st([_vp, _i64, _vp, _i64, _vp, _vp, _i32, _f64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "evrep_gwd_padded_l1": _st([_vp, _i64, _i32, _vp, _i64, _i32, _f64, _vp, _vp, _vp]),
    "evrep_gwd_batch_scratch_bytes": (ctypes.c_size_t, [_i32, _i32, _i32, _i64, _i64]),
    "evrep_gwd_padded_l1_batch": _st([_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i64, _f64, _vp, _vp, _vp]),
    "evrep_otmi_scratch_bytes": (ctypes.c_size_t, [_i32]),
    "evrep_otmi_event_clouds": _st([_vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp]),
    "evrep_otmi_rep_clouds": _st([_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "evrep_otmi_rep_clouds_bank": _st([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "evrep_filter_pixel_fsm": _st([_PP, _vp, _vp, _vp, _i32, _f64, _vp, _vp, _vp, _vp]),
    "evrep_filter_background": _st([_PP, _vp, _vp, _vp, _f64, _i32, _vp, _vp, _vp, _vp]),
    "evrep_filter_mask_gather": _st([_vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _vp]),
    "evrep_filter_cell_map": _st([_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "evrep_filter_compact_scratch_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "evrep_filter_compact": _st([_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "evrep_time_to_index": _st([_vp, _i64, _vp, _i64, _vp, _vp]),
    "evrep_windows_gather": _st([_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "evrep_nimg_prepare_scratch_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "evrep_nimg_prepare": _st([_vp, _vp, _i32, _vp, _vp, _f64, _f64, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evrep_dist_scratch_bytes": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "evrep_dist": _st([_vp, _i32, _i32, _i32, _f64, _f32, _vp, _vp, _vp]),
    "evrep_dense_rank_scratch_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "evrep_dense_rank_f32": _st([_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "evrep_time_index_scratch_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "evrep_time_index": _st([_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "evrep_sort_image_scratch_bytes": (ctypes.c_size_t, [_i32, _i32, _i32, _i32]),
    "evrep_sort_image": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _I32P, _i32, _vp, _vp, _vp, _vp]),
    "evrep_nimg_study_rows_scratch_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "evrep_nimg_study_rows": _st([_vp, _vp, _vp, _vp, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evrep_detector_input": _st([_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                 _vp, _vp, _vp, _f32, _vp, _vp]),
    "evrep_resize_tap_tables": _st([_vp, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp]),
    "evrep_detector_input_frames_scratch_bytes": (ctypes.c_size_t, [_i32]),
    "evrep_detector_input_frames": _st([_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _f32, _vp, _vp, _vp]),
    "evrep_nms": _st([_vp, _i32, _i32, _i32, _f32, _f64, ctypes.c_uint32, _I32P, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "evrep_det_match": _st([_vp, _vp, _i32, _i32, _vp, _i64, _vp, _i32, _i32, ctypes.POINTER(ctypes.c_float), _i32, ctypes.c_uint32, _vp, _i32,
                            _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evrep_det_ap_workspace_bytes": (ctypes.c_size_t, [_i64, _i32, _i32]),
    "evrep_det_ap": _st([_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                         ctypes.c_size_t, _vp]),
    "evrep_det_ap_gather": _st([_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "evrep_det_targets_pad": _st([_vp, _i64, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "evrep_tal_workspace_bytes": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "evrep_tal_assign": _st([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp]),
    "evrep_atss_workspace_bytes": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "evrep_atss_assign": _st([_vp, _I32P, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp]),
    "evrep_detloss_decode": _st([_vp, _vp, _vp, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp]),
    "evrep_detloss_workspace_bytes": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "evrep_detloss": _st([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f64, _f64, _f64, ctypes.c_uint32, _vp, _vp,
                          _vp, _vp, _vp, _vp]),
    "evrep_detloss_distill_workspace_bytes": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "evrep_detloss_distill": _st([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f64, _f64, _f64, _f64, _f64,
                                  _f64, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "evrep_detloss_cwd_workspace_bytes": (ctypes.c_size_t, [_vp, _i32]),
    "evrep_detloss_cwd": _st([_vp, _i32, _f64, ctypes.c_uint32, _vp, _vp, _vp]),
    "evrep_dethead_predict": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp]),
    "evrep_dethead_train": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp]),
    "evrep_dethead_train_backward": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "evrep_cast16_host": _st([_vp, _vp, _i64, _i32, _i32]),
    "evrep_detloss_cwd_typed_workspace_bytes": (ctypes.c_size_t, [_vp, _i32]),
    "evrep_detloss_cwd_typed": _st([_vp, _i32, _f64, ctypes.c_uint32, _i32, _i32, _vp, _vp, _vp]),
    "evrep_dethead_predict_typed": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _i32, _vp, _vp]),
    "evrep_dethead_train_typed": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _i32, _vp, _vp, _vp]),
    "evrep_dethead_train_backward_typed": _st([_vp, _i32, _i32, _i32, _i32, ctypes.c_uint32, _i32, _vp, _vp, _vp, _vp]),
    "evrep_train_step": _st([_vp, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _f64, _f64, _i32, ctypes.c_uint32, _vp]),
    "evrep_ema_update": _st([_vp, _i32, _vp, _i64, _vp, _vp]),
    "evrep_voxel_normalize_scratch_bytes": (ctypes.c_size_t, [_i32, _i32, _i32, _i32]),
    "evrep_voxel_normalize": _st([_vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "evrep_decode_scratch_bytes": (ctypes.c_size_t, [_i64]),
    "evrep_decode_state_init": _st([_vp, _vp]),
    "evrep_decode_dat": _st([_vp, _i64, _i32, _i64, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "evrep_decode_bin5": _st([_vp, _i64, _i64, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "evrep_dat_seek_time": _st([_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "evrep_render_state": _st([_PP, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _vp]),
    "evrep_render_compose": _st([_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp]),
}
# evrep_render_compose: RenderingType's values, the flag of cast=False
RENDER_RED_BLUE_OVERLAP, RENDER_RED_BLUE_NO_OVERLAP, RENDER_BLACK_WHITE_NO_OVERLAP, RENDER_TIME_SURFACE, RENDER_EVENT_FRAME = 1, 2, 3, 4, 5
RENDER_JITTER = 1
# evrep_decode_dat / evrep_decode_bin5: modes, the overrun bit of the state's n_in, the fields of the state, the largest n
DECODE_STRICT, DECODE_DROP_OOB = 0, 1
DECODE_N_IN_OVERRUN = 1 << 62
DECODE_STATE_FIELDS = ("n_in", "n_out", "oob_count", "oob_first", "desc_count", "desc_first", "t_first", "t_last")
DECODE_MAX_N = 1 << 30
# evrep_voxel_normalize: flags
VOXNORM_NORMALIZE = 1
# evrep_time_index / evrep_sort_image: modes, per-window status bits (NO_INDEX << polarity class), flags, limits
TIME_INDEX_RAW, TIME_INDEX_RANK = 0, 1
SORT_EMPTY, SORT_DECREASING, SORT_NO_INDEX = 1, 2, 4
SORT_STRICT, SORT_USE_IMAGE = 1, 2
SORT_MAX_B, SORT_MAX_Q = 1 << 20, 16
# evrep_nimg_study_rows: the row sets to write, per-window status bits
STUDY_MDES, STUDY_STACK, STUDY_TORE = 1, 2, 4
STUDY_EMPTY, STUDY_FUTURE, STUDY_T_RANGE, STUDY_FLAT, STUDY_UNORDERED = 1, 2, 4, 8, 16
# evrep_est_voxel_backward: the largest piecewise-linear table (its 2 * nseg float64 sums live in LDS)
EST_BWD_MAX_SEG = 8192
# evrep_est_prepare: status bits, the largest B
EST_PREP_DESCENDING, EST_PREP_BAD_INDEX, EST_PREP_BAD_POLARITY, EST_PREP_OUT_OF_FRAME = 1, 2, 4, 8
EST_PREP_MAX_B = 65535
# evrep_detector_input: per-sample flags
DETIN_WARP, DETIN_FLIPUD, DETIN_FLIPLR = 1, 2, 4
# evrep_nms: flags, limits
NMS_MULTI_LABEL, NMS_AGNOSTIC = 1, 2
NMS_MAX_DET, NMS_MAX_CLASSES, NMS_MAX_ROWS = 1024, 4096, 1 << 24
# evrep_det_match: flags, limits, per-image status bits
DETEVAL_NATIVE, DETEVAL_SKIP_EMPTY = 1, 2
DETEVAL_MAX_LABELS, DETEVAL_MAX_T, DETEVAL_MAX_TARGETS = 1024, 16, 1 << 24
DETEVAL_ST_LABEL_OVERFLOW, DETEVAL_ST_BAD_CLASS, DETEVAL_ST_BAD_COUNT = 1, 2, 4
# evrep_det_ap: the rows of a radix tile and of a scan tile, the status bits, the points of the curves and of compute_ap
AP_SORT_TILE, AP_SCAN_TILE = 2048, 512
AP_GATHER_CHUNK, AP_GATHER_IMAGES = 1024, 256      # evrep_det_ap_gather: targets / images per round of its second launch, images per round of its first
AP_ST_BAD_CLASS, AP_ST_NAN_CONF = 1, 2
AP_PX, AP_X = 1000, 101
# evrep_det_targets_pad / evrep_tal_assign: flag, limits, per-image status bits
TAL_F32_OUT = 1
TAL_MAX_TOPK, TAL_MAX_LABELS, TAL_MAX_CLASSES, TAL_MAX_ANCHORS, TAL_MAX_POWER = 64, 1024, 4096, 1 << 24, 16
TAL_ST_LABEL_OVERFLOW, TAL_ST_BAD_CLASS, TAL_ST_NONFINITE = 1, 2, 4
# evrep_atss_assign: flags, limits (the shapes' limits and the status bits are the TAL ones)
ATSS_F32_BOXES, ATSS_F32_SCORES = 1, 2
ATSS_MAX_TOPK, ATSS_MAX_LEVELS, ATSS_MAX_CANDIDATES = 32, 8, 256
# evrep_detloss_decode / evrep_detloss: flags, the greatest reg_max, per-image status bit
DETLOSS_USE_DFL, DETLOSS_NO_GRAD, DETLOSS_F32_TARGETS = 1, 2, 4
DETLOSS_MAX_REG = 32
DETLOSS_ST_BAD_LABEL = 1
# evrep_detloss_distill: the most classes; evrep_detloss_cwd: the most levels, the longest row that is staged in LDS
DISTILL_MAX_CLASSES = 2048
CWD_MAX_LEVELS, CWD_STAGE = 3, 4096
# evrep_dethead_*: flag, the most levels, the anchors of a staged tile
DETHEAD_USE_DFL = 1
DETHEAD_MAX_LEVELS, DETHEAD_TILE = 8, 64
# the *_typed entries: the dtype codes of the maps (DetheadLevel, DetheadGradLevel and CwdLevel hold plain addresses and serve
# the typed entries as they are: the typed structs of the header differ in their pointee types only)
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
MAP_DTYPES = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
# evrep_train_step / evrep_ema_update: per-tensor flags, the call's flags, the elements of a chunk, the most groups, the words
# of the hyper row in front of the groups' (lr, momentum, weight_decay), the words of the scaler's state
STEP_HAS_GRAD, STEP_HAS_EMA, STEP_EMA_ONLY = 1, 2, 4
STEP_ZERO_GRAD, STEP_NO_CHECK, STEP_KEEP_SCALE = 1, 2, 4
STEP_CHUNK, STEP_MAX_GROUPS, STEP_HYPER_EMA, STEP_AMP_WORDS = 4096, 16, 2, 3
# evrep_resize_tap_tables: interpolation codes; the columns of an axis descriptor
TAPS_LINEAR, TAPS_AREA, TAPS_IDENTITY = 0, 1, 2
TAPS_AXIS_FIELDS = 6


class DetinFrame(ctypes.Structure):
    """evrep_detin_frame: one sample of evrep_detector_input_frames."""
    _fields_ = [("src", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("rh", ctypes.c_int32), ("rw", ctypes.c_int32), ("T1", ctypes.c_int32),
                ("row1", ctypes.c_int32), ("col1", ctypes.c_int32), ("wrow1", ctypes.c_int32), ("wcol1", ctypes.c_int32),
                ("nh", ctypes.c_int32), ("nw", ctypes.c_int32), ("T2", ctypes.c_int32),
                ("row2", ctypes.c_int32), ("col2", ctypes.c_int32), ("wrow2", ctypes.c_int32), ("wcol2", ctypes.c_int32),
                ("top", ctypes.c_int32), ("left", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


class DetheadLevel(ctypes.Structure):
    """evrep_dethead_level: one level of evrep_dethead_predict / evrep_dethead_train."""
    _fields_ = [("cls", ctypes.c_void_p), ("reg", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("stride", ctypes.c_float)]


class CwdLevel(ctypes.Structure):
    """evrep_cwd_level: one level of evrep_detloss_cwd."""
    _fields_ = [("s", ctypes.c_void_p), ("t", ctypes.c_void_p), ("grad_s", ctypes.c_void_p), ("n", ctypes.c_int32), ("c", ctypes.c_int32),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class DetheadGradLevel(ctypes.Structure):
    """evrep_dethead_grad_level: one level of evrep_dethead_train_backward."""
    _fields_ = [("gcls", ctypes.c_void_p), ("greg", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class StepTensor(ctypes.Structure):
    """evrep_step_tensor: one tensor of evrep_train_step / evrep_ema_update."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("buf", ctypes.c_void_p), ("ema", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("group", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class StepChunk(ctypes.Structure):
    """evrep_step_chunk: count elements of a tensor from its element `first` on."""
    _fields_ = [("first", ctypes.c_int64), ("tensor", ctypes.c_int32), ("count", ctypes.c_int32)]


# evrep_dist / evrep_dense_rank_f32: limits
DIST_MAX_B, RANK_MAX_SEGMENTS = 1 << 20, 1 << 24
# evrep_nimg_prepare: mode flags, per-window parameter flags, per-window status bits
NIMG_TRAIN, NIMG_P_UINT8 = 1, 2
AUG_TIME_FLIP, AUG_X_FLIP = 1, 2
AUG_EMPTY, AUG_FLAT_TIME, AUG_BAD_SLICE = 1, 2, 4
# evrep_windows_gather: rebase modes, per-window status bits, limits
REBASE_NONE, REBASE_FIRST, REBASE_GIVEN = 0, 1, 2
WST_BAD_RANGE, WST_T_OVERFLOW, WST_BAD_OFFSETS = 1, 2, 4
WINDOWS_MAX_QUERIES, WINDOWS_MAX_B = 1 << 30, 1 << 24
# evrep_filter_pixel_fsm kinds
FILTER_REFRACTORY, FILTER_CONTRAST, FILTER_CHANGE_MAP = 0, 1, 2
FILTER_MAX_RADIUS = 4

# evrep_plan_init_ex flags.  The C library reads no environment variable; the A/B switches of the tests and tools
# are translated here, when a plan is made.
# (tests/test_capi_cpu.py holds this table to the EVREP_PLAN_* defines of include/evrep.h, name for name)
PLAN_NO_KEY_PASS = 1
PLAN_THREE_KERNEL = 2
PLAN_FORCE_KEY_SORTED = 4
PLAN_BIG_BLOCKS = 8
PLAN_NO_FUSED_SCATTER = 16
PLAN_X_SPAN2 = 64
PLAN_X_STAGE128 = 128
PLAN_X_TAIL_MERGE = 256
PLAN_X_STAGE64 = 512
PLAN_X_HANDOVER2 = 1024
PLAN_X_HANDOVER_DENSE = 2048
PLAN_X_NO_SWEEP_MAIN = 4096
PLAN_X_NO_MONSTER_HANDOVER = 8192
PLAN_X_VOXEL_ORDERED = 16384
PLAN_X_TORE_ORDERED = 32768
PLAN_X_POLSTATS_ORDERED = 65536
PLAN_X_ESTACK_ORDERED = 131072
PLAN_X_MDES_ORDERED = 262144
PLAN_X_MDES_STREAM = 524288
PLAN_X_TS_STREAM = 1048576
PLAN_X_TS_ORDERED = 2097152
PLAN_X_MDES_NO_COOP = 4194304
_ENV_FLAGS = (
    ("EVREP_BIN_CLASSIC", PLAN_NO_KEY_PASS),
    ("EVREP_BIN_THREE_KERNEL", PLAN_THREE_KERNEL),
    ("EVREP_BIN_KEY_SORTED", PLAN_FORCE_KEY_SORTED),
    ("EVREP_KS_BIG_BLOCKS", PLAN_BIG_BLOCKS),
    ("EVREP_NO_FUSED_SCATTER", PLAN_NO_FUSED_SCATTER),
    ("EVREP_X_SPAN2", PLAN_X_SPAN2),
    ("EVREP_X_STAGE128", PLAN_X_STAGE128),
    ("EVREP_X_TAIL_MERGE", PLAN_X_TAIL_MERGE),
    ("EVREP_X_STAGE64", PLAN_X_STAGE64),
    ("EVREP_X_HANDOVER2", PLAN_X_HANDOVER2),
    ("EVREP_X_HANDOVER_DENSE", PLAN_X_HANDOVER_DENSE),
    ("EVREP_X_NO_SWEEP_MAIN", PLAN_X_NO_SWEEP_MAIN),
    ("EVREP_X_NO_MONSTER_HANDOVER", PLAN_X_NO_MONSTER_HANDOVER),
    ("EVREP_X_VOXEL_ORDERED", PLAN_X_VOXEL_ORDERED),
    ("EVREP_X_TORE_ORDERED", PLAN_X_TORE_ORDERED),
    ("EVREP_X_POLSTATS_ORDERED", PLAN_X_POLSTATS_ORDERED),
    ("EVREP_X_ESTACK_ORDERED", PLAN_X_ESTACK_ORDERED),
    ("EVREP_X_MDES_ORDERED", PLAN_X_MDES_ORDERED),
    ("EVREP_X_MDES_STREAM", PLAN_X_MDES_STREAM),
    ("EVREP_X_TS_STREAM", PLAN_X_TS_STREAM),
    ("EVREP_X_TS_ORDERED", PLAN_X_TS_ORDERED),
    ("EVREP_X_MDES_NO_COOP", PLAN_X_MDES_NO_COOP),
)


# (the per-sample wrappers translate the switches on every call -- a test may flip one between two samples: read CPython's own
#  dictionary behind os.environ instead of twenty-odd os.environ.get calls, 10 us of a 100 us sample)
_ENV_DATA = getattr(os.environ, "_data", None)
try:
    _ENV_KEYS = tuple((os.environ.encodekey(name), bit) for name, bit in _ENV_FLAGS) if isinstance(_ENV_DATA, dict) else None
    _PACING_KEY = os.environ.encodekey("EVREP_PACING") if _ENV_KEYS is not None else None
except AttributeError:
    _ENV_KEYS = _PACING_KEY = None


def plan_flags_from_env():
    flags = 0
    if _ENV_KEYS is not None:
        data = _ENV_DATA
        for key, bit in _ENV_KEYS:
            if data.get(key):
                flags |= bit
        return flags
    for name, bit in _ENV_FLAGS:
        if os.environ.get(name):
            flags |= bit
    return flags


def pacing_from_env():
    """EVREP_PACING: -1 automatic (default), 0 off, > 0 hold in 10 ns ticks (A/B timing only)."""
    if _PACING_KEY is not None and _PACING_KEY not in _ENV_DATA:
        return None
    v = os.environ.get("EVREP_PACING")
    return int(v) if v not in (None, "") else None


_lib = _api = None


class EvrepError(RuntimeError):
    pass


def load():
    """The raw handle: libevrep.so as the C ABI, status codes returned as they are (the C-ABI tests, bench.py and tools call
    it).  Raises (loudly) if the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EvrepError(
            "libevrep.so is missing (%s). Build it with `python -m event_representation_study_amd.build`; "
            "there is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.evrep_abi_version.restype = ctypes.c_int
    lib.evrep_abi_version.argtypes = []
    if lib.evrep_abi_version() != ABI_VERSION and not (os.environ.get("EVREP_LIB_PATH") and os.environ.get("EVREP_ABI_ANY")):   # (before the symbols are bound: a stale library says so, not AttributeError; EVREP_ABI_ANY: A/B timing of an older build through EVREP_LIB_PATH, tools only)
        raise EvrepError("libevrep.so ABI %d != binding ABI %d: rebuild with `python -m event_representation_study_amd.build`"
                         % (lib.evrep_abi_version(), ABI_VERSION))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def api():
    """The checked handle, for the package: a namespace of one function per SYMBOLS entry with the raw handle's argtypes and
    restype; a status other than EVREP_OK raises EvrepError naming the function.  The functions are objects of their own
    (CDLL.__getitem__ makes a fresh one per call), so the raw handle keeps returning codes."""
    global _api
    if _api is None:
        lib, ns = load(), types.SimpleNamespace()
        for name, entry in SYMBOLS.items():
            fn = lib[name]
            fn.restype, fn.argtypes = entry
            if isinstance(entry, Status):
                fn.errcheck = _errcheck
            setattr(ns, name, fn)
        _api = ns
    return _api


def _errcheck(rc, fn, args):
    if rc != EVREP_OK:
        raise EvrepError(failure(rc, fn.__name__))
    return rc


_STATUS_NAMES = {EVREP_EINVAL: "EVREP_EINVAL (bad argument)", EVREP_EWORKSPACE: "EVREP_EWORKSPACE",
                 EVREP_EHIP: "EVREP_EHIP", EVREP_ENOTBINNED: "EVREP_ENOTBINNED"}


def failure(rc, what=""):
    """The text of the EvrepError for status `rc` of the call `what` (check and the checked handle share it)."""
    msg = _STATUS_NAMES.get(rc, "rc=%d" % rc)
    if rc == EVREP_EHIP:
        msg += ": " + (load().evrep_last_hip_error() or b"").decode()
    return "%s failed: %s" % (what or "libevrep call", msg)


def check(rc, what=""):
    """For a status the raw handle returned."""
    if rc != EVREP_OK:
        raise EvrepError(failure(rc, what))


def require_gpu():
    if not torch.cuda.is_available():
        raise EvrepError("no HIP device visible: the builders run on an MI355X only (no CPU fallback)")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """A tensor's address as a c_void_p argument; None stays None (ctypes passes NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def scratch(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def want(t, what, dtype, shape=None, numel=None, device=None):
    """The one check that `t` is the tensor a kernel will read at data_ptr(): a contiguous torch tensor of `dtype` (one, or a
    tuple of them), of `shape` (None entries are free) or of `numel` elements, on `device` (a torch.device, or "cuda" for any
    HIP device).  Returns t; ValueError naming `what` and what was expected otherwise."""
    # (on the per-sample path: a few attribute reads when the tensor is right, the text only when it is not)
    ok = isinstance(t, torch.Tensor) and (t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype) and t.is_contiguous()
    if ok and shape is not None and tuple(t.shape) != shape:
        ok = len(t.shape) == len(shape) and all(s is None or s == v for s, v in zip(shape, t.shape))
    if ok and numel is not None:
        ok = t.numel() == numel
    if ok and device is not None:
        ok = t.is_cuda if device == "cuda" else t.device == device
    if not ok:
        dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
        size = "" if shape is None and numel is None else \
            (" of %d elements" % numel if shape is None else " of shape (%s)" % ", ".join("*" if s is None else str(int(s)) for s in shape))
        raise ValueError("%s must be a contiguous %s tensor%s%s" % (what, " / ".join(str(d) for d in dtypes), size,
                                                                   "" if device is None else " on %s" % (device,)))
    return t


def int32_array(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])
