#!/usr/bin/env python3
"""Scratch sizes as a published contract: what every evrep_*_scratch_bytes function of libevrep.so returns for a handful of
argument tuples -- one per edge of its formula (a refused argument, the stated maximum and one beyond, sizes either side of
a multiple of the 128-point tile / of 256 bytes) -- written to scratch_sizes.json.  Run it on the library of the commit whose
sizes are to be kept (EVREP_LIB_PATH names another build than the tree's); tests/test_capi_cpu.py holds every later
library to the numbers.  No device is needed: the functions are host arithmetic."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from event_representation_study_amd import _lib  # noqa: E402

CASES = {
    # (n, m): the 128-point tile of max(n, m), and of each cloud
    "evrep_gwd_scratch_bytes": [(0, 10), (10, -1), (1, 1), (128, 128), (129, 128), (128, 257), (300, 257), (12500, 14400)],
    # (P, ds, dt, n_cap, m_cap): the split form up to 15 dimensions, float32 beyond; 32 is the last dimension
    "evrep_gwd_batch_scratch_bytes": [(0, 4, 14, 100, 100), (1, 0, 14, 100, 100), (1, 4, 33, 100, 100), (1, 4, 14, 0, 100),
                                      (1, 4, 4, 128, 128), (3, 4, 14, 129, 128), (3, 15, 15, 300, 257), (3, 16, 15, 300, 257),
                                      (144, 4, 14, 1250, 1440), (65535, 32, 32, 1, 1), (65536, 32, 32, 1, 1)],
    "evrep_otmi_scratch_bytes": [(0,), (-1,), (1,), (2,), (3,), (64,), (65535,)],
    # (n, m, precision): a row of a multiple of 512 bytes is padded
    "evrep_gw_scratch_bytes": [(0, 4, 0), (4, 0, 1), (1, 1, 0), (1, 1, 1), (63, 65, 0), (64, 64, 0), (64, 128, 1), (128, 64, 1),
                               (129, 127, 1), (1000, 500, 0), (1000, 500, 2)],
    # (B, H, W, bins)
    "evrep_voxel_normalize_scratch_bytes": [(0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 8, 17), (65536, 8, 8, 2), (1, 46341, 46341, 1),
                                            (1, 8, 8, 2), (2, 480, 640, 5), (3, 8, 8, 16), (65535, 1, 1, 1)],
    # (total_events, nseg): slices of 1024 events, 512 rows at the most
    "evrep_est_backward_scratch_bytes": [(-1, 4), (0, 0), (0, 8193), (0, 1), (1024, 16), (1025, 16), (1025, 17), (524288, 8),
                                         (524289, 8), (1 << 30, 8192)],
    # (n, B)
    "evrep_est_prepare_scratch_bytes": [(0, 1), (1, 0), (1, 65536), (1, 1), (1, 63), (1, 64), (1000, 127), (1000, 128), (1000, 65535)],
    # (B, total)
    "evrep_filter_compact_scratch_bytes": [(0, 10), (1, -1), (1, 0), (32, 1 << 20), (65536, 1 << 31)],
    "evrep_decode_scratch_bytes": [(-1,), (0,), (1,), (1 << 30,)],
    "evrep_nimg_prepare_scratch_bytes": [(0, 10), (1, -1), ((1 << 24) + 1, 10), (1, 0), (5, 10), (8, 10), (64, 1 << 31), (1 << 24, 10)],
    # (B, H, W): 2B thresholds and 2B * H * W times, each rounded up to 256 bytes
    "evrep_dist_scratch_bytes": [(0, 8, 8), (1, 0, 8), (1, 8, 4097), ((1 << 20) + 1, 8, 8), (1 << 20, 4096, 4096), (1, 1, 1), (1, 8, 8),
                                 (32, 8, 8), (33, 7, 9), (4, 480, 640)],
    # (S, total)
    "evrep_dense_rank_scratch_bytes": [(0, 10), (1, -1), ((1 << 24) + 1, 10), (1, (1 << 40) + 1), (1, 0), (1, 64), (2, 65), (1 << 24, 1 << 40)],
    # (B, total)
    "evrep_time_index_scratch_bytes": [(0, 10), (-1, 10), ((1 << 20) + 1, 10), (1, -1), (1, 1 << 32), (1, 0), (64, 10), (65, 10),
                                       (1 << 20, (1 << 32) - 1)],
    # (B, H, W, K)
    "evrep_sort_image_scratch_bytes": [(0, 8, 8, 1), (1, 8, 8, 0), (1, 8, 8, 3), (1, 4097, 8, 1), ((1 << 20) + 1, 8, 8, 1), (1, 1, 1, 1),
                                       (1, 8, 8, 1), (1, 8, 8, 2), (3, 7, 9, 2), (2, 480, 640, 2)],
    "evrep_nimg_study_rows_scratch_bytes": [(0, 10), (1, -1), ((1 << 24) + 1, 10), (1, 0), (3, 10), (4, 10), (5, 10), (1 << 24, 1 << 31)],
    "evrep_detector_input_frames_scratch_bytes": [(0,), (65536,), (1,), (3,), (65535,)],
}

if __name__ == "__main__":
    lib = _lib.load()
    assert sorted(CASES) == sorted(name for name in _lib.SYMBOLS if name.endswith("_scratch_bytes")), "every size function"
    out = {name: [[list(args), int(getattr(lib, name)(*args))] for args in CASES[name]] for name in sorted(CASES)}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "scratch_sizes.json"), "w") as f:
        f.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(name), json.dumps(rows)) for name, rows in out.items()) + "\n}\n")   # a line per function
    print(open(f.name).read())
