"""-m gpu: bench.py --dump-outputs writes what the LAST timed step computed -- the whole last window and the seeded
sample of the (B, H, W, 12) output -- bit-exact against the oracle on the windows that step built."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal

pytestmark = pytest.mark.gpu

H, W = 480, 640
DUMP_SAMPLE = 3000000       # bench.DUMP_SAMPLE


@pytest.mark.parametrize("pipeline", [False, True])
def test_dump_outputs_hold_the_last_timed_step(tmp_path, oracle, pipeline):
    from event_representation_study_amd.synthetic import make_events
    B, N, steps = 2, 5000, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--batch", str(B),
           "--events", str(N), "--resident-batches", "2", "--dump-outputs", str(tmp_path)] + (["--pipeline"] if pipeline else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert res["steps"] == steps and res["ms_per_step"] > 0
    # two resident batches alternate, step k builds batch k % 2 (window i of batch j: seed j * B + i): step 3 -> batch 1,
    # while the warm-up step built batch 0
    j = (steps - 1) % 2
    ref = np.stack([oracle.ergo12(make_events(N, W, H, seed=j * B + i), H, W) for i in range(B)])
    assert_bit_equal(np.load(tmp_path / "optimized_last_window.npy"), ref[-1], "last window")
    idx = np.unique(np.random.default_rng(0).integers(0, ref.size, size=DUMP_SAMPLE))
    assert_bit_equal(np.load(tmp_path / "optimized_sample.npy"), ref.reshape(-1)[idx], "sample")
