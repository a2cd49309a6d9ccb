"""GPU: bench.py on one GPU, plain and with --full.  A plain run carries the headline and nothing that needs a run of its own; --full adds the
secondary legs, post passes and CPU baselines after the same timed steps, which compute the same outputs either way."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "kernel_ms_per_step", "roofline")
FULL_ONLY = ("plain_batches", "chain2", "plain_two_in_flight", "per_sample", "per_sample_xoroshiro", "group_fold", "host_default",
             "host_buffer_ms_per_step", "host_buffer_chain_ms_per_step", "post_passes", "cpu_baseline", "cpu_baseline_c1")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--width", "320", "--height", "181", "--spp", "8",
           "--prewarm", "0"] + list(extra)
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_carries_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    for k in HEADLINE:
        assert k in plain, k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["higher_is_better"] is True and plain["unit"] == "Msamples/s" and plain["dtype"] == "f32"
    assert (plain["steps"], plain["warmup"], plain["batches_per_launch"], plain["launches"]) == (4, 1, 4, 1)
    assert not [k for k in FULL_ONLY if k in plain], plain.keys()

    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"))
    for k in HEADLINE:
        assert k in full, k
    assert not [k for k in FULL_ONLY if k not in full], full.keys()
    assert full["cpu_baseline"]["value"] > 0 and full["plain_batches"]["value"] > 0 and full["chain2"]["value"] > 0
    assert set(full["post_passes"]) >= {"1920x1080", "3840x2160"}
    assert (full["steps"], full["warmup"], full["batches_per_launch"], full["launches"]) == (4, 1, 4, 1)

    # the timed steps are the same steps: their outputs are bit for bit the same with and without --full
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and {"color.npy", "ray_count.npy"} <= set(names)
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
