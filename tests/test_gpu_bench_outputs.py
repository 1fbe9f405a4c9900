"""GPU: bench.py's one-GPU command line.  A plain run times exactly --steps frames and its line holds the headline only; --dump-outputs writes
what the last timed frame returned, the same bits again on a run with the same frame; --full adds the secondary blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = {"fitted", "train", "multi_frame", "drop_in", "nav", "cpu_baseline", "cpu_config1", "psnr_vs_oracle_db"}


def _bench(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--res", "200"] + args, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_times_its_steps_and_dumps_the_last_frame(tmp_path):
    a, b, c = (str(tmp_path / n) for n in "abc")
    j = _bench(["--steps", "5", "--warmup", "2", "--dump-outputs", a])
    assert j["steps"] == 5 and j["config"]["frames_per_gpu"] == 5 and j["ms_per_step"] > 0 and j["value"] > 0
    assert not SECONDARY & set(j)
    out = _load(a)
    assert set(out) == {"image", "depth", "weights_sum", "stats"}
    assert out["image"].dtype == np.float32 and out["image"].shape == (1, 200 * 200, 3) and out["stats"].dtype == np.float64
    assert 0 < out["stats"][0] <= j["config"]["samples_per_ray"] * 5 * 200 * 200
    _bench(["--steps", "13", "--warmup", "0", "--dump-outputs", b])          # last frame = pose 12 % 8 = 4 again: the same bits
    _bench(["--steps", "6", "--warmup", "2", "--dump-outputs", c])           # last frame = pose 5
    again, other = _load(b), _load(c)
    for k in out:
        assert np.array_equal(out[k], again[k]), k
    assert not np.array_equal(out["image"], other["image"])


def test_full_run_adds_the_secondary_blocks():
    j = _bench(["--full", "--steps", "3", "--warmup", "1", "--fit-steps", "96", "--train-steps", "16", "--fit-frames", "2", "--cpu-res", "48",
                "--fit-cpu-res", "48", "--nav-iters", "2", "--drop-in-frames", "1", "--frames-per-launch", "2"])
    assert SECONDARY <= set(j) and j["steps"] == 3
    assert j["train"]["steps"] == 16 and j["fitted"]["frames"] == 2 and j["multi_frame"]["frames_per_launch"] == 2
    assert j["psnr_vs_oracle_db"] > 60
