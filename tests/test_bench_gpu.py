"""GPU tests of bench.py's plain run: the headline line alone, and --dump-outputs (what the timed path computed in its last step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert out and all(f.endswith(".npy") for f in os.listdir(d))
    return out


def test_plain_run_dumps_the_last_step(hiplib, tmp_path):
    """A plain run prints the headline line without the --full legs; --dump-outputs writes float32 / float64 arrays of the last
    timed step (the step's 2 x 16 images, 16 stereo and brute-force matches, the windows of its keyframes), at most 64 MB, and a
    second run with the same arguments writes the same arrays."""
    import bench
    steps, warmup = 3, 1
    runs = []
    for k in range(2):
        d = _bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / str(k)))
        assert all(key in d for key in HEADLINE) and d["steps"] == steps and d["warmup"] == warmup
        assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True
        assert not any(key in d for key in ("roofline", "pcie_inclusive", "contiguous", "cpu_baseline", "tracker", "global_ba"))
        runs.append(_load(tmp_path / str(k)))
    a, b = runs
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    counts = a["keypoint_counts"]
    assert len(counts) == 2 * bench.FRAMES_PER_STEP and counts.min() > 100
    assert len(a["keypoints"]) == len(a["descriptors"]) == counts.sum()
    assert len(a["stereo_depth"]) == len(a["bf_knn2"]) == counts[0::2].sum()
    last = warmup + steps - 1
    n_kf = sum(1 for g in range(last * bench.FRAMES_PER_STEP, (last + 1) * bench.FRAMES_PER_STEP) if g % bench.KF_INTERVAL == 0)
    assert a["ba_poses"].shape == (n_kf, bench.BA_KF, 7) and a["ba_points"].shape == (n_kf, bench.BA_PTS, 3)
    assert np.all(np.nanmin(a["ba_log"][:, :, 1], axis=1) < a["ba_log"][:, 0, 0])         # every window lowered its chi2
    assert sorted(a) == sorted(b)
    for name in a:
        if name.startswith("ba_"):
            assert np.allclose(a[name], b[name], rtol=1e-9, atol=1e-9, equal_nan=True), name
        else:
            assert np.array_equal(a[name], b[name]), name
